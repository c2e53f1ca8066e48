"""TEST INFRASTRUCTURE ONLY -- runs oracle/_ref/ref_dump (the reference's own code, built by oracle/ref_dump/build.sh)
on one problem description and reads its dump back.  Used by tests/test_ref_dump.py and by oracle/ref_golden.py; needs
nothing but numpy, so it also works where the product library is not built."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
ROBOTS = {"monoped": 0, "biped": 1, "hyq": 2, "anymal": 3, "go1": 4}                                   # RobotModel::Robot
TERRAINS = {"flat": 0, "block": 1, "stairs": 2, "gap": 3, "slope": 4, "chimney": 5, "chimney_lr": 6}   # HeightMap::TerrainID
PARAM_KEYS = ("dt_dynamic", "dt_rom", "duration_base_poly", "polys_per_swing", "polys_per_stance_force", "dt_base_motion",
              "base_z_init")


def available():
    """True where oracle/_ref/ref_dump was built (here, or on the box this tree was copied from)."""
    status = os.path.join(REF, "STATUS")
    return os.path.exists(os.path.join(REF, "ref_dump")) and os.path.exists(status) and open(status).read().strip() == "available"


def deps():
    p = os.path.join(REF, "DEPS")
    return open(p).read().strip() if os.path.exists(p) else "unknown"


def command(prefix, robot, terrain, mask, x="guess", durations=None, contact=None, combo=0, T=0.0, goal_x=1.0, params=None,
            csv_heights=None, extra=(), sample_dt=None, guess_times=None, planes=None):
    """The ref_dump command line for one problem; writes the input files it names next to `prefix`.  `params` holds any
    of PARAM_KEYS; `x` is "guess" or the variable vector; the schedule is either (durations, contact) or (combo, T).
    The fpowr extractors on that x: sample_dt (GetTrajectory), guess_times (ExtractInitialGuesses) and planes =
    (regions (n, 7) [position xyz | orientation xyzw], one (k, 2) array of local boundary points per region, time horizon)
    for ExtractFootstepPlan; read_extracted() reads what they wrote."""
    params = dict(params or {})
    if isinstance(x, str):
        xarg = x
    else:
        xarg = prefix + "_xin.txt"
        np.savetxt(xarg, np.asarray(x), fmt="%.17g")
    cmd = [os.path.join(REF, "ref_dump"), str(ROBOTS[robot]), str(TERRAINS.get(terrain, 0)), str(int(combo)), "%.17g" % T, str(int(mask)),
           xarg, "%.17g" % goal_x, prefix]
    if durations is not None:
        with open(prefix + "_phases_in.txt", "w") as f:
            for d, c in zip(durations, contact):
                f.write("%d %s\n" % (int(c), " ".join("%.17g" % v for v in d)))
        cmd += ["--phases", prefix + "_phases_in.txt"]
    if "dt_dynamic" in params or "dt_rom" in params:
        cmd += ["--dt", "%.17g" % params.get("dt_dynamic", 0.0), "%.17g" % params.get("dt_rom", 0.0)]
    if any(k in params for k in PARAM_KEYS[2:]):
        z = params.get("base_z_init", float("nan"))
        cmd += ["--params", "%.17g" % params.get("duration_base_poly", 0.0), str(int(params.get("polys_per_swing", 0))),
                str(int(params.get("polys_per_stance_force", 0))), "%.17g" % params.get("dt_base_motion", 0.0),
                "nan" if z != z else "%.17g" % z]
    if terrain == "csv":
        np.savetxt(prefix + "_heights.csv", np.asarray(csv_heights), fmt="%.17g", delimiter=",")
        cmd += ["--csv", prefix + "_heights.csv"]
    if sample_dt is not None:
        cmd += ["--sample", "%.17g" % sample_dt]
    if guess_times is not None:
        np.savetxt(prefix + "_guess_times.txt", np.asarray(guess_times, dtype=np.float64), fmt="%.17g")
        cmd += ["--guess-times", prefix + "_guess_times.txt"]
    if planes is not None:
        regions, boundaries, horizon = planes
        with open(prefix + "_planes.txt", "w") as f:
            for r, b in zip(np.asarray(regions, dtype=np.float64).reshape(-1, 7), boundaries):
                b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
                f.write(" ".join("%.17g" % v for v in list(r) + [len(b)] + list(b.reshape(-1))) + "\n")
        cmd += ["--planes", prefix + "_planes.txt", "%.17g" % horizon]
    return cmd + list(extra)


def read_extracted(prefix, n_ee):
    """What --sample / --guess-times / --planes wrote, for those that were given: traj (n, 20 + 13 n_ee), guess (n, 49),
    plan_duration (steps) and plan_contact_set (steps, n_ee)."""
    out = {}
    if os.path.exists(prefix + "_traj.txt"):
        out["traj"] = np.loadtxt(prefix + "_traj.txt", ndmin=2)
        assert out["traj"].shape[1] == 20 + 13 * n_ee
    if os.path.exists(prefix + "_guess.txt"):
        out["guess"] = np.loadtxt(prefix + "_guess.txt", ndmin=2)
        assert out["guess"].shape[1] == 49
    if os.path.exists(prefix + "_plan.txt"):
        plan = np.loadtxt(prefix + "_plan.txt", ndmin=2)
        assert plan.shape[1] == 1 + n_ee
        out["plan_duration"] = plan[:, 0].copy()
        out["plan_contact_set"] = plan[:, 1:].astype(np.int32)
    return out


def read(prefix):
    """The dump of one ref_dump run as a dict of numpy arrays (+ the set tables and the schedule)."""
    trip = np.loadtxt(prefix + "_jac.txt", ndmin=2)
    out = dict(x=np.loadtxt(prefix + "_x.txt", ndmin=1), g=np.loadtxt(prefix + "_g.txt", ndmin=1),
               jac_row=trip[:, 0].astype(np.int32), jac_col=trip[:, 1].astype(np.int32), jac_val=trip[:, 2].copy())
    b = np.loadtxt(prefix + "_bounds.txt", ndmin=2)
    xb = np.loadtxt(prefix + "_xbounds.txt", ndmin=2)
    out.update(g_lower=b[:, 0].copy(), g_upper=b[:, 1].copy(), x_lower=xb[:, 0].copy(), x_upper=xb[:, 1].copy())
    con, var = [], []
    for line in open(prefix + "_sets.txt"):
        kind, name, rows = line.split()
        (con if kind == "con" else var).append((name, int(rows)))
    out["con_sets"], out["var_sets"] = con, var
    durations, contact = [], []
    for line in open(prefix + "_phases.txt"):
        t = line.split()
        contact.append(int(t[0]))
        durations.append([float(v) for v in t[1:]])
    out["durations"], out["contact"] = durations, contact
    return out


def run(prefix, *args, timeout=600, **kw):
    cmd = command(prefix, *args, **kw)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("ref_dump exit %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
    out = read(prefix)
    out.update(read_extracted(prefix, len(out["contact"])))
    return out


TERRAIN_BASIS_VALUES = 27   # ref_dump --terrain-points: three normalised basis vectors, then their six derivatives


def terrain_points(prefix, terrain_ids, xy, with_basis, csv_heights=None, timeout=600):
    """ref_dump --terrain-points: the reference's terrains at the points xy (n, 2) of terrain_ids (n,) (HeightMap::TerrainID,
    7 = HeightMapFromCSV over csv_heights).  Returns (values (n, 4) [h, hx, hy, hxx], basis (k, 27) for the k points whose
    with_basis flag is set, in their order)."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    flags = np.asarray(with_basis, dtype=bool)
    rec = np.column_stack([np.asarray(terrain_ids, dtype=np.float64), xy, flags.astype(np.float64)])
    np.ascontiguousarray(rec).tofile(prefix + "_points.bin")
    cmd = [os.path.join(REF, "ref_dump"), "--terrain-points", prefix + "_points.bin", prefix + "_terrain.bin"]
    if csv_heights is not None:
        np.savetxt(prefix + "_heights.csv", np.asarray(csv_heights), fmt="%.17g", delimiter=",")
        cmd += ["--csv", prefix + "_heights.csv"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("ref_dump exit %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
    out = np.fromfile(prefix + "_terrain.bin", dtype=np.float64)
    width = 4 + TERRAIN_BASIS_VALUES * flags.astype(np.int64)
    start = np.concatenate([[0], np.cumsum(width)])
    assert out.size == start[-1], (out.size, start[-1])
    values = out[start[:-1, None] + np.arange(4)[None, :]]
    basis = out[start[:-1][flags][:, None] + 4 + np.arange(TERRAIN_BASIS_VALUES)[None, :]] if flags.any() else np.zeros((0, TERRAIN_BASIS_VALUES))
    return values, basis


def _segment_run(prefix, doubles, timeout):
    np.ascontiguousarray(doubles, dtype=np.float64).tofile(prefix + "_segments_in.bin")
    cmd = [os.path.join(REF, "ref_dump"), "--segment-points", prefix + "_segments_in.bin", prefix + "_segments_out.bin"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("ref_dump exit %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
    return np.fromfile(prefix + "_segments_out.bin", dtype=np.float64)


def segment_points(prefix, lists, point_list, point_t, timeout=600):
    """ref_dump --segment-points, mode 0: Spline::GetSegmentID and GetLocalTime at the times point_t (n,) on the duration lists
    lists[point_list[k]].  Returns (id (n,) int32, t_local (n,)); ref_dump refuses (exit code 5) a time for which the lookup
    is not defined."""
    parts = [[0.0, float(len(lists))]]
    for d in lists:
        parts += [[float(len(d))], np.asarray(d, dtype=np.float64)]
    parts += [[float(len(point_t))], np.column_stack([np.asarray(point_list, dtype=np.float64), np.asarray(point_t, dtype=np.float64)]).ravel()]
    out = _segment_run(prefix, np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]), timeout).reshape(-1, 3)
    assert len(out) == len(point_t) and np.array_equal(out[:, 0], out[:, 1]), "GetLocalTime's id is GetSegmentID's"
    return out[:, 0].astype(np.int32), out[:, 2].copy()


def segment_durations(prefix, cases, timeout=600):
    """ref_dump --segment-points, mode 1: per case (n_phases, in contact at start, polynomials per swing phase, per stance phase
    of the force, given durations, schedule variables) the reference's (phase durations after PhaseDurations::SetVariables,
    ConvertPhaseToPolyDurations of the ee-motion nodes, of the ee-force nodes)."""
    parts = [[1.0, float(len(cases))]]
    for n, contact, pps, ppf, given, variables in cases:
        assert len(given) == n and len(variables) == n - 1
        parts += [[float(n), float(bool(contact)), float(pps), float(ppf)], given, variables]
    out = _segment_run(prefix, np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]), timeout)
    res, at = [], 0
    for n, *_ in cases:
        ph = out[at:at + n]
        nm = int(out[at + n])
        md = out[at + n + 1:at + n + 1 + nm]
        nf = int(out[at + n + 1 + nm])
        fd = out[at + n + 2 + nm:at + n + 2 + nm + nf]
        at += n + 2 + nm + nf
        res.append((ph.copy(), md.copy(), fd.copy()))
    assert at == out.size
    return res


def plane_points(prefix, scenes, timeout=600):
    """ref_dump --plane-points: per scene (regions (n, 7) [position xyz, orientation xyzw], local boundary rings [(k, 2)], query
    points (m, 2)) the reference's (world rings as PlanarRegionsToPolygons made them [(k, 2)], GetNearestPlaneIndex per point (m,)
    int32, bg::distance per point and region (m, n))."""
    parts = [[float(len(scenes))]]
    for regions, rings, points in scenes:
        regions = np.asarray(regions, dtype=np.float64).reshape(-1, 7)
        assert len(regions) == len(rings)
        parts.append([float(len(rings))])
        for pose, ring in zip(regions, rings):
            ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
            parts += [pose, [float(len(ring))], ring.ravel()]
        points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
        parts += [[float(len(points))], points.ravel()]
    np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]).tofile(prefix + "_planes_in.bin")
    cmd = [os.path.join(REF, "ref_dump"), "--plane-points", prefix + "_planes_in.bin", prefix + "_planes_out.bin"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("ref_dump exit %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
    out = np.fromfile(prefix + "_planes_out.bin", dtype=np.float64)
    res, at = [], 0
    for regions, rings, points in scenes:
        world = []
        for ring in rings:
            k = len(np.asarray(ring).reshape(-1, 2))
            world.append(out[at:at + 2 * k].reshape(k, 2).copy())
            at += 2 * k
        m, n = len(np.asarray(points).reshape(-1, 2)), len(rings)
        index = out[at:at + m].astype(np.int32)
        assert np.array_equal(index, out[at:at + m])
        at += m
        res.append((world, index, out[at:at + m * n].reshape(m, n).copy()))
        at += m * n
    assert at == out.size, (at, out.size)
    return res


def _attitude_run(prefix, mode, rows, timeout):
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    np.concatenate([[float(mode), float(len(rows))], rows.ravel()]).tofile(prefix + "_attitude_in.bin")
    cmd = [os.path.join(REF, "ref_dump"), "--attitude-points", prefix + "_attitude_in.bin", prefix + "_attitude_out.bin"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        raise RuntimeError("ref_dump exit %d: %s\n%s" % (r.returncode, " ".join(cmd), (r.stdout + r.stderr)[-2000:]))
    return np.fromfile(prefix + "_attitude_out.bin", dtype=np.float64)


def attitude_quaternions(prefix, R, timeout=600):
    """ref_dump --attitude-points, mode 0: Eigen::Quaterniond(R) of the build's Eigen (deps()) on matrices R (n, 9) row-major, as
    (n, 4) x y z w"""
    out = _attitude_run(prefix, 0, np.asarray(R, dtype=np.float64).reshape(-1, 9), timeout).reshape(-1, 4)
    assert len(out) == len(R)
    return out


def attitude_states(prefix, nodes, timeout=600):
    """ref_dump --attitude-points, mode 1: per row of nodes (n, 12) [p0 v0 p1 v1] of a one-polynomial Euler-angle spline of
    duration 1 the reference's (state (9) GetPoint(0) returned, GetRotationMatrixBaseToWorld (9), GetQuaternionBaseToWorld (4,
    x y z w), GetAngularVelocityInWorld (3), GetAngularAccelerationInWorld (3)) of that state"""
    out = _attitude_run(prefix, 1, np.asarray(nodes, dtype=np.float64).reshape(-1, 12), timeout).reshape(-1, 28)
    assert len(out) == len(nodes)
    return out[:, :9].copy(), out[:, 9:18].copy(), out[:, 18:22].copy(), out[:, 22:25].copy(), out[:, 25:28].copy()


def case_args(case):
    """(args, kwargs) of command() / run() for a tests.common.Case (every field a Case can set reaches the reference)."""
    p = case.params
    params = {k: getattr(p, k) for k in PARAM_KEYS}
    kw = dict(durations=case.sched.durations(), contact=case.sched.contact(), params=params)
    if case.terrain == "csv":
        kw["csv_heights"] = case.grid.heights
    return (case.robot, case.terrain, p.constraint_sets), kw


def formulation_states(case, goal_x=1.0):
    """(initial base position, final base position, initial feet) that oracle/ref_dump/ref_dump.cc sets up around the
    formulation for a tests.common.Case: nominal stance on the ground, the base at base_z_init (default: nominal
    height), the goal at goal_x with the base at nominal height above the terrain (nlp_formulation.cc:105-108)."""
    lin0, ee0 = case.nominal_start()
    z_nominal = lin0[2]
    z = case.params.base_z_init
    if z == z:
        lin0 = [0.0, 0.0, z]
    return lin0, [goal_x, 0.0, case.P.terrain_probe(goal_x, 0.0)[0] + z_nominal], ee0
