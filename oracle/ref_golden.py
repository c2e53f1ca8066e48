"""TEST INFRASTRUCTURE ONLY -- records what the reference's own code computes as fixtures tests/golden/ref_*.npz:

    python -m oracle.ref_golden [names...]          (no name: every case of CASES)

Runs only where oracle/_ref/ref_dump exists (oracle/ref_dump/build.sh, i.e. where the reference sources are).  A
fixture holds the case description (robot, terrain, schedule, every parameter, CSV heights if any), the Jacobian pattern
once (jac_row, jac_col), constraint and variable bounds (rows lower / upper), the set tables, and for each of several x: x, g, jac_val --
recorded outputs of the reference's programs, nothing else.  tests/test_ref_golden.py replays them against the oracle,
the structure builder (CPU) and the device (GPU) on boxes that do not have the reference.

    python -m oracle.ref_golden --traj [names...]   (the fixtures tests/golden/reftraj_*.npz, see TRAJ_CASES below)
    python -m oracle.ref_golden --terrain [names...]   (tests/golden/refterrain_*.npz, see TERRAIN_FIXTURES below)
    python -m oracle.ref_golden --segments          (tests/golden/refsegment.npz, see record_segments below)
    python -m oracle.ref_golden --planes            (tests/golden/refplane.npz, see record_planes below)
    python -m oracle.ref_golden --attitude          (tests/golden/refattitude.npz, see record_attitude below)
    python -m oracle.ref_golden --attitude --check  (records afresh and compares with the committed file, writes nothing)

The cases are chosen for what the mpmath fixtures and the hand known-answers cannot reach: entries the reference DEFINES
rather than derives (force rows x footholds on curved terrain, terrain rows of gridded terrain, explicit zeros), bounds,
every robot and constraint name, optimised timings, odd schedules, and the BASELINE sizes where the quirk lives."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_EE = {"monoped": 1, "biped": 2, "hyq": 4, "anymal": 4, "go1": 4}


def _combo(robot, combo, T, scale=1.0):
    import towr_amd as ta

    return ta.gait_combo(N_EE[robot], combo, T, scale)


def _sched(durs, contact):
    import towr_amd as ta

    return ta.schedule(durs, contact)


def _mp_schedule(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    durs, o = [], 0
    for k in d["n_phases"]:
        durs.append(d["phase_durations"][o:o + k])
        o += k
    return _sched(durs, list(d["contact_at_start"]))


def _k(T, K):
    dt = T / (K - 1.5)
    return dict(dt_dynamic=dt, dt_rom=dt)


def _phases(n_ee, n_ph, T, start_contact, seed):
    rng = np.random.default_rng(seed)
    durs = []
    for _ in range(n_ee):
        d = rng.uniform(0.2, 0.6, size=n_ph)
        durs.append(d * (T / d.sum()))
    return _sched(durs, [int(start_contact)] * n_ee)


# name -> (robot, terrain, schedule builder, params, x families); an x family is ("guess" | "perturbed" | "wild" | "snapped" | "junctions", seed)
W2 = (("wild", 1), ("wild", 2))
P1 = (("perturbed", 1),)
W1 = (("wild", 1),)
COARSE = dict(dt_dynamic=0.3, dt_rom=0.25, duration_base_poly=0.2, dt_base_motion=0.11)
CASES = {
    # the quirk entries: force + terrain sets at wild footholds spread over the terrain features
    # (quirk_gap runs on the schedule and, first, at the x of tests/golden/mp_full_anymal_trot_gap.npz, so that the mpmath
    # chain-rule values of the same entries can serve as a negative control in tests/test_ref_golden.py)
    "quirk_gap": ("anymal", "gap", lambda: _mp_schedule("mp_full_anymal_trot_gap"), dict(constraint_sets=17),
                  (("mp_full_anymal_trot_gap", 0), ("wild", 1), ("wild", 2))),
    "quirk_stairs": ("anymal", "stairs", lambda: _combo("anymal", 0, 2.4), dict(constraint_sets=17), W2),
    "quirk_block": ("hyq", "block", lambda: _combo("hyq", 2, 1.8), dict(constraint_sets=17), W2),
    "quirk_slope": ("biped", "slope", lambda: _combo("biped", 1, 1.6), dict(constraint_sets=17), W2),
    "quirk_chimney": ("go1", "chimney", lambda: _combo("go1", 3, 2.0), dict(constraint_sets=17), W2),
    "quirk_chimney_lr": ("monoped", "chimney_lr", lambda: _combo("monoped", 2, 2.0), dict(constraint_sets=17), W2),
    "quirk_gap_default_sets": ("biped", "gap", lambda: _combo("biped", 0, 1.6, 0.9), dict(constraint_sets=63, dt_dynamic=0.2, dt_rom=0.2), W1),
    # every robot, every constraint name incl. baseMotion, optimised timings
    "every_monoped": ("monoped", "flat", lambda: _combo("monoped", 2, 1.2), dict(constraint_sets=255, base_z_init=0.58, **COARSE), P1),
    "every_biped": ("biped", "slope", lambda: _combo("biped", 1, 1.2), dict(constraint_sets=255, base_z_init=0.65, **COARSE), W1),
    "every_hyq": ("hyq", "chimney", lambda: _combo("hyq", 3, 1.0), dict(constraint_sets=255, base_z_init=0.58, **COARSE), P1),
    "every_anymal": ("anymal", "stairs", lambda: _combo("anymal", 1, 1.0), dict(constraint_sets=255, base_z_init=0.42, **COARSE), W1),
    "every_go1": ("go1", "block", lambda: _combo("go1", 0, 1.2), dict(constraint_sets=255, base_z_init=0.3, **COARSE), P1),
    "timings_63_monoped": ("monoped", "stairs", lambda: _combo("monoped", 1, 1.2), dict(constraint_sets=63, dt_dynamic=0.2, dt_rom=0.2), W1),
    "timings_127_biped": ("biped", "gap", lambda: _combo("biped", 0, 1.2), dict(constraint_sets=127, **COARSE), P1),
    # junctions of the optimised phases on the thresholds of the segment lookup (Case.x_junctions: an accumulated sum on
    # fl(t - 1e-10) of a time node t, on its neighbours, on t itself); K = 12 and one x: what the size budget of this set leaves
    "timings_junctions_biped": ("biped", "gap", lambda: _combo("biped", 0, 1.2), dict(constraint_sets=127, duration_base_poly=0.2, **_k(1.2, 12)),
                                (("junctions", 1),)),
    "timings_rom_only": ("biped", "flat", lambda: _combo("biped", 2, 1.2), dict(constraint_sets=64 | 8, dt_rom=0.21), W1),
    "timings_dynamic_only": ("biped", "block", lambda: _combo("biped", 2, 1.2), dict(constraint_sets=64 | 2, dt_dynamic=0.23), P1),
    "timings_terrain_force": ("hyq", "slope", lambda: _combo("hyq", 1, 1.2), dict(constraint_sets=64 | 16 | 1), W1),
    "polys_3_1": ("biped", "stairs", lambda: _combo("biped", 3, 1.2), dict(constraint_sets=63, polys_per_swing=3, polys_per_stance_force=1, **COARSE), P1),
    "polys_1_4_timings": ("monoped", "gap", lambda: _combo("monoped", 0, 1.2), dict(constraint_sets=127, polys_per_swing=1, polys_per_stance_force=4,
                                                                                  **COARSE), W1),
    "fine_base_spline": ("monoped", "slope", lambda: _combo("monoped", 2, 0.9), dict(constraint_sets=31 | 128, duration_base_poly=0.023, base_z_init=0.6,
                                                                                    dt_dynamic=0.27, dt_rom=0.3, dt_base_motion=0.1), P1),
    # schedules
    "flight_start_end": ("biped", "gap", lambda: _phases(2, 4, 1.3, False, 11), dict(constraint_sets=31, **COARSE), W1),   # swing, stance, swing, stance
    "flight_start_ends_in_flight": ("monoped", "block", lambda: _phases(1, 3, 1.1, False, 12), dict(constraint_sets=31 | 64, **COARSE), P1),
    "standing_one_phase": ("anymal", "flat", lambda: _phases(4, 1, 0.9, True, 13), dict(constraint_sets=31 | 128, base_z_init=0.45, **COARSE), P1),
    "phases_31": ("monoped", "stairs", lambda: _phases(1, 31, 9.0, True, 14), dict(constraint_sets=63 | 64, dt_dynamic=1.1, dt_rom=0.9, duration_base_poly=0.9), W1),
    "two_nodes": ("hyq", "slope", lambda: _combo("hyq", 0, 1.2), dict(constraint_sets=63, dt_dynamic=1.7, dt_rom=1.3, duration_base_poly=0.3), W1),
    # gridded terrain, footholds snapped onto cell edges
    "csv_snapped": ("anymal", "csv", lambda: _combo("anymal", 1, 1.2), dict(constraint_sets=17), (("snapped", 1), ("snapped", 2))),
    # BASELINE sizes: C1-C3 at default x families, C4 / C5 (where the quirk lives) at one wild and one perturbed x each
    "c1_hopper": ("monoped", "flat", lambda: _sched([[0.4, 0.2, 0.4, 0.2, 0.4, 0.2, 0.2]], [1]), dict(), (("guess", 0), ("perturbed", 1))),
    "c2_biped_k100": ("biped", "flat", lambda: _combo("biped", 0, 2.0), _k(2.0, 100), (("guess", 0),)),
    "c3_anymal_trot_k200": ("anymal", "flat", lambda: _combo("anymal", 1, 2.0), _k(2.0, 200), (("guess", 0),)),
    "c4_gap_k200_wild": ("anymal", "gap", lambda: _combo("anymal", 2, 1.8, 0.9), _k(1.8, 200), W1),
    "c4_gap_k200_perturbed": ("anymal", "gap", lambda: _combo("anymal", 2, 1.8, 0.9), _k(1.8, 200), P1),
    "c5_stairs_k200_wild": ("anymal", "stairs", lambda: _combo("anymal", 0, 2.4, 1.1), _k(2.4, 200), W1),
    "c5_stairs_k200_perturbed": ("anymal", "stairs", lambda: _combo("anymal", 0, 2.4, 1.1), _k(2.4, 200), P1),
}


def csv_heights(name):
    rng = np.random.default_rng(21 + len(name))
    return np.round(rng.uniform(0.0, 0.3, size=(16, 22)), 2)


def make_x(case, family, seed):
    if family.startswith("mp_"):
        return np.load(os.path.join(GOLDEN, family + ".npz"))["x"].copy()
    if family == "guess":
        return case.x_guess()
    if family == "perturbed":
        return case.x_perturbed(seed)
    if family == "junctions":
        return case.x_junctions(seed)
    x = case.x_wild(seed)
    if family == "snapped":   # a third of the foothold coordinates next to the edges of the 0.17 m cells (inside and outside
        # the slope window), a tenth of them exactly ON an edge (k * 0.17 as the double product: the tie of the cell index)
        rng = np.random.default_rng(500 + seed)
        for vs in case.S.var_sets:
            if vs["name"].startswith("ee-motion"):
                seg = x[vs["offset"]:vs["offset"] + vs["size"]]
                pick = rng.random(seg.size) < 0.35
                seg[pick] = np.round(seg[pick] / 0.17) * 0.17 + rng.uniform(-0.004, 0.004, size=pick.sum())
                exact = rng.random(seg.size) < 0.1
                seg[exact] = np.round(seg[exact] / 0.17) * 0.17
    return x


def save_npz_lzma(path, arrays):
    """An .npz (numpy.load reads it like any other) whose members are LZMA-compressed: the Jacobian values repeat over
    long distances (the same polynomial weights at every sample), which deflate's 32 KB window cannot see -- 424 KB
    instead of 655 KB for the values of a K = 200 problem."""
    import zipfile

    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_LZMA) as z:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_LZMA
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def record(name, workdir):
    from oracle import ref_run
    from tests.common import Case

    robot, terrain, sched, params, families = CASES[name]
    grid = csv_heights(name) if terrain == "csv" else None
    case = Case(robot, terrain, sched(), grid=grid, **params)
    args, kw = ref_run.case_args(case)
    xs, gs, js, first = [], [], [], None
    for family, seed in families:
        x = make_x(case, family, seed)
        d = ref_run.run(os.path.join(workdir, "%s_%s%d" % (name, family, seed)), *args, x=x, **kw)
        assert np.array_equal(d["x"], x)
        if first is None:
            first = d
        assert np.array_equal(d["jac_row"], first["jac_row"]) and np.array_equal(d["jac_col"], first["jac_col"]), "the pattern must not depend on x"
        xs.append(x), gs.append(d["g"]), js.append(d["jac_val"])
    p = case.params
    out = dict(robot=robot, terrain=terrain, n_phases=np.array([len(v) for v in first["durations"]], dtype=np.int32),
               phase_durations=np.concatenate(case.sched.durations()), contact_at_start=np.array(case.sched.contact(), dtype=np.int32),
               constraint_sets=np.int32(p.constraint_sets), x_family=np.array(["%s%d" % f for f in families]),
               jac_row=first["jac_row"], jac_col=first["jac_col"], g_bounds=np.array([first["g_lower"], first["g_upper"]]),
               x_bounds=np.array([first["x_lower"], first["x_upper"]]),
               con_names=np.array([n for n, _ in first["con_sets"]]), con_rows=np.array([r for _, r in first["con_sets"]], dtype=np.int32),
               var_names=np.array([n for n, _ in first["var_sets"]]), var_rows=np.array([r for _, r in first["var_sets"]], dtype=np.int32),
               x=np.array(xs), g=np.array(gs), jac_val=np.array(js), reference_deps=ref_run.deps())
    out["params"] = np.array([getattr(p, k) for k in ref_run.PARAM_KEYS], dtype=np.float64)   # in the order of ref_run.PARAM_KEYS
    if grid is not None:
        out["csv_heights"] = grid
    path = os.path.join(GOLDEN, "ref_%s.npz" % name)
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), len(first["g"]), len(first["jac_row"])


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/reftraj_<case>.npz: what fpowr's extractors (footstep_plan_extractor.h, initial_guess_extractor.h,
# nearest_plane_lookup.h -- the reference's own headers, run by ref_dump --sample / --guess-times / --planes) produce on a
# solution x.  (The prefix keeps them out of the ref_*.npz glob and its size budget.)  Per case: the problem description
# with the keys of the ref_* fixtures, x[k], dt and traj[k] = GetTrajectory(x[k], dt), guess_times and guess[k] =
# ExtractInitialGuesses, the planar regions (regions, region_start, region_xy) and, from ExtractFootstepPlan at the
# reference's fixed 0.01 s and its 2 s horizon, plan_steps[k], plan_duration[k], plan_contact_set[k] (padded to the
# longest plan with NaN / -2) plus plan_state[k]: the rows of GetTrajectory(x[k], 0.01) at which the contact flags
# change, i.e. the footstep states themselves (the quadrupeds record traj at a coarser dt to stay within the size budget).
# tests/test_ref_traj.py states what the set has to cover and asserts it on the recorded arrays.
PLAN_DT, PLAN_HORIZON = 0.01, 2.0   # footstep_plan_extractor.h:87, footstep_plan_server.cc:31
# name -> (robot, terrain, schedule builder, params, dt, x seeds, scale of base-ang)
TRAJ_CASES = {
    "hopper": ("monoped", "flat", lambda: _sched([[0.4, 0.2, 0.4, 0.2, 0.4, 0.2, 0.2]], [1]), dict(constraint_sets=63), 0.01, (1, 2), 4.0),
    "monoped_timings": ("monoped", "stairs", lambda: _combo("monoped", 1, 1.2), dict(constraint_sets=127, polys_per_swing=3, duration_base_poly=0.13),
                        0.01, (3,), 5.0),
    "biped_swing_start": ("biped", "gap", lambda: _phases(2, 4, 1.3, False, 11), dict(constraint_sets=31), 0.01, (4,), 6.0),
    "biped_timings": ("biped", "flat", lambda: _combo("biped", 0, 1.2), dict(constraint_sets=127, polys_per_stance_force=2), 0.01, (5,), 4.0),
    "anymal_stairs": ("anymal", "stairs", lambda: _combo("anymal", 1, 2.0), dict(constraint_sets=63), 0.025, (6,), 5.0),
    "anymal_gap_timings": ("anymal", "gap", lambda: _combo("anymal", 0, 2.0), dict(constraint_sets=127), 0.03, (7,), 5.0),
    # an eighth field: the schedule variables are those of Case.x_junctions(seed, times = the accumulated sample times), and
    # the guess times add the threshold doubles of every junction of that x with their neighbouring doubles
    "biped_junctions": ("biped", "stairs", lambda: _combo("biped", 0, 1.2), dict(constraint_sets=127, polys_per_swing=3, **_k(1.2, 32)), 0.01, (8, 3),
                        4.0, "junctions"),
}


def traj_regions():
    """The planar regions every reftraj fixture carries: (regions (n, 7) [position xyz | orientation xyzw], list of local
    boundary points).  Boundary points are multiples of 1/64 (exact in the message's float32).  0 and 1 overlap; 1 is
    counter-clockwise; 2 is not closed; 3 is tilted, with a quaternion that is not normalised; 4 has three points (below
    the minimum of a ring: it holds nothing, only its two edges are near); 5 and 6 are one square listed twice, so every
    contact nearest to it is exactly equidistant from both and the first-wins rule decides."""
    sq = lambda x0, x1, y0, y1: np.array([[x0, y0], [x0, y1], [x1, y1], [x1, y0], [x0, y0]])   # clockwise, closed
    c, s_ = np.cos(0.15), np.sin(0.15)
    tilt = np.array([np.sin(0.25), 0.0, 0.0, np.cos(0.25)])              # 0.5 rad about x ...
    yaw = np.array([0.0, 0.0, np.sin(0.35), np.cos(0.35)])               # ... then 0.7 rad about z
    x1, y1, z1, w1 = yaw
    x2, y2, z2, w2 = tilt
    q = 2.0 * np.array([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                        w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2])
    regions = [[0.0, 0.0, 0.0, 0, 0, 0, 1], [0.5, 0.0, 0.05, 0, 0, s_, c], [0.875, 0.25, 0.0, 0, 0, 0, 1], [1.125, -0.25, 0.1, *q],
               [0.25, -0.625, 0.0, 0, 0, 0, 1], [1.375, 0.0, 0.2, 0, 0, 0, 1], [1.375, 0.0, 0.2, 0, 0, 0, 1]]
    pent = np.array([[0.25, 0.0], [0.078125, -0.234375], [-0.203125, -0.140625], [-0.203125, 0.140625], [0.078125, 0.234375]])   # open
    bounds = [sq(-0.5, 0.5, -0.125, 0.5), sq(-0.375, 0.25, -0.375, 0.375)[::-1].copy(), pent, sq(-0.25, 0.25, -0.1875, 0.1875),
              np.array([[-0.125, 0.0], [0.125, 0.0], [0.0, -0.125]]), sq(-0.0625, 0.0625, -0.0625, 0.0625), sq(-0.0625, 0.0625, -0.0625, 0.0625)]
    for b in bounds:
        assert np.array_equal(b.astype(np.float32).astype(np.float64), b)
    return np.array(regions, dtype=np.float64), bounds


def sample_times_defined(T, dt, times=()):
    """The trap of GetTrajectory: it samples while t <= T + 1e-5, and the reference's Spline::GetSegmentID is undefined
    beyond T + 1e-10.  True when no accumulated sample time and none of `times` leaves what is defined."""
    t = 0.0
    while t <= T + 1e-5:
        if t > T + 1e-10:
            return False
        t += dt
    return all(0.0 <= v <= T + 1e-10 for v in times)


def make_traj_x(case, seed, ang_scale):
    """x_perturbed (timings included) with base-ang scaled and shaken, so that the rotation leaves the trace > 0 branch"""
    x = case.x_perturbed(seed, sigma=0.25)
    rng = np.random.default_rng(700 + seed)
    for vs in case.S.var_sets:
        a, b = vs["offset"], vs["offset"] + vs["size"]
        if vs["name"] == "base-ang":
            x[a:b] = x[a:b] * ang_scale + rng.normal(size=b - a) * 1.5
        if vs["name"].startswith("ee-schedule"):   # back to +- 10 % of the given durations
            e = int(vs["name"][len("ee-schedule"):])
            x[a:b] = np.asarray(case.sched.durations()[e][:-1]) * (1.0 + 0.1 * rng.uniform(-1, 1, size=b - a))
    return x


def junction_schedules(case, x):
    """per foot of a case with optimised timings at x: (phase, ee-motion polynomial, ee-force polynomial) durations"""
    from tests import segment_points as sp

    out, p = [], case.params
    for vs in case.S.var_sets:
        if vs["name"].startswith("ee-schedule"):
            e = int(vs["name"][len("ee-schedule"):])
            ph = sp.set_variables(case.sched.durations()[e], x[vs["offset"]:vs["offset"] + vs["size"]])
            contact = bool(case.sched.contact()[e])
            out.append((ph, sp.poly_durations(ph, contact, p.polys_per_swing), sp.poly_durations(ph, not contact, p.polys_per_stance_force)))
    return out


def make_junction_traj(case, seeds, ang_scale, dt, T):
    """(the x of a junction fixture, the guess times on their thresholds)"""
    from tests import segment_points as sp

    t, samples = 0.0, []
    while t <= T + 1e-5:
        samples.append(t)
        t += dt
    xs, extra = [], []
    for seed in seeds:
        x = make_traj_x(case, seed, ang_scale)
        xj = case.x_junctions(seed, times=samples)
        for vs in case.S.var_sets:
            if vs["name"].startswith("ee-schedule"):
                x[vs["offset"]:vs["offset"] + vs["size"]] = xj[vs["offset"]:vs["offset"] + vs["size"]]
        xs.append(x)
        for lists in junction_schedules(case, x):
            for d in lists:
                for acc in sp.sums(d)[:-1]:
                    thr = sp.threshold(acc)
                    extra += [thr, float(np.nextafter(thr, -np.inf)), float(np.nextafter(thr, np.inf))]
    return xs, np.array(sorted(set(extra)))[::-1]


def compute_traj(name, workdir):
    """the arrays of reftraj_<name>.npz, from a run of the reference's code"""
    from oracle import ref_run
    from tests.common import Case

    robot, terrain, sched, params, dt, seeds, ang_scale = TRAJ_CASES[name][:7]
    junctions = len(TRAJ_CASES[name]) > 7
    case = Case(robot, terrain, sched(), **params)
    n_ee, p = N_EE[robot], case.params
    T = float(np.sum(case.sched.durations()[0]))
    rng = np.random.default_rng(len(name))
    times = np.concatenate([[0.0, T, p.duration_base_poly, 2 * p.duration_base_poly, case.sched.durations()[0][0], 0.5 * T],
                            rng.uniform(0.0, T, 66)])
    junction_x = None
    if junctions:
        junction_x, extra = make_junction_traj(case, seeds, ang_scale, dt, T)
        times = np.concatenate([times[:16], extra])
    assert len(times) > 64 and np.any(np.diff(times) < 0)
    for step in (dt, PLAN_DT):
        if not sample_times_defined(T, step, times):
            raise SystemExit("%s: dt = %g or a guess time leaves [0, T + 1e-10] (T = %.17g)" % (name, step, T))
    regions, bounds = traj_regions()
    args, kw = ref_run.case_args(case)
    xs, trajs, guesses, durs, sets, states = [], [], [], [], [], []
    for k, seed in enumerate(seeds):
        x = junction_x[k] if junctions else make_traj_x(case, seed, ang_scale)
        d = ref_run.run(os.path.join(workdir, "%s_%d" % (name, seed)), *args, x=x, sample_dt=dt, guess_times=times,
                        planes=(regions, bounds, PLAN_HORIZON), **kw)
        fine = ref_run.run(os.path.join(workdir, "%s_%d_fine" % (name, seed)), *args, x=x, sample_dt=PLAN_DT, **kw)["traj"]
        assert np.array_equal(d["x"], x)
        flags = fine[:, 20::13][:, :n_ee]
        change = np.concatenate([[True], np.any(flags[1:] != flags[:-1], axis=1)])
        assert change.sum() == len(d["plan_duration"]), "the footstep states are where the flags of the 0.01 s trajectory change"
        xs.append(x), trajs.append(d["traj"]), guesses.append(d["guess"])
        durs.append(d["plan_duration"]), sets.append(d["plan_contact_set"]), states.append(fine[change])
    steps = np.array([len(v) for v in durs], dtype=np.int32)
    pad = lambda rows, fill, dtype: np.array([np.concatenate([v, np.full((steps.max() - len(v),) + v.shape[1:], fill, dtype=dtype)]) for v in rows])
    out = dict(robot=robot, terrain=terrain, n_phases=np.array([len(v) for v in case.sched.durations()], dtype=np.int32),
               phase_durations=np.concatenate(case.sched.durations()), contact_at_start=np.array(case.sched.contact(), dtype=np.int32),
               constraint_sets=np.int32(p.constraint_sets), params=np.array([getattr(p, k) for k in ref_run.PARAM_KEYS], dtype=np.float64),
               var_names=np.array([n for n, _ in d["var_sets"]]), var_rows=np.array([r for _, r in d["var_sets"]], dtype=np.int32),
               x=np.array(xs), dt=np.float64(dt), traj=np.array(trajs), guess_times=times, guess=np.array(guesses),
               regions=regions, region_start=np.concatenate([[0], np.cumsum([len(b) for b in bounds])]).astype(np.int32),
               region_xy=np.concatenate(bounds), plan_dt=np.float64(PLAN_DT), plan_horizon=np.float64(PLAN_HORIZON), plan_steps=steps,
               plan_duration=pad(durs, np.nan, np.float64), plan_contact_set=pad(sets, -2, np.int32), plan_state=pad(states, np.nan, np.float64),
               reference_deps=ref_run.deps())
    return out


def record_traj(name, workdir):
    out = compute_traj(name, workdir)
    path = os.path.join(GOLDEN, "reftraj_%s.npz" % name)
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), out["traj"].shape[1], int(out["plan_steps"].max())


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/refterrain_<analytic|csv>.npz: the reference's terrain classes (ref_dump --terrain-points) at the points of
# tests/terrain_points.py -- every breakpoint, its neighbouring doubles, the slope-band thresholds of the CSV steps in both
# roundings.  Per file: terrain_id (n), xy (n, 2), values (n, 4) [h, hx, hy, hxx], force_index (k) = the points of the
# force subset and basis (k, 27) = their three normalised basis vectors and six derivatives; the CSV file adds its heights.
# tests/test_terrain_probe.py regenerates the points, compares the oracle bit for bit (CPU) and the device (GPU).
TERRAIN_FIXTURES = ("analytic", "csv")


def terrain_fixture_points(name):
    """(terrain_id (n,), xy (n, 2), force_index (k,), csv heights or None) of one refterrain fixture"""
    from tests import terrain_points as tp

    keys = tp.ANALYTIC if name == "analytic" else ("csv",)
    sub = tp.force_subset()
    ids, xy, fi, at = [], [], [], 0
    for key in keys:
        p = tp.points(key)
        ids.append(np.full(len(p), tp.TERRAIN_ID[key], dtype=np.int32))
        xy.append(p)
        fi.append(at + np.asarray(sub[key][0], dtype=np.int64))
        at += len(p)
    return np.concatenate(ids), np.concatenate(xy), np.concatenate(fi), (tp.CSV_HEIGHTS if name == "csv" else None)


def record_terrain(name, workdir):
    from oracle import ref_run

    ids, xy, fi, heights = terrain_fixture_points(name)
    flags = np.zeros(len(ids), dtype=bool)
    flags[fi] = True
    values, basis = ref_run.terrain_points(os.path.join(workdir, "terrain_" + name), ids, xy, flags, csv_heights=heights)
    order = np.argsort(fi, kind="stable")              # ref_dump answers in point order
    b = np.empty_like(basis)
    b[order] = basis
    out = dict(terrain_id=ids, xy=xy, values=values, force_index=fi, basis=b, reference_deps=ref_run.deps())
    if heights is not None:
        out["csv_heights"] = heights
    path = os.path.join(GOLDEN, "refterrain_%s.npz" % name)
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), len(ids), len(fi)


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/refsegment.npz: Spline::GetSegmentID / GetLocalTime (ref_dump --segment-points) at the defined points of
# tests/segment_points.py -- every junction threshold of every list and its neighbouring doubles -- and
# PhaseDurations::SetVariables + ConvertPhaseToPolyDurations on its duration cases.  The file holds the lists (list_start,
# durations) and per point point_list, point_t, seg_id (uint8) and t_local; per duration case its inputs (case_head
# [n_phases, contact, pps, ppf], case_given, case_vars) and the reference's case_ph, case_md, case_fd with their starts.
# tests/test_segment_probe.py regenerates the points, compares the oracle and mp_ref bit for bit (CPU) and the device (GPU).
def compute_segments(workdir):
    from oracle import ref_run
    from tests import segment_points as sp

    p = sp.points()
    sel = np.nonzero(p["defined"])[0]
    lists = [sp.list_of(k) for k in range(len(p["list_start"]) - 1)]
    for k, t in zip(p["point_list"][sel], p["point_t"][sel]):   # (ref_dump refuses them as well, with exit code 5)
        if not (t >= 0.0 and sp.reaches(sp.sums(lists[k])[-1], float(t))):
            raise SystemExit("list %d, t = %.17g lies outside what Spline::GetSegmentID defines" % (k, t))
    ids, tl = ref_run.segment_points(os.path.join(workdir, "segments"), lists, p["point_list"][sel], p["point_t"][sel])
    assert ids.min() >= 0 and ids.max() < 256
    cases = sp.duration_cases()
    res = ref_run.segment_durations(os.path.join(workdir, "durations"), cases)
    starts = lambda arrs: np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int32)
    out = dict(list_start=p["list_start"], durations=p["durations"], point_list=p["point_list"][sel].astype(np.uint8), point_t=p["point_t"][sel],
               seg_id=ids.astype(np.uint8), t_local=tl,
               case_head=np.array([c[:4] for c in cases], dtype=np.int32), case_given=np.concatenate([c[4] for c in cases]),
               case_vars=np.concatenate([c[5] for c in cases]), case_ph=np.concatenate([r[0] for r in res]),
               case_md=np.concatenate([r[1] for r in res]), case_md_start=starts([r[1] for r in res]),
               case_fd=np.concatenate([r[2] for r in res]), case_fd_start=starts([r[2] for r in res]), reference_deps=ref_run.deps())
    assert len(p["list_start"]) - 1 < 256
    return out


def record_segments(workdir):
    out = compute_segments(workdir)
    path = os.path.join(GOLDEN, "refsegment.npz")
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), len(out["point_t"]), len(out["case_head"])


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/refplane.npz: fpowr::PlanarRegionsToPolygons and NearestPlaneLookup::GetNearestPlaneIndex (ref_dump
# --plane-points) on the scenes of tests/plane_points.py.  What it pins: the reference's own loop -- the DBL_MAX start, the
# strict `<`, -1 where nothing is below DBL_MAX, the first of equal distances wins -- and the tf transform of the boundary
# points (quaternion -> matrix -> world), both compiled from the reference's header.  The polygon geometry under them
# (bg::distance: covered_by and the distance to the ring) is the stand-in's of oracle/ref_dump/subset/fpowr_deps/boost, written
# from Boost 1.71's published algorithm: Boost itself is not executed.  The file holds per scene its regions and local rings
# (scene_region_start, regions, ring_start, local_xy), world_xy (the reference's polygons), the query points (scene_point_start,
# points) with index (int8) per point, and distance per (point, region) point-major (scene_pair_start, distance).
# tests/test_plane_probe.py regenerates the scenes and compares the oracle (CPU) and the device (GPU); tests/test_planes_edges.py
# runs them through twr_batch_contact_planes.
def compute_planes(workdir):
    from oracle import ref_run
    from tests import plane_points as pp

    scenes = pp.scenes()
    res = ref_run.plane_points(os.path.join(workdir, "planes"), [(s["regions"], s["rings"], s["points"]) for s in scenes])
    starts = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rings = [r for s in scenes for r in s["rings"]]
    index = np.concatenate([r[1] for r in res])
    assert index.min() >= -1 and index.max() < 127
    return dict(scene_region_start=starts([len(s["rings"]) for s in scenes]),
                regions=np.concatenate([s["regions"].reshape(-1, 7) for s in scenes]), ring_start=starts([len(r) for r in rings]),
                local_xy=np.concatenate([r.reshape(-1, 2) for r in rings]).astype(np.float32),
                world_xy=np.concatenate([w.reshape(-1, 2) for r in res for w in r[0]] + [np.zeros((0, 2))]),
                scene_point_start=starts([len(s["points"]) for s in scenes]), points=np.concatenate([s["points"] for s in scenes]),
                index=index.astype(np.int8), scene_pair_start=starts([r[2].size for r in res]),
                distance=np.concatenate([r[2].ravel() for r in res]), reference_deps=ref_run.deps())


def record_planes(workdir):
    out = compute_planes(workdir)
    path = os.path.join(GOLDEN, "refplane.npz")
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), len(out["points"]), len(out["distance"])


# ---------------------------------------------------------------------------------------------------------------------
# tests/golden/refattitude.npz: the attitude of the base (ref_dump --attitude-points) at the points of tests/attitude_points.py.
# quat_R (n, 9) and quat_q (n, 4, x y z w) = Eigen::Quaterniond(R) of the Eigen the build uses -- reference_deps names it; with
# the subset that is this project's own statement of the conversion, so these rows pin the device to a restatement, not to Eigen.
# euler_state (n, 9) = what the reference's one-polynomial NodeSpline returns at t = 0 for the nodes of attitude_points.spline_nodes
# (the input of the rows that follow, and of the probe), euler_R, euler_q, euler_omega, euler_omega_dot = EulerConverter's
# GetRotationMatrixBaseToWorld, GetQuaternionBaseToWorld, GetAngularVelocityInWorld, GetAngularAccelerationInWorld: the
# reference's own statements.  There is no reference code for the frame change, so the file holds nothing for it.
# tests/test_attitude_probe.py regenerates the points and compares the restatement (CPU) and the device (GPU).
def compute_attitude(workdir):
    from oracle import ref_run
    from tests import attitude_points as ap

    p = ap.points()
    q = ref_run.attitude_quaternions(os.path.join(workdir, "quat"), p["quat"])
    nodes = np.array([ap.spline_nodes(s) for s in p["euler"]])
    state, R, eq, w, wd = ref_run.attitude_states(os.path.join(workdir, "euler"), nodes)
    return dict(quat_R=p["quat"], quat_group=p["quat_group"], quat_q=q, euler_group=p["euler_group"], euler_state=state, euler_R=R,
                euler_q=eq, euler_omega=w, euler_omega_dot=wd, reference_deps=ref_run.deps())


ATTITUDE_LIBM_FREE = ("quat_R", "quat_group", "quat_q", "euler_group", "euler_state")   # keys that no sin / cos of the host feeds


def check_attitude(workdir):
    """python -m oracle.ref_golden --attitude --check: a fresh recording against the committed refattitude.npz, key by key.
    Returns the lines of the report and whether the recipe reproduced the file: byte for byte in ATTITUDE_LIBM_FREE; the other
    keys pass through the host's libm, which need not be the same function everywhere, and may differ by its rounding (an entry
    of R by 36 * 2^-53: twice the 9 roundings counted in tests/test_attitude_probe.py on a sum of terms of at most 2).
    This is run by hand where the reference is present; it is not part of the test suite."""
    out, f = compute_attitude(workdir), np.load(os.path.join(GOLDEN, "refattitude.npz"))
    lines, ok = [], set(out) == set(f.files)
    for key in f.files:
        if key == "reference_deps":
            continue
        a, b = np.asarray(out[key]), f[key]
        if a.dtype != b.dtype or a.shape != b.shape:
            lines.append("%-16s dtype or shape differ: %s %s against %s %s" % (key, a.dtype, a.shape, b.dtype, b.shape))
            ok = False
            continue
        rows = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
        if len(rows) == 0:
            lines.append("%-16s equal" % key)
            continue
        worst = float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))
        lines.append("%-16s %d rows differ, first %s, largest |difference| %.3e" % (key, len(rows), rows[:8].tolist(), worst))
        if key in ATTITUDE_LIBM_FREE or (key == "euler_R" and worst > 36 * 2.0 ** -53):
            ok = False
    return lines, ok


def record_attitude(workdir):
    out = compute_attitude(workdir)
    path = os.path.join(GOLDEN, "refattitude.npz")
    save_npz_lzma(path, out)
    return path, os.path.getsize(path), len(out["quat_q"]), len(out["euler_q"])


def main(names):
    from oracle import ref_run

    if not ref_run.available():
        raise SystemExit("oracle/_ref/ref_dump is not built: run oracle/ref_dump/build.sh where the reference sources are")
    total = 0
    if names and names[0] == "--terrain":
        with tempfile.TemporaryDirectory() as work:
            for name in names[1:] or list(TERRAIN_FIXTURES):
                path, size, n, k = record_terrain(name, work)
                total += size
                print("%-40s points=%6d force=%4d %8d bytes" % (os.path.basename(path), n, k, size))
        print("total %d bytes" % total)
        return
    if names and names[0] == "--segments":
        with tempfile.TemporaryDirectory() as work:
            path, size, n, k = record_segments(work)
        print("%-40s points=%6d duration cases=%3d %8d bytes" % (os.path.basename(path), n, k, size))
        return
    if names and names[0] == "--planes":
        with tempfile.TemporaryDirectory() as work:
            path, size, n, k = record_planes(work)
        print("%-40s points=%6d (ring, point) pairs=%6d %8d bytes" % (os.path.basename(path), n, k, size))
        return
    if names[:2] == ["--attitude", "--check"]:
        with tempfile.TemporaryDirectory() as work:
            lines, ok = check_attitude(work)
        print("\n".join(lines))
        if not ok:
            raise SystemExit("refattitude.npz is NOT reproduced by this build of the reference")
        print("refattitude.npz is reproduced")
        return
    if names and names[0] == "--attitude":
        with tempfile.TemporaryDirectory() as work:
            path, size, n, k = record_attitude(work)
        print("%-40s matrices=%6d states=%6d %8d bytes" % (os.path.basename(path), n, k, size))
        return
    if names and names[0] == "--traj":
        with tempfile.TemporaryDirectory() as work:
            for name in names[1:] or list(TRAJ_CASES):
                path, size, n, steps = record_traj(name, work)
                total += size
                print("%-40s samples=%4d steps=%3d %8d bytes" % (os.path.basename(path), n, steps, size))
        print("total %d bytes" % total)
        return
    with tempfile.TemporaryDirectory() as work:
        for name in names or list(CASES):
            path, size, m, nnz = record(name, work)
            total += size
            print("%-34s m=%6d nnz=%7d %8d bytes" % (os.path.basename(path), m, nnz, size))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main(sys.argv[1:])
