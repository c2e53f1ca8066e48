"""the recipe that compiles the REAL reference sources (oracle/ref_dump/) and dumps what
they compute -- g, the Jacobian triplets, bounds, the initial guess, set names and gait tables.  Eigen3 and ifopt are
used where they are installed; elsewhere the reference's sources run on the subset under oracle/ref_dump/subset (its own
tests: test_eigen_subset.py).  Where the reference sources are present the CPU tests below build the recipe and compare
the oracle and the structure builder with the running reference; where they are absent they skip, and
tests/test_ref_golden.py carries the recorded results instead."""
import concurrent.futures
import glob
import os
import subprocess

import numpy as np
import pytest

from oracle import ref_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref")
REFERENCE_SRC = os.path.join(os.environ.get("TOWR_REFERENCE_DIR", "/root/reference/towr"), "src")
WORKERS = min(16, os.cpu_count() or 1)
# seeds of the random walk; TOWR_REF_WALK_SEEDS can only widen it
WALK_SEEDS = max(300, int(os.environ.get("TOWR_REF_WALK_SEEDS", "300")))
_built = {}


def _tail(name, n=25):
    path = os.path.join(REF, name)
    return "---- %s\n%s" % (name, "".join(open(path, errors="replace").readlines()[-n:]) if os.path.exists(path) else "(missing)\n")


def reference_built():
    """Builds the recipe once per session.  The one reason to skip is that the reference sources are absent.  Where they
    are present the recipe has no dependency left whose absence would excuse it (the subset stands in for Eigen3 / ifopt),
    so anything but "available" -- the subset, the driver or the recipe no longer compile -- fails the test."""
    if not os.path.isdir(REFERENCE_SRC):
        pytest.skip("the reference sources are not on this box")
    if "status" not in _built:
        r = subprocess.run(["bash", os.path.join(ROOT, "oracle", "ref_dump", "build.sh")], capture_output=True, text=True, timeout=1200)
        _built["status"] = open(os.path.join(REF, "STATUS")).read().strip()
        _built["log"] = r.stdout + r.stderr
    assert _built["status"] == "available", "%s\n%s\n%s%s" % (_built["status"], _built["log"], _tail("configure.log"), _tail("build.log"))


def close(a, b):
    """the project's bar on plain numbers (bounds, the initial guess): 1e-9 relative + 1e-12 (tests/common.py at scale 1)"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-9 * np.abs(b) + 1e-12))


def compare_case(case, d, x, what, worst, guess_args=None):
    """One reference dump `d` at `x` against the oracle (case.P) and the structure builder (case.S): set tables, pattern,
    bounds, g and Jacobian through assert_parity with the reference as `ref`; with guess_args also the initial guess and
    the variable bounds.  `worst` collects the largest errors seen, relative to the scale assert_parity uses."""
    from tests.common import assert_parity, row_scale, set_scale

    S, P = case.S, case.P
    assert [(s["name"], s["size"]) for s in S.con_sets] == d["con_sets"] == list(P.con_sets), what
    assert [(s["name"], s["size"]) for s in S.var_sets] == d["var_sets"] == list(P.var_sets), what
    og, rp, ci, ov = P.eval(x)
    rows = np.repeat(np.arange(P.m, dtype=np.int32), np.diff(rp))
    assert np.array_equal(d["jac_row"], rows) and np.array_equal(d["jac_col"], ci), what + ": oracle pattern"
    assert np.array_equal(S.row_ptr, rp) and np.array_equal(S.col_idx, d["jac_col"]), what + ": structure pattern"
    for lo, up in (S.bounds(), P.bounds()):
        assert close(lo, d["g_lower"]) and close(up, d["g_upper"]), what + ": constraint bounds"
    assert_parity(S, og, ov, d["g"], d["jac_val"], what, x=x)
    gs, js = np.maximum(set_scale(S.con_sets, d["g"]), 1e-300), np.maximum(row_scale(S.row_ptr, d["jac_val"]), 1e-300)
    worst["g"] = max(worst.get("g", 0.0), float((np.abs(og - d["g"]) / gs).max()))
    worst["jac"] = max(worst.get("jac", 0.0), float((np.abs(ov - d["jac_val"]) / js).max()) if len(ov) else 0.0)
    if guess_args is not None:
        lin0, lin1, ee0 = guess_args
        for who in (S, P):
            assert close(who.initial_guess(lin0, [0, 0, 0], lin1, [0, 0, 0], ee0), d["x"]), what + ": initial guess"
            init, final = np.zeros(12), np.zeros(12)
            init[:3], final[:3] = lin0, lin1
            lo, up = who.variable_bounds(init, final, ee0)
            assert close(lo, d["x_lower"]) and close(up, d["x_upper"]), what + ": variable bounds"


guess_args_of = ref_run.formulation_states


def test_reference_build_recipe_reports_its_availability(tmp_path):
    reference_built()
    import towr_amd as ta
    from oracle import binding as ob
    from tests.common import Case

    worst = {}
    for robot, terrain, combo, T, mask, n_ee in (("monoped", "flat", 2, 2.0, 63, 1), ("anymal", "gap", 1, 2.0, 27, 4), ("biped", "stairs", 1, 2.0, 255, 2),
                                                 ("go1", "block", 0, 2.4, 191, 4)):
        case = Case(robot, terrain, ta.gait_combo(n_ee, combo, T), constraint_sets=mask,
                    **(dict(base_z_init=0.55) if mask & 128 else {}))
        prefix = str(tmp_path / ("r%s" % robot))
        d = ref_run.run(prefix, robot, terrain, mask, combo=combo, T=T, params=dict(base_z_init=0.55) if mask & 128 else None)
        assert len(d["durations"]) == n_ee and all(close(a, b) for a, b in zip(d["durations"], case.sched.durations()))
        compare_case(case, d, d["x"], "%s/%s" % (robot, terrain), worst, guess_args=guess_args_of(case))

    # every golden fixture (tests/golden/mp_*.npz: the cases the oracle is pinned on, BASELINE sizes included): the
    # fixture's schedule, discretisation and x go to the real reference as files; its g / Jacobian / bounds must equal
    # the oracle's
    from tests.test_oracle_golden import load_fixture

    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "mp_*.npz"))):
        d, P = load_fixture(path)
        sets = int(d["constraint_sets"]) if "constraint_sets" in d.files else 27
        prefix = str(tmp_path / os.path.basename(path)[:-4])
        pd, o = [], 0
        for k in d["n_phases"]:
            pd.append(d["phase_durations"][o:o + k])
            o += k
        params = dict(base_z_init=0.6)   # (what load_fixture gives the oracle; it centres baseMotion's z bound)
        if "dt_dynamic" in d.files:
            params.update(dt_dynamic=float(d["dt_dynamic"]), dt_rom=float(d["dt_rom"]))
        extra = []
        if str(d["terrain"]) == "grid_map":   # the fpowr fixture: the real `Grid` over the fixture's elevation layer (needs ROS packages)
            el = d["grid_elevation"]
            with open(prefix + "_grid.txt", "w") as f:
                f.write("%d %d\n" % el.shape)
                f.write("\n".join("%.9g" % v for v in el.reshape(-1, order="F")) + "\n")
            extra = ["--grid-map", prefix + "_grid.txt", "%.17g" % float(d["grid_resolution"]), "%.17g" % d["grid_position"][0],
                     "%.17g" % d["grid_position"][1]]
        cmd = ref_run.command(prefix, str(d["robot"]), str(d["terrain"]), sets, x=d["x"], durations=pd, contact=list(d["contact_at_start"]),
                              params=params, extra=extra)
        rc = subprocess.call(cmd, stdout=subprocess.DEVNULL)
        if rc == 4 and str(d["terrain"]) == "grid_map":
            print("skipped %s: grid_map_ros / convex_plane_decomposition_msgs are not on this box" % os.path.basename(path))
            continue
        assert rc == 0, cmd
        r = ref_run.read(prefix)
        g, trip_r, trip_c, trip_v = r["g"], r["jac_row"], r["jac_col"], r["jac_val"]
        # (the structure builder on the same problem: the per-row / per-set bar of assert_parity, pattern, bounds, set tables)
        dts = dict(dt_dynamic=params["dt_dynamic"], dt_rom=params["dt_rom"]) if "dt_dynamic" in params else {}
        case = Case(str(d["robot"]), str(d["terrain"]), ta.schedule(pd, list(d["contact_at_start"])), constraint_sets=sets, base_z_init=0.6, **dts)
        compare_case(case, r, d["x"], os.path.basename(path), worst)
        og, rp, ci, ov = P.eval(d["x"])
        rows = np.repeat(np.arange(P.m), np.diff(rp))
        assert g.shape == og.shape and np.abs(g - og).max() <= 1e-9 * max(1.0, np.abs(og).max()), path
        assert np.array_equal(trip_r, rows) and np.array_equal(trip_c, ci), path
        assert np.abs(trip_v - ov).max() <= 1e-9 * max(1.0, np.abs(ov).max()), path
        lo, up = P.bounds()
        assert close(lo, r["g_lower"]) and close(up, r["g_upper"]), path
        assert r["con_sets"] == list(P.con_sets) and r["var_sets"] == list(P.var_sets), path
    print("oracle vs reference, worst error / scale: g %.3e, Jacobian %.3e" % (worst["g"], worst["jac"]))


def test_gait_tables_against_the_reference(tmp_path):
    """twr_gait_combo and the oracle's table vs what the reference's GaitGenerator produced, for every n_ee x combo."""
    reference_built()
    import towr_amd as ta
    from oracle import binding as ob

    for n_ee, robot in ((1, "monoped"), (2, "biped"), (4, "anymal")):
        for combo in range(5):   # GaitGenerator::Combos C0..C4
            for T in (2.0, 3.1):
                d = ref_run.run(str(tmp_path / ("g%d_%d" % (n_ee, combo))), robot, "flat", 1, combo=combo, T=T)
                s = ta.gait_combo(n_ee, combo, T)
                od, oc = ob.gait(n_ee, combo, T)
                assert d["contact"] == s.contact() == list(oc), (n_ee, combo)
                for a, b, c in zip(d["durations"], s.durations(), od):
                    assert close(b, a) and close(c, a), (n_ee, combo, a, b)


def test_random_walk_against_the_reference(tmp_path):
    """random_case(seed) for a few hundred seeds, each at the reference's own initial guess, at x_perturbed and at x_wild:
    the reference vs the oracle through assert_parity, the reference's pattern vs Structure.row_ptr / col_idx, bounds,
    variable bounds, initial guess and set tables.  (`grid_map` terrain needs ROS packages and is left out.)
    Every sixth problem also runs fpowr's GetTrajectory in the reference (ref_dump --sample) at its perturbed x, against the
    oracle's sample_trajectory at the bar of tests/test_ref_traj.py."""
    reference_built()
    from oracle.ref_golden import sample_times_defined
    from tests.common import random_case
    from tests.test_ref_traj import check_records, traj_exact_columns

    worst, done, sampled = {}, 0, 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=WORKERS) as pool:
        for first in range(0, WALK_SEEDS, 64):   # (in chunks: the structures of a chunk are alive while its dumps run)
            jobs = []
            for seed in range(first, min(first + 64, WALK_SEEDS)):
                case = random_case(seed)
                if case.terrain == "grid_map":
                    continue
                args, kw = ref_run.case_args(case)
                for tag, x in (("guess", "guess"), ("perturbed", case.x_perturbed(seed)), ("wild", case.x_wild(seed))):
                    prefix = str(tmp_path / ("s%d_%s" % (seed, tag)))
                    more = {}
                    if tag == "perturbed" and seed % 6 == 0:   # between 40 and 90 samples, none where the reference is undefined
                        T = float(np.sum(case.sched.durations()[0]))
                        dts = [T / n for n in range(40 + seed % 50, 140) if sample_times_defined(T, T / n)]
                        more = dict(sample_dt=dts[0])
                    jobs.append((case, seed, tag, x, pool.submit(ref_run.run, prefix, *args, x=x, **more, **kw)))
            for case, seed, tag, x, fut in jobs:
                d = fut.result()
                what = "seed %d (%s/%s, sets %d) at %s" % (seed, case.robot, case.terrain, case.params.constraint_sets, tag)
                if tag == "guess":
                    compare_case(case, d, d["x"], what, worst, guess_args=guess_args_of(case))
                else:
                    assert np.array_equal(d["x"], x), what
                    compare_case(case, d, x, what, worst)
                    if "traj" in d:
                        dt = d["traj"][1, 0]
                        check_records(case.P.sample_trajectory(x, dt), d["traj"], traj_exact_columns(case.model.n_ee), what + " trajectory", worst, "traj")
                        sampled += 1
                done += 1
                for f in glob.glob(str(tmp_path / ("s%d_%s_*" % (seed, tag)))):
                    os.remove(f)
    assert done >= 2 * WALK_SEEDS and sampled >= WALK_SEEDS // 8
    print("random walk: %d dumps, oracle vs reference worst error / scale: g %.3e, Jacobian %.3e; %d trajectories, worst %.3e" % (
        done, worst["g"], worst["jac"], sampled, worst["traj"]))


BINDING_CASES = (("monoped", "flat", 2, 2.0, 63), ("biped", "slope", 1, 1.6, 255), ("hyq", "chimney", 3, 2.0, 63), ("anymal", "gap", 1, 2.0, 27),
                 ("anymal", "stairs", 0, 2.4, 127), ("go1", "block", 2, 1.8, 63), ("anymal", "csv", 1, 2.0, 63))


@pytest.mark.gpu
def test_towr_binding_against_the_real_reference(tmp_path):
    """towr_amd/csrc/towr_binding.h compiled against the REAL towr headers (ref_dump --binding): the device sets it
    returns for an NlpFormulation equal the reference's own sets -- names, rows, bounds, values, Jacobian -- on the
    reference's guess, on a perturbed and on a wild x, for one case per robot and a CSV terrain.  The executable is built
    where the reference sources are (oracle/ref_dump/build.sh) and travels with the tree; skips where it is missing.
    Every run is a child process under its own timeout, and nothing further starts after the first failure."""
    if not ref_run.available():
        pytest.skip("oracle/_ref/ref_dump is not built on this box (needs the reference sources)")
    import towr_amd as ta
    from tests.common import Case

    rng = np.random.default_rng(5)
    for robot, terrain, combo, T, mask in BINDING_CASES:
        n_ee = ta.model_preset(robot, terrain).n_ee
        grid = np.round(rng.uniform(0.0, 0.25, size=(14, 20)), 2) if terrain == "csv" else None
        case = Case(robot, terrain, ta.gait_combo(n_ee, combo, T), grid=grid, constraint_sets=mask, **(dict(base_z_init=0.5) if mask & 128 else {}))
        for tag, x in (("guess", "guess"), ("perturbed", case.x_perturbed(3)), ("wild", case.x_wild(3))):
            prefix = str(tmp_path / ("b_%s_%s_%s" % (robot, terrain, tag)))
            cmd = ref_run.command(prefix, robot, terrain, mask, x=x, combo=combo, T=T, params=dict(base_z_init=0.5) if mask & 128 else None,
                                  csv_heights=grid, extra=["--binding"])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            line = [ln for ln in r.stdout.split("\n") if ln.startswith("binding:")]
            print(robot, terrain, tag, line)
            assert r.returncode == 0 and "structure equal" in r.stdout, " ".join(cmd) + "\n" + r.stdout[-1500:] + r.stderr[-1500:]
