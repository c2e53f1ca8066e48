"""tests/golden/reftraj_*.npz are recorded outputs of the reference's OWN sweep post-processing (oracle/ref_golden.py
--traj, run where the reference sources are): fpowr's GetTrajectory, ExtractInitialGuesses and ExtractFootstepPlan with
its NearestPlaneLookup, executed from the reference's headers on stand-ins for ROS / xpp / tf / boost::geometry
(oracle/ref_dump/subset/fpowr_deps, tests/test_ros_subset.py).  Per case: the problem, x[k], traj[k] at the fixture's dt,
guess[k] at guess_times, planar regions, and the footstep plan at the reference's fixed 0.01 s and 2 s horizon
(plan_steps, plan_duration, plan_contact_set, and plan_state = the footstep states themselves).

CPU tier: the oracle's sample_trajectory / initial_guess_samples / contact_plan + nearest_plane against every fixture;
what the fixture set has to cover, asserted on the recorded arrays alone; the fixtures reproduced where the reference is
present; negative controls on the comparison.
GPU tier: twr_batch_sample, twr_batch_initial_guess, twr_batch_contact_plan and twr_batch_contact_planes against the
fixtures; the expected values come from tests/golden/ only, never from the oracle.

The bar is the project's (tests/common.py): sample times, contact flags, step counts and plane indices are equal;
every other field obeys |got - ref| <= 1e-9 |ref| + 1e-12 scale, with scale = the largest |ref| of that column."""
import fnmatch
import glob
import os

import numpy as np
import pytest

import towr_amd as ta
from oracle import ref_run

from .common import FLOOR, RTOL, Case
from .test_ros_subset import ring_distance, ring_side

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "reftraj_*.npz")))
IDS = [os.path.basename(p)[8:-4] for p in FIXTURES]


def traj_exact_columns(n_ee):
    return [0] + [20 + 13 * e for e in range(n_ee)]       # the sample time and the contact flag of every foot


def check_records(got, ref, exact, what, worst=None, kind=None):
    """One array of records against the reference's: the columns `exact` bit-equal, the others at the bar.  `worst`
    collects the largest error / column scale per record kind."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, "%s: %s records for %s" % (what, got.shape, ref.shape)
    same = got[:, exact] == ref[:, exact]
    assert same.all(), "%s: sample times / contact flags differ at record %d" % (what, int(np.nonzero(~same.all(axis=1))[0][0]))
    scale = np.abs(ref).max(axis=0, keepdims=True)
    err = np.abs(got - ref)
    bad = ~(err <= RTOL * np.abs(ref) + FLOOR * scale)
    rel = err / np.maximum(scale, 1e-300)
    if worst is not None:
        worst[kind] = max(worst.get(kind, 0.0), float(np.nan_to_num(rel, nan=np.inf).max()))
    assert not bad.any(), "%s: %d values off, worst |err| / scale %.3e in column %d" % (
        what, int(bad.sum()), float(np.nan_to_num(rel, nan=np.inf)[bad].max()), int(np.nonzero(bad.any(axis=0))[0][0]))


def check_plan(fx, k, steps, duration, contact_set, what, worst=None):
    """A footstep plan against the reference's message: step count and plane indices equal, durations at the bar."""
    n = int(fx.plan_steps[k])
    assert int(steps) == n, "%s: %d footstep states for %d" % (what, int(steps), n)
    ref_set, ref_dur = fx.plan_contact_set[k, :n], fx.plan_duration[k, :n]
    contact_set, duration = np.asarray(contact_set)[:n], np.asarray(duration)[:n]
    assert np.array_equal(contact_set, ref_set), "%s: plane indices differ at (step, foot) %s" % (what, np.argwhere(contact_set != ref_set)[0])
    flags = fx.plan_state[k, :n][:, traj_exact_columns(fx.n_ee)[1:]]
    assert np.array_equal(contact_set == -1, flags == 0), what + ": contact_set is -1 exactly where the foot is in the air"
    scale = np.abs(ref_dur).max()
    err = np.abs(duration - ref_dur)
    if worst is not None:
        worst["plan duration"] = max(worst.get("plan duration", 0.0), float(np.nan_to_num(err / scale, nan=np.inf).max()))
    assert np.all(err <= RTOL * np.abs(ref_dur) + FLOOR * scale), "%s: durations off by %.3e" % (what, float(np.nan_to_num(err, nan=np.inf).max()))


class TrajFixture:
    def __init__(self, path):
        d = np.load(path)
        self.name = os.path.basename(path)[8:-4]
        self.d = {k: d[k] for k in d.files}
        for k in ("x", "traj", "guess", "guess_times", "regions", "region_start", "region_xy", "plan_steps", "plan_duration", "plan_contact_set",
                  "plan_state"):
            setattr(self, k, self.d[k])
        self.dt, self.plan_dt, self.plan_horizon = float(d["dt"]), float(d["plan_dt"]), float(d["plan_horizon"])
        self.durations, o = [], 0
        for n in d["n_phases"]:
            self.durations.append(d["phase_durations"][o:o + n])
            o += n
        self.n_ee = len(self.durations)
        self.T = float(np.sum(self.durations[0]))
        self.params = dict(zip(ref_run.PARAM_KEYS, d["params"]))
        for k in ("polys_per_swing", "polys_per_stance_force"):
            self.params[k] = int(self.params[k])
        if self.params["base_z_init"] != self.params["base_z_init"]:
            del self.params["base_z_init"]
        self.mask = int(d["constraint_sets"])
        self._args = (str(d["robot"]), str(d["terrain"]), ta.schedule(self.durations, list(d["contact_at_start"])))
        self._S = self._case = None

    @property
    def S(self):
        """the structure alone (what the GPU tier needs: the oracle stays out of that path)"""
        if self._S is None:
            self._S = ta.Structure(ta.model_preset(*self._args[:2]), self._args[2], ta.params_default(constraint_sets=self.mask, **self.params))
        return self._S

    @property
    def case(self):
        if self._case is None:
            self._case = Case(*self._args, constraint_sets=self.mask, **self.params)
        return self._case

    def boundaries(self):
        return [self.region_xy[self.region_start[i]:self.region_start[i + 1]] for i in range(len(self.regions))]

    def world_polygons(self):
        """the regions as world x, y rings, in numpy (rotation of the normalised quaternion, then the shift)"""
        out = []
        for r, b in zip(self.regions, self.boundaries()):
            x, y, z, w = r[3:] / np.linalg.norm(r[3:])
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z)]])
            out.append(b @ R.T + r[:2])
        return out


def accumulated_times_defined(T, dt):
    """GetTrajectory samples while t <= T + 1e-5; the reference's segment lookup is defined up to T + 1e-10 only"""
    t, n = 0.0, 0
    while t <= T + 1e-5:
        if t > T + 1e-10:
            return False, n
        t += dt
        n += 1
    return True, n


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_the_fixture_set_covers_what_it_is_there_for():
    """Asserted on the recorded reference data alone (no oracle, no device)."""
    assert 5 <= len(FIXTURES) <= 7
    sizes = [os.path.getsize(p) for p in FIXTURES]
    assert max(sizes) <= 1 << 20 and sum(sizes) <= 1500000, sizes
    for p in FIXTURES:   # the globs (and the budget test) of the other fixture families must not pick these up
        assert not fnmatch.fnmatch(os.path.basename(p), "ref_*.npz") and not fnmatch.fnmatch(os.path.basename(p), "mp_*.npz")
    assert not set(FIXTURES) & set(glob.glob(os.path.join(HERE, "golden", "ref_*.npz")) + glob.glob(os.path.join(HERE, "golden", "mp_*.npz")))
    fxs = [TrajFixture(p) for p in FIXTURES]
    assert {fx.n_ee for fx in fxs} == {1, 2, 4}
    assert {"gap", "stairs"} <= {str(fx.d["terrain"]) for fx in fxs}
    assert any(fx.params["polys_per_swing"] == 3 and fx.params["duration_base_poly"] not in (0.1, 0.0) for fx in fxs)
    timings_perturbed = swing_start = at_junction = between = tie_away = tie_inside = False
    branches = np.zeros(4, dtype=int)
    overlapping = unclosed = counter_clockwise = tilted = few_points = False
    for fx in fxs:
        ex = traj_exact_columns(fx.n_ee)
        assert fx.traj.shape[1] > 64 and len(fx.guess_times) > 64           # more than one work item of 64 samples
        # the trap: no sample of GetTrajectory (at dt, and at the plan's 0.01 s) and no guess time where the reference is undefined
        for dt in (fx.dt, fx.plan_dt):
            ok, n = accumulated_times_defined(fx.T, dt)
            assert ok, (fx.name, dt)
            if dt == fx.dt:
                assert n == fx.traj.shape[1], (fx.name, n, fx.traj.shape)
        t = np.zeros(fx.traj.shape[1])
        for i in range(1, len(t)):
            t[i] = t[i - 1] + fx.dt
        assert all(np.array_equal(tr[:, 0], t) for tr in fx.traj), fx.name + ": the sample times are the accumulated t += dt"
        assert np.all((fx.guess_times >= 0) & (fx.guess_times <= fx.T + 1e-10))
        assert all(np.array_equal(g[:, 0], fx.guess_times) for g in fx.guess)
        # guess times: 0, T, a junction of the base polynomials, unsorted
        poly = fx.params["duration_base_poly"]
        assert 0.0 in fx.guess_times and fx.T in fx.guess_times and poly in fx.guess_times and np.any(np.diff(fx.guess_times) < 0), fx.name
        # optimised timings with the duration variables away from the given schedule
        if fx.mask & 64:
            o = 0
            for name, rows in zip(fx.d["var_names"], fx.d["var_rows"]):
                if str(name).startswith("ee-schedule"):
                    e = int(str(name)[len("ee-schedule"):])
                    given = fx.durations[e][:-1]
                    assert rows == len(given)
                    for x in fx.x:
                        timings_perturbed |= bool(np.abs(x[o:o + rows] - given).max() > 0.005)
                o += int(rows)
            assert o == fx.x.shape[1]
            assert all(c == 1 for c in fx.d["contact_at_start"]), fx.name + ": optimised timings on feet that start in stance"
        for e, c in enumerate(fx.d["contact_at_start"]):
            if c == 0:
                assert all(tr[0, ex[1 + e]] == 0.0 for tr in fx.traj)
                swing_start = True
            else:
                assert all(tr[0, ex[1 + e]] == 1.0 for tr in fx.traj)
        # samples at and between the phase junctions (fixed timings: the junctions are those of the given schedule)
        if not fx.mask & 64:
            junctions = np.unique(np.concatenate([np.cumsum(d)[:-1] for d in fx.durations if len(d) > 1]))
            gap = np.abs(t[:, None] - junctions[None, :]).min(axis=1)
            at_junction |= bool((gap <= 1e-10).any())
            between |= bool((gap > 1e-10).any())
        # the four branches of Quaterniond(R): trace = 4 w^2 - 1 > 0, else the largest diagonal entry = the largest of |x|, |y|, |z|
        q = fx.traj[:, :, 10:14].reshape(-1, 4)
        assert np.allclose((q ** 2).sum(axis=1), 1.0, rtol=0, atol=1e-12)
        pos = 4 * q[:, 0] ** 2 - 1 > 0
        branches[0] += pos.sum()
        for i in range(3):
            branches[1 + i] += ((~pos) & (np.argmax(np.abs(q[:, 1:]), axis=1) == i)).sum()
        # the regions
        polys = fx.world_polygons()
        for i, (r, b) in enumerate(zip(fx.regions, fx.boundaries())):
            unclosed |= len(b) >= 4 and not np.array_equal(b[0], b[-1])
            area = 0.5 * float((b[:-1, 0] * b[1:, 1] - b[1:, 0] * b[:-1, 1]).sum() + (b[-1, 0] * b[0, 1] - b[0, 0] * b[-1, 1]))
            counter_clockwise |= len(b) >= 4 and area > 0 and r[3] == 0 and r[4] == 0
            tilted |= bool(r[3] != 0 or r[4] != 0)
            few_points |= len(b) < 4
            overlapping |= any(ring_side(polys[j], v) > 0 for j in range(len(polys)) if j != i for v in polys[i])
            assert np.array_equal(b.astype(np.float32).astype(np.float64), b)      # exact in the message's float32
        # the plan: -1 exactly in the air; ties between regions decided for the first
        for k in range(len(fx.x)):
            n = int(fx.plan_steps[k])
            st = fx.plan_state[k, :n]
            assert n >= 2 and np.isnan(fx.plan_duration[k, n:]).all() and (fx.plan_contact_set[k, n:] == -2).all()
            assert np.array_equal(fx.plan_contact_set[k, :n] == -1, st[:, ex[1:]] == 0)
            assert st[0, 0] == 0.0 and np.all(np.diff(st[:, 0]) > 0)
            assert np.array_equal(fx.plan_duration[k, :n - 1], np.diff(st[:, 0])) and fx.plan_duration[k, n - 1] == fx.plan_horizon - st[n - 1, 0]
            for s in range(n):
                for e in range(fx.n_ee):
                    if st[s, ex[1 + e]] != 0:
                        dist = np.array([ring_distance(pl, st[s, ex[1 + e] + 1:ex[1 + e] + 3]) for pl in polys])
                        nearest = np.nonzero(dist == dist.min())[0]
                        if len(nearest) > 1 and fx.plan_contact_set[k, s, e] == nearest[0]:
                            tie_away |= bool(dist.min() > 1e-6)
                            tie_inside |= bool(dist.min() == 0.0)
    assert timings_perturbed and swing_start and at_junction and between
    assert np.all(branches > 0), branches
    assert overlapping and unclosed and counter_clockwise and tilted and few_points
    assert tie_away and tie_inside, "two regions equidistant from a contact, outside both and inside both"


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_oracle_matches_the_reference_extractors(path):
    from oracle import binding as ob

    fx = TrajFixture(path)
    P = fx.case.P
    worst = {}
    world = ob.planes_world_xy(fx.regions, fx.region_xy, fx.region_start)
    for poly, mine in zip(fx.world_polygons(), [world[fx.region_start[i]:fx.region_start[i + 1]] for i in range(len(fx.regions))]):
        assert np.allclose(mine, poly, rtol=0, atol=1e-14)
    ex = traj_exact_columns(fx.n_ee)
    for k in range(len(fx.x)):
        what = "%s x[%d]" % (fx.name, k)
        check_records(P.sample_trajectory(fx.x[k], fx.dt), fx.traj[k], ex, what + " trajectory", worst, "trajectory")
        check_records(P.initial_guess_samples(fx.x[k], fx.guess_times), fx.guess[k], [0], what + " guess", worst, "guess")
        plan = P.contact_plan(fx.x[k], fx.plan_dt, fx.plan_horizon)
        n, ne = len(plan), fx.n_ee
        sets = np.full((n, ne), -1, dtype=np.int32)
        for s in range(n):
            for e in range(ne):
                if plan[s, 2 + e] != 0:
                    sets[s, e] = ob.nearest_plane(world, fx.region_start, plan[s, 2 + ne + 3 * e], plan[s, 2 + ne + 3 * e + 1])
        check_plan(fx, k, n, plan[:, 1], sets, what + " plan", worst)
        # ... and the footstep states themselves: time and flags equal, foot positions at the bar
        st = fx.plan_state[k, :n]
        feet = np.concatenate([st[:, c + 1:c + 4] for c in ex[1:]], axis=1)
        check_records(np.concatenate([plan[:, :1], plan[:, 2:]], axis=1), np.concatenate([st[:, ex], feet], axis=1), list(range(1 + ne)),
                      what + " footstep states", worst, "footstep state")
    print("%s: oracle vs reference, worst error / scale: %s" % (fx.name, ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


def test_negative_controls_on_the_comparison():
    """The comparison must see what it is there to see.  On a copy of one fixture: (a) a field scaled by 1 + 1e-8,
    (b) a flipped contact flag, (c) a plane index moved by one -- each must be reported, and nothing is reported on the
    untouched copy."""
    from oracle import binding as ob

    fx = TrajFixture(os.path.join(HERE, "golden", "reftraj_anymal_stairs.npz"))
    P, ex = fx.case.P, traj_exact_columns(fx.n_ee)
    got = P.sample_trajectory(fx.x[0], fx.dt)
    guess = P.initial_guess_samples(fx.x[0], fx.guess_times)
    plan = P.contact_plan(fx.x[0], fx.plan_dt, fx.plan_horizon)
    world = ob.planes_world_xy(fx.regions, fx.region_xy, fx.region_start)
    sets = np.array([[ob.nearest_plane(world, fx.region_start, plan[s, 6 + 3 * e], plan[s, 7 + 3 * e]) if plan[s, 2 + e] else -1 for e in range(4)]
                     for s in range(len(plan))], dtype=np.int32)
    check_records(got, fx.traj[0], ex, "untouched")
    check_records(guess, fx.guess[0], [0], "untouched")
    check_plan(fx, 0, len(plan), plan[:, 1], sets, "untouched")

    def reported(fn, needle):
        try:
            fn()
        except AssertionError as e:
            return needle in str(e)
        return False

    # (a) one field of one record, the largest of its column, in the trajectory and in the guess
    for ref, mine, exact in ((fx.traj[0], got, ex), (fx.guess[0], guess, [0])):
        free = [c for c in range(ref.shape[1]) if c not in exact and np.abs(ref[:, c]).max() > 0]
        assert len(free) >= 30
        for c in (free[0], free[len(free) // 2], free[-1]):
            bad = ref.copy()
            r = int(np.abs(bad[:, c]).argmax())
            bad[r, c] *= 1 + 1e-8
            assert reported(lambda: check_records(mine, bad, exact, "tampered"), "values off"), "(a) a relative error of 1e-8 in column %d went unnoticed" % c
    # (b) a flipped contact flag
    bad = fx.traj[0].copy()
    bad[17, ex[2]] = 1.0 - bad[17, ex[2]]
    assert reported(lambda: check_records(got, bad, ex, "tampered"), "contact flags differ"), "(b) a flipped contact flag went unnoticed"
    # (c) a plane index moved by one (of a foot in contact), and a duration off by 1e-8
    s, e = np.argwhere(fx.plan_contact_set[0, :len(plan)] >= 0)[3]
    truth = fx.plan_contact_set.copy()
    try:
        fx.plan_contact_set[0, s, e] += 1
        assert reported(lambda: check_plan(fx, 0, len(plan), plan[:, 1], sets, "tampered"), "plane indices differ"), "(c) a moved plane index went unnoticed"
    finally:
        fx.plan_contact_set[:] = truth
    truth = fx.plan_duration.copy()
    try:
        fx.plan_duration[0, 2] *= 1 + 1e-8
        assert reported(lambda: check_plan(fx, 0, len(plan), plan[:, 1], sets, "tampered"), "durations off")
    finally:
        fx.plan_duration[:] = truth
    assert reported(lambda: check_plan(fx, 0, len(plan) - 1, plan[:-1, 1], sets[:-1], "tampered"), "footstep states for")


def test_the_fixtures_are_reproduced_by_the_reference(tmp_path):
    """Where the reference sources are present: build the recipe, run the reference's extractors again and require every
    recorded array back, bit for bit (same skip rule as tests/test_ref_dump.py)."""
    from oracle import ref_golden
    from tests.test_ref_dump import reference_built

    reference_built()
    assert "fpowr extractors on stand-ins" in ref_run.deps()
    assert sorted(IDS) == sorted(ref_golden.TRAJ_CASES)
    for path, name in zip(FIXTURES, IDS):
        again, d = ref_golden.compute_traj(name, str(tmp_path)), np.load(path)
        assert set(again) == set(d.files)
        for k in d.files:
            if k == "reference_deps":
                continue   # (which Eigen / ifopt the recording box had)
            a, b = np.asarray(again[k]), d[k]
            assert a.shape == b.shape and a.dtype.kind == b.dtype.kind, (name, k)
            assert np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b), "%s: %s is not reproduced" % (name, k)


# ---------------------------------------------------------------------------------------------------------------- GPU tier
def _group(n_ee):
    fxs = [fx for fx in (TrajFixture(p) for p in FIXTURES) if fx.n_ee == n_ee]
    probs = [(i, fx, k) for i, fx in enumerate(fxs) for k in range(len(fx.x))]
    return fxs, probs


PAD = 5   # doubles between the records of two problems: must stay untouched


def _run_extractors(fxs, probs, tiles=1):
    """All problems of `probs`, `tiles` times over, in one ragged batch with NaN-prefilled outputs: twr_batch_sample once
    per dt of a fixture, twr_batch_initial_guess once per fixture (its times), twr_batch_contact_plan at the reference's
    0.01 s / 2 s, then twr_batch_contact_planes once per fixture (its regions).  Returns host arrays."""
    import torch

    n_ee = fxs[0].n_ee
    order = [i for i, _, _ in probs] * tiles
    batch = ta.Batch([fx.S for fx in fxs], order, device=0)
    x = torch.from_numpy(np.tile(np.concatenate([fx.x[k] for _, fx, k in probs]), tiles)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rec = 20 + 13 * n_ee
    out = dict(n=len(order))
    for fx in fxs:
        for other in fxs:   # every problem of the batch is sampled at every dt: stay clear of the undefined window everywhere
            assert accumulated_times_defined(other.T, fx.dt)[0] and accumulated_times_defined(other.T, fx.plan_dt)[0]
    for dt in sorted({fx.dt for fx in fxs}):
        stride = max(fx.S.sample_count(dt) for fx in fxs) * rec + PAD
        buf = torch.full((len(order) * stride,), float("nan"), dtype=torch.float64, device="cuda")
        batch.sample_device(x.data_ptr(), dt, buf.data_ptr(), stride, st)
        torch.cuda.synchronize()
        out["traj", dt] = buf.cpu().numpy().reshape(len(order), stride)
    for i, fx in enumerate(fxs):
        tt = torch.from_numpy(fx.guess_times).cuda()
        stride = 49 * len(fx.guess_times) + PAD
        buf = torch.full((len(order) * stride,), float("nan"), dtype=torch.float64, device="cuda")
        batch.initial_guess_device(x.data_ptr(), tt.data_ptr(), len(fx.guess_times), buf.data_ptr(), stride, st)
        torch.cuda.synchronize()
        out["guess", i] = buf.cpu().numpy().reshape(len(order), stride)
    max_steps = max(fx.S.contact_steps_max() for fx in fxs)
    plan = torch.full((len(order), max_steps, 2 + 4 * n_ee), float("nan"), dtype=torch.float64, device="cuda")
    counts = torch.full((len(order),), -1, dtype=torch.int32, device="cuda")
    batch.contact_plan_device(x.data_ptr(), fxs[0].plan_dt, fxs[0].plan_horizon, plan.data_ptr(), max_steps, counts.data_ptr(), st)
    torch.cuda.synchronize()
    out["plan"], out["counts"] = plan.cpu().numpy(), counts.cpu().numpy()
    for i, fx in enumerate(fxs):
        planes = ta.Planes(fx.regions, fx.boundaries(), device=0)
        idx = torch.full((len(order), max_steps, n_ee), -7, dtype=torch.int32, device="cuda")
        batch.contact_planes_device(planes, plan.data_ptr(), counts.data_ptr(), max_steps, idx.data_ptr(), st)
        torch.cuda.synchronize()
        out["planes", i] = idx.cpu().numpy()
    return out


def _check_against_fixtures(out, probs, first, what, worst):
    """problems first .. first + len(probs) - 1 of the batch against the fixtures"""
    for q, (i, fx, k) in enumerate(probs):
        p, ne = first + q, fx.n_ee
        tag = "%s, %s x[%d]" % (what, fx.name, k)
        ex = traj_exact_columns(ne)
        n = fx.traj.shape[1]
        assert fx.S.sample_count(fx.dt) == n, tag
        row = out["traj", fx.dt][p]
        check_records(row[:n * (20 + 13 * ne)].reshape(n, -1), fx.traj[k], ex, tag + " trajectory", worst, "trajectory")
        assert np.isnan(row[n * (20 + 13 * ne):]).all(), tag + ": written past the trajectory records"
        row = out["guess", i][p]
        check_records(row[:49 * len(fx.guess_times)].reshape(-1, 49), fx.guess[k], [0], tag + " guess", worst, "guess")
        assert np.isnan(row[49 * len(fx.guess_times):]).all(), tag + ": written past the guess records"
        steps = int(out["counts"][p])
        plan = out["plan"][p]
        sets = out["planes", i][p]
        assert 0 <= steps <= plan.shape[0], tag
        check_plan(fx, k, steps, plan[:, 1], sets, tag + " plan", worst)
        assert np.isnan(plan[steps:]).all() and (sets[steps:] == -1).all(), tag + ": written past the footstep states"
        st = fx.plan_state[k, :steps]
        feet = np.concatenate([st[:, c + 1:c + 4] for c in ex[1:]], axis=1)
        check_records(np.concatenate([plan[:steps, :1], plan[:steps, 2:]], axis=1), np.concatenate([st[:, ex], feet], axis=1), list(range(1 + ne)),
                      tag + " footstep states", worst, "footstep state")


@pytest.mark.gpu
@pytest.mark.parametrize("n_ee", [1, 2, 4])
def test_device_matches_the_reference_extractors(n_ee):
    """All fixture problems with the same number of feet in one ragged batch, NaN-prefilled outputs, against the recorded
    outputs of the reference's extractors: trajectory and guess records, footstep plans with their plane indices, the
    footstep states; nothing written past a problem's records."""
    fxs, probs = _group(n_ee)
    assert probs
    out = _run_extractors(fxs, probs)
    worst = {}
    _check_against_fixtures(out, probs, 0, "device", worst)
    print("n_ee %d: %d problems of %d fixtures, device vs reference extractors, worst error / scale: %s" % (
        n_ee, len(probs), len(fxs), ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


@pytest.mark.gpu
@pytest.mark.parametrize("n_ee", [1, 2, 4])
def test_device_matches_the_reference_extractors_in_a_large_batch(n_ee):
    """The same problems tiled to a batch of >= 256: the first and the last tile against the fixtures, every tile
    bit-equal to the first (same problems, same x)."""
    fxs, probs = _group(n_ee)
    tiles = -(-256 // len(probs))
    out = _run_extractors(fxs, probs, tiles)
    assert out["n"] >= 256
    for t in (0, tiles - 1):
        _check_against_fixtures(out, probs, t * len(probs), "device, tile %d of %d" % (t, tiles), {})
    for key, a in out.items():
        if key == "n":
            continue
        a = a.reshape(tiles, -1)
        assert np.array_equal(a, np.broadcast_to(a[0], a.shape), equal_nan=a.dtype.kind == "f"), "tiles differ in %s" % (key,)
