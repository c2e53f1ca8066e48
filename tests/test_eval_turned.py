"""Turned and far Euler angles through every evaluation kernel that holds a rotation, against the oracle.

The points of the other tests keep every Euler angle below 3*pi/4, so the evaluation kernels never leave the first quadrant and
its two neighbours.  Here six rows of the instantiation matrix (tests/eval_matrix.py), which between them claim every kernel
family with a rotation in it, run at
  Case.x_turned   (even problems)  angles k*pi/2 + delta, k = -6 .. 6: all four quadrants, negative n, the multiples of pi/2
                                   themselves and their neighbouring doubles;
  Case.x_far      (odd problems)   |angle| in [5e4, 3e5]: both sides of the 1e5 switch of sincos_fast inside one quad.
Per row, for EVAL_BOTH, EVAL_JACOBIAN and EVAL_VALUES, each without and with per-kernel events: parity with the oracle on every
problem, the same bits from the fused and the separate launches, and under EVAL_BOTH the bits of the one-problem batch.

Tolerances.  Turned points meet the parity bar of tests/common.py unchanged (the oracle moves by less than 1 % of the bar when
every base-ang variable moves one ulp: checked below without a GPU).  At far points the problem itself is ill-conditioned:
one ulp of an angle of 1e5 is 1.5e-11 rad, and the interpolated angle -- a four-term Hermite sum, about nine roundings, so about
9 ulp on the device's side and 9 on the oracle's -- carries that into every sine.  The allowance there comes from the reference
alone: per constraint row and per Jacobian row, NUDGE = 32 (18 rounded up to a power of two) times the largest change the
oracle's own output shows in that row when every base-ang variable moves one ulp up, and separately one ulp down; it is added to
the parity bar.  A wrong quadrant, a wrong branch or a broken broadcast is an error of order 1.

Each GPU test prints its worst error as a fraction of the bar (turned) and of bar + allowance (far); run with -s."""
import functools

import numpy as np
import pytest

import towr_amd as ta
from tests import eval_matrix
from tests.common import FLOOR, RTOL, assert_parity, linear_row_scale, row_scale, set_scale
from tests.test_eval_scores import _oracle_scores

ROW_NAMES = ("k40_two", "k40_one", "t16_one", "p40_two", "p40p6_p40", "p40_k40")
ROWS = [r for r in eval_matrix.parse()[1] if r["name"] in ROW_NAMES]
STRUCTS = sorted({s for r in ROWS for s in r["structs"]})
POOL = 2                  # distinct points per structure and kind
# The seeds of the turned points.  Between nodes a tenth of a second apart the angles run through a quarter turn or more, and at
# seed 1 one dynamic Jacobian entry of the oracle moves by 1.01 % of the bar under the one-ulp nudge; at these it is <= 0.22 %
# (test_oracle_is_finite_and_steady_at_turned_points holds the chosen seeds to 1 %).
TURNED_SEEDS = (0, 2)
NUDGE = 32.0
SAMPLE_STRUCTS = ("k40", "p40a")
SAMPLE_DT = 0.01
SAMPLE_TOL = 1e-10        # the bound of test_trajectory_sampling / test_initial_guess_samples


def _kind(p):
    return "turned" if p % 2 == 0 else "far"


@functools.lru_cache(maxsize=None)
def _x(name, kind, i):
    case = eval_matrix.make_case(name)
    x = case.x_turned(TURNED_SEEDS[i]) if kind == "turned" else case.x_far(i)
    x.flags.writeable = False
    return x


def _nudge_change(name, kind, i):
    """(g, jac of the oracle, and per entry the largest change under a one-ulp nudge of base-ang, up and down)"""
    case = eval_matrix.make_case(name)
    rg, _, _, rj = case.P.eval(_x(name, kind, i))
    dg, dj = np.zeros_like(rg), np.zeros_like(rj)
    for direction in (1, -1):
        ng, _, _, nj = case.P.eval(case.nudged(_x(name, kind, i), direction))
        dg, dj = np.maximum(dg, np.abs(ng - rg)), np.maximum(dj, np.abs(nj - rj))
    return rg, rj, dg, dj


@functools.lru_cache(maxsize=None)
def _ref(name, kind, i):
    """(g, jac, allowance on g, allowance on jac): the allowances are zero at turned points"""
    case = eval_matrix.make_case(name)
    if kind == "turned":
        rg, _, _, rj = case.P.eval(_x(name, kind, i))
        return rg, rj, np.zeros_like(rg), np.zeros_like(rj)
    rg, rj, dg, dj = _nudge_change(name, kind, i)
    return rg, rj, NUDGE * dg, NUDGE * row_scale(case.S.row_ptr, dj)


def _bars(S, rg, rj, x):
    gscale = np.maximum(set_scale(S.con_sets, rg), linear_row_scale(S, rj, np.asarray(x)))
    return RTOL * np.abs(rg) + FLOOR * gscale, RTOL * np.abs(rj) + FLOOR * row_scale(S.row_ptr, rj)


def _fraction(got, ref, tol):
    ok = tol > 0
    return float((np.abs(got - ref)[ok] / tol[ok]).max(initial=0.0))


def _assert_far(S, g, j, rg, rj, ag, aj, what, x):
    bar_g, bar_j = _bars(S, rg, rj, x)
    for name, got, ref, tol in (("constraint", g, rg, bar_g + ag), ("Jacobian", j, rj, bar_j + aj)):
        err = np.abs(got - ref)
        bad = np.nonzero(~(err <= tol))[0]
        assert bad.size == 0, "%s: %d %s values off, worst |err| %.3e (bar + allowance %.3e) at %d" % (
            what, bad.size, name, err[bad].max(), tol[bad[err[bad].argmax()]], bad[err[bad].argmax()])


def _claimed(rows):
    return {c for r in rows for claims in r["claims"].values() for c in claims}


# ------------------------------------------------------------------ CPU tier: conditions on the rows and on the reference
def test_rows_claim_every_kernel_family_with_a_rotation():
    assert [r["name"] for r in ROWS] and {r["name"] for r in ROWS} == set(ROW_NAMES)
    claimed = _claimed(ROWS)
    for family in ("dyn_kernel<", "dyn_uniform_kernel<", "eval_fused_kernel<", "rom_kernel<", "dyn_phase_kernel<0,", "dyn_phase_kernel<40,",
                   "rom_phase_kernel<0,", "rom_phase_kernel<24,", "eval_values_kernel<", "eval_scores_kernel<"):
        assert any(c.startswith(family) for c in claimed), "no row claims %s...>" % family
    for r in ROWS:
        assert 2 <= len(r["order"]) <= 5 and r["kind"] == "cheap"
        assert all(int(eval_matrix.parse()[0][s].get("K", 40)) <= 40 for s in r["structs"])


def test_turned_points_visit_every_quadrant():
    from tests.common import nearest_quarter_turn
    for name in STRUCTS:
        case = eval_matrix.make_case(name)
        idx = case.euler_positions()
        for i in range(POOL):
            x, base = _x(name, "turned", i), case.x_perturbed(TURNED_SEEDS[i])
            rest = np.ones(x.size, dtype=bool)
            rest[idx.ravel()] = False
            assert np.array_equal(x[rest], base[rest]), "only the Euler angles of base-ang change"
            th = x[idx]
            assert np.abs(th).max() <= 6 * np.pi / 2 + 0.7 and np.abs(th).max() > 3 * np.pi / 4
            n = np.rint(th * (2 / np.pi)).astype(int)
            for sgn in (1, -1):
                assert set(np.unique(n[sgn * n > 0] & 3)) == {0, 1, 2, 3}, (name, i)
            exact = np.array([nearest_quarter_turn(int(k)) for k in n.ravel()]).reshape(th.shape)
            on, beside = th == exact, (th == np.nextafter(exact, np.inf)) | (th == np.nextafter(exact, -np.inf))
            assert 0.12 < on.mean() < 0.4 and 0.12 < beside.mean() < 0.4, (name, i, on.mean(), beside.mean())
            assert (np.abs(th - exact)[~on & ~beside] < 0.7).all()


def test_nearest_quarter_turns_are_nearest():
    import mpmath
    from tests.common import nearest_quarter_turn
    mpmath.mp.dps = 60
    for k in range(-6, 7):
        v = nearest_quarter_turn(k)
        d = abs(mpmath.mpf(v) - k * mpmath.pi / 2)
        assert all(d <= abs(mpmath.mpf(float(w)) - k * mpmath.pi / 2) for w in (np.nextafter(v, np.inf), np.nextafter(v, -np.inf)))


def test_far_points_straddle_the_switch():
    for name in STRUCTS:
        case = eval_matrix.make_case(name)
        for i in range(POOL):
            a = np.abs(_x(name, "far", i)[case.euler_positions()])
            assert a.min() >= 5e4 and a.max() <= 3e5
            both = ((a < 1e5).any(axis=1) & (a >= 1e5).any(axis=1))
            assert both.all(), "every node triple has angles on both sides of 1e5"
            signs = np.sign(_x(name, "far", i)[case.euler_positions()])
            assert (signs > 0).any() and (signs < 0).any()


def test_oracle_is_finite_and_steady_at_turned_points():
    """the reference-side conditions behind the tolerances: finite outputs at both kinds of point (pitch = pi/2 included),
    and at turned points a one-ulp nudge of base-ang moves no entry by more than 1 % of the parity bar"""
    worst = 0.0
    for name in STRUCTS:
        S = eval_matrix.make_case(name).S
        for i in range(POOL):
            rg, rj, ag, aj = _ref(name, "far", i)
            assert np.isfinite(rg).all() and np.isfinite(rj).all() and np.isfinite(ag).all() and np.isfinite(aj).all()
            assert ag.max() > 0 and aj.max() > 0
            rg, rj, dg, dj = _nudge_change(name, "turned", i)
            assert np.isfinite(rg).all() and np.isfinite(rj).all()
            bar_g, bar_j = _bars(S, rg, rj, _x(name, "turned", i))
            worst = max(worst, _fraction(rg + dg, rg, bar_g), _fraction(rj + dj, rj, bar_j))
    print("\nturned points: a one-ulp nudge of base-ang moves the oracle by at most %.3g of the parity bar" % worst)
    assert worst < 0.01


def _sample_points():
    """(structure, kind, seed) of the four problems of the sampling test: both kinds on both structures"""
    a, b = SAMPLE_STRUCTS
    return [(a, "turned", 0), (b, "far", 0), (a, "far", 1), (b, "turned", 1)]


_ANGULAR = (slice(10, 14), slice(14, 17), slice(17, 20))   # quaternion, angular velocity, angular acceleration of a sample record


@functools.lru_cache(maxsize=None)
def _sample_ref(name, kind, i):
    """(trajectory of the oracle, allowance): the allowance is NUDGE times the largest change of the field's group (quaternion,
    omega, omega-dot) in that sample under the one-ulp nudges at far points, zero at turned points and on every other field"""
    case = eval_matrix.make_case(name)
    ref = case.P.sample_trajectory(_x(name, kind, i), SAMPLE_DT)
    change = np.zeros_like(ref)
    for direction in (1, -1):
        change = np.maximum(change, np.abs(case.P.sample_trajectory(case.nudged(_x(name, kind, i), direction), SAMPLE_DT) - ref))
    allow = np.zeros_like(ref)
    for grp in _ANGULAR:
        allow[:, grp] = NUDGE * change[:, grp].max(axis=1, keepdims=True)
    return ref, change, (allow if kind == "far" else np.zeros_like(ref))


def _on_branch(ref, margin=1e-6):
    """samples whose quaternion sits on a branch of its extraction from R (the reference's: trace > 0, else the largest
    diagonal entry): trace(R) = 4 w^2 - 1 within `margin` of 0, or trace <= 0 and the two largest of x^2, y^2, z^2 (the order
    of the diagonal entries) within `margin` of each other.  Rotations by exact quarter turns about the axes -- a node whose
    three angles are multiples of pi/2 -- land there: a cyclic permutation matrix has trace 0, a half turn about a face
    diagonal has two equal diagonal entries.  Either side of a branch is the same rotation, as q or as -q."""
    q = ref[:, 10:14]
    trace = 4.0 * q[:, 0] ** 2 - 1.0
    sq = np.sort(q[:, 1:] ** 2, axis=1)
    return (np.abs(trace) < margin) | ((trace <= margin) & (sq[:, 2] - sq[:, 1] < margin))


def _align_sign(got, ref, rows):
    """got with the quaternion of the samples `rows` negated where that brings it closer to the reference's"""
    out = np.array(got)
    flip = rows & ((out[:, 10:14] * ref[:, 10:14]).sum(axis=1) < 0)
    out[flip, 10:14] *= -1.0
    return out


def test_oracle_trajectory_is_steady_at_turned_points():
    """the reference-side condition behind the sampling bound at turned points: a one-ulp nudge of base-ang moves no field by
    more than 1 % of the bound -- except the sign of the quaternion at the few samples that sit on a branch of its
    extraction, which the GPU test therefore compares up to that sign"""
    for name, kind, i in _sample_points():
        ref, change, _ = _sample_ref(name, kind, i)
        assert np.isfinite(ref).all()
        if kind == "turned":
            case = eval_matrix.make_case(name)
            scale = np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1.0)
            branch = _on_branch(ref)
            assert branch.sum() <= 0.1 * len(ref), (name, i, branch.sum())
            assert (change[~branch] / scale).max() < 0.01 * SAMPLE_TOL, (name, i, (change[~branch] / scale).max())
            for direction in (1, -1):
                moved = _align_sign(case.P.sample_trajectory(case.nudged(_x(name, kind, i), direction), SAMPLE_DT), ref, branch)
                assert (np.abs(moved - ref) / scale).max() < 0.01 * SAMPLE_TOL, (name, i, direction)


# ------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row_at_turned_and_far_points(row):
    import torch
    from tests.test_eval_matrix import _run, _same_bits
    names = [row["structs"][s] for s in row["order"]]
    n = len(names)
    seen, key = {}, []
    for p, nm in enumerate(names):
        k = (nm, _kind(p))
        key.append((nm, _kind(p), seen.get(k, 0) % POOL))
        seen[k] = seen.get(k, 0) + 1
    cases = [eval_matrix.make_case(nm) for nm in row["structs"]]
    batch = ta.Batch([c.S for c in cases], row["order"], device=0)
    d_x = torch.from_numpy(np.concatenate([_x(*k) for k in key])).cuda()
    worst = {"turned": 0.0, "far": 0.0}
    for flags in (ta.EVAL_BOTH, ta.EVAL_JACOBIAN, ta.EVAL_VALUES):
        out = {}
        for events in (False, True):
            what = "%s flags %d events %d" % (row["name"], flags, events)
            planned = {s["instantiation"] for s in batch.eval_plan(flags, events)}
            missing = set(eval_matrix.claims_of(row, flags, events)) - planned
            assert not missing, "%s: the device plans %s, the row claims %s as well" % (what, sorted(planned), sorted(missing))
            out[events] = _run(batch, d_x, flags, events, what)
            for p in range(n):
                S = cases[row["order"][p]].S
                rg, rj, ag, aj = _ref(*key[p])
                x = _x(*key[p])
                g = out[events][0][batch.g_off[p]:batch.g_off[p + 1]].cpu().numpy() if flags & ta.EVAL_VALUES else rg
                j = out[events][1][batch.jac_off[p]:batch.jac_off[p + 1]].cpu().numpy() if flags & ta.EVAL_JACOBIAN else rj
                where = "%s problem %d (%s, %s point %d)" % ((what, p) + key[p])
                bar_g, bar_j = _bars(S, rg, rj, x)
                kind = key[p][1]
                worst[kind] = max(worst[kind], _fraction(g, rg, bar_g + ag), _fraction(j, rj, bar_j + aj))
                if kind == "turned":
                    assert_parity(S, g, j, rg, rj, where, x=x)
                else:
                    _assert_far(S, g, j, rg, rj, ag, aj, where, x)
                if flags == ta.EVAL_BOTH and not events:   # the same bits as the structure alone in a batch
                    sg, sj = _solo(*key[p])
                    assert np.array_equal(g.view(np.int64), sg.view(np.int64)), where + ": g differs from the one-problem batch"
                    assert np.array_equal(j.view(np.int64), sj.view(np.int64)), where + ": jac differs from the one-problem batch"
        if flags & ta.EVAL_VALUES:
            assert _same_bits(out[False][0], out[True][0]), "%s flags %d: g differs between the fused and the separate launches" % (row["name"], flags)
        if flags & ta.EVAL_JACOBIAN:
            assert _same_bits(out[False][1], out[True][1]), "%s flags %d: jac differs between the fused and the separate launches" % (row["name"], flags)
        del out
    if row["claims"]["scores"]:
        _check_scores(row, batch, cases, key, d_x)
    print("\n%s: %d problems, worst error %.3g of the parity bar at turned points, %.3g of bar + allowance at far points"
          % (row["name"], n, worst["turned"], worst["far"]))


@functools.lru_cache(maxsize=None)
def _solo(name, kind, i):
    """EVAL_BOTH of one problem alone in a batch, as numpy"""
    import torch
    from tests.test_eval_matrix import _run
    batch = ta.Batch([eval_matrix.make_case(name).S], [0], device=0)
    g, j = _run(batch, torch.from_numpy(np.array(_x(name, kind, i))).cuda(), ta.EVAL_BOTH, False, "%s alone" % name)
    return g.cpu().numpy(), j.cpu().numpy()


def _check_scores(row, batch, cases, key, d_x):
    """eval_scores_device against numpy on the oracle's g, as tests/test_eval_matrix.py _check_scores does; at far points the
    allowance of a family is that of its rows: their largest for the maximum, their sum for the sum"""
    import torch
    from tests.test_eval_matrix import _Out
    planned = {s["instantiation"] for s in batch.eval_plan(request="scores")}
    assert set(row["claims"]["scores"]) <= planned, "%s: the device plans %s" % (row["name"], sorted(planned))
    n = batch.n_problems
    g = _Out(int(batch.g_off[-1]))
    scores = torch.full((n, 16), -1.0, dtype=torch.float64, device="cuda")
    batch.eval_scores_device(d_x.data_ptr(), scores.data_ptr(), d_g=0 if batch.scores_without_g else g.ptr(),
                             stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert g.guards_intact() and (g.untouched() if batch.scores_without_g else g.fully_written())
    table = scores.cpu().numpy()
    for p in range(n):
        case = cases[row["order"][p]]
        want = _oracle_scores(case, _x(*key[p]))
        ag = _ref(*key[p])[2]
        allow = np.zeros((8, 2))
        for cs in case.S.con_sets:
            fam = [i for i, f in enumerate(ta.FAMILIES) if cs["name"].startswith(f)][0]
            a = ag[cs["offset"]:cs["offset"] + cs["size"]]
            allow[fam, 0] = max(allow[fam, 0], a.max(initial=0.0))
            allow[fam, 1] += a.sum()
        got = table[p].reshape(8, 2)
        assert not np.isnan(want).any() and not np.isnan(got).any(), (row["name"], p, got, want)
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want) + 1e-9 + allow), (row["name"], p, key[p], got, want, allow)


@pytest.mark.gpu
def test_sampling_and_initial_guess_at_turned_and_far_points():
    """sample_device against P.sample_trajectory and initial_guess_device against the oracle's initial-guess restatement, at
    the bounds of test_trajectory_sampling / test_initial_guess_samples; at far points the quaternion, angular velocity and
    angular acceleration (the fields a sine enters) get the nudge allowance.  At turned points a node whose three angles are
    quarter turns puts the quaternion on a branch of its extraction from R, where the reference itself flips between q and -q
    under a one-ulp nudge (_on_branch): those samples, a few per trajectory, are compared up to that sign at the same bound."""
    import torch
    points = _sample_points()
    names = list(SAMPLE_STRUCTS)
    cases = [eval_matrix.make_case(nm) for nm in names]
    order = [names.index(nm) for nm, _, _ in points]
    batch = ta.Batch([c.S for c in cases], order, device=0)
    st = torch.cuda.current_stream().cuda_stream
    x = torch.from_numpy(np.concatenate([_x(*k) for k in points])).cuda()
    rec = 20 + 13 * 4
    counts = [cases[s].S.sample_count(SAMPLE_DT) for s in order]
    stride = max(counts) * rec
    out = torch.full((len(order) * stride,), float("nan"), dtype=torch.float64, device="cuda")
    batch.sample_device(x.data_ptr(), SAMPLE_DT, out.data_ptr(), stride, st)
    torch.cuda.synchronize()
    oh = out.cpu().numpy()
    worst = {"turned": 0.0, "far": 0.0}
    for p, k in enumerate(points):
        ref, _, allow = _sample_ref(*k)
        assert ref.shape == (counts[p], rec)
        got = oh[p * stride:p * stride + counts[p] * rec].reshape(counts[p], rec)
        if k[1] == "turned":   # (q and -q are one rotation: where the reference's extraction sits on a branch, either may come out)
            got = _align_sign(got, ref, _on_branch(ref))
        assert np.array_equal(got[:, 0], ref[:, 0])
        for e in range(4):
            assert np.array_equal(got[:, 20 + 13 * e], ref[:, 20 + 13 * e])
        tol = SAMPLE_TOL * np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1.0) + allow
        frac = np.abs(got - ref) / tol
        worst[k[1]] = max(worst[k[1]], float(frac.max()))
        assert frac.max() < 1.0, "sample, problem %d %s: field %d off by %.3g of its bound" % (p, k, int(frac.max(axis=0).argmax()), frac.max())

    T = 2.0
    times = np.concatenate([[0.0, T, 0.1, 0.2, 0.13, 1.0], np.random.default_rng(5).uniform(0.0, T, 70)])
    stride = 49 * len(times) + 3
    tt = torch.from_numpy(times).cuda()
    out = torch.full((len(order) * stride,), float("nan"), dtype=torch.float64, device="cuda")
    batch.initial_guess_device(x.data_ptr(), tt.data_ptr(), len(times), out.data_ptr(), stride, st)
    torch.cuda.synchronize()
    oh = out.cpu().numpy()
    for p, k in enumerate(points):
        ref = cases[order[p]].P.initial_guess_samples(_x(*k), times)
        got = oh[p * stride:p * stride + 49 * len(times)].reshape(len(times), 49)
        assert np.array_equal(got[:, 0], times)
        assert np.array_equal(got[:, 25:37], np.zeros((len(times), 12)))
        assert np.isnan(oh[p * stride + 49 * len(times):(p + 1) * stride]).all()
        err = np.abs(got - ref) / np.maximum(np.abs(ref).max(axis=0, keepdims=True), 1.0)
        assert err.max() < SAMPLE_TOL, "initial guess, problem %d %s: field %d off by %.3e" % (p, k, int(err.max(axis=0).argmax()), err.max())
    print("\nsampling: worst error %.3g of the bound at turned points, %.3g of bound + allowance at far points" % (worst["turned"], worst["far"]))
