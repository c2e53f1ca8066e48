"""twr_batch_checks and twr_batch_check_scores through the C ABI, on Go1 with twr_model_preset.

Batches (at most four problems each).  The shapes of tests/test_joints.py, chosen for the 64-sample round boundary of the fold:
  (i) exactly 64 samples   (ii) two structures with 65 and 129 samples   (iii) optimised timings   (iv) dt > T: one sample
and one per terrain kind that matters:
  stairs  x such that swing samples lie on either side of x = 1.0 and of x = 1.4 and some go under a tread
  block   footholds in the 3 cm ramp of the Block: a sloped basis under a stance force
  grid    a 60 x 44 `Grid` map at 5 cm (the layer recipe of tests/test_grid_map_update.py), before and after
          twr_batch_grid_map_update_device on the same stream
and a monoped and a biped on Stairs: the kernels are instantiated per number of feet.  The file passes on either build of the
checks kernel (direct reads, LDS-staged).
References
  check records   tests/check_points.py checks_numpy on the device's own trajectory records, heights and slopes from the oracle
                  problem's terrain_probe_full: bit for bit
  scores          check_points.fold of the device's check records: bit for bit
  constraint rows the `dynamic` and `rangeofmotion-e` rows of twr_batch_eval(TWR_EVAL_VALUES) on the same x, sampled on their own
                  grids: within the parity bar of tests/common.py.  Measured on the MI355X (largest difference over the four
                  problems, relative to the set's scale): dynamic 5.8e-15, range of motion 3.2e-15."""
import ctypes as C
import functools

import numpy as np
import pytest

import towr_amd as ta

from . import check_points as cp
from . import segment_points as sp
from .common import FLOOR, RTOL, Case, parity_violations
from .test_ik_ref import same_bits
from .test_joints import DT2, dt_for, gentle_x

SIZE, RES, POS_A, POS_B = (60, 44), 0.05, (1.0, 0.05), (0.9, -0.05)
TREC, CREC = 20 + 13 * 4, 7 + 5 * 4


def _torch():
    import torch
    return torch


def layer(seed):
    """tests/test_grid_map_update.py layer(): a ramp along x plus noise, float32 [size_x, size_y]"""
    rng = np.random.default_rng(seed)
    return (0.03 * np.arange(SIZE[0])[:, None] * RES + rng.uniform(-0.05, 0.25, size=SIZE)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "c1_2.0":
        return Case("go1", "flat", ta.gait_combo(4, 1, 2.0))
    if name == "c0_65":       # 1.29 / 0.02 = 64.5: 65 samples at DT2
        return Case("go1", "flat", ta.gait_combo(4, 0, 1.29))
    if name == "c1_129":      # 2.57 / 0.02 = 128.5: 129 samples at DT2
        return Case("go1", "flat", ta.gait_combo(4, 1, 2.57))
    if name == "timings":
        return Case("go1", "flat", ta.gait_combo(4, 1, 1.6), constraint_sets=ta.SETS_ALL)
    if name == "stairs":
        return Case("go1", "stairs", ta.gait_combo(4, 1, 2.0))
    if name == "block":
        return Case("go1", "block", ta.gait_combo(4, 0, 1.6))
    if name in ("grid_a", "grid_b"):     # (grid_b: the create path on the second layer, for its oracle problem only)
        return Case("go1", "grid_map", ta.gait_combo(4, 1, 2.0), grid=(layer(1), RES, POS_A) if name == "grid_a" else (layer(2), RES, POS_B))
    raise KeyError(name)


def x_of(name, seed):
    """flat cases: the gentle x of tests/test_joints.py.  Terrain cases: the guess of a walk that crosses the terrain's features
    with the same gentle noise; Block also gets three footholds inside its ramp 0.7 <= x <= 0.73."""
    c = case(name)
    if name in ("c1_2.0", "c0_65", "c1_129", "timings"):
        return gentle_x(c, seed)
    x = gentle_x(c, seed) - c.x_guess(goal_x=0.05) + c.x_guess(goal_x={"stairs": 1.8, "block": 1.2}.get(name, 1.4))
    if name == "block":
        idx = c.footholds()
        x[idx[2::7, 0][:3]] = [0.705, 0.715, 0.729]
    return x


BATCHES = {
    "i_64": (("c1_2.0", "c1_2.0"), lambda cs: dt_for(cs[0].S, 64, 2.0)),
    "ii_65_129": (("c0_65", "c1_129", "c0_65"), lambda cs: DT2),
    "iii_timings": (("timings", "timings"), lambda cs: 0.01),
    "iv_one_sample": (("c1_2.0", "c0_65"), lambda cs: 3.0),
    "stairs": (("stairs", "stairs"), lambda cs: 0.01),
    "block": (("block", "c0_65", "block"), lambda cs: 0.01),
    "grid": (("grid_a", "grid_a"), lambda cs: 0.01),
}


class Run:
    """one batch on the device with its x: trajectory records, check records and scores"""

    def __init__(self, names, dt, xs=None, seed0=0):
        torch = _torch()
        self.names = names
        self.cases = [case(n) for n in names]
        structs, index = [], []
        for c in self.cases:
            if c.S not in structs:
                structs.append(c.S)
            index.append(structs.index(c.S))
        self.batch = ta.Batch(structs, index, device=0)
        self.model = self.cases[0].model
        self.dt = float(dt)
        self.xs = [x_of(n, seed0 + p) for p, n in enumerate(names)] if xs is None else xs
        self.counts = [c.S.sample_count(self.dt) for c in self.cases]
        self.n_max = max(self.counts)
        self.tstride, self.cstride = self.n_max * TREC + 3, self.n_max * CREC + 5      # (not the tightest strides)
        n = len(self.cases)
        self.x = torch.from_numpy(np.concatenate(self.xs)).cuda()
        self.traj = torch.full((n * self.tstride,), float("nan"), dtype=torch.float64, device="cuda")
        self.checks = torch.full((n * self.cstride,), float("nan"), dtype=torch.float64, device="cuda")
        self.scores = torch.full((n, 8), -7.0, dtype=torch.float64, device="cuda")

    def check(self, st=None):
        st = _torch().cuda.current_stream().cuda_stream if st is None else st
        self.batch.checks_device(self.model, self.traj.data_ptr(), self.tstride, self.dt, self.checks.data_ptr(), self.cstride, st)
        self.batch.check_scores_device(self.checks.data_ptr(), self.cstride, self.dt, self.scores.data_ptr(), st)

    def go(self, st=None):
        st = _torch().cuda.current_stream().cuda_stream if st is None else st
        self.batch.sample_device(self.x.data_ptr(), self.dt, self.traj.data_ptr(), self.tstride, st)
        self.check(st)

    def done(self):
        self.go()
        _torch().cuda.synchronize()
        return self

    def traj_of(self, p, traj=None):
        t = self.traj.cpu().numpy() if traj is None else traj
        return t[p * self.tstride:p * self.tstride + self.counts[p] * TREC].reshape(-1, TREC)

    def checks_of(self, p, checks=None):
        c = self.checks if checks is None else checks
        return c.cpu().numpy()[p * self.cstride:p * self.cstride + self.counts[p] * CREC].reshape(-1, CREC)

    def want(self, p, oracle_case=None, traj=None):
        """the numpy restatement on the device's own trajectory records of problem p"""
        c = oracle_case or self.cases[p]
        return cp.checks_numpy(self.traj_of(p, traj), cp.consts_of(c.model), cp.oracle_terrain(c.P))

    def assert_padding(self):
        pad = self.checks.cpu().numpy().reshape(len(self.cases), self.cstride)
        for p, n in enumerate(self.counts):
            assert np.isnan(pad[p, n * CREC:]).all(), "nothing is written behind a problem's records"


@functools.lru_cache(maxsize=None)
def run(name):
    names, dt = BATCHES[name]
    return Run(names, dt([case(n) for n in names])).done()


def swing_legs(traj, checks):
    """x of the foot and clearance of every leg-sample with contact 0"""
    legs = cp.legs_of(checks, 4)
    x = np.column_stack([traj[:, 21 + 13 * e] for e in range(4)])
    swing = legs[:, :, cp.CONTACT] == 0.0
    return x[swing], legs[:, :, cp.CLEAR][swing]


def assert_not_vacuous(name, r):
    """the terrain cases reach what they are there for, judged on the CPU restatement"""
    for p, c in enumerate(r.cases):
        traj, want = r.traj_of(p), r.want(p)
        if r.names[p] == "stairs":
            x, clear = swing_legs(traj, want)
            assert (x < 1.0).any() and ((x >= 1.0) & (x < 1.4)).any() and (x >= 1.4).any(), "swing samples on every side of both risers"
            assert (clear < 0).any() and (clear > 0).any(), "a swing foot under a tread, and one above it"
        if r.names[p] == "block":
            hx = np.array([c.P.terrain_probe_full(a, b)[1] for e in range(4) for a, b in zip(traj[:, 21 + 13 * e], traj[:, 22 + 13 * e])])
            stance = np.concatenate([traj[:, 20 + 13 * e] for e in range(4)]) != 0.0
            assert (hx[stance] != 0).any() and (hx[stance] == 0).any(), "a stance foot on the ramp: a sloped basis"
        if r.names[p] == "grid_a":
            h = cp.legs_of(want, 4)[:, :, cp.CLEAR]
            assert np.isfinite(h).all() and (np.abs(h) < 1.0).all() and np.unique(h).size > 100, "the walk stays on the map"


# ------------------------------------------------------------------ 1, 2: records and scores
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_check_records_equal_the_numpy_restatement_bit_for_bit(name):
    r = run(name)
    assert ta.check_rec(4) == CREC and ta.CHECK_SCORE_REC == 8
    if name in ("i_64", "ii_65_129", "iv_one_sample"):
        assert r.counts == {"i_64": [64, 64], "ii_65_129": [65, 129, 65], "iv_one_sample": [1, 1]}[name]
    assert_not_vacuous(name, r)
    for p in range(len(r.cases)):
        traj, got, want = r.traj_of(p), r.checks_of(p), r.want(p)
        assert np.isfinite(traj).all() and np.isfinite(got).all()
        eq = same_bits(got, want)
        assert eq.all(), (name, p, np.argwhere(~eq)[:8].tolist(), got[~eq][:8].tolist(), want[~eq][:8].tolist())
        assert same_bits(got[:, 0], traj[:, 0]).all()
    r.assert_padding()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_scores_equal_the_numpy_fold_of_the_check_records(name):
    r = run(name)
    got = r.scores.cpu().numpy()
    for p in range(len(r.cases)):
        want = cp.fold(r.checks_of(p), 4)
        assert same_bits(got[p], want).all(), (name, p, got[p].tolist(), want.tolist())
        assert got[p][0] == r.counts[p] and got[p][5] < 1e20 and got[p][6] < 1e20 and got[p][7] > -np.inf
    if name == "stairs":
        assert got[0][3] < 0, "the swing foot under the tread is what score [3] reports"


@pytest.mark.gpu
def test_a_grid_map_update_on_the_same_stream_is_seen_by_the_checks_behind_it():
    """checks on layer A, the update to layer B (another centre, a rolled buffer) and checks again, enqueued on one stream without
    a host synchronisation in between: the first records are A's, the second B's (clearances of the new layer)"""
    from .test_grid_map_update import dev_layer, rolled
    torch = _torch()
    names, _ = BATCHES["grid"]
    r = Run(names, 0.01).done()         # (warm: the work list exists, the module is loaded)
    checks_a = torch.full_like(r.checks, float("nan"))
    start = (17, 5)
    d = dev_layer(rolled(layer(2), start))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    st = s.cuda_stream
    r.batch.sample_device(r.x.data_ptr(), r.dt, r.traj.data_ptr(), r.tstride, st)
    r.batch.checks_device(r.model, r.traj.data_ptr(), r.tstride, r.dt, checks_a.data_ptr(), r.cstride, st)
    r.batch.update_grid_map_device(case("grid_a").grid, d, start, POS_B, st)
    r.check(st)
    s.synchronize()
    torch.cuda.synchronize()
    traj = r.traj.cpu().numpy()
    for p in range(len(names)):
        a, b = r.checks_of(p, checks_a), r.checks_of(p)
        want_a, want_b = r.want(p, traj=traj), r.want(p, oracle_case=case("grid_b"), traj=traj)
        assert same_bits(a, want_a).all() and same_bits(b, want_b).all()
        assert same_bits(a, run("grid").checks_of(p)).all()
        assert not same_bits(cp.legs_of(a, 4)[:, :, cp.CLEAR], cp.legs_of(b, 4)[:, :, cp.CLEAR]).all(), "the layers differ"
        assert same_bits(r.scores.cpu().numpy()[p], cp.fold(b, 4)).all()


# ------------------------------------------------------------------ 3: the constraint rows on their own grids
TIE = ("c1_2.0", "stairs", "block", "timings")


def rows_of(S, name):
    cs = [s for s in S.con_sets if s["name"] == name][0]
    return cs["offset"], cs["size"]


@functools.lru_cache(maxsize=None)
def tie(which):
    """the four problems sampled on the grid of the dynamic (dt_dynamic) or the range-of-motion constraint (dt_rom), and g"""
    torch = _torch()
    dt = getattr(case(TIE[0]).params, which)
    assert all(getattr(case(n).params, which) == dt for n in TIE)
    r = Run(TIE, dt).done()
    g = torch.full((int(r.batch.g_off[-1]),), float("nan"), dtype=torch.float64, device="cuda")
    r.batch.eval_device(r.x.data_ptr(), g.data_ptr(), 0, ta.EVAL_VALUES, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return r, g.cpu().numpy()


def on_nodes(r, p, dt):
    """how many leading samples of problem p sit on the constraint's time nodes, bit for bit: all of the accumulated ones (the node
    T appended behind them has no sample), and at most one sample beyond them"""
    T = sp.sums(r.cases[p].sched.durations()[0])[-1]
    nodes = np.array(sp.time_nodes(T, dt)[:-1])
    t = r.traj_of(p)[:, 0]
    m = min(len(t), len(nodes))
    assert m == len(nodes) and len(t) - m <= 1 and same_bits(t[:m], nodes[:m]).all()
    return m


@pytest.mark.gpu
def test_residual_meets_the_dynamic_rows_on_their_grid():
    r, g = tie("dt_dynamic")
    worst = 0.0
    for p, c in enumerate(r.cases):
        m = on_nodes(r, p, r.dt)
        off, size = rows_of(c.S, "dynamic")
        ref = g[r.batch.g_off[p] + off:r.batch.g_off[p] + off + size]
        assert size == 6 * (m + 1) and np.isfinite(ref).all()
        scale = np.abs(ref).max()
        got = r.checks_of(p)[:m, 1:7].reshape(-1)
        bad, err = parity_violations(got, ref[:6 * m], np.full(6 * m, scale))
        worst = max(worst, float(err.max() / scale))
        print("\n%s: residual against the dynamic rows, %d nodes: largest difference %.3e of the set's scale %.3e" % (TIE[p], m, err.max() / scale, scale))
        assert bad.size == 0, (TIE[p], bad[:8].tolist(), err[bad][:8].tolist())
    assert worst > 0.0, "a quaternion and Euler angles: not the same expression"


@pytest.mark.gpu
def test_rom_meets_the_range_of_motion_rows_on_their_grid():
    """rom is a difference of the row's value and constants, so its error bar is the row's: RTOL |g_d| + FLOOR scale, the largest
    over the three dimensions"""
    r, g = tie("dt_rom")
    for p, c in enumerate(r.cases):
        m = on_nodes(r, p, r.dt)
        k = cp.consts_of(c.model)
        for e in range(4):
            off, size = rows_of(c.S, "rangeofmotion-%d" % e)
            ref = g[r.batch.g_off[p] + off:r.batch.g_off[p] + off + size]
            assert size == 3 * (m + 1) and np.isfinite(ref).all()
            scale = np.abs(ref).max()
            foot = ref[:3 * m].reshape(m, 3)
            want = (np.abs(foot - k["nominal"][e]) - k["max_dev"]).max(axis=1)
            tol = (RTOL * np.abs(foot) + FLOOR * scale).max(axis=1)
            err = np.abs(cp.legs_of(r.checks_of(p), 4)[:m, e, cp.ROM] - want)
            print("\n%s foot %d: rom against the rows, %d nodes: largest difference %.3e of the set's scale %.3e" % (TIE[p], e, m, err.max() / scale, scale))
            assert (err <= tol).all(), (TIE[p], e, float(err.max()))


# ------------------------------------------------------------------ 4: position independence, repeatability
@pytest.mark.gpu
def test_same_bits_in_another_slot_of_another_batch_and_on_two_streams():
    torch = _torch()
    a = run("ii_65_129")
    names = ("c1_2.0", "c1_129", "timings", "c0_65")        # problem 1 of (ii) now sits in slot 1 behind another structure, ...
    xs = [x_of(names[0], 50), a.xs[1], x_of(names[2], 51), a.xs[0]]      # ... its problem 0 in slot 3
    b = Run(names, DT2, xs=xs).done()
    for src, dst in ((1, 1), (0, 3)):
        assert same_bits(b.scores.cpu().numpy()[dst], a.scores.cpu().numpy()[src]).all()
        assert same_bits(b.checks_of(dst), a.checks_of(src)).all()
    one, two = Run(BATCHES["ii_65_129"][0], DT2, xs=a.xs).done(), Run(names, DT2, xs=xs).done()     # (warm)
    for r in (one, two):
        r.checks.fill_(float("nan"))
        r.scores.fill_(-7.0)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    one.go(s1.cuda_stream)
    two.go(s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    for r, ref in ((one, a), (two, b)):
        assert same_bits(r.checks.cpu().numpy(), ref.checks.cpu().numpy()).all()
        assert same_bits(r.scores.cpu().numpy(), ref.scores.cpu().numpy()).all()


# ------------------------------------------------------------------ 5: graph
@pytest.mark.gpu
def test_graph_of_map_update_sample_checks_scores_replays_on_a_new_x_and_layer():
    from .jac_device import capture
    from .test_grid_map_update import dev_layer, rolled
    torch = _torch()
    names, _ = BATCHES["grid"]
    r = Run(names, 0.01, seed0=20).done()            # (warm: the sample work list exists before the capture)
    start = (46, 0)
    d = dev_layer(rolled(layer(1), start))

    def step(st):
        r.batch.update_grid_map_device(case("grid_a").grid, d, start, POS_B, st)
        r.go(st)

    graph = capture(step)
    xs2 = [x_of(n, 30 + p) for p, n in enumerate(names)]
    r.x.copy_(torch.from_numpy(np.concatenate(xs2)))
    d.copy_(dev_layer(rolled(layer(2), start)))
    r.checks.fill_(float("nan"))
    r.scores.fill_(-2.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed_c, replayed_s = r.checks.cpu().numpy().copy(), r.scores.cpu().numpy().copy()
    eager = Run(names, 0.01, xs=xs2)
    eager.batch.update_grid_map_device(case("grid_a").grid, dev_layer(layer(2)), (0, 0), POS_B)
    eager.done()
    assert same_bits(replayed_c, eager.checks.cpu().numpy()).all() and same_bits(replayed_s, eager.scores.cpu().numpy()).all()
    for p in range(len(names)):
        assert same_bits(eager.checks_of(p), eager.want(p, oracle_case=case("grid_b"))).all(), "the replay ran on the new layer"
    assert not same_bits(replayed_s, run("grid").scores.cpu().numpy()).all()


# ------------------------------------------------------------------ 6: hostile records
POISON = (np.nan, np.inf, -np.inf, 1e300, -1e300)
FOOT_Z, FORCE_Z = lambda e: 20 + 13 * e + 3, lambda e: 20 + 13 * e + 12
HOSTILE = {}          # sample -> (kind, leg or quaternion component, value)
for _i, _v in enumerate(POISON):
    HOSTILE[3 + 12 * _i] = ("foot", _i % 4, _v)
    HOSTILE[7 + 12 * _i] = ("force", (_i + 1) % 4, _v)
    HOSTILE[11 + 12 * _i] = ("quat", _i % 4, _v)
HOSTILE[63] = ("quat0", 0, 0.0)


@pytest.mark.gpu
def test_hostile_records_are_contained_in_their_sample():
    """NaN, +-Inf and +-1e300 in the z of one foot, in the z of one force and in one quaternion component of single samples of
    problem 1, and a zero quaternion.  No fault; every poisoned record has the bits of the restatement on it; the fields made
    from the bad number are NaN where it is NaN or the quaternion cannot be normalised (an infinite or huge foot or force gives,
    by the same formulas, infinite or huge fields, and NaN where it meets a zero factor); every other field of that record, every
    other record and problem 0 keep the bits of the clean run; the scores that see a NaN are NaN."""
    torch = _torch()
    clean = run("i_64")
    r = Run(BATCHES["i_64"][0], clean.dt, xs=clean.xs)
    traj = clean.traj.cpu().numpy().copy()
    rec = traj[r.tstride:r.tstride + 64 * TREC].reshape(64, TREC)
    for s, (kind, k, v) in HOSTILE.items():
        if kind == "foot":
            rec[s, FOOT_Z(k)] = v
        elif kind == "force":
            rec[s, FORCE_Z(k)] = v
        elif kind == "quat":
            rec[s, 10 + k] = v
        else:
            rec[s, 10:14] = 0.0
    r.traj.copy_(torch.from_numpy(traj))
    r.check()
    torch.cuda.synchronize()
    assert same_bits(r.checks_of(0), clean.checks_of(0)).all() and same_bits(r.scores.cpu().numpy()[0], clean.scores.cpu().numpy()[0]).all()
    got, was, want = r.checks_of(1), clean.checks_of(1), r.want(1)
    hit = np.zeros(64, dtype=bool)
    hit[list(HOSTILE)] = True
    assert same_bits(got[~hit], was[~hit]).all() and same_bits(got[:, 0], was[:, 0]).all()
    assert same_bits(got, want).all()
    leg = lambda e: slice(cp.HEAD + cp.LEG * e, cp.HEAD + cp.LEG * (e + 1))
    for s, (kind, k, v) in HOSTILE.items():
        touched = np.zeros(CREC, dtype=bool)
        if kind == "foot":        # p_e.z: clearance and rom of the leg; f x (p_base - p_e) on angular x (f_y d_z) and y (f_x d_z), which a
            f = traj[r.tstride:].reshape(-1)[s * TREC + 20 + 13 * k + 10:s * TREC + 20 + 13 * k + 13]      # swing leg's zero force hides from a finite z
            touched[[cp.HEAD + cp.LEG * k + cp.CLEAR, cp.HEAD + cp.LEG * k + cp.ROM]] = True
            touched[1], touched[2] = not np.isfinite(v) or f[1] != 0.0, not np.isfinite(v) or f[0] != 0.0
        elif kind == "force":     # f_e.z: f_n and cone of the leg, angular x and y, linear z
            touched[[1, 2, 6, cp.HEAD + cp.LEG * k + cp.FN, cp.HEAD + cp.LEG * k + cp.CONE]] = True
        else:                     # R: the angular residual and every leg's rom
            touched[[1, 2, 3] + [cp.HEAD + cp.LEG * e + cp.ROM for e in range(4)]] = True
        assert same_bits(got[s][~touched], was[s][~touched]).all(), (s, kind, "a field not made from the bad number changed")
        assert not same_bits(got[s][touched], was[s][touched]).any(), (s, kind, "every field made from it shows it")
        if np.isnan(v) or kind in ("quat", "quat0"):
            assert np.isnan(got[s][touched]).all(), (s, kind, v, got[s][touched].tolist())
        else:
            assert not (np.abs(got[s][touched]) < 1e200).any(), (s, kind, v, got[s][touched].tolist())
    r.assert_padding()
    sc = r.scores.cpu().numpy()[1]
    assert same_bits(sc, cp.fold(got, 4)).all() and sc[0] == 64
    assert np.isnan(sc[[1, 2, 7]]).all() and np.isnan(sc[3:7]).any(), sc.tolist()


@pytest.mark.gpu
def test_a_hostile_foothold_on_a_grid_map_stays_behind_the_range_checks_of_the_lookup():
    """the one index a record reaches is the cell lookup of the terrain, from p_e.x and p_e.y: NaN, +-Inf and +-1e300 in the x or the
    y of one foot of single samples of problem 1 of the `Grid` batch (as tests/test_start_device.py does for twr_batch_start).  No
    fault; outside the map the height is FLT_MAX, so the clearance is z - FLT_MAX; rom is NaN or huge; t, the linear residual, the
    contact flag and every other leg of the record, every other record and problem 0 keep the bits of the clean run; the scores
    are the fold of the records."""
    torch = _torch()
    clean = run("grid")
    r = Run(BATCHES["grid"][0], clean.dt, xs=clean.xs)
    traj = clean.traj.cpu().numpy().copy()
    n = clean.counts[1]
    rec = traj[r.tstride:r.tstride + n * TREC].reshape(n, TREC)
    sites = {}
    for i, v in enumerate(POISON):
        for j, axis in enumerate((0, 1)):
            s, k = 5 + 19 * i + 7 * j, (i + j) % 4
            sites[s] = (k, axis, v)
            rec[s, 21 + 13 * k + axis] = v
    assert max(sites) < n and len(sites) == 10
    r.traj.copy_(torch.from_numpy(traj))
    r.check()
    torch.cuda.synchronize()          # (a fault would raise here)
    assert same_bits(r.checks_of(0), clean.checks_of(0)).all() and same_bits(r.scores.cpu().numpy()[0], clean.scores.cpu().numpy()[0]).all()
    got, was = r.checks_of(1), clean.checks_of(1)
    hit = np.zeros(n, dtype=bool)
    hit[list(sites)] = True
    assert same_bits(got[~hit], was[~hit]).all()
    flt_max = float(np.finfo(np.float32).max)
    for s, (k, axis, v) in sites.items():
        touched = np.zeros(CREC, dtype=bool)
        touched[[1, 2, 3] + [cp.HEAD + cp.LEG * k + f for f in (cp.CLEAR, cp.FN, cp.CONE, cp.ROM)]] = True
        assert same_bits(got[s][~touched], was[s][~touched]).all(), (s, k, axis, v)
        rom, clear = got[s][cp.HEAD + cp.LEG * k + cp.ROM], got[s][cp.HEAD + cp.LEG * k + cp.CLEAR]
        assert not abs(rom) < 1e200, (s, v, rom)
        if not np.isnan(v):
            assert clear == rec[s, 23 + 13 * k] - flt_max, (s, v, clear)
    r.assert_padding()
    assert same_bits(r.scores.cpu().numpy()[1], cp.fold(got, 4)).all()


# ------------------------------------------------------------------ one and two feet (the kernels are instantiated per n_ee)
@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["monoped", "biped"])
def test_one_and_two_feet_equal_the_restatement_bit_for_bit(robot):
    """a monoped and a biped on Stairs, 201 samples each (items of 64, 64, 64 and 9 records), two problems: records, scores, padding"""
    from .common import hopper_schedule
    torch = _torch()
    c = Case(robot, "stairs", hopper_schedule() if robot == "monoped" else ta.gait_combo(2, 0, 2.0))
    n_ee = int(c.model.n_ee)
    assert n_ee == {"monoped": 1, "biped": 2}[robot]
    trec, crec, dt = 20 + 13 * n_ee, ta.check_rec(n_ee), 0.01
    xs = [c.x_perturbed(seed, goal_x=1.5, sigma=0.02) for seed in (0, 1)]
    batch = ta.Batch([c.S], [0, 0], device=0)
    n = c.S.sample_count(dt)
    assert n == 201
    tstride, cstride = n * trec + 3, n * crec + 5
    x = torch.from_numpy(np.concatenate(xs)).cuda()
    traj = torch.full((2 * tstride,), float("nan"), dtype=torch.float64, device="cuda")
    checks = torch.full((2 * cstride,), float("nan"), dtype=torch.float64, device="cuda")
    scores = torch.full((2, 8), -7.0, dtype=torch.float64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    batch.sample_device(x.data_ptr(), dt, traj.data_ptr(), tstride, st)
    batch.checks_device(c.model, traj.data_ptr(), tstride, dt, checks.data_ptr(), cstride, st)
    batch.check_scores_device(checks.data_ptr(), cstride, dt, scores.data_ptr(), st)
    torch.cuda.synchronize()
    t, k, sc = traj.cpu().numpy().reshape(2, tstride), checks.cpu().numpy().reshape(2, cstride), scores.cpu().numpy()
    for p in range(2):
        rec, got = t[p, :n * trec].reshape(n, trec), k[p, :n * crec].reshape(n, crec)
        want = cp.checks_numpy(rec, cp.consts_of(c.model), cp.oracle_terrain(c.P))
        assert np.isfinite(rec).all()
        eq = same_bits(got, want)
        assert eq.all(), (robot, p, np.argwhere(~eq)[:8].tolist())
        assert np.isnan(k[p, n * crec:]).all(), "nothing is written behind a problem's records"
        assert same_bits(sc[p], cp.fold(got, n_ee)).all() and sc[p][0] == n


# ------------------------------------------------------------------ 7: arguments
@pytest.mark.gpu
def test_argument_checks():
    torch = _torch()
    r = run("i_64")
    L, b = ta.lib(), r.batch._h
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    tr, ch, sc = (C.c_void_p(t.data_ptr()) for t in (r.traj, r.checks, r.scores))
    before_c, before_s = r.checks.clone(), r.scores.clone()

    def invalid(rc, word):
        msg = L.twr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg, word)

    off = lambda p: C.c_void_p(p.value + 4)
    m = C.byref(r.model)
    invalid(L.twr_batch_checks(None, m, tr, r.tstride, r.dt, ch, r.cstride, st), "null batch")
    invalid(L.twr_batch_checks(b, None, tr, r.tstride, r.dt, ch, r.cstride, st), "null model")
    invalid(L.twr_batch_checks(b, m, None, r.tstride, r.dt, ch, r.cstride, st), "null")
    invalid(L.twr_batch_checks(b, m, tr, r.tstride, r.dt, None, r.cstride, st), "null")
    invalid(L.twr_batch_checks(b, m, off(tr), r.tstride, r.dt, ch, r.cstride, st), "aligned")
    invalid(L.twr_batch_checks(b, m, tr, r.tstride, r.dt, off(ch), r.cstride, st), "aligned")
    invalid(L.twr_batch_checks(b, m, tr, 64 * TREC - 1, r.dt, ch, r.cstride, st), "traj_stride")
    invalid(L.twr_batch_checks(b, m, tr, r.tstride, r.dt, ch, 64 * CREC - 1, st), "check_stride")
    invalid(L.twr_batch_checks(b, m, tr, -1, r.dt, ch, r.cstride, st), "stride")
    invalid(L.twr_batch_checks(b, m, tr, r.tstride, r.dt, ch, -1, st), "stride")
    invalid(L.twr_batch_check_scores(None, ch, r.cstride, r.dt, sc, st), "null batch")
    invalid(L.twr_batch_check_scores(b, None, r.cstride, r.dt, sc, st), "null")
    invalid(L.twr_batch_check_scores(b, ch, r.cstride, r.dt, None, st), "null")
    invalid(L.twr_batch_check_scores(b, off(ch), r.cstride, r.dt, sc, st), "aligned")
    invalid(L.twr_batch_check_scores(b, ch, r.cstride, r.dt, off(sc), st), "aligned")
    invalid(L.twr_batch_check_scores(b, ch, 64 * CREC - 1, r.dt, sc, st), "check_stride")
    invalid(L.twr_batch_check_scores(b, ch, -1, r.dt, sc, st), "stride")
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        invalid(L.twr_batch_checks(b, m, tr, r.tstride, dt, ch, r.cstride, st), "dt")
        invalid(L.twr_batch_check_scores(b, ch, r.cstride, dt, sc, st), "dt")

    def model(**kw):
        k = ta.model_preset("go1", "flat")
        for name, (index, v) in kw.items():
            if index is None:
                setattr(k, name, v)
            elif isinstance(index, tuple):
                getattr(k, name)[index[0]][index[1]] = v
            else:
                getattr(k, name)[index] = v
        return C.byref(k)

    for kw, word in ((dict(n_ee=(None, 2)), "n_ee"), (dict(n_ee=(None, 0)), "n_ee"), (dict(n_ee=(None, 5)), "n_ee"),
                     (dict(nominal_stance=((2, 1), float("nan"))), "nominal_stance"), (dict(nominal_stance=((0, 0), float("inf"))), "nominal_stance"),
                     (dict(max_dev=(1, float("nan"))), "max_dev"), (dict(max_dev=(0, -0.01)), "max_dev"), (dict(max_dev=(2, float("inf"))), "max_dev"),
                     (dict(force_limit=(None, float("nan"))), "force_limit"), (dict(force_limit=(None, -float("inf"))), "force_limit")):
        invalid(L.twr_batch_checks(b, model(**kw), tr, r.tstride, r.dt, ch, r.cstride, st), word)
    torch.cuda.synchronize()
    assert same_bits(before_c.cpu().numpy(), r.checks.cpu().numpy()).all() and torch.equal(before_s, r.scores), "a refused call writes nothing"
    # the tightest strides are accepted: the records of problem 0 alone, through a one-problem batch
    one = Run(("c1_2.0",), r.dt, xs=[r.xs[0]])
    one.tstride, one.cstride = 64 * TREC, 64 * CREC
    one.done()
    assert same_bits(one.checks.cpu().numpy()[:64 * CREC], r.checks_of(0).reshape(-1)).all()
    assert same_bits(one.scores.cpu().numpy()[0], r.scores.cpu().numpy()[0]).all()
