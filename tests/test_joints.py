"""twr_batch_joints, twr_batch_joint_scores and twr_batch_eval_joint_scores through the C ABI, on Go1 with the preset descriptor.

Batches (at most four problems each), chosen for the round boundaries of the one-wave-per-problem fold (64 samples a round):
  (i)    gait combo C1 on flat ground, dt such that twr_structure_sample_count is exactly 64: one full round
  (ii)   two structures in one batch with 65 and 129 samples: one sample into the second and the third round, where the
         previous sample's angles are carried from lane 63
  (iii)  an optimised-timings structure (durations from x)
  (iv)   dt > T: one sample, no velocity
References
  joint records   a numpy restatement on the device's own trajectory records: R(q)^T (p - b) in the device's order of plainly
                  rounded operations (the kernels do not contract them, so the hip-frame foot is the same double), then
                  tests/ik_points.py ik_numpy, which tests/test_ik_ref.py pins to the reference's recording.  Angles within the
                  bound of that file (C_IK), flags and over-reach equal; the x used keeps every foot in the interior class.
  scores          a numpy fold of the device's joint records: counts and [7] exact, [3] - [5] bit-equal (max, min and a single
                  division are order-free)
  fused call      the three-call composition, bit for bit"""
import ctypes as C
import functools

import numpy as np
import pytest

import towr_amd as ta

from . import ik_points as ip
from .common import Case
from .test_ik_ref import angle_bounds, same_bits

DT2 = 0.02


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def kin():
    return ta.leg_kinematics_preset("go1")


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
    raise KeyError(name)


def gentle_x(c, seed):
    """the interpolated initial guess over 5 cm with small noise: every foot stays in the interior class"""
    x = c.x_guess(goal_x=0.05)
    rng = np.random.default_rng(4100 + seed)
    scale = np.ones(c.S.n)
    for vs in c.S.var_sets:
        a, b = vs["offset"], vs["offset"] + vs["size"]
        if vs["name"] == "base-lin":
            scale[a:b] = np.tile([0.01] * 3 + [0.05] * 3, vs["size"] // 6)
        elif vs["name"] == "base-ang":
            scale[a:b] = np.tile([0.05] * 3 + [0.1] * 3, vs["size"] // 6)
        elif vs["name"].startswith("ee-motion"):
            scale[a:b] = 0.01
        elif vs["name"].startswith("ee-schedule"):
            scale[a:b] = 0.01
        else:
            scale[a:b] = 10.0
    return x + rng.normal(size=c.S.n) * scale


def dt_for(S, n, T):
    dt = T / (n - 0.5)
    assert S.sample_count(dt) == n
    return dt


BATCHES = {
    "i_64": (("c1_2.0", "c1_2.0"), lambda cs: dt_for(cs[0].S, 64, 2.0)),
    "ii_65_129": (("c0_65", "c1_129", "c0_65"), lambda cs: DT2),
    "iii_timings": (("timings", "timings"), lambda cs: 0.01),
    "iv_one_sample": (("c1_2.0", "c0_65"), lambda cs: 3.0),
}


class Run:
    """one batch on the device with its x: trajectory records, joint records, scores of the composition and of the fused call"""

    def __init__(self, names, dt, xs=None, seed0=0):
        torch = _torch()
        self.cases = [case(n) for n in names]
        structs, index = [], []
        for c in self.cases:
            if c.S not in structs:
                structs.append(c.S)
            index.append(structs.index(c.S))
        self.batch = ta.Batch(structs, index, device=0)
        self.dt = float(dt)
        self.xs = [gentle_x(c, seed0 + p) for p, c in enumerate(self.cases)] if xs is None else xs
        self.counts = [c.S.sample_count(self.dt) for c in self.cases]
        self.n_max = max(self.counts)
        self.trec, self.jrec = 20 + 13 * 4, ta.joint_rec(4)
        self.tstride, self.jstride = self.n_max * self.trec + 3, self.n_max * self.jrec + 5      # (not the tightest strides)
        n = len(self.cases)
        self.x = torch.from_numpy(np.concatenate(self.xs)).cuda()
        self.traj = torch.full((n * self.tstride,), float("nan"), dtype=torch.float64, device="cuda")
        self.joints = torch.full((n * self.jstride,), float("nan"), dtype=torch.float64, device="cuda")
        self.scores = torch.full((n, 8), -7.0, dtype=torch.float64, device="cuda")
        self.fused = torch.full((n, 8), -9.0, dtype=torch.float64, device="cuda")

    def compose(self, st=None):
        torch = _torch()
        st = torch.cuda.current_stream().cuda_stream if st is None else st
        b, k = self.batch, kin()
        b.sample_device(self.x.data_ptr(), self.dt, self.traj.data_ptr(), self.tstride, st)
        b.joints_device(k, self.traj.data_ptr(), self.tstride, self.dt, self.joints.data_ptr(), self.jstride, st)
        b.joint_scores_device(k, self.joints.data_ptr(), self.jstride, self.dt, self.scores.data_ptr(), st)

    def fuse(self, st=None):
        torch = _torch()
        st = torch.cuda.current_stream().cuda_stream if st is None else st
        self.batch.eval_joint_scores_device(kin(), self.x.data_ptr(), self.dt, self.fused.data_ptr(), st)

    def both(self):
        self.compose()
        self.fuse()
        _torch().cuda.synchronize()
        return self

    def traj_of(self, p):
        return self.traj.cpu().numpy()[p * self.tstride:p * self.tstride + self.counts[p] * self.trec].reshape(-1, self.trec)

    def joints_of(self, p):
        return self.joints.cpu().numpy()[p * self.jstride:p * self.jstride + self.counts[p] * self.jrec].reshape(-1, self.jrec)


@functools.lru_cache(maxsize=None)
def run(name):
    names, dt = BATCHES[name]
    return Run(names, dt([case(n) for n in names])).both()


def frame_rotation(q):
    """R[3][3] of arrays (n,): base_frame_rotation (kernels/joints.h) on quaternions q (n, 4) w x y z, in the device's order of
    plainly rounded operations; a norm that is not finite gives NaN like a norm of 0"""
    with np.errstate(all="ignore"):
        w, x, y, z = (np.array(q[:, i], dtype=np.float64) for i in range(4))
        n = np.sqrt(x * x + y * y + z * z + w * w)
        n = np.where(n < np.inf, n, n - n)
        w, x, y, z = w / n, x / n, y / n, z / n
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
        return [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def frame_vector(R, p_base, p_ee):
    """(n, 3): base_frame (kernels/joints.h) on frame_rotation's R and points (n, 3)"""
    with np.errstate(all="ignore"):
        d = p_ee - p_base
        return np.column_stack([R[0][i] * d[:, 0] + R[1][i] * d[:, 1] + R[2][i] * d[:, 2] for i in range(3)])


def hip_feet(traj):
    """[n, 4, 3] hip-frame feet of trajectory records, in the device's order of operations (kernels/joints.h base_frame_rotation,
    base_frame, leg_ik_of_foot)"""
    R = frame_rotation(traj[:, 10:14])
    out = np.empty((len(traj), 4, 3))
    for e in range(4):
        out[:, e] = frame_vector(R, traj[:, 1:4], traj[:, 21 + 13 * e:24 + 13 * e])
    return out * ip.MIRROR[None] - ip.BASE_TO_HIP[None, None]


def over_reach(r):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(r), r, np.maximum(np.maximum(r - (ip.LU + ip.LL), abs(ip.LU - ip.LL) - r), 0.0))


def fold(joints, dt):
    """the eight scores of one problem's joint records [n, 1 + 5 * 4]"""
    legs = joints[:, 1:].reshape(len(joints), 4, 5)
    q, fl, ov = legs[:, :, :3], legs[:, :, 3].astype(np.int64), legs[:, :, 4]
    nanmax = lambda a, empty: (np.nan if np.isnan(a).any() else float(a.max())) if a.size else empty
    unreach = (fl & 3) != 0
    with np.errstate(all="ignore"):
        vel = np.abs(q[1:] - q[:-1]) / dt
        margin = np.minimum(q - ip.Q_MIN, ip.Q_MAX - q).min(axis=2)[fl == 0]
    first = np.nonzero(unreach.any(axis=1))[0]
    return np.array([len(joints), unreach.sum(), ((fl & 28) != 0).sum(), nanmax(ov, 0.0), nanmax(vel, 0.0),
                     (np.nan if np.isnan(margin).any() else float(margin.min())) if margin.size else 1e20,
                     ((fl & 32) != 0).sum(), first[0] if first.size else -1.0], dtype=np.float64)


# ------------------------------------------------------------------ records, scores, the fused call
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_joint_records_equal_the_numpy_restatement(name):
    r = run(name)
    assert r.counts == {"i_64": [64, 64], "ii_65_129": [65, 129, 65], "iii_timings": r.counts, "iv_one_sample": [1, 1]}[name]
    worst = 0.0
    for p in range(len(r.cases)):
        traj, got = r.traj_of(p), r.joints_of(p)
        assert np.isfinite(traj).all() and same_bits(got[:, 0], traj[:, 0]).all()
        hip = hip_feet(traj).reshape(-1, 3)
        q, fl, cb, cg, rr = ip.ik_numpy(hip, np.tile(ip.KNEE_BEND, len(traj)))
        assert (fl == 0).all() and (rr >= 0.05).all() and (rr <= 0.42).all() and (np.abs(cb) <= 0.999).all() and (np.abs(cg) <= 0.999).all(), \
            "the test's x leaves the interior class"
        legs = got[:, 1:].reshape(-1, 5)
        assert np.array_equal(legs[:, 3], fl.astype(np.float64)) and same_bits(legs[:, 4], over_reach(rr)).all()
        err, bound = np.abs(legs[:, :3] - q), angle_bounds(cb, cg)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
    pad = r.joints.cpu().numpy().reshape(len(r.cases), r.jstride)
    for p, n in enumerate(r.counts):
        assert np.isnan(pad[p, n * r.jrec:]).all(), "nothing is written behind a problem's records"
    print("\n%s: joint records within %.4f of the bound" % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_scores_equal_the_numpy_fold_and_the_fused_call_the_composition(name):
    r = run(name)
    got, fused = r.scores.cpu().numpy(), r.fused.cpu().numpy()
    for p in range(len(r.cases)):
        want = fold(r.joints_of(p), r.dt)
        assert same_bits(got[p], want).all(), (name, p, got[p].tolist(), want.tolist())
        assert got[p][0] == r.counts[p] and got[p][1] == 0 and got[p][7] == -1 and got[p][5] < 1e20
        assert (got[p][4] > 0) == (r.counts[p] > 1)
    assert same_bits(fused, got).all(), (name, fused.tolist(), got.tolist())


@pytest.mark.gpu
def test_same_bits_in_another_slot_of_another_batch():
    a = run("ii_65_129")
    names = ("c1_2.0", "c1_129", "timings", "c0_65")        # problem 1 of (ii) now sits in slot 1 behind another structure, ...
    xs = [gentle_x(case(names[0]), 50), a.xs[1], gentle_x(case(names[2]), 51), a.xs[0]]      # ... its problem 0 in slot 3
    b = Run(names, DT2, xs=xs).both()
    for src, dst in ((1, 1), (0, 3)):
        assert same_bits(b.fused.cpu().numpy()[dst], a.fused.cpu().numpy()[src]).all()
        assert same_bits(b.scores.cpu().numpy()[dst], a.scores.cpu().numpy()[src]).all()
        assert same_bits(b.joints_of(dst), a.joints_of(src)).all()


@pytest.mark.gpu
def test_graph_replay_on_a_new_x():
    torch = _torch()
    names, dt = BATCHES["ii_65_129"]
    r = Run(names, DT2, seed0=20).both()            # (warm: the sample work list exists before the capture)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        r.fuse(s.cuda_stream)
        r.compose(s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = torch.cuda.current_stream().cuda_stream
        r.fuse(st)
        r.compose(st)
    xs2 = [gentle_x(c, 30 + p) for p, c in enumerate(r.cases)]
    r.x.copy_(torch.from_numpy(np.concatenate(xs2)))
    r.fused.fill_(-1.0)
    r.scores.fill_(-2.0)
    graph.replay()
    torch.cuda.synchronize()
    replayed_f, replayed_s = r.fused.cpu().numpy().copy(), r.scores.cpu().numpy().copy()
    eager = Run(names, DT2, xs=xs2).both()
    assert same_bits(replayed_f, eager.fused.cpu().numpy()).all() and same_bits(replayed_s, eager.scores.cpu().numpy()).all()
    assert not same_bits(replayed_f, run("ii_65_129").fused.cpu().numpy()).all()


# ------------------------------------------------------------------ an unreachable foothold, hostile x
def first_node_z(c, ee):
    """index into x of the z of foot ee's first ee-motion node: the third column of the first row of terrain-ee-motion_<ee>"""
    S = c.S
    cs = [s for s in S.con_sets if s["name"] == "terrain-ee-motion_%d" % ee][0]
    cols = S.col_idx[S.row_ptr[cs["offset"]]:S.row_ptr[cs["offset"] + 1]]
    assert len(cols) == 3
    return int(cols[2])


@pytest.mark.gpu
def test_a_provoked_over_reach_is_found_and_stays_in_its_problem():
    clean = run("i_64")
    c = clean.cases[1]
    xs = [clean.xs[0].copy(), clean.xs[1].copy()]
    base_z = 0.3                                  # the hip's height in the guess: the first node goes 0.6 m below it
    xs[1][first_node_z(c, 2)] = base_z - 0.6
    r = Run(BATCHES["i_64"][0], clean.dt, xs=xs).both()
    got, fused = r.scores.cpu().numpy(), r.fused.cpu().numpy()
    assert same_bits(got, fused).all()
    assert same_bits(got[0], clean.scores.cpu().numpy()[0]).all(), "the other problem keeps the bits of the clean run"
    assert got[1][1] > 0 and got[1][7] == 0, got[1].tolist()
    hip = hip_feet(r.traj_of(1))[0, 2]
    excess = float(np.sqrt(hip[0] ** 2 + hip[1] ** 2 + hip[2] ** 2) - (ip.LU + ip.LL))
    assert 0.1 < excess < 0.3 and got[1][3] >= excess * (1 - 1e-12), (excess, got[1][3])
    assert same_bits(got[1], fold(r.joints_of(1), r.dt)).all()
    legs = r.joints_of(1)[0, 1:].reshape(4, 5)
    assert int(legs[2, 3]) & 3 == 3 and same_bits(legs[2, 2], 0.0) and abs(legs[2, 4] - excess) <= 1e-12


@pytest.mark.gpu
def test_hostile_x_is_contained_in_its_problem():
    """bad numbers in one problem's x: no fault, that problem reports them -- NaN node values as NaN leg-samples or NaN maxima,
    +-1e300 as an infinite over-reach (measured: [1] = 499 unreachable leg-samples, [3] = inf, [6] = 0: no angle is NaN there,
    by the reference's own clamp) -- and the others keep their bits (containment, as test_hostile_x_is_contained of the
    evaluation kernels)"""
    clean = run("ii_65_129")
    for kind, value in enumerate((np.nan, 1e300, -1e300)):
        xs = [x.copy() for x in clean.xs]
        S = clean.cases[1].S
        rng = np.random.default_rng(600 + kind)
        for vs in S.var_sets:
            if vs["name"] in ("base-lin", "base-ang") or vs["name"].startswith("ee-motion"):
                hit = vs["offset"] + rng.choice(vs["size"], size=max(2, vs["size"] // 8), replace=False)
                xs[1][hit] = value
        r = Run(BATCHES["ii_65_129"][0], DT2, xs=xs).both()
        got, fused = r.scores.cpu().numpy(), r.fused.cpu().numpy()
        assert same_bits(got, fused).all()
        for p in (0, 2):
            assert same_bits(got[p], clean.scores.cpu().numpy()[p]).all()
        assert got[1][0] == 129
        if np.isnan(value):
            assert got[1][6] > 0 or np.isnan(got[1][3:6]).any(), got[1].tolist()
        else:
            # +-1e300 stays finite through the splines and the frame change; the squares overflow in the leg IK: r = Inf, the HFE
            # cosine Inf / Inf is the reference's NaN -> +1, the KFE cosine -Inf -> -1, so every angle is finite by the
            # reference's own rules and the bad number surfaces as an infinite over-reach of unreachable legs
            assert got[1][3] == np.inf and got[1][1] > 0 and got[1][7] >= 0, got[1].tolist()
        assert same_bits(got[1], fold(r.joints_of(1), r.dt)).all()


# ------------------------------------------------------------------ the quaternion of the records
def joints_of_edited_records(clean, edit):
    """(a Run on clean's batch shape whose trajectory records are clean's with `edit(records of problem p, p)` applied, after
    twr_batch_joints and twr_batch_joint_scores on them)"""
    torch = _torch()
    r = Run(BATCHES["i_64"][0], clean.dt, xs=clean.xs)
    traj = clean.traj.cpu().numpy().copy()
    for p, n in enumerate(clean.counts):
        edit(traj[p * clean.tstride:p * clean.tstride + n * clean.trec].reshape(n, clean.trec), p)
    r.traj.copy_(torch.from_numpy(traj))
    st = torch.cuda.current_stream().cuda_stream
    r.batch.joints_device(kin(), r.traj.data_ptr(), r.tstride, r.dt, r.joints.data_ptr(), r.jstride, st)
    r.batch.joint_scores_device(kin(), r.joints.data_ptr(), r.jstride, r.dt, r.scores.data_ptr(), st)
    torch.cuda.synchronize()
    return r


@pytest.mark.gpu
def test_joints_ignore_the_sign_and_a_power_of_two_of_the_quaternion():
    """q and -q are one rotation and every product of the frame change is even in q; the normalisation is exact under a power of
    two (the squares, their sum, the root and the quotients scale without rounding): the joint records keep every bit"""
    clean = run("i_64")

    def edit(rec, p):
        s = np.arange(len(rec))
        rec[s % 2 == 1, 10:14] *= -1.0
        rec[(s // 2) % 3 == 1, 10:14] *= 2.0
        rec[(s // 2) % 3 == 2, 10:14] *= 0.5
        assert (s % 2 == 1).sum() == len(rec) // 2

    r = joints_of_edited_records(clean, edit)
    assert not same_bits(r.traj.cpu().numpy(), clean.traj.cpu().numpy()).all()
    assert same_bits(r.joints.cpu().numpy(), clean.joints.cpu().numpy()).all()
    assert same_bits(r.scores.cpu().numpy(), clean.scores.cpu().numpy()).all()


HOSTILE_Q = {3: (0.0, 0.0, 0.0, 0.0), 17: (np.nan, 0.1, 0.2, 0.3), 18: (0.9, 0.1, np.nan, 0.3), 31: (np.inf, 0.1, 0.2, 0.3),
             32: (0.9, -np.inf, 0.2, 0.3), 45: (1e200, 1e200, 1e200, 1e200), 46: (0.9, 0.1, 0.2, 1e200), 62: (1e-200, 1e-200, 1e-200, 1e-200),
             63: (0.0, 1e-200, 0.0, 0.0)}


@pytest.mark.gpu
def test_a_quaternion_that_cannot_be_normalised_is_flagged_and_stays_in_its_sample():
    """zero, NaN, Inf, 1e200 (the squares overflow) and 1e-200 (they underflow to a norm of 0) in the quaternion of some records
    of problem 1: every leg of those samples carries the NaN flag and NaN angles, every other sample and problem 0 keep the bits
    of the clean run, and nothing is written behind a problem's records"""
    clean = run("i_64")

    def edit(rec, p):
        if p == 1:
            for s, q in HOSTILE_Q.items():
                rec[s, 10:14] = q

    r = joints_of_edited_records(clean, edit)
    assert same_bits(r.joints_of(0), clean.joints_of(0)).all()
    got, was = r.joints_of(1), clean.joints_of(1)
    hit = np.zeros(len(got), dtype=bool)
    hit[list(HOSTILE_Q)] = True
    assert same_bits(got[~hit], was[~hit]).all() and same_bits(got[:, 0], was[:, 0]).all()
    legs = got[hit][:, 1:].reshape(-1, 5)
    assert ((legs[:, 3].astype(np.int64) & 32) != 0).all(), legs[:, 3].tolist()
    assert np.isnan(legs[:, :3]).any(axis=1).all()
    pad = r.joints.cpu().numpy().reshape(len(r.cases), r.jstride)
    for p, n in enumerate(r.counts):
        assert np.isnan(pad[p, n * r.jrec:]).all(), "nothing is written behind a problem's records"
    sc, sc0 = r.scores.cpu().numpy(), clean.scores.cpu().numpy()
    assert same_bits(sc[0], sc0[0]).all()
    assert sc[1][6] == 4 * len(HOSTILE_Q) and same_bits(sc[1], fold(got, r.dt)).all(), sc[1].tolist()


# ------------------------------------------------------------------ argument checks
@pytest.mark.gpu
def test_argument_checks():
    torch = _torch()
    r = run("i_64")
    L, b, k = ta.lib(), r.batch._h, kin()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x, tr, jo, sc = (C.c_void_p(t.data_ptr()) for t in (r.x, r.traj, r.joints, r.fused))
    before = r.fused.clone()

    def invalid(rc, word):
        msg = L.twr_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    off = lambda p: C.c_void_p(p.value + 4)
    kp = C.byref(k)
    invalid(L.twr_batch_eval_joint_scores(b, kp, None, r.dt, sc, st), "null")
    invalid(L.twr_batch_eval_joint_scores(b, kp, x, r.dt, None, st), "null")
    invalid(L.twr_batch_eval_joint_scores(None, kp, x, r.dt, sc, st), "null batch")
    invalid(L.twr_batch_eval_joint_scores(b, None, x, r.dt, sc, st), "null kin")
    invalid(L.twr_batch_eval_joint_scores(b, kp, off(x), r.dt, sc, st), "aligned")
    invalid(L.twr_batch_eval_joint_scores(b, kp, x, r.dt, off(sc), st), "aligned")
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        invalid(L.twr_batch_eval_joint_scores(b, kp, x, dt, sc, st), "dt")
        invalid(L.twr_batch_joints(b, kp, tr, r.tstride, dt, jo, r.jstride, st), "dt")
        invalid(L.twr_batch_joint_scores(b, kp, jo, r.jstride, dt, sc, st), "dt")
    invalid(L.twr_batch_joints(b, kp, None, r.tstride, r.dt, jo, r.jstride, st), "null")
    invalid(L.twr_batch_joints(b, kp, tr, r.tstride, r.dt, None, r.jstride, st), "null")
    invalid(L.twr_batch_joints(b, kp, off(tr), r.tstride, r.dt, jo, r.jstride, st), "aligned")
    invalid(L.twr_batch_joints(b, kp, tr, 64 * r.trec - 1, r.dt, jo, r.jstride, st), "traj_stride")
    invalid(L.twr_batch_joints(b, kp, tr, r.tstride, r.dt, jo, 64 * r.jrec - 1, st), "joint_stride")
    invalid(L.twr_batch_joints(b, kp, tr, -1, r.dt, jo, r.jstride, st), "stride")
    invalid(L.twr_batch_joint_scores(b, kp, None, r.jstride, r.dt, sc, st), "null")
    invalid(L.twr_batch_joint_scores(b, kp, jo, r.jstride, r.dt, off(sc), st), "aligned")
    invalid(L.twr_batch_joint_scores(b, kp, jo, 64 * r.jrec - 1, r.dt, sc, st), "joint_stride")
    two = ta.leg_kinematics_preset("go1")
    two.n_ee = 2
    for rc in (L.twr_batch_eval_joint_scores(b, C.byref(two), x, r.dt, sc, st), L.twr_batch_joints(b, C.byref(two), tr, r.tstride, r.dt, jo, r.jstride, st),
               L.twr_batch_joint_scores(b, C.byref(two), jo, r.jstride, r.dt, sc, st)):
        invalid(rc, "n_ee")
    bad = ta.leg_kinematics_preset("go1")
    bad.length_shank = float("nan")
    invalid(L.twr_batch_eval_joint_scores(b, C.byref(bad), x, r.dt, sc, st), "length_shank")
    torch.cuda.synchronize()
    assert torch.equal(before, r.fused), "a refused call writes nothing"
    # the tightest strides are accepted
    assert L.twr_batch_joint_scores(b, kp, jo, r.jstride, r.dt, sc, st) == 0
    torch.cuda.synchronize()
    assert same_bits(r.fused.cpu().numpy(), r.scores.cpu().numpy()).all()
