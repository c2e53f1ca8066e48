"""The attitude of the base on every branch and tie: quat_of_rotation, base_frame_rotation and base_frame (kernels/joints.h) and
sample_angular (kernels/sample.h), against the reference's recorded answers, a numpy restatement and mpmath.

tests/attitude_probe.hip is a stand-alone program that includes those two headers and what they include, nothing else of the
product; it is compiled here with the product's CXXFLAGS for util_tu.o, started as a fresh child process per mode and fed the
points of tests/attitude_points.py (its docstring lists the groups).

References
  quat     tests/golden/refattitude.npz quat_q: Eigen::Quaterniond(R) of the Eigen that built ref_dump, recorded by
           oracle/ref_golden.py --attitude through ref_dump --attitude-points.  reference_deps names that Eigen; with the subset
           under oracle/ref_dump/subset it is this project's own statement of the conversion.  attitude_points.quat_of_rotation is
           the same statement in numpy, in the device's order; all three sum the trace as (m00 + m11) + m22.
  euler    the same file: the reference's own EulerConverter (rotation matrix, quaternion, angular velocity and acceleration) on
           the state its NodeSpline returned, which is also the probe's input; and mpmath at 40 digits on those doubles.
  frame    no reference code exists; frame_rotation / frame_vector of tests/test_joints.py restate the source in numpy, mpmath gives
           the exact rotation by the normalised quaternion.

Bounds, with u = 2^-53 and every rounded operation costing a relative u
  q of an orthogonal R   The input is an exact rotation R* of a unit quaternion q* whose entries were rounded once: |R - R*| <= u per
           entry.  The argument of the square root is 4 q_i^2 in exact arithmetic (q_i = w on the trace branch); it collects 3 u
           from the three diagonal entries, 2 u + 3 u from the two sums of the diagonal and 4 u from the + 1.0: 12 u absolute.  The
           branch rules give 4 q_i^2 >= 1 (trace > 0 is w^2 > 1/4; otherwise q_i is the largest of x, y, z and w^2 <= 1/4, so
           q_i^2 >= (1 - 1/4) / 3), so the root is off by 6 u relative plus its own u, q_i = 0.5 * root likewise, 0.5 / root by 8 u.
           Another component is (a - b) * (0.5 / root) with a -+ b = 4 q_i q_j exactly: 2 u from the entries and 2 u from the
           rounded difference, halved by 0.5 / root <= 1/2, plus (8 + 1) u of a product that is at most 1: 11 u.  C_Q = 12 leaves
           one u for the second-order terms and the ulp by which a moved entry can shift the branch rule.
             |q| = 1:   | |q|^2 - 1 | <= 2 |q*| |d| <= 2 * 2 C_Q u = 4 C_Q u       (|d| <= sqrt(4) C_Q u in the 2-norm)
             R(q / |q|) against the input:   normalising at most doubles the distance to q* (4 C_Q u in the 2-norm), every entry
             of R(q) on unit quaternions has a gradient of norm 2, and the input itself is u off: (8 C_Q + 1) u per entry.
  omega, omega_dot   per component C * u * sum |terms| + TINY, the terms being the monomials of euler_converter.cc:133-166 with exact
           sines and cosines.  A sine or cosine within k ulp is within 2 k u relative.  The longest term of omega, cy cz xd, has
           two of them and two products, and a row has at most three terms in whatever order (two additions): C = 4 k + 4.  The
           longest term of omega_dot, cz sy yd xd, has two, three products and the subtraction inside Mdot, and a row has five
           terms (four additions): C = 4 k + 8.  The reference calls libm (k = 1: C = 8 and 12); the device calls sincos_fast, for
           which tests/test_trig_probe.py asserts k = ULP_FAST below 1e5 and ULP_LIB above (C' = 12 and 16, 20 and 24 for a far
           angle).  Contraction into fused multiply-adds only removes roundings, so the bound holds for the probe's and for the
           kernels' choice of fusing alike.  TINY = 16 * 2^-1074 covers products that underflow (rates of 1e-300).
  frame    n^2 = x^2 + y^2 + z^2 + w^2 is a sum of positive terms, 4 u relative; the root 3 u; a component / n 4 u; a product of two
           components times two 9 u.  A diagonal entry 1 - (a + b): the sum 10 u of at most 2, and u from the subtraction: 21 u.
           An off-diagonal entry a -+ b with |a| + |b| <= 1: 9 u and u from the sum.  C_FR = 21 per entry of R.
           The vector: d = p_ee - p_base costs u per component, every product R_ki d_k (C_FR + 2) u |d_k|, the two additions 2 u
           of sum |d_k|: C_FV = 25 times u times the 1-norm of d, plus TINY.

The GPU tests print the worst case they measured as a fraction of each bound (run with -s); DESIGN section 5 "Base attitude" quotes
them."""
import functools
import glob
import os

import numpy as np
import pytest

from . import attitude_points as ap
from .probe import GOLDEN, Probe, bits, load_fixture
from .test_joints import frame_rotation, frame_vector
from .test_trig_probe import SWITCH, ULP_FAST, ULP_LIB

U = 2.0 ** -53
TINY = 16 * 2.0 ** -1074
C_Q = 12.0
C_NORM, C_BACK = 4 * C_Q, 8 * C_Q + 1
C_OMEGA = lambda k: 4 * k + 4
C_OMEGA_DOT = lambda k: 4 * k + 8
C_FR, C_FV = 21.0, 25.0
C_ROT = 9.0              # an entry of the reference's rotation matrix, counted in test_recorded_rotations_against_mpmath
# How close to a branch boundary the reference's R must be where the device takes another branch: an entry of the device's R is
# within ROT_TOL = 16 u of the exact one (tests/test_trig_probe.py), one of the reference's within 2 C_ROT u; the trace adds three
# entries and two roundings of a sum of at most 3, the difference of two diagonal entries two entries and one rounding
FLIP_TRACE = 3 * (16 + 2 * C_ROT) + 6
FLIP_DIAGONAL = 2 * (16 + 2 * C_ROT) + 2
ORTHOGONAL = ("cube", "small_w", "random")     # exact rotations rounded once per entry
PROBE = Probe("attitude_probe")


def fixture():
    return load_fixture("refattitude")


def _mp():
    import mpmath
    mpmath.mp.dps = 40
    return mpmath


def same(a, b):
    """bit for bit, a NaN being equal to a NaN of any payload"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.isnan(a) & np.isnan(b)) | (bits(a) == bits(b))


def probe_input(rows):
    return np.concatenate([[float(len(rows))], np.asarray(rows, dtype=np.float64).ravel()])


def _input(mode):
    return probe_input({"quat": lambda: ap.points()["quat"], "euler": lambda: fixture()["euler_state"], "frame": lambda: ap.points()["frame"]}[mode]())


def _probe(mode):
    """the probe's raw output for `mode`, from a child process of its own (the failure rule of tests/probe.py)"""
    return PROBE.run(mode, _input(mode))


@functools.lru_cache(maxsize=None)
def restated():
    """(q (n, 4) x y z w, branch (n,)) of the numpy restatement at the quat points"""
    q, b = ap.quats(ap.points()["quat"])
    q.flags.writeable = False
    return q, b


@functools.lru_cache(maxsize=None)
def angular_reference():
    """per state of the fixture (omega (3 mpf), sum |terms| (3), omega_dot (3), sum |terms| (3)): euler_converter.cc:133-166 in
    mpmath on the recorded doubles"""
    mp = _mp()
    out = []
    for s in fixture()["euler_state"]:
        y, z = mp.mpf(float(s[1])), mp.mpf(float(s[2]))
        xd, yd, zd, xa, ya, za = (mp.mpf(float(v)) for v in s[3:])
        sy, cy, sz, cz = mp.sin(y), mp.cos(y), mp.sin(z), mp.cos(z)
        w = [[cy * cz * xd, -sz * yd], [cy * sz * xd, cz * yd], [-sy * xd, zd]]
        wd = [[-cz * sy * yd * xd, -cy * sz * zd * xd, -cz * zd * yd, cy * cz * xa, -sz * ya],
              [cy * cz * zd * xd, -sy * sz * yd * xd, -sz * zd * yd, cy * sz * xa, cz * ya],
              [-cy * yd * xd, -sy * xa, za]]
        out.append(([mp.fsum(t) for t in w], [mp.fsum(abs(v) for v in t) for t in w],
                    [mp.fsum(t) for t in wd], [mp.fsum(abs(v) for v in t) for t in wd]))
    return out


def angular_worst(omega, omega_dot, ulps):
    """the worst error of omega and of omega_dot (n, 3) as fractions of C(k) u sum |terms| + TINY, k = ulps[i] per state"""
    mp = _mp()
    worst = [0.0, 0.0]
    for i, (w, sw, wd, swd) in enumerate(angular_reference()):
        for which, got, ref, terms, c in ((0, omega[i], w, sw, C_OMEGA(ulps[i])), (1, omega_dot[i], wd, swd, C_OMEGA_DOT(ulps[i]))):
            for d in range(3):
                frac = float(abs(mp.mpf(float(got[d])) - ref[d]) / (c * U * terms[d] + TINY))
                worst[which] = max(worst[which], frac)
    return worst


def back_and_norm(R, q):
    """(worst |R(q / |q|) - R| over the entries, | |q|^2 - 1 |) in units of u, in mpmath; q is x y z w"""
    mp = _mp()
    x, y, z, w = (mp.mpf(float(v)) for v in q)
    n = w * w + x * x + y * y + z * z
    back = [n - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), n - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), n - 2 * (x * x + y * y)]
    return float(max(abs(b / n - mp.mpf(float(r))) for b, r in zip(back, R)) / U), float(abs(n - 1) / U)


# ------------------------------------------------------------------ CPU tier
def test_probe_compiles_without_warning():
    """(CPU tier) hipcc compiles and links the probe for gfx950 with the product's flags, without a GPU and without a warning;
    the input parser refuses a file whose count does not match before anything reaches a device"""
    PROBE.refuses([], None, "usage")
    PROBE.refuses(["attitude"], _input("quat"), "usage")
    for mode in ("quat", "euler", "frame"):
        data = _input(mode)
        PROBE.refuses([mode], data[:-1], "truncated")
        PROBE.refuses([mode], np.concatenate([data, [0.0]]), "trailing data")
        PROBE.refuses([mode], np.concatenate([[0.0], data[1:]]), "point count")
        PROBE.refuses([mode], np.concatenate([[np.nan], data[1:]]), "point count")
    PROBE.refuses(["quat"], np.concatenate([[1.5], np.zeros(9)]), "point count")
    PROBE.refuses(["frame"], np.zeros(0), "truncated")


def test_points_cover_what_they_claim():
    """(CPU tier) the groups hold what the docstring of tests/attitude_points.py says"""
    p = ap.points()
    R, (q, branch) = p["quat"], restated()
    assert 1500 <= len(R) <= 4000 and 1500 <= len(p["euler"]) <= 4000 and 3000 <= len(p["frame"]) <= 8000
    cube = R[ap.group("quat", "cube")]
    assert len(cube) == 24 and set(np.unique(cube)) == {-1.0, 0.0, 1.0}
    for m in cube.reshape(-1, 3, 3):
        assert np.array_equal(m @ m.T, np.eye(3)) and np.linalg.det(m) > 0
    diag = cube[:, [0, 4, 8]]
    assert (np.abs(diag).sum(axis=1) == 0).sum() == 8, "trace 0 and a triple tie at once"
    half = diag.sum(axis=1) == -1
    assert (half & (np.sort(diag, axis=1)[:, 1] == np.sort(diag, axis=1)[:, 2])).sum() == 6, "half turns with two tied largest entries"
    # the trace takes both signs around 0 and 0 itself; each strict > of the diagonal is met from both sides and at equality
    sel = ap.group("quat", "cube") | ap.group("quat", "cube_ulp") | ap.group("quat", "ties")
    d = R[sel][:, [0, 4, 8]]
    tr = (d[:, 0] + d[:, 1]) + d[:, 2]
    assert (tr == 0).sum() >= 8 and ((tr > 0) & (tr < 1e-15)).sum() >= 8 and ((tr < 0) & (tr > -1e-15)).sum() >= 8
    low = d[tr <= 0]
    for name in ("cube_ulp", "ties"):
        g = R[ap.group("quat", name)][:, [0, 4, 8]]
        g = g[(g[:, 0] + g[:, 1]) + g[:, 2] <= 0]
        first = np.where(g[:, 1] > g[:, 0], g[:, 1], g[:, 0])
        for a, b in ((g[:, 1], g[:, 0]), (g[:, 2], first)):
            assert (a > b).sum() >= 4 and (a < b).sum() >= 4 and (a == b).sum() >= 4, name
            near = np.abs(a - b) <= 4 * U * np.maximum(np.abs(a), 1e-17)
            assert ((a > b) & near).sum() >= 2 and ((a < b) & near).sum() >= 2, name + ": the orderings an ulp apart"
    assert len(low) >= 200
    # small w, of both signs, down to where w * w underflows
    small = q[ap.group("quat", "small_w")]
    for w in (1e-8, 1e-160, 1e-170):
        for s in (1.0, -1.0):
            assert (np.abs(small[:, 3] / (s * w) - 1.0) < 1e-6).sum() >= 3, (w, s)
    # the two orders of the trace: they differ on every point of the group, at least once in the sign of the trace
    t = R[ap.group("quat", "trace_order")][:, [0, 4, 8]]
    left, right = (t[:, 0] + t[:, 1]) + t[:, 2], t[:, 0] + (t[:, 1] + t[:, 2])
    assert ((left > 0) != (right > 0)).sum() >= 2
    q_right = ap.quats(R[ap.group("quat", "trace_order")], trace_right=True)[0]
    rotation_like = np.abs(np.abs(np.linalg.det(R[ap.group("quat", "trace_order")].reshape(-1, 3, 3))) - 1.0) < 1e-9
    assert rotation_like.sum() >= 16 and (bits(q_right) != bits(q[ap.group("quat", "trace_order")])).any(axis=1)[rotation_like].all()
    # 1024 random rotations, at least 128 on each branch
    counts = np.bincount(branch[ap.group("quat", "random")], minlength=4)
    assert counts.sum() == 1024 and counts.min() >= 128, counts
    off = lambda m: np.abs(np.einsum("nij,nkj->nik", m.reshape(-1, 3, 3), m.reshape(-1, 3, 3)) - np.eye(3)).max(axis=(1, 2))
    assert off(R[ap.group("quat", "random")]).max() < 8 * U
    sk = off(R[ap.group("quat", "skewed")])
    assert ((sk > 1e-14) & (sk < 1e-11)).sum() >= 32 and (sk > 2.9).sum() >= 16
    host = R[ap.group("quat", "hostile")]
    assert np.isnan(host).any(axis=1).sum() >= 9 and np.isposinf(host).any() and np.isneginf(host).any() and (host == 1e300).any()
    assert np.isfinite(R[~ap.group("quat", "hostile")]).all()
    # euler
    e = p["euler"]
    quarter = e[ap.group("euler", "quarter")][:, :3]
    assert len(np.unique(bits(quarter), axis=0)) == 64 and set(np.unique(quarter)) == {k * ap.HALF_PI for k in range(4)}
    assert ap.group("euler", "quarter_near").sum() == 64 * 3 * 4
    sing = e[ap.group("euler", "singular")]
    assert (sing[:, 1] == ap.HALF_PI).any() and (sing[:, 1] == -ap.HALF_PI).any() and (sing[:, 3:6] != 0).all()
    far = np.abs(e[ap.group("euler", "far")][:, :3])
    assert (far < SWITCH).any() and (far >= SWITCH).any() and far.min() > 4e4
    rates = e[ap.group("euler", "rates")]
    assert (rates[:, 3:] == 0).all(axis=1).sum() >= 3
    for v in (1e-300, 1.0, 1e6):
        for slot in range(3, 9):
            assert ((rates[:, slot] == v) & ((rates[:, 3:] != 0).sum(axis=1) == 1)).any(), (v, slot)
    kept = ap.group("euler", "random").sum() + ap.group("euler", "far").sum()
    assert ap.group("euler", "random").sum() == 1024 and kept >= 0.99 * p["euler_draws"], (kept, p["euler_draws"])
    # (a band of 1e-6 is so thin that the draws may all survive: the filter's rejections are shown on states that sit on a boundary)
    on_boundary = [not ap.clear_of_branches(ap.reference_rotation(s)) for s in quarter]
    assert sum(on_boundary) >= 32 and not all(on_boundary), "the quarter-turn triples with trace 0 or a tied diagonal are refused"
    refused = lambda *angles: not ap.clear_of_branches(ap.reference_rotation(angles))
    assert refused(np.pi, 0.0, ap.HALF_PI + 1e-7) and not refused(np.pi, 0.0, ap.HALF_PI + 1e-2), "a half turn with a tied diagonal"
    assert refused(0.0, 0.0, 2 * np.pi / 3 + 1e-7) and not refused(0.0, 0.0, 2 * np.pi / 3 + 1e-2), "a third of a turn: trace 0"
    assert all(ap.clear_of_branches(ap.reference_rotation(s)) for s in e[ap.group("euler", "random") | ap.group("euler", "far")][:, :3])
    # frame
    f, fq = p["frame"], p["frame"][:, :4]
    unit, scaled, neg = fq[ap.group("frame", "unit")], fq[ap.group("frame", "scaled")], fq[ap.group("frame", "negated")]
    fin = ~ap.group("quat", "hostile")
    keep = fin & ~(ap.group("quat", "random") & (np.cumsum(ap.group("quat", "random")) % 4 != 1))
    assert np.array_equal(bits(unit), bits(q[keep][:, [3, 0, 1, 2]]))
    assert np.array_equal(bits(scaled), bits(np.concatenate([unit * 2.0 ** k for k in (-300, -1, 1, 300)]))) and np.array_equal(bits(neg), bits(-unit))
    norms = np.linalg.norm(fq[ap.group("frame", "nonunit")], axis=1)
    assert norms.min() < 1e-2 and norms.max() > 1e2 and norms.min() >= 1e-3 * (1 - 1e-9) and norms.max() <= 1e3 * (1 + 1e-9)
    assert ((fq[ap.group("frame", "single")] != 0).sum(axis=1) == 1).all()
    d = f[:, 7:] - f[:, 4:7]
    size = np.abs(d).max(axis=1)
    assert (size == 0).sum() >= 100 and ((size > 0) & (size < 1e-299)).sum() >= 100 and (size > 1e5).sum() >= 100
    assert ((size > 1e-2) & (size < 0.5)).sum() >= 2000
    h = fq[ap.group("frame", "hostile")]
    assert (h == 0).all(axis=1).any() and np.isnan(h).any() and np.isposinf(h).any() and np.isneginf(h).any()
    assert (np.abs(h) == 1e200).all(axis=1).any() and (np.abs(h) == 1e-200).all(axis=1).any()
    assert np.isfinite(fq[~ap.group("frame", "hostile")]).all()


def test_fixture_holds_the_points():
    """(CPU tier) refattitude.npz was recorded at exactly the points of tests/attitude_points.py: the matrices bit for bit; of
    the states the angles and rates bit for bit and the accelerations as the reference's spline rounded them"""
    f, p = fixture(), ap.points()
    assert same(f["quat_R"], p["quat"]).all() and np.array_equal(f["quat_group"], p["quat_group"])
    assert np.array_equal(f["euler_group"], p["euler_group"])
    st, want = f["euler_state"], p["euler"]
    assert np.array_equal(bits(st[:, :6]), bits(want[:, :6]))
    # a(0) = -6 (p0 - p1) - 4 v0 with p1 = p0 + (a + 4 v0) / 6 formed in doubles: p1 carries half an ulp of itself, times 6,
    # and a few roundings of the result's own size
    slack = 8 * U * (6 * np.abs(want[:, :3]) + 4 * np.abs(want[:, 3:6]) + np.abs(want[:, 6:]))
    assert (np.abs(st[:, 6:] - want[:, 6:]) <= slack).all()
    zero = (want[:, :6] == 0).all(axis=1)
    assert zero.sum() >= 7 and (np.abs(st[zero, 6:] - want[zero, 6:]) <= 2 * U * np.abs(want[zero, 6:])).all(), "1e-300 survives at a zero state"
    assert str(f["reference_deps"]) not in ("", "unknown")
    assert os.path.getsize(os.path.join(GOLDEN, "refattitude.npz")) < 400 * 1024


def test_restatement_equals_the_recorded_conversion_bit_for_bit():
    """(CPU tier) the numpy restatement, in the device's order of operations, gives the recorded Eigen::Quaterniond(R) on every
    finite group (and the same NaN pattern and finite components on the hostile one), and the recorded
    GetQuaternionBaseToWorld from the recorded GetRotationMatrixBaseToWorld"""
    f = fixture()
    q, _ = restated()
    assert same(q, f["quat_q"]).all()
    assert np.array_equal(bits(q[~ap.group("quat", "hostile")]), bits(f["quat_q"][~ap.group("quat", "hostile")]))
    assert np.array_equal(bits(ap.quats(f["euler_R"])[0]), bits(f["euler_q"]))


def test_restatement_equals_the_sampled_trajectories_bit_for_bit():
    """(CPU tier) on the reftraj_* fixtures: the restatement applied to the oracle's rotation matrix of a sample gives the
    quaternion of the oracle's sample_trajectory, bit for bit"""
    from oracle import binding as ob
    from .test_ref_traj import TrajFixture

    paths = sorted(glob.glob(os.path.join(GOLDEN, "reftraj_*.npz")))
    assert paths
    seen, branches = 0, np.zeros(4, dtype=np.int64)
    for path in paths:
        fx = TrajFixture(path)
        x = fx.x[0]
        traj = fx.case.P.sample_trajectory(x, fx.dt)
        # the Euler angles of the same samples are in the initial-guess records (state: base-lin p, base-ang p, ...); a spline
        # whose two nodes hold them returns them unchanged at t = 0, so euler_probe's R is the oracle's matrix of those angles
        angles = fx.case.P.initial_guess_samples(x, traj[:, 0])[:, 4:7]
        zero = np.zeros(3)
        R = [ob.euler_probe(np.concatenate([e, zero, e, zero]), 1.0, 0.0)["R"].ravel() for e in angles]
        q, b = ap.quats(np.array(R))
        assert np.array_equal(bits(q[:, [3, 0, 1, 2]]), bits(traj[:, 10:14])), fx.name
        seen += len(traj)
        branches += np.bincount(b, minlength=4)
    assert seen >= 500 and (branches > 0).all(), (seen, branches)


def test_negative_controls_on_the_points():
    """(CPU tier) the points have teeth: each mutant of the conversion disagrees with the recording in the group meant for it --
    `>=` for the strict comparisons on the cube rotations (10 of 24) and the ties, the operands of qw exchanged on the cube
    rotations (8 of 24) and at small w, qj and qk exchanged, and the other order of the trace's sum on trace_order only"""
    f, R = fixture(), ap.points()["quat"]
    differs = lambda **mutant: (bits(ap.quats(R, **mutant)[0]) != bits(f["quat_q"])).any(axis=1) & ~ap.group("quat", "hostile")
    count = lambda d, name: int(d[ap.group("quat", name)].sum())
    tie = differs(tie_ge=True)
    assert count(tie, "cube") == 10 and count(tie, "cube_ulp") >= 24 and count(tie, "ties") >= 24
    assert count(tie, "random") == 0, "only ties tell >= from >"
    qw = differs(swap_qw=True)
    assert count(qw, "cube") == 8 and count(qw, "small_w") >= 18 and count(qw, "ties") >= 24
    # what the comparison up to sign of the trajectory tests cannot see: q and the mutant's q agree to 1e-10 up to sign
    sel = qw & (ap.group("quat", "small_w") | ap.group("quat", "cube") | ap.group("quat", "ties"))
    a, b = ap.quats(R[sel], swap_qw=True)[0], f["quat_q"][sel]
    hidden = np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)) < 1e-10
    # (w = +-1e-160 and +-1e-170 next to each of the three axes)
    assert hidden.sum() >= 12, "points on which the swapped qw passes a 1e-10 comparison up to sign"
    jk = differs(swap_jk=True)
    assert count(jk, "cube") >= 8 and count(jk, "ties") >= 24 and count(jk, "random") >= 512
    order = differs(trace_right=True)
    assert count(order, "trace_order") >= 24 and count(order, "cube") == 0 and count(order, "ties") == 0


def test_recorded_quaternions_reproduce_their_rotations():
    """(CPU tier) mpmath at 40 digits: on the orthogonal groups the recorded q has | |q|^2 - 1 | <= C_NORM u and R(q / |q|) is
    within C_BACK u of the input, entry by entry (the bounds of the docstring)"""
    f = fixture()
    worst_back = worst_norm = 0.0
    for name in ORTHOGONAL:
        for R, q in zip(f["quat_R"][ap.group("quat", name)], f["quat_q"][ap.group("quat", name)]):
            back, norm = back_and_norm(R, q)
            worst_back, worst_norm = max(worst_back, back / C_BACK), max(worst_norm, norm / C_NORM)
    print("\nrecorded q: R(q) within %.3f of the bound, |q|^2 - 1 within %.3f" % (worst_back, worst_norm))
    assert worst_back <= 1.0 and worst_norm <= 1.0


def test_recorded_angular_rates_against_mpmath():
    """(CPU tier) the recorded GetAngularVelocityInWorld and GetAngularAccelerationInWorld lie within C u sum |terms| of mpmath on
    the recorded state, C = 8 and 12 from libm's 1 ulp and the operation count"""
    f = fixture()
    worst = angular_worst(f["euler_omega"], f["euler_omega_dot"], np.ones(len(f["euler_state"])))
    print("\nrecorded omega within %.3f of the bound, omega_dot within %.3f" % tuple(worst))
    assert max(worst) <= 1.0


def rotation_worst(R, states):
    """the worst error of the entries of R (n, 9) as a fraction of C_ROT u sum |terms| of GetRotationMatrixBaseToWorld
    (euler_converter.cc:207-221) in mpmath at the angles of `states`"""
    mp = _mp()
    worst = 0.0
    for got, s in zip(R, states):
        x, y, z = (mp.mpf(float(v)) for v in s[:3])
        sx, cx, sy, cy, sz, cz = mp.sin(x), mp.cos(x), mp.sin(y), mp.cos(y), mp.sin(z), mp.cos(z)
        terms = [[cy * cz], [cz * sx * sy, -cx * sz], [sx * sz, cx * cz * sy], [cy * sz], [cx * cz, sx * sy * sz], [cx * sy * sz, -cz * sx],
                 [-sy], [cy * sx], [cx * cy]]
        for g, t in zip(got, terms):
            worst = max(worst, float(abs(mp.mpf(float(g)) - mp.fsum(t)) / (C_ROT * U * mp.fsum(abs(v) for v in t) + TINY)))
    return worst


def test_recorded_rotations_against_mpmath():
    """(CPU tier) the recorded GetRotationMatrixBaseToWorld lies within C_ROT u sum |terms| of mpmath per entry: a term has at most
    three sines or cosines at libm's 1 ulp (2 u each) and two products, an entry one sum: C_ROT = 9"""
    f = fixture()
    worst = rotation_worst(f["euler_R"], f["euler_state"])
    print("\nrecorded R within %.3f of the bound" % worst)
    assert worst <= 1.0


# Whether the recipe reproduces refattitude.npz is NOT a test of this suite: `python -m oracle.ref_golden --attitude --check`
# records afresh where the reference is built and compares key by key (byte for byte where no libm call feeds the key).  As a
# test it failed once on a GPU host for a reason that was not found and could not be reproduced, so it is run by hand.


# ------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
def test_quat_of_rotation_on_device():
    """quat_of_rotation, one thread per matrix: bit for bit the recording and the restatement on every finite point (the function
    has no multiply-add to fuse), the restatement's NaN pattern and finite components on the hostile ones"""
    f = fixture()
    got = _probe("quat").reshape(-1, 4)
    want, _ = restated()
    assert len(got) == len(want)
    fin = ~ap.group("quat", "hostile")
    for name in ap.QUAT_GROUPS[:-1]:
        g = ap.group("quat", name)
        bad = np.nonzero((bits(got[g]) != bits(want[g])).any(axis=1) | (bits(got[g]) != bits(f["quat_q"][g])).any(axis=1))[0]
        assert len(bad) == 0, "%s: %d points differ, first: R = %r device %r restatement %r" % (
            name, len(bad), ap.points()["quat"][g][bad[0]].tolist(), got[g][bad[0]].tolist(), want[g][bad[0]].tolist())
    assert not np.isnan(got[fin]).any()
    h = ~fin
    assert np.array_equal(np.isnan(got[h]), np.isnan(want[h])) and same(got[h], want[h]).all()
    print("\nquat: %d finite points bit-equal to the recording and the restatement, %d hostile ones to the restatement" % (fin.sum(), h.sum()))


@pytest.mark.gpu
def test_sample_angular_on_device():
    """sample_angular on the recorded states: q is bit for bit the restatement applied to the R the probe returned; against the
    reference's q no branch flips in the random and far groups, and a flip elsewhere is the restatement's on the device's R;
    omega and omega_dot within C' u sum |terms| of mpmath"""
    f = fixture()
    raw = _probe("euler").reshape(-1, 19)
    st = f["euler_state"]
    assert len(raw) == len(st) and not np.isnan(raw).any()
    R, q = raw[:, :9], raw[:, 9:13]
    want, branch = ap.quats(R)
    bad = np.nonzero((bits(q) != bits(want)).any(axis=1))[0]
    assert len(bad) == 0, "%d states: q is not the restatement of the device's R, first %r: %r against %r" % (
        len(bad), st[bad[0]].tolist(), q[bad[0]].tolist(), want[bad[0]].tolist())
    ref_branch = ap.quats(f["euler_R"])[1]
    flips = branch != ref_branch
    steady = ap.group("euler", "random") | ap.group("euler", "far")
    assert not flips[steady].any(), "%d branch flips away from every branch boundary" % flips[steady].sum()
    for i in np.nonzero(flips)[0]:      # a flip elsewhere: the reference's R sits on the boundary that was crossed, to rounding
        d = f["euler_R"][i][[0, 4, 8]]
        on_trace = abs((d[0] + d[1]) + d[2]) <= FLIP_TRACE * U
        top = np.sort(d)
        on_tie = top[2] - top[1] <= FLIP_DIAGONAL * U
        assert on_trace if (branch[i] == 0) != (ref_branch[i] == 0) else on_tie, (st[i].tolist(), int(branch[i]), int(ref_branch[i]))
    # (where the branch is the reference's, so is q, at the bar of the trajectory tests and without their sign alignment)
    assert (np.abs(q[steady] - f["euler_q"][steady]).max(axis=1) < 1e-10).all()
    ulps = np.where((np.abs(st[:, 1:3]) < SWITCH).all(axis=1), ULP_FAST, ULP_LIB)
    worst = angular_worst(raw[:, 13:16], raw[:, 16:19], ulps)
    print("\neuler: %d states, q bit-equal to the restatement of the device's R, %d branch flips (none in random / far), omega within %.3f of "
          "the bound, omega_dot within %.3f" % (len(st), flips.sum(), worst[0], worst[1]))
    assert max(worst) <= 1.0


@pytest.mark.gpu
def test_base_frame_on_device():
    """base_frame_rotation and base_frame: bit for bit the numpy restatement in the source's order (both are fp contract(off)), the
    NaN / Inf pattern of the restatement on the hostile quaternions, and within C_FR u per entry of R and C_FV u |d|_1 per component
    of the vector of mpmath's exact rotation by the normalised quaternion"""
    mp = _mp()
    p = ap.points()["frame"]
    raw = _probe("frame").reshape(-1, 12)
    assert len(raw) == len(p)
    R = frame_rotation(p[:, :4])
    want = np.column_stack([R[r][c] for r in range(3) for c in range(3)] + [frame_vector(R, p[:, 4:7], p[:, 7:10])])
    host = ap.group("frame", "hostile")
    assert np.array_equal(bits(raw[~host]), bits(want[~host])) and np.isfinite(raw[~host]).all()
    assert np.array_equal(np.isnan(raw[host]), np.isnan(want[host])) and same(raw[host], want[host]).all()
    with np.errstate(all="ignore"):
        norm = np.sqrt((p[host][:, :4] ** 2).sum(axis=1))
    no_norm = ~((norm > 0) & (norm < np.inf))
    assert no_norm.sum() >= 30 and (~no_norm).sum() >= 4
    assert np.array_equal(np.isnan(raw[host][:, 9:]).any(axis=1), no_norm), "NaN exactly where the norm in doubles is 0, Inf or NaN"
    worst_r = worst_v = 0.0
    for row, got in zip(p[~host], raw[~host]):
        w, x, y, z = (mp.mpf(float(v)) for v in row[:4])
        n = w * w + x * x + y * y + z * z
        exact = [[(n - 2 * (y * y + z * z)) / n, 2 * (x * y - w * z) / n, 2 * (x * z + w * y) / n],
                 [2 * (x * y + w * z) / n, (n - 2 * (x * x + z * z)) / n, 2 * (y * z - w * x) / n],
                 [2 * (x * z - w * y) / n, 2 * (y * z + w * x) / n, (n - 2 * (x * x + y * y)) / n]]
        d = [mp.mpf(float(row[7 + k])) - mp.mpf(float(row[4 + k])) for k in range(3)]
        d1 = abs(d[0]) + abs(d[1]) + abs(d[2])
        for r in range(3):
            for c in range(3):
                worst_r = max(worst_r, float(abs(mp.mpf(float(got[3 * r + c])) - exact[r][c]) / (C_FR * U)))
        for i in range(3):
            v = exact[0][i] * d[0] + exact[1][i] * d[1] + exact[2][i] * d[2]
            worst_v = max(worst_v, float(abs(mp.mpf(float(got[9 + i])) - v) / (C_FV * U * d1 + TINY)))
    print("\nframe: %d points bit-equal to the restatement, R within %.3f of the bound, the vector within %.3f; %d hostile ones" % (
        (~host).sum(), worst_r, worst_v, host.sum()))
    assert worst_r <= 1.0 and worst_v <= 1.0
