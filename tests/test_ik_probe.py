"""leg_ik and leg_ik_of_foot of kernels/joints.h against the reference's recorded answers, class by class.

tests/ik_probe.hip is a stand-alone program that includes that header and what it includes, nothing else of the product; it is
compiled here with the product's CXXFLAGS for util_tu.o, started as a fresh child process per mode and fed the feet of
tests/ik_points.py.  The reference is tests/golden/refik_go1.npz (tests/test_ik_ref.py pins it); the bound and its count
C_IK = 121 are in that file's docstring: per angle C_IK * 2^-53 * (1 + 1 / sqrt(1 - c^2)) * pi, the 1 / sqrt term dropped where
no acos takes an unclamped argument.

  interior     every angle within the bound, flags bit-equal (all zero)
  over_reach   flags bit-equal; KFE (exactly 0) and what depends on beta = acos(1) = 0 bit-equal where the reference's value is an
               exact zero or a limit; HAA / HFE within the bound without the 1 / sqrt term
  stretch      r within 8 ulp of lu + ll: the rounding of the cosine may fall on either side of -1, so angles within
               sqrt(2 C_IK 2^-53) (acos near -1 turns an error e of its argument into sqrt(2 e)), FK(q) within 1e-7 m of the
               foot (sqrt(2^-53) times the leg length is 1e-8, times ten), flags 1 / 2 compared only where mpmath's exact
               cosine is farther than C_IK 2^-53 from +-1, the limit flags always
  branch       flags bit-equal; every angle the reference returns as a limit value or an exact +-0 bit-equal (+0 and -0 are
               different); the rest within the bound
  non_finite   the same angles NaN, flags equal, finite angles bit-equal
  whole body   the four legs' mirrors, hip offset and bends against GetAllJointAngles: near feet within the bound, far feet as
               over_reach / branch

The GPU tests print the worst case they measured as a fraction of the bound (run with -s); DESIGN section 5 "Leg inverse
kinematics" quotes them."""
import numpy as np
import pytest

import towr_amd as ta

from . import ik_points as ip
from .probe import Probe, bits
from .test_ik_ref import C_IK, PI, U, acos_factor, angle_bounds, fixture, mp_leg_ik, same_bits

PROBE = Probe("ik_probe")


def descriptor_doubles(k):
    return np.concatenate([[k.n_ee], list(k.knee_bend), np.array([list(m) for m in k.mirror]).ravel(), list(k.base_to_hip),
                           list(k.hfe_to_haa), [k.length_thigh, k.length_shank], list(k.q_min), list(k.q_max)]).astype(np.float64)


def probe_input(mode):
    k = descriptor_doubles(ta.leg_kinematics_preset("go1"))
    if mode == "leg":
        feet, bends, _ = ip.leg_points()
        return np.concatenate([k, [float(len(feet))], np.column_stack([feet, bends]).ravel()])
    body = ip.body_points()
    return np.concatenate([k, [float(len(body))], body.ravel()])


def _probe(mode):
    """[n, 8] per leg: q_HAA q_HFE q_KFE flags cos_beta cos_gamma r over_reach, from a child process of its own"""
    return PROBE.run(mode, probe_input(mode)).reshape(-1, 8)


def test_probe_compiles_without_warning():
    """(CPU tier) hipcc compiles and links the probe for gfx950 with the product's flags, without a GPU and without a warning;
    the input parser refuses a file whose count does not add up before anything reaches a device"""
    PROBE.refuses([], None, "usage")
    PROBE.refuses(["leg"], probe_input("leg")[:-1], "truncated")


def _reference():
    """per leg-level foot: the recorded angles and numpy's flags and cosines of the same formulas (their class decides the bound)"""
    feet, bends, sl = ip.leg_points()
    _q, fl, cb, cg, r = ip.ik_numpy(feet, bends)
    return feet, bends, sl, fixture()["leg_q"], fl, cb, cg, r


def _pinned(ref):
    """where the reference's angle is a limit value or an exact +-0"""
    out = np.zeros(ref.shape, dtype=bool)
    for lim in list(ip.Q_MIN) + list(ip.Q_MAX) + [0.0, -0.0]:
        out |= bits(ref) == bits(np.array(lim))
    return out


def _check_class(name, got, ref, fl, cb, cg, rows, pinned_exact):
    g, want = got[rows, :3], ref[rows]
    assert np.array_equal(got[rows, 3].astype(np.int64), fl[rows]), "%s: flags differ at rows %r" % (
        name, np.nonzero(got[rows, 3].astype(np.int64) != fl[rows])[0][:8].tolist())
    assert (np.isnan(g) == np.isnan(want)).all(), name
    bound = angle_bounds(cb[rows], cg[rows])
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, g, 0.0) - np.where(fin, want, 0.0)), 0.0)
    worst = float((err / bound).max())
    assert (err <= bound).all(), "%s: worst error %.3f of the bound" % (name, worst)
    if pinned_exact:
        pin = _pinned(want)
        assert same_bits(g[pin], want[pin]).all(), "%s: %d limit values or exact zeros differ in bits" % (name, int((~same_bits(g[pin], want[pin])).sum()))
    return worst


@pytest.mark.gpu
def test_interior_within_the_bound():
    feet, bends, sl, ref, fl, cb, cg, r = _reference()
    got = _probe("leg")
    rows = np.arange(sl["interior"].start, sl["interior"].stop)
    worst = _check_class("interior", got, ref, fl, cb, cg, rows, False)
    assert np.abs(got[rows, 4] - cb[rows]).max() <= C_IK * U and np.abs(got[rows, 5] - cg[rows]).max() <= C_IK * U
    assert (np.abs(got[rows, 6] - r[rows]) <= C_IK * U * r[rows]).all() and (got[rows, 7] == 0.0).all()
    print("\nleg_ik on %d interior feet: worst |dq| %.4f of the bound (C = %g)" % (len(rows), worst, C_IK))


@pytest.mark.gpu
def test_over_reach_flags_and_exact_values():
    feet, bends, sl, ref, fl, cb, cg, r = _reference()
    got = _probe("leg")
    rows = np.arange(sl["over_reach"].start, sl["over_reach"].stop)
    assert (acos_factor(cb[rows]) == 0).all() and (acos_factor(cg[rows]) == 0).all()      # both clamped: no 1 / sqrt term
    worst = _check_class("over_reach", got, ref, fl, cb, cg, rows, True)
    assert same_bits(got[rows, 2], 0.0).all(), "KFE of an over-reaching foot is exactly +0"
    want_over = r[rows] - ip.REACH
    assert (np.abs(got[rows, 7] - want_over) <= C_IK * U * r[rows]).all()
    print("\nleg_ik on %d over-reaching feet: worst |dq| %.4f of the bound" % (len(rows), worst))


@pytest.mark.gpu
def test_stretch_band():
    import mpmath
    feet, bends, sl, ref, fl, cb, cg, r = _reference()
    got = _probe("leg")
    rows = np.arange(sl["stretch"].start, sl["stretch"].stop)
    tol = np.sqrt(2 * C_IK * U)
    assert (np.abs(got[rows, :3] - ref[rows]) <= tol).all()
    assert np.abs(ip.fk(got[rows, :3], bends[rows]) - feet[rows]).max() <= 1e-7
    gf = got[rows, 3].astype(np.int64)
    assert np.array_equal(gf & ~3, fl[rows] & ~3), "limit and NaN flags"
    compared = 0
    for k, row in enumerate(rows):
        _q, mcb, mcg = mp_leg_ik(feet[row], int(bends[row]))
        for bit, c in ((1, mcb), (2, mcg)):
            if min(abs(c - 1), abs(c + 1)) > C_IK * U:
                compared += 1
                assert (gf[k] & bit) == (int(fl[row]) & bit), (feet[row].tolist(), bit)
    print("\nleg_ik on %d feet of the stretch band: worst |dq| %.3g rad (allowed %.3g), %d flag bits compared" % (
        len(rows), float(np.abs(got[rows, :3] - ref[rows]).max()), tol, compared))


@pytest.mark.gpu
def test_branch_cuts_and_signed_zeros():
    feet, bends, sl, ref, fl, cb, cg, r = _reference()
    got = _probe("leg")
    rows = np.arange(sl["branch"].start, sl["branch"].stop)
    worst = _check_class("branch", got, ref, fl, cb, cg, rows, True)
    print("\nleg_ik on %d branch-cut feet: worst |dq| of the unpinned angles %.4f of the bound" % (len(rows), worst))


@pytest.mark.gpu
def test_non_finite_feet():
    feet, bends, sl, ref, fl, cb, cg, r = _reference()
    got = _probe("leg")
    rows = np.arange(sl["non_finite"].start, sl["non_finite"].stop)
    assert np.array_equal(got[rows, 3].astype(np.int64), fl[rows])
    assert (np.isnan(got[rows, :3]) == np.isnan(ref[rows])).all()
    assert same_bits(got[rows, :3], ref[rows]).all(), "finite angles of a non-finite foot bit-equal (KFE = -pi for x = NaN)"
    k = np.nonzero(np.isnan(feet[rows, 0]) & (feet[rows, 1] == 0.0) & (bends[rows] == 0))[0]
    assert k.size and same_bits(got[rows[k[0]], 2], -PI) and np.isnan(got[rows[k[0]], 1])


@pytest.mark.gpu
def test_whole_body_mirrors_and_bends():
    got = _probe("body")
    fx = fixture()
    hip = ip.body_to_hip(fx["body_feet"]).reshape(-1, 3)
    bend = np.tile(ip.KNEE_BEND, len(hip) // 4)
    _q, fl, cb, cg, r = ip.ik_numpy(hip, bend)
    ref = fx["body_q"].reshape(-1, 3)
    near = np.arange(4 * ip.N_BODY_NEAR)
    worst = _check_class("whole body, near", got, ref, fl, cb, cg, near, False)
    far = np.arange(4 * ip.N_BODY_NEAR, len(ref))
    _check_class("whole body, far", got, ref, fl, cb, cg, far, True)
    print("\nleg_ik_of_foot on %d bodies: worst |dq| %.4f of the bound" % (len(ref) // 4, worst))
