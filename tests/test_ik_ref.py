"""The reference's Go1 leg inverse kinematics as a fixture, and what stands on it without a GPU (CPU tier).

tests/golden/refik_go1.npz holds the feet of tests/ik_points.py and what the reference's own GetJointAngles (both knee bends)
and GetAllJointAngles return for them, recorded by tests/ik_ref/record.py: the reference's two source files compiled where they
lie (g++ -O2 -ffp-contract=off) against stand-ins for the few Eigen / xpp types they use.  Where the reference's sources are
present the fixture is re-recorded and must come out bit for bit; everywhere it is held to a 60-digit mpmath evaluation of the
same formulas, so it is pinned by two independent means.

The bound, for this file, test_ik_probe.py and test_joints.py.  Per angle
    |dq| <= C_IK * 2^-53 * (1 + 1 / sqrt(1 - c^2)) * pi
with c the law-of-cosines argument the angle's acos takes (cos_beta for HFE, cos_gamma for KFE, no such term for HAA, and none
where the argument was clamped: acos of exactly +-1 is exact).  C_IK = 121 counts, in units of 2^-53 relative error, the roundings
of the longest chain of BOTH sides of a comparison, an operation's count being its operands' plus one and a libm call counting
L = 2 on the host (glibc: within 1 ulp) and L = 4 on the device (atan2, sin, cos, acos of the device library: within 2 ulp):
    q_HAA = -atan2(y, -z)                       L
    c, s = cos, sin(q_HAA)                      2 L, absolute (the argument's L and the call's)
    z' = s y + c z (+ hfe_to_haa)               both terms have the sign of -rho, rho = |(y, z)|: 2 sqrt(2) L + 1 per term, two
                                                additions, the offset's addition: 2.83 L + 4
    sq = x^2 + z'^2                             2 (2.83 L + 4) + 1 and one addition: 5.66 L + 10
    r = sqrt(sq)                                2.83 L + 6
    cos_gamma = (ll^2 + lu^2 - sq) / (2 ll lu)  absolute: the constants 3, sq / (2 ll lu) <= 1.94 (r <= 0.42) times 5.66 L + 11,
                                                the denominator and the division 3: 10.98 L + 27.3
    cos_beta = (lu^2 + sq - ll^2) / (2 lu r)    absolute: lu / (2 r) <= 2.13 (r >= 0.05) times 5, r / (2 lu) < 1 times 5.66 L + 12,
                                                the denominator and the division 2.83 L + 9: 8.41 L + 31.5
cos_gamma is the longer one: 10.98 * (2 + 4) + 2 * 27.3 = 120.5 -> 121; it passes through acos with the factor 1 / sqrt(1 - c^2).
What does not pass through an acos -- alpha = atan2(-z', +-x) - pi/2 (2.5 L + 4), the acos calls themselves (L), the final
addition or subtraction (1) -- stays below 3.5 L + 6 per side = 47 together and is covered by the "1 +" of the bound.  On the
interior class (|c| <= 0.999, so 1 / sqrt <= 22.4) the bound stays below 121 * 2^-53 * 23.4 * pi = 9.9e-13 rad."""
import ctypes as C
import os

import numpy as np
import pytest

import towr_amd as ta

from . import ik_points as ip
from .ik_ref import record
from .probe import bits, load_fixture

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refik_go1.npz")
U = 2.0 ** -53
C_IK = 121.0
PI = ip.PI


def same_bits(a, b):
    """element-wise: the same double, +0 and -0 taken as different (all NaNs taken as the same)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def fixture():
    return load_fixture("refik_go1")


def acos_factor(c):
    """1 / sqrt(1 - c^2) where acos takes c itself, 0 where the clamp hands it exactly +-1 (or the NaN rule does)"""
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(all="ignore"):
        inside = np.abs(c) < 1.0
        return np.where(inside, 1.0 / np.sqrt(np.where(inside, 1.0 - c * c, 1.0)), 0.0)


def angle_bounds(cb, cg, c_total=C_IK):
    """[n, 3] the bound per angle (HAA, HFE, KFE) from the two cosines"""
    one = np.ones_like(np.asarray(cb, dtype=np.float64))
    return c_total * U * PI * np.column_stack([one, 1.0 + acos_factor(cb), 1.0 + acos_factor(cg)])


def mp_leg_ik(p, bend):
    """the reference's formulas at 60 digits on the double inputs (and its double constants): (q[3] as mpf, cos_beta, cos_gamma)
    before any clamp or limit -- for feet where neither acts"""
    import mpmath
    mp = mpmath.mp
    mp.dps = 60
    x, y, z = (mp.mpf(float(v)) for v in p)
    lu, ll, pi = mp.mpf(ip.LU), mp.mpf(ip.LL), mp.mpf(PI)
    q_haa = -mp.atan2(y, -z)
    c, s = mp.cos(q_haa), mp.sin(q_haa)
    zr = s * y + c * z
    sq = x * x + zr * zr
    alpha = (mp.atan2(-zr, x) if bend == 0 else mp.atan2(-zr, -x)) - pi / 2
    cb = (lu * lu + sq - ll * ll) / (2 * lu * mp.sqrt(sq))
    cg = (ll * ll + lu * lu - sq) / (2 * ll * lu)
    return [q_haa, alpha + mp.acos(cb), mp.acos(cg) - pi], cb, cg


# ------------------------------------------------------------------ the fixture
def test_fixture_holds_the_generated_points():
    fx = fixture()
    feet, bends, sl = ip.leg_points()
    assert same_bits(fx["leg_feet"], feet).all() and np.array_equal(fx["leg_bend"], bends)
    assert same_bits(fx["body_feet"], ip.body_points()).all()
    assert fx["leg_q"].shape == (len(feet), 3) and fx["body_q"].shape == (len(ip.body_points()), 4, 3)
    assert sl["interior"].stop - sl["interior"].start == 2 * ip.N_INTERIOR
    assert os.path.getsize(GOLDEN) <= 400 << 10
    assert all(v.dtype == np.float64 for v in fx.values())


@pytest.mark.skipif(not record.available(), reason="the reference's sources are not present")
def test_fixture_rerecorded_bit_for_bit():
    new, fx = record.compute(), fixture()
    assert set(new) == set(fx)
    for k in fx:
        assert new[k].shape == fx[k].shape and same_bits(new[k], fx[k]).all(), k


def test_classes_are_what_they_claim():
    fx = fixture()
    feet, bends, sl = ip.leg_points()
    q, fl, cb, cg, r = ip.ik_numpy(feet, bends)
    i = sl["interior"]
    assert (fl[i] == 0).all() and (r[i] >= 0.05).all() and (r[i] <= 0.42).all()
    assert (np.abs(cb[i]) <= 0.999).all() and (np.abs(cg[i]) <= 0.999).all()
    assert angle_bounds(cb[i], cg[i]).max() < 1e-12
    o = sl["over_reach"]
    assert (r[o] >= ip.REACH * (1 + 1e-6)).all() and ((fl[o] & 3) == 3).all()
    s = sl["stretch"]
    assert (np.abs(r[s] - ip.REACH) <= 10 * np.spacing(ip.REACH)).all()
    assert ((fl[s] & 2) != 0).any() and ((fl[s] & 2) == 0).any(), "the band straddles the clamp"
    b = sl["branch"]
    ref = fx["leg_q"][b]
    assert ((fl[b] & 4) != 0).sum() >= 8 and ((fl[b] & 8) != 0).sum() >= 4, "limit-enforced feet"
    assert (same_bits(ref[:, 0], ip.Q_MAX[0])).sum() >= 8 and same_bits(ref[:, 1], ip.Q_MAX[1]).sum() >= 4
    assert (bits(ref[:, 0]) == bits(np.array(-0.0))).any() and same_bits(ref[:, 0], -PI).any() and same_bits(ref[:, 0], PI / 2).any()
    n = sl["non_finite"]
    assert np.isnan(fx["leg_q"][n]).any() and ((fl[n] & 32) != 0).all()


def test_the_reference_quirks_are_in_the_fixture():
    """the behaviours the device has to keep, read from the recording"""
    fx = fixture()
    feet, bends = fx["leg_feet"], fx["leg_bend"]

    def recorded(p, bend=0):
        hit = np.nonzero(same_bits(feet, np.asarray(p, dtype=np.float64)).all(axis=1) & (bends == bend))[0]
        assert hit.size, p
        return fx["leg_q"][hit[0]]

    assert same_bits(recorded([0.0, 0.0, 0.3])[0], -PI)                    # -atan2(+0, -0.3)
    assert same_bits(recorded([0.0, -0.0, 0.3])[0], PI / 2)                # +pi, then limited to 90 degrees
    assert same_bits(recorded([0.0, 0.0, -0.3])[0], -0.0)
    assert same_bits(recorded([0.0, 0.0, 0.0]), [-PI, -PI / 2, -PI]).all()   # the 0/0 cosine becomes +1
    q = recorded([np.nan, 0.0, -0.3])
    assert same_bits(q[0], -0.0) and np.isnan(q[1]) and same_bits(q[2], -PI)  # KFE is not NaN
    assert same_bits(recorded([0.0, 0.0, -0.5]), [-0.0, 0.0, 0.0]).all()


def test_fixture_agrees_with_mpmath_on_the_interior():
    fx = fixture()
    feet, bends, sl = ip.leg_points()
    _q, _fl, cb, cg, _r = ip.ik_numpy(feet, bends)
    i = sl["interior"]
    bound = angle_bounds(cb[i], cg[i])
    worst = 0.0
    import mpmath
    for k, row in enumerate(range(i.start, i.stop)):
        want, mcb, mcg = mp_leg_ik(feet[row], int(bends[row]))
        assert abs(mcb - float(cb[row])) <= C_IK * U and abs(mcg - float(cg[row])) <= C_IK * U
        for j in range(3):
            err = float(abs(mpmath.mpf(float(fx["leg_q"][row, j])) - want[j]))
            worst = max(worst, err / bound[k, j])
            assert err <= bound[k, j], (feet[row].tolist(), int(bends[row]), j, err / bound[k, j])
    print("\nrecorded reference against mpmath, %d interior feet: worst error %.4f of the bound" % (i.stop - i.start, worst))


def test_whole_body_recording_is_the_leg_recording_of_the_mirrored_feet():
    """GetAllJointAngles = the mirror, the hip offset and the bend per leg, then GetJointAngles: against mpmath on the near feet"""
    fx = fixture()
    hip = ip.body_to_hip(fx["body_feet"])
    bend = np.tile(ip.KNEE_BEND, len(hip))
    q, fl, cb, cg, _r = ip.ik_numpy(hip.reshape(-1, 3), bend)
    near = np.arange(4 * ip.N_BODY_NEAR)
    assert (fl[near] == 0).all() and (np.abs(cb[near]) <= 0.999).all() and (np.abs(cg[near]) <= 0.999).all()
    ref = fx["body_q"].reshape(-1, 3)
    assert (np.abs(q[near] - ref[near]) <= angle_bounds(cb[near], cg[near])).all()
    import mpmath
    for row in near[::16]:
        want, _, _ = mp_leg_ik(hip.reshape(-1, 3)[row], int(bend[row]))
        for j in range(3):
            assert abs(mpmath.mpf(float(ref[row, j])) - want[j]) <= angle_bounds(cb[row:row + 1], cg[row:row + 1])[0, j]
    far = np.arange(4 * ip.N_BODY_NEAR, len(ref))
    fin = np.isfinite(ref[far]) & np.isfinite(q[far])
    assert (np.isfinite(ref[far]) == np.isfinite(q[far])).all() and (fl[far] != 0).any()


def test_forward_kinematics_round_trip():
    fx = fixture()
    feet, bends, sl = ip.leg_points()
    i = sl["interior"]
    err = np.abs(ip.fk(fx["leg_q"][i], bends[i]) - feet[i]).max()
    print("\nFK(q) - p on the interior class: %.3g m" % err)
    assert err <= 1e-12


def test_numpy_restatement_is_pinned_by_the_fixture():
    """ik_numpy (what test_joints.py restates the device with): within the bound of the recording on the interior, the same
    NaNs, limit values and zeros everywhere"""
    fx = fixture()
    feet, bends, sl = ip.leg_points()
    q, fl, cb, cg, _r = ip.ik_numpy(feet, bends)
    ref = fx["leg_q"]
    i = sl["interior"]
    assert (np.abs(q[i] - ref[i]) <= angle_bounds(cb[i], cg[i])).all()
    assert (np.isnan(q) == np.isnan(ref)).all()
    for lim in list(ip.Q_MIN) + list(ip.Q_MAX) + [0.0, -0.0]:
        at = bits(ref) == bits(np.array(lim))
        outside = ~np.isin(np.arange(len(ref)), np.arange(sl["stretch"].start, sl["stretch"].stop))
        assert (bits(q)[at & outside[:, None]] == bits(np.array(lim))).all(), lim


# ------------------------------------------------------------------ the preset and the descriptor
def test_preset_constants_are_the_recorded_doubles():
    fx = fixture()
    k = ta.leg_kinematics_preset("go1")
    c = fx["constants"]
    assert same_bits(list(k.base_to_hip), c[0:3]).all() and same_bits(list(k.hfe_to_haa), c[3:6]).all()
    assert same_bits(k.length_thigh, c[6]) and same_bits(k.length_shank, c[7])
    assert same_bits(list(k.q_min), ip.Q_MIN).all() and same_bits(list(k.q_max), ip.Q_MAX).all()
    assert np.array_equal(np.array([list(m) for m in k.mirror]), ip.MIRROR) and list(k.knee_bend) == list(ip.KNEE_BEND) and k.n_ee == 4
    # the limits as the reference returns them: HAA max (a foot turned past 90 degrees), HFE max (a foot far behind), HAA min and
    # KFE min (-pi, met exactly), HFE min (the foot on the hip), KFE max (a stretched leg)
    ref = fx["leg_q"]
    for j in range(3):
        assert same_bits(ref[:, j], k.q_max[j]).any() and same_bits(ref[:, j], k.q_min[j]).any(), j
        finite = ref[:, j][np.isfinite(ref[:, j])]
        assert finite.max() == k.q_max[j] and finite.min() == k.q_min[j]


@pytest.mark.parametrize("robot", ["monoped", "biped", "hyq", "anymal"])
def test_preset_is_unsupported_for_robots_without_reference_ik(robot):
    k = ta.LegKinematics()
    assert ta.lib().twr_leg_kinematics_preset(ta.ROBOTS[robot], C.byref(k)) == -5      # TWR_ERR_UNSUPPORTED
    assert ta.lib().twr_leg_kinematics_preset(ta.ROBOTS["go1"], None) == -1
    assert ta.lib().twr_leg_kinematics_preset(17, C.byref(k)) == -1


def _spoil(field, index, value):
    k = ta.leg_kinematics_preset("go1")
    if index is None:
        setattr(k, field, value)
    elif isinstance(index, tuple):
        getattr(k, field)[index[0]][index[1]] = value
    else:
        getattr(k, field)[index] = value
    return k


BAD_DESCRIPTORS = [("n_ee", None, 0), ("n_ee", None, 5), ("knee_bend", 1, 2), ("mirror", (2, 0), 0.5), ("mirror", (0, 1), float("nan")),
                   ("base_to_hip", 1, float("inf")), ("hfe_to_haa", 2, float("nan")), ("length_thigh", None, 0.0),
                   ("length_thigh", None, float("inf")), ("length_shank", None, -0.2), ("length_shank", None, float("nan")),
                   ("q_min", 1, 2.0), ("q_min", 0, float("nan")), ("q_max", 2, float("nan"))]


@pytest.mark.parametrize("field,index,value", BAD_DESCRIPTORS)
def test_descriptor_validation_names_the_field(field, index, value):
    """every call validates the descriptor first, before the batch or a device is looked at: without either here"""
    k = _spoil(field, index, value)
    named = "q_min" if field == "q_max" else field
    L = ta.lib()
    for rc in (L.twr_batch_joints(None, C.byref(k), None, 0, 0.01, None, 0, None),
               L.twr_batch_joint_scores(None, C.byref(k), None, 0, 0.01, None, None),
               L.twr_batch_eval_joint_scores(None, C.byref(k), None, 0.01, None, None)):
        assert rc == -1 and named in L.twr_last_error().decode(), L.twr_last_error().decode()
    good = ta.leg_kinematics_preset("go1")
    assert L.twr_batch_eval_joint_scores(None, C.byref(good), None, 0.01, None, None) == -1 and "null batch" in L.twr_last_error().decode()
    assert L.twr_batch_eval_joint_scores(None, None, None, 0.01, None, None) == -1 and "null kin" in L.twr_last_error().decode()


def test_record_layout_constants():
    assert ta.joint_rec(4) == 21 and ta.joint_rec(1) == 6 and ta.JOINT_SCORE_REC == 8
    assert C.sizeof(ta.LegKinematics) == 4 * 5 + 4 + 8 * (12 + 3 + 3 + 2 + 6)
