"""tests/check_points.py checks_numpy, the restatement tests/test_checks.py holds the device to, on cases worked by hand (slots and
signs named) and, for the dynamics residual, against mpmath at 40 digits within a bound counted from the operations.  No GPU."""
import functools

import numpy as np

import towr_amd as ta

from . import check_points as cp
from .common import Case


@functools.lru_cache(maxsize=None)
def go1():
    return cp.consts_of(ta.model_preset("go1", "flat"))


def standing(consts, base_z=None):
    """one record: the base at rest over the origin with the identity attitude, the feet in the nominal stance on z = 0, all in
    contact, each carrying a quarter (1 / n_ee) of the weight"""
    n_ee = consts["n_ee"]
    r = np.zeros(20 + 13 * n_ee)
    r[3] = -consts["nominal"][0][2] if base_z is None else base_z
    r[10] = 1.0
    for e in range(n_ee):
        l = r[20 + 13 * e:33 + 13 * e]
        l[0] = 1.0
        l[1:3] = consts["nominal"][e][:2]
        l[12] = consts["mass"] * consts["gravity"] / n_ee
    return r


def test_static_stance_on_flat_ground_is_in_balance():
    c = go1()
    assert c["n_ee"] == 4 and c["mu"] > 0
    out = cp.checks_numpy(standing(c), c, cp.flat_terrain(0.0))[0]
    assert out[0] == 0.0
    assert (out[1:7] == 0.0).all(), "angular (1:4) and linear (4:7) residual vanish exactly: %r" % out[1:7].tolist()
    legs = cp.legs_of(out[None], 4)[0]
    fz = c["mass"] * c["gravity"] / 4
    assert (legs[:, cp.CONTACT] == 1.0).all() and (legs[:, cp.CLEAR] == 0.0).all()
    assert (legs[:, cp.FN] == fz).all() and (legs[:, cp.CONE] == c["mu"] * fz).all()
    # the feet sit on the nominal stance: every |foot_B - nominal| is 0, rom is the largest -max_dev
    assert (legs[:, cp.ROM] == -c["max_dev"].min()).all() and (legs[:, cp.ROM] < 0).all()
    s = cp.fold(out[None], 4)
    assert s.tolist() == [1.0, 0.0, 0.0, 1e20, 0.0, fz, c["mu"] * fz, -c["max_dev"].min()]


def test_signs_of_the_residual():
    """a missing force leaves +m g on linear z; a force too many on foot 0 leaves -f there and its moment f x (p_base - p_0) with
    the sign of GetDynamicViolation on the angular rows"""
    c = go1()
    r = standing(c)
    for e in range(4):
        r[20 + 13 * e + 12] = 0.0
    out = cp.checks_numpy(r, c, cp.flat_terrain())[0]
    assert out[6] == c["mass"] * c["gravity"] and (out[1:6] == 0.0).all()
    r = standing(c)
    r[20 + 12] += 10.0
    out = cp.checks_numpy(r, c, cp.flat_terrain())[0]
    d = r[1:4] - r[21:24]
    assert abs(out[6] + 10.0) < 1e-12 and abs(out[1] + (-10.0 * d[1])) < 1e-12 and abs(out[2] + 10.0 * d[0]) < 1e-12 and out[3] == 0.0
    # an acceleration: m a on the linear rows
    r = standing(c)
    r[7:10] = [0.5, -0.25, 2.0]
    out = cp.checks_numpy(r, c, cp.flat_terrain())[0]
    assert np.allclose(out[4:7], c["mass"] * np.array([0.5, -0.25, 2.0]), rtol=0, atol=1e-12)


def test_a_tangential_force_of_mu_fn_is_on_the_cone():
    c = go1()
    fz = 40.0
    for slot, sign in ((10, 1.0), (10, -1.0), (11, 1.0), (11, -1.0)):
        r = standing(c)
        r[20 + 13 * 2 + 12] = fz
        r[20 + 13 * 2 + slot] = sign * c["mu"] * fz
        legs = cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0]
        assert legs[2, cp.FN] == fz and legs[2, cp.CONE] == 0.0
        r[20 + 13 * 2 + slot] *= 1.5
        assert cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0][2, cp.CONE] == -0.5 * c["mu"] * fz, "outside: negative"
    # a pulling force: f_n < 0 and the cone with it
    r = standing(c)
    r[20 + 12] = -5.0
    legs = cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0]
    assert legs[0, cp.FN] == -5.0 and legs[0, cp.CONE] == -5.0 * c["mu"]


def test_a_foot_one_centimetre_under_a_stairs_tread():
    case = Case("go1", "stairs", ta.gait_combo(4, 0, 1.2))
    c = cp.consts_of(case.model)
    terrain = cp.oracle_terrain(case.P)
    r = standing(c)
    for e, (x, z) in enumerate(((1.2, 0.19), (0.99, 0.05), (1.45, 0.4), (2.5, -0.02))):     # first tread, before it, second tread, behind
        r[20 + 13 * e + 1], r[20 + 13 * e + 3] = x, z
    legs = cp.legs_of(cp.checks_numpy(r, c, terrain), 4)[0]
    assert legs[0, cp.CLEAR] == 0.19 - 0.2 and abs(legs[0, cp.CLEAR] + 0.01) < 1e-15
    assert legs[1, cp.CLEAR] == 0.05 and legs[2, cp.CLEAR] == 0.0 and legs[3, cp.CLEAR] == -0.02
    s = cp.fold(cp.checks_numpy(r, c, terrain), 4)
    assert s[3] == 1e20 and s[4] == 0.05, "all four in contact: no swing clearance, the largest |clearance| of a stance foot"
    r[20] = r[20 + 13] = 0.0
    s = cp.fold(cp.checks_numpy(r, c, terrain), 4)
    assert s[3] == 0.19 - 0.2 and s[4] == 0.02, "feet 0 and 1 swing: the lowest clearance is the foot under the tread"


def test_a_foot_on_the_face_of_the_range_of_motion_box():
    c = dict(go1())
    c["nominal"] = np.array([[0.25, 0.125, -0.5], [0.25, -0.125, -0.5], [-0.25, 0.125, -0.5], [-0.25, -0.125, -0.5]])   # dyadic: every
    c["max_dev"] = np.array([0.125, 0.0625, 0.125])                                                                    # sum below is exact
    r = standing(c, base_z=0.5)
    for e, d in enumerate((0, 1, 2, 0)):
        r[20 + 13 * e + 1 + d] += (-1.0 if e == 3 else 1.0) * c["max_dev"][d]
    legs = cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0]
    assert (legs[:, cp.ROM] == 0.0).all(), legs[:, cp.ROM].tolist()
    r[20 + 13 + 2] += 0.03125          # foot 1 a further 1/32 m out along y: outside by that much
    r[20 + 1] -= 0.03125               # foot 0 back inside along x: the nearest face is now y's, 1/16 m away
    legs = cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0]
    assert legs[1, cp.ROM] == 0.03125 and legs[0, cp.ROM] == -0.03125
    # the box is the base's: a yaw of 90 degrees turns a foot ahead of the base into one beside it
    r = standing(c, base_z=0.5)
    r[10:14] = [np.sqrt(0.5), 0.0, 0.0, np.sqrt(0.5)]
    legs = cp.legs_of(cp.checks_numpy(r, c, cp.flat_terrain()), 4)[0]
    assert abs(legs[0, cp.ROM] - (abs(-0.25 - 0.125) - 0.0625)) < 1e-15      # foot_B = (y, -x, z) = (0.125, -0.25, -0.5): y is worst


def test_nan_in_one_leg_stays_in_its_fields_and_the_residual():
    c = go1()
    clean = cp.checks_numpy(standing(c), c, cp.flat_terrain())[0]
    r = standing(c)
    r[20 + 13 * 1 + 11] = np.nan
    out = cp.checks_numpy(r, c, cp.flat_terrain())[0]
    legs, was = cp.legs_of(out[None], 4)[0], cp.legs_of(clean[None], 4)[0]
    assert np.isnan(legs[1, [cp.FN, cp.CONE]]).all() and legs[1, cp.CLEAR] == 0.0 and legs[1, cp.ROM] == was[1, cp.ROM]
    assert np.array_equal(legs[[0, 2, 3]], was[[0, 2, 3]])
    s = cp.fold(out[None], 4)
    assert np.isnan(s[[1, 2, 5, 6]]).all() and s[3] == 1e20 and s[4] == 0.0 and s[7] == was[0, cp.ROM]


def test_residual_against_mpmath_within_the_counted_bound():
    c = go1()
    rec = cp.random_records(200, c, seed=5)
    got = cp.checks_numpy(rec, c, cp.flat_terrain())[:, 1:7]
    bound = cp.C_CHECK * cp.U * cp.residual_scales(rec, c)
    assert cp.C_CHECK == 61.0 and (bound > 0).all()
    import mpmath
    worst = 0.0
    for k in range(len(rec)):
        want = cp.residual_mp(rec[k], c, dps=40)
        for j in range(6):
            err = float(abs(mpmath.mpf(float(got[k, j])) - want[j]))
            worst = max(worst, err / bound[k, j])
            assert err <= bound[k, j], (k, j, err / bound[k, j])
    print("\nresidual against mpmath, %d records: worst error %.4f of the bound" % (len(rec), worst))
    assert worst > 1e-4, "the bound is of the order of the error, not a formality"
