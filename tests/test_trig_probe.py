"""sincos_fast, rotation() and rotation_quad() of kernels/spline_math.h against mpmath at 60 digits.

tests/trig_probe.hip is a stand-alone program that includes that header alone; it is compiled here, started as a fresh child
process per mode and fed seeded inputs that reach every quadrant, the neighbourhood of the multiples of pi/2 (where the
three-term reduction earns its keep), both sides of the 1e5 switch to the integer reduction of sincos_far, and the special
values.

  finite |x| < 1e5     sine and cosine each within 2 ulp of the reference value (1 ulp above the 1.38 ulp that the documented
                       recipe reaches with exact FMAs)
  1e5 <= |x| < inf     within 4 ulp, the OpenCL bound for double sin / cos.  (The device library's sincos, which this branch
                       called at first, misses it at 6381956970095103 * 2^797, the double closest to a multiple of pi/2:
                       its cosine, 4.69e-19, came out 405 ulp off.  sincos_far replaced the call.)
  +-0                  the sine keeps the sign of zero, the cosine is exactly 1
  +-Inf, NaN           both results are NaN
  rotation()           every entry of R within 16 * 2^-53 of the mpmath rotation (entries are at most 1, built from at most three
                       factors carrying <= 2 ulp each, plus one sum)
  rotation_quad()      the four lanes of a quad hold the same bits, and the bits of rotation() on the same triple -- also where
                       the three working lanes take different branches before the broadcast

The GPU tests print the worst case they measured (run with -s); DESIGN section 5 "Trigonometry" quotes them."""
import functools
import math
import os

import numpy as np
import pytest

from .probe import Probe

SWITCH = 1.0e5               # sincos_fast hands |x| >= SWITCH to sincos_far
K_FAST = 63661               # the largest k with k * pi/2 < SWITCH
HARD_CASE = math.ldexp(6381956970095103.0, 797)   # the double closest to a multiple of pi/2 (relative to its size)
ULP_FAST, ULP_LIB = 2.0, 4.0
ROT_TOL = 16.0 * 2.0 ** -53
N_TRIPLES = 4096


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath.mp


def _with_neighbours(v):
    """v, and the doubles one and two ulp below and above each"""
    v = np.asarray(v, dtype=np.float64)
    up1, dn1 = np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
    return np.stack([np.nextafter(dn1, -np.inf), dn1, v, up1, np.nextafter(up1, np.inf)], axis=1).ravel()


def _nearest_multiple(ks):
    mp = _mp()
    half_pi = mp.pi / 2
    return np.array([float(int(k) * half_pi) for k in ks], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def sincos_inputs():
    """name -> inputs of that family, in a fixed order (seeded)"""
    rng = np.random.default_rng(20261020)
    sign = lambda n: rng.choice([-1.0, 1.0], size=n)
    fam = {}
    fam["uniform"] = rng.uniform(-10.0, 10.0, 4096)
    fam["log_small"] = sign(4096) * np.clip(np.exp2(rng.uniform(-1074.0, math.log2(SWITCH), 4096)), 2.0 ** -1074, np.nextafter(SWITCH, 0.0))
    fam["multiples_all"] = _with_neighbours(_nearest_multiple(range(-64, 65)))
    fam["multiples_random"] = _with_neighbours(_nearest_multiple(rng.integers(-K_FAST, K_FAST + 1, 2000)))
    fam["switch"] = np.array([s * v for s in (1.0, -1.0) for v in (np.nextafter(SWITCH, 0.0), SWITCH, np.nextafter(SWITCH, np.inf))])
    fam["log_large"] = sign(2048) * np.clip(10.0 ** rng.uniform(5.0, 300.0, 2048), SWITCH, 1e300)
    fam["multiples_large"] = _nearest_multiple(np.exp2(rng.uniform(math.log2(K_FAST + 1), 52.0, 500)).astype(np.int64).clip(K_FAST + 1, 2 ** 52))
    fam["hard_case"] = np.array([HARD_CASE])
    tiny = 2.0 ** -1074
    dbl_min = 2.0 ** -1022
    fam["special"] = np.array([0.0, -0.0, tiny, -tiny, dbl_min, -dbl_min, np.inf, -np.inf, np.nan])
    return fam


COUNTS = {"uniform": 4096, "log_small": 4096, "multiples_all": 129 * 5, "multiples_random": 2000 * 5, "switch": 6, "log_large": 2048,
          "multiples_large": 500, "hard_case": 1, "special": 9}
# which sides of the switch the three angles of a mixed triple lie on (1 = at or above it): every pattern that diverges
MIXED_PATTERNS = [(0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]


@functools.lru_cache(maxsize=None)
def triple_inputs():
    """(triples[N_TRIPLES, 3], mixed[N_TRIPLES]): finite angles of the sincos families; a quarter near multiples of pi/2, a
    quarter anywhere below the switch, a quarter at or above it, and a quarter `mixed`: both sides inside one triple"""
    fam = sincos_inputs()
    rng = np.random.default_rng(77)
    near = np.concatenate([fam["multiples_all"], fam["multiples_random"]])
    small = np.concatenate([fam["uniform"], fam["log_small"], near, fam["switch"][np.abs(fam["switch"]) < SWITCH]])
    large = np.concatenate([fam["log_large"], fam["multiples_large"], fam["hard_case"], fam["switch"][np.abs(fam["switch"]) >= SWITCH]])
    q = N_TRIPLES // 4
    t = np.empty((N_TRIPLES, 3))
    t[:q] = rng.choice(near, (q, 3))
    t[q:2 * q] = rng.choice(small, (q, 3))
    t[2 * q:3 * q] = rng.choice(large, (q, 3))
    for i in range(q):
        for a, above in enumerate(MIXED_PATTERNS[i % 6]):
            t[3 * q + i, a] = rng.choice(large if above else small)
    mixed = np.zeros(N_TRIPLES, dtype=bool)
    mixed[3 * q:] = True
    return t, mixed


def _exponent(v):
    """floor(log2 |v|) of a non-zero mpf"""
    return v.exp + int(v.man).bit_length() - 1


def _ulp_of(v):
    """the spacing of doubles at the reference value v (an mpf)"""
    if v == 0:
        return math.ldexp(1.0, -1074)
    return math.ldexp(1.0, max(_exponent(v), -1022) - 52)


@functools.lru_cache(maxsize=None)
def _sincos_ref(values):
    """((sin, cos) as mpf) of every finite value, once"""
    mp = _mp()
    return [(mp.sin(mp.mpf(v)), mp.cos(mp.mpf(v))) for v in values]


def _ulp_error(got, ref):
    mp = _mp()
    return float(abs(mp.mpf(float(got)) - ref) / _ulp_of(ref))


# ------------------------------------------------------------------ running the probe (tests/probe.py)
# (plain flags of its own, not the product's CXXFLAGS as the other probes: other flags would change what it measures)
PROBE = Probe("trig_probe", flags=["-O3", "-std=c++17", "-Wall", "-Wextra"])


def _probe(mode):
    """the probe's output for `mode` on this file's inputs, from a child process of its own"""
    return PROBE.run(mode, np.concatenate(list(sincos_inputs().values())) if mode == "sincos" else triple_inputs()[0])


# ------------------------------------------------------------------ CPU tier
def test_probe_compiles_without_warning():
    """(CPU tier) hipcc compiles and links the probe for gfx950 without a GPU and without a warning"""
    assert os.path.exists(PROBE.build())
    PROBE.refuses([], None, "usage")


def test_inputs_cover_every_family():
    """(CPU tier) the generator produces every family with its count, all four quadrants below the switch, the values next
    to multiples of pi/2, both sides of the switch, and triples whose lanes diverge in every pattern"""
    fam = sincos_inputs()
    assert {k: len(v) for k, v in fam.items()} == COUNTS
    assert np.abs(fam["uniform"]).max() <= 10.0
    a = np.abs(fam["log_small"])
    assert a.min() >= 2.0 ** -1074 and a.max() < SWITCH and (a < 2.0 ** -1022).any() and (a > 1e4).any()
    for name in ("uniform", "log_small", "multiples_random", "log_large"):
        assert (fam[name] < 0).any() and (fam[name] > 0).any(), name
    for name in ("multiples_all", "multiples_random"):
        v = fam[name].reshape(-1, 5)
        assert np.abs(v).max() < SWITCH
        assert np.all(np.diff(v, axis=1) > 0), "five consecutive doubles around each multiple"
        k = np.rint(v[:, 2] * (2.0 / np.pi))
        mp = _mp()
        for vi, ki in zip(v[::37, 2], k[::37]):      # the middle one is the double nearest k * pi/2
            assert abs(mp.mpf(float(vi)) - int(ki) * mp.pi / 2) <= _ulp_of(mp.mpf(float(vi))) / 2
    assert set(np.rint(fam["multiples_all"].reshape(-1, 5)[:, 2] * (2.0 / np.pi)).astype(int)) == set(range(-64, 65))
    assert np.abs(fam["multiples_random"]).max() > 0.9 * SWITCH
    s = fam["switch"]
    assert sorted(np.abs(s)) == sorted(2 * [np.nextafter(SWITCH, 0.0), SWITCH, np.nextafter(SWITCH, np.inf)])
    a = np.abs(fam["log_large"])
    assert a.min() >= SWITCH and a.max() <= 1e300 and (a > 1e290).any() and (a < 1e15).any()
    a = np.abs(fam["multiples_large"])
    assert a.min() > K_FAST * np.pi / 2 and a.max() <= 2.0 ** 52 * np.pi / 2 * (1 + 1e-15) and (a > 1e14).any()
    assert fam["hard_case"][0] == 6381956970095103 * 2.0 ** 797
    sp = fam["special"]
    assert np.isnan(sp).sum() == 1 and np.isinf(sp).sum() == 2 and (sp == 0).sum() == 2 and np.signbit(sp[sp == 0]).sum() == 1
    assert (np.abs(sp) == 2.0 ** -1074).sum() == 2 and (np.abs(sp) == 2.0 ** -1022).sum() == 2

    below = np.concatenate([v for v in fam.values()])
    below = below[np.abs(below) < SWITCH]
    n = np.rint(below * (2.0 / np.pi)).astype(np.int64)
    for sgn in (-1, 1):                                   # n & 3 of a negative n is its own case
        assert set(np.unique(n[sgn * n > 0] & 3)) == {0, 1, 2, 3}

    t, mixed = triple_inputs()
    assert t.shape == (N_TRIPLES, 3) and np.isfinite(t).all() and mixed.sum() == N_TRIPLES // 4
    above = np.abs(t) >= SWITCH
    patterns = {tuple(int(b) for b in row) for row in above[mixed]}
    assert patterns == set(MIXED_PATTERNS)
    assert (above.sum(axis=1) == 0).sum() >= N_TRIPLES // 2 and (above.sum(axis=1) == 3).sum() >= N_TRIPLES // 4


# ------------------------------------------------------------------ GPU tier
def _check_sincos(x, s, c, what):
    """the ulp bounds on finite inputs; returns (worst ulp below the switch, worst at or above it)"""
    ref = _sincos_ref(tuple(float(v) for v in x))
    worst = {True: (0.0, None), False: (0.0, None)}
    bad = []
    for xi, si, ci, (rs, rc) in zip(x, s, c, ref):
        fast = abs(xi) < SWITCH
        e = max(_ulp_error(si, rs), _ulp_error(ci, rc)) if np.isfinite(si) and np.isfinite(ci) else float("inf")
        if e > worst[fast][0]:
            worst[fast] = (e, xi)
        if not e <= (ULP_FAST if fast else ULP_LIB):
            bad.append((float(xi), float(si), float(ci), e))
    print("\n%s: worst error" % what, " and ".join("%.3f ulp at x = %r %s" % (e, float(xi), side) for (e, xi), side in
                                                     ((worst[True], "below 1e5"), (worst[False], "at or above 1e5")) if xi is not None))
    assert not bad, "%s: %d results off, e.g. (x, sin, cos, ulp) %s" % (what, len(bad), bad[:5])
    return worst[True][0], worst[False][0]


@pytest.mark.gpu
def test_sincos_fast_against_mpmath():
    fam = sincos_inputs()
    x = np.concatenate(list(fam.values()))
    out = _probe("sincos").reshape(-1, 2)
    assert out.shape[0] == x.size
    s, c = out[:, 0], out[:, 1]
    finite = np.isfinite(x)
    at, worst = 0, (0.0, 0.0)
    for name, v in fam.items():                # (one line per family)
        sl = slice(at, at + len(v))
        at += len(v)
        ok = finite[sl]
        worst = tuple(map(max, worst, _check_sincos(x[sl][ok], s[sl][ok], c[sl][ok], "sincos_fast, %s (%d inputs)" % (name, ok.sum()))))
    print("sincos_fast, all %d finite inputs: worst error %.3f ulp below 1e5, %.3f ulp at or above it" % ((finite.sum(),) + worst))
    zero = x == 0
    assert np.array_equal(np.signbit(s[zero]), np.signbit(x[zero])) and np.all(s[zero] == 0), "the sine of +-0 keeps the sign of zero"
    assert np.all(c[zero] == 1.0), "the cosine of +-0 is exactly 1"
    assert np.isnan(s[~finite]).all() and np.isnan(c[~finite]).all(), "+-Inf and NaN give NaN"


def _rotation_ref(t):
    """R (row-major, 9 mpf) of one triple"""
    (sx, cx), (sy, cy), (sz, cz) = _sincos_ref(tuple(float(v) for v in t))
    return [cy * cz, cz * sx * sy - cx * sz, sx * sz + cx * cz * sy,
            cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx,
            -sy, cy * sx, cx * cy]


@pytest.mark.gpu
def test_rotation_against_mpmath():
    mp = _mp()
    t, _ = triple_inputs()
    out = _probe("rot").reshape(N_TRIPLES, 15)
    assert np.isfinite(out).all()
    _check_sincos(t.ravel(), out[:, 9::2].ravel(), out[:, 10::2].ravel(), "rotation(), the six sines and cosines of %d triples" % N_TRIPLES)
    worst, where = 0.0, None
    for i in range(N_TRIPLES):
        for k, r in enumerate(_rotation_ref(t[i])):
            e = float(abs(mp.mpf(float(out[i, k])) - r))
            if e > worst:
                worst, where = e, (i, k)
    print("rotation(): worst entry error %.3g = %.2f x 2^-53 (triple %s %r)" % (worst, worst * 2.0 ** 53, where, t[where[0]].tolist() if where else None))
    assert worst <= ROT_TOL


@pytest.mark.gpu
def test_rotation_quad_is_rotation_bit_for_bit():
    t, mixed = triple_inputs()
    one = _probe("rot").reshape(N_TRIPLES, 1, 15).view(np.int64)
    quad = _probe("rotquad").reshape(N_TRIPLES, 4, 15).view(np.int64)
    lanes_differ = np.nonzero((quad != quad[:, :1]).any(axis=(1, 2)))[0]
    assert lanes_differ.size == 0, "the lanes of %d quads disagree (%d of them mixed-branch), first: triple %d %r" % (
        lanes_differ.size, mixed[lanes_differ].sum(), lanes_differ[0], t[lanes_differ[0]].tolist())
    differ = np.nonzero((quad != one).any(axis=(1, 2)))[0]
    assert differ.size == 0, "rotation_quad differs from rotation() on %d triples (%d of them mixed-branch), first: triple %d %r" % (
        differ.size, mixed[differ].sum(), differ[0], t[differ[0]].tolist())
