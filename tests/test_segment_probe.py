"""locate_segment (kernels/spline_math.h), phase_poly_durations_wave (kernels/phase_durations.h) and hermite_all on every junction
threshold, against the reference's recorded answers.

tests/segment_probe.hip is a stand-alone program that includes those two headers and what they include, nothing else of the
product; it is compiled here with the product's CXXFLAGS for kernels.o, started as a fresh child process per mode and fed the
points of tests/segment_points.py: per duration list and junction the accumulated sum A_i, the largest double t with
fl(t - 1e-10) <= A_i, the doubles one and two ulp on each side of both, +-0, the grid times of the optimised-timings structures
and 16 uniform times per segment; lists of every length 1 .. 17 and of 31, 32, 63, 64, with zero durations, durations below
1e-10 and thirds that do not sum back.

References
  lookup        tests/golden/refsegment.npz: Spline::GetSegmentID / GetLocalTime themselves, recorded by oracle/ref_golden.py
                --segments through ref_dump --segment-points.  The oracle and mp_ref.locate in doubles must equal it bit for bit
                (CPU tier).  Where the reference finds no segment it is undefined and was never asked: the device is held to
                segment_points.convention (id = n - 1, t_local = t minus the durations before the last, one after the other).
  durations     the same file: PhaseDurations::SetVariables + ConvertPhaseToPolyDurations on given schedule variables.
  hermite_all   mpmath at 60 digits on polynomial.cc:140-234 at the exact (t, T), the device being given iT = fl(1 / T).
Bounds for the device
  lookup, durations   bit-equal: every operation is one correctly rounded add, subtract or divide on both sides and nothing can
                be contracted.
  hermite_all   per weight C_HERMITE * 2^-53 * sum |terms|, the terms being the weight's monomials in t and 1 / T.  C_HERMITE =
                10 counts the roundings of the longest chain, an operation's count being those of its operands plus one and a
                multiplication by a power of two counting nothing: iT = fl(1 / T) 1, iT2 = iT * iT 3, iT3 = iT2 * iT 5, t2 1,
                t3 = t2 * t 2, the term 2 t3 iT3 of w_p0 2 + 5 + 1 = 8, and the two additions that follow it 10.  (The velocity
                weights reach 9: 6 t2 is 2, times iT3 8, one subtraction; the acceleration weights 8.)  Contraction into
                fused multiply-adds only removes roundings.  The doubles next to 0 itself are subnormal, where products
                underflow and no relative bound holds; what the lookup yields one and two ulp of a junction sum past that
                junction (t_local of 1e-16 and the like) stands in for them.

The GPU tests print the worst case they measured as a fraction of the bound (run with -s); DESIGN section 5 "Segment junctions"
quotes it."""
import functools
import os
import tempfile

import numpy as np
import pytest

from oracle import binding as ob
from oracle import mp_ref, ref_golden, ref_run

from . import segment_points as sp
from .probe import GOLDEN, Probe, load_fixture, bits as _bits    # (the assertions below keep the name they were written with)

U = 2.0 ** -53
C_HERMITE = 10.0     # the roundings of the longest chain of hermite_all (w_p0), counted in the docstring
MAX_PHASES, MAX_POLYS = 32, 64
DUR_OUT = MAX_PHASES + 2 * MAX_POLYS


def fixture():
    return load_fixture("refsegment")


def fixture_case(k):
    """(ph, md, fd) the reference gave for duration case k"""
    f = fixture()
    n_before = int(f["case_head"][:k, 0].sum())
    n = int(f["case_head"][k, 0])
    return (f["case_ph"][n_before:n_before + n], f["case_md"][f["case_md_start"][k]:f["case_md_start"][k + 1]],
            f["case_fd"][f["case_fd_start"][k]:f["case_fd_start"][k + 1]])


# ------------------------------------------------------------------ running the probe (tests/probe.py)
PROBE = Probe("segment_probe")


@functools.lru_cache(maxsize=None)
def hermite_points():
    """(n, 2) of (t_local, T): what the lookup produced at the defined points of the perturbed structure lists that carry a
    grid and of the lists with durations below eps or thirds that do not sum back, and per duration T of those lists 0, T and
    T's neighbours"""
    f, p = fixture(), sp.points()
    keep = np.array([(grid is not None and "/perturbed/" in name) or name.startswith(("thirds", "sixths", "below_eps", "close_pair"))
                     for name, _, grid, _ in sp.lists()])
    sel = keep[f["point_list"]]
    T = p["durations"][p["list_start"][f["point_list"][sel].astype(np.int64)] + f["seg_id"][sel]]
    pairs = [np.column_stack([f["t_local"][sel], T])]
    for dur in np.unique(T):
        pairs.append(np.array([(t, dur) for t in [0.0] + sp.neighbours(float(dur))]))
    out = np.concatenate(pairs)
    out = out[out[:, 1] > 0.0]
    out = np.unique(out, axis=0)
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def hermite_reference():
    """(weights (n, 12), sum of |terms| (n, 12)) of d{pos, vel, acc}/d{p0, v0, p1, v1} (polynomial.cc:140-234) at
    hermite_points(), mpmath at 60 digits, rounded to doubles only for the comparison (kept as mpf)"""
    import mpmath
    mpmath.mp.dps = 60
    mpf = mpmath.mpf
    W, S = [], []
    for t, T in hermite_points():
        t, T = mpf(float(t)), mpf(float(T))
        s = t / T
        s2, s3 = s * s, s * s * s
        a = abs
        terms = [[2 * s3, -3 * s2, 1], [t, -2 * t * s, t * s2], [3 * s2, -2 * s3], [t * s2, -t * s],
                 [6 * s2 / T, -6 * s / T], [3 * s2, -4 * s, 1], [6 * s / T, -6 * s2 / T], [3 * s2, -2 * s],
                 [12 * s / T ** 2, -6 / T ** 2], [6 * s / T, -4 / T], [6 / T ** 2, -12 * s / T ** 2], [6 * s / T, -2 / T]]
        W.append([mpmath.fsum(x) for x in terms])
        S.append([mpmath.fsum(a(v) for v in x) for x in terms])
    return W, S


def locate_input():
    p = sp.points()
    parts = [[float(len(p["list_start"]) - 1)]]
    for k in range(len(p["list_start"]) - 1):
        d = sp.list_of(k)
        parts += [[float(len(d))], d]
    parts += [[float(len(p["point_t"]))], np.column_stack([p["point_list"].astype(np.float64), p["point_t"]]).ravel()]
    return np.concatenate([np.asarray(v, dtype=np.float64) for v in parts])


def durations_input():
    parts = [[float(len(sp.duration_cases()))]]
    for n, contact, pps, ppf, given, variables in sp.duration_cases():
        parts += [[float(n), float(contact), float(pps), float(ppf), sp.sums(given)[-1]], variables]
    return np.concatenate([np.asarray(v, dtype=np.float64) for v in parts])


def hermite_input():
    h = hermite_points()
    return np.concatenate([[float(len(h))], np.column_stack([h[:, 0], 1.0 / h[:, 1]]).ravel()])


def _probe(mode):
    """the probe's raw output for `mode`, from a child process of its own; a failed run is remembered and not started again,
    and after a device failure no probe is (the failure rule of tests/probe.py)"""
    data = {"locate": locate_input, "durations64": durations_input, "durations256": durations_input, "hermite": hermite_input}[mode]()
    return PROBE.run(mode, data)


# ------------------------------------------------------------------ CPU tier
def test_probe_compiles_without_warning():
    """(CPU tier) hipcc compiles and links the probe for gfx950 with the product's flags, without a GPU and without a warning;
    the input parser refuses a file whose counts do not add up before anything reaches a device"""
    PROBE.refuses([], None, "usage")
    for mode, data in (("locate", locate_input()), ("durations64", durations_input()), ("hermite", hermite_input())):
        PROBE.refuses([mode], data[:-1], "truncated")
    PROBE.refuses(["locate"], np.concatenate([[1.0, 65.0], np.full(65, 0.1), [1.0, 0.0, 0.05]]), "list length")


def test_points_cover_what_they_claim():
    """(CPU tier) the point set holds what the module's docstring says, and the threshold doubles are thresholds"""
    p = sp.points()
    n = len(p["point_t"])
    assert 20000 <= n <= 45000, n
    lengths = set(int(v) for v in np.diff(p["list_start"]))
    assert set(sp.LENGTHS) <= lengths
    assert p["defined"].sum() >= 20000 and (~p["defined"]).sum() >= 2 * (len(p["list_start"]) - 1)
    assert np.all(np.diff(p["point_list"]) >= 0), "ordered by list"
    for k in range(len(p["list_start"]) - 1):
        d = sp.list_of(k)
        mine = set(_bits(p["point_t"][p["point_list"] == k]).tolist())
        for acc in sp.sums(d):
            thr = sp.threshold(acc)
            up = float(np.nextafter(thr, np.inf))
            assert sp.reaches(acc, thr) and not sp.reaches(acc, up)
            assert {int(_bits([v])[0]) for v in sp.neighbours(acc) + sp.neighbours(thr)} <= mine
        assert {int(_bits([0.0])[0]), int(_bits([-0.0])[0])} <= mine
    # the defined and the undefined points meet at the total's threshold
    ids, _tl, found = sp.expected_convention()
    assert np.array_equal(found, p["defined"])
    last = np.diff(p["list_start"])[p["point_list"]] - 1
    assert np.all(ids[~found] == last[~found])


def test_fixture_holds_the_points():
    """(CPU tier) refsegment.npz was recorded at exactly the defined points and the duration cases of tests/segment_points.py"""
    f, p = fixture(), sp.points()
    sel = p["defined"]
    assert np.array_equal(f["list_start"], p["list_start"]) and np.array_equal(_bits(f["durations"]), _bits(p["durations"]))
    assert np.array_equal(f["point_list"], p["point_list"][sel]) and np.array_equal(_bits(f["point_t"]), _bits(p["point_t"][sel]))
    cases = sp.duration_cases()
    assert np.array_equal(f["case_head"], np.array([c[:4] for c in cases], dtype=np.int32))
    assert np.array_equal(_bits(f["case_given"]), _bits(np.concatenate([c[4] for c in cases])))
    assert np.array_equal(_bits(f["case_vars"]), _bits(np.concatenate([c[5] for c in cases])))
    assert os.path.getsize(os.path.join(GOLDEN, "refsegment.npz")) < 600 * 1024


def test_oracle_and_mp_ref_equal_the_reference_bit_for_bit():
    """(CPU tier) the oracle's NodeSpline::GetLocalTime, mp_ref.locate run in doubles and the stated convention all give the
    recorded id and the recorded bits of t_local at every defined point; the oracle finds no segment at every undefined one"""
    f, p = fixture(), sp.points()
    ids_c, tl_c, _found = sp.expected_convention()
    sel = p["defined"]
    assert np.array_equal(ids_c[sel], f["seg_id"]) and np.array_equal(_bits(tl_c[sel]), _bits(f["t_local"]))
    for k in range(len(p["list_start"]) - 1):
        d = sp.list_of(k)
        mine = p["point_list"] == k
        ids, tl = ob.locate(d, p["point_t"][mine])
        inside = sel[mine]
        frows = f["point_list"] == k
        assert np.array_equal(ids[inside], f["seg_id"][frows]), sp.lists()[k][0]
        assert np.array_equal(_bits(tl[inside]), _bits(f["t_local"][frows])), sp.lists()[k][0]
        assert np.all(ids[~inside] == -1)
        dl = [float(v) for v in d]
        got = [mp_ref.locate(float(t), dl) for t in p["point_t"][mine][inside]]
        assert [g[0] for g in got] == f["seg_id"][frows].tolist()
        assert np.array_equal(_bits([g[1] for g in got]), _bits(f["t_local"][frows])), sp.lists()[k][0]


def test_duration_conversion_equals_the_reference_bit_for_bit():
    """(CPU tier) PhaseDurations::SetVariables + ConvertPhaseToPolyDurations: the oracle and the plain-double restatement the
    lists are built with give the recorded bits"""
    for k, case in enumerate(sp.duration_cases()):
        ref = fixture_case(k)
        for got in (sp.case_lists(case), ob.phase_poly_durations(*case)):
            for a, b in zip(got, ref):
                assert len(a) == len(b) and np.array_equal(_bits(a), _bits(b)), (k, case[:4])


def test_phase_and_polynomial_lookups_disagree_at_thresholds():
    """(CPU tier) the reference takes current_phase from the phase durations and the polynomial from the polynomial durations,
    whose accumulated sums differ by rounding: the points hold times at which the polynomial found lies in another phase than
    the phase lookup says -- in the recorded reference itself"""
    f = fixture()
    names = [name for name, _, _, _ in sp.lists()]
    index = {name: k for k, name in enumerate(names)}
    contact = {"%s/ee%d" % (s[0], s[1]): s[2] for s in sp.structure_schedules()}
    disagree = 0
    for k, name in enumerate(names):
        head, _, kind = name.rpartition("/")
        if not kind.startswith("motion") or head + "/phase" not in index or head.rpartition("/")[0] not in contact:
            continue
        n = int(kind[len("motion"):])
        rows_m, rows_p = f["point_list"] == k, f["point_list"] == index[head + "/phase"]
        phase_of = []
        constant = contact[head.rpartition("/")[0]]
        for ph in range(len(sp.list_of(index[head + "/phase"]))):
            phase_of += [ph] * (1 if constant else n)
            constant = not constant
        tm = dict(zip(_bits(f["point_t"][rows_m]).tolist(), f["seg_id"][rows_m].tolist()))
        tp_ = dict(zip(_bits(f["point_t"][rows_p]).tolist(), f["seg_id"][rows_p].tolist()))
        disagree += sum(1 for b in tm.keys() & tp_.keys() if phase_of[tm[b]] != tp_[b])
    assert disagree >= 10, disagree


def test_recorder_refuses_undefined_points_and_reproduces_the_fixture():
    """(CPU tier, where the reference is built) ref_dump --segment-points exits with code 5 for a time beyond the last
    threshold, and a fresh recording equals the committed file"""
    if not ref_run.available():
        pytest.skip("oracle/_ref/ref_dump is not built on this box")
    with tempfile.TemporaryDirectory() as work:
        d = [0.3, 0.2]
        thr = sp.threshold(sp.sums(d)[-1])
        ids, tl = ref_run.segment_points(os.path.join(work, "a"), [d], [0], [thr])
        assert ids[0] == 1 and tl[0] == thr - 0.3
        with pytest.raises(RuntimeError, match="exit 5"):
            ref_run.segment_points(os.path.join(work, "b"), [d], [0], [float(np.nextafter(thr, np.inf))])
        out, f = ref_golden.compute_segments(work), fixture()
        for key in f:
            if key != "reference_deps":
                assert out[key].dtype == f[key].dtype and np.array_equal(out[key].view(np.uint8), f[key].view(np.uint8)), key


# ------------------------------------------------------------------ GPU tier
@pytest.mark.gpu
def test_locate_segment_on_device():
    """locate_segment on durations staged in LDS, one lane per (list, t): the recorded id and the recorded bits of t_local at
    every defined point, the stated convention at every undefined one"""
    f, p = fixture(), sp.points()
    raw = _probe("locate").reshape(-1, 2)
    assert len(raw) == len(p["point_t"]) and not np.isnan(raw[:, 0]).any()
    ids, tl = raw[:, 0].astype(np.int64), raw[:, 1]
    sel = p["defined"]
    bad = np.nonzero((ids[sel] != f["seg_id"]) | (_bits(tl[sel]) != _bits(f["t_local"])))[0]
    names = [name for name, _, _, _ in sp.lists()]
    print("\nlocate: %d defined points, %d differ from the reference" % (sel.sum(), len(bad)))
    assert len(bad) == 0, "%d points differ, first: list %s t = %r: device (%d, %r), reference (%d, %r)" % (
        len(bad), names[f["point_list"][bad[0]]], f["point_t"][bad[0]], ids[sel][bad[0]], tl[sel][bad[0]], f["seg_id"][bad[0]],
        f["t_local"][bad[0]])
    ids_c, tl_c, _found = sp.expected_convention()
    und = ~sel
    bad = np.nonzero((ids[und] != ids_c[und]) | (_bits(tl[und]) != _bits(tl_c[und])))[0]
    print("locate: %d undefined points, %d differ from the convention" % (und.sum(), len(bad)))
    assert len(bad) == 0, "%d undefined points differ from id = n - 1, t_local = t - sum of the others" % len(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("threads", [64, 256])
def test_phase_poly_durations_on_device(threads):
    """phase_poly_durations_wave on a hand-filled PhaseTables / PhasePoly blob, called by 64 and by 256 threads: ph (the last
    duration t_total - sum included), the ee-motion and the ee-force polynomial durations bit for bit the reference's"""
    raw = _probe("durations%d" % threads).reshape(-1, DUR_OUT)
    assert len(raw) == len(sp.duration_cases())
    for k, case in enumerate(sp.duration_cases()):
        ph, md, fd = fixture_case(k)
        for got, ref, what in ((raw[k, :MAX_PHASES], ph, "ph"), (raw[k, MAX_PHASES:MAX_PHASES + MAX_POLYS], md, "md"),
                               (raw[k, MAX_PHASES + MAX_POLYS:], fd, "fd")):
            assert np.array_equal(_bits(got[:len(ref)]), _bits(ref)), (k, case[:4], what)
            assert np.isnan(got[len(ref):]).all(), (k, case[:4], what, "written beyond its count")


@pytest.mark.gpu
def test_hermite_all_on_device():
    """hermite_all at t_local in {0, T, T's neighbours, what the lookup produced} with iT = fl(1 / T), within C_HERMITE * 2^-53
    * sum |terms| of the 60-digit value per weight"""
    import mpmath
    raw = _probe("hermite").reshape(-1, 12)
    W, S = hermite_reference()
    assert len(raw) == len(W) and not np.isnan(raw).any()
    worst, at = 0.0, None
    for i in range(len(W)):
        for j in range(12):
            bound = C_HERMITE * U * S[i][j]
            err = abs(mpmath.mpf(float(raw[i, j])) - W[i][j])
            if bound == 0:      # every term is zero (t = 0): so is the weight, exactly
                assert err == 0, (tuple(hermite_points()[i]), j, raw[i, j])
                continue
            frac = float(err / bound)
            if frac > worst:
                worst, at = frac, (i, j)
    print("\nhermite_all: %d points, worst error %.3f of the bound (point %r, weight %d)" % (len(W), worst, tuple(hermite_points()[at[0]]), at[1]))
    assert worst <= 1.0
