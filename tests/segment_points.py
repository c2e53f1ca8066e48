"""The points at which the segment lookup of kernels/spline_math.h (locate_segment) can decide otherwise than the reference's
Spline::GetSegmentID / GetLocalTime (spline.cc:48-78): duration lists and, per list, times on and next to every junction
threshold.  Seeded and deterministic; shared by tests/test_segment_probe.py (the CPU tier and the device probe) and
oracle/ref_golden.py --segments (the recorded reference).  Needs no GPU.

The lookup returns the first i with A_i >= fl(t - EPS), A_i the sequentially accumulated sum of the durations.  Per list and
junction the times are A_i, the threshold double (the LARGEST t with fl(t - EPS) <= A_i, found by bisection on that predicate
in plain doubles: fl(A_i + EPS) is it at most junctions, not at all) and the doubles one and two ulp on each side of both; +0 and -0; the
grid times of the structures the lists come from; 16 uniform times inside every segment.

A time for which no accumulated sum reaches fl(t - EPS) is outside what the reference defines (it runs past assert(false)):
those points are kept apart (`defined` is False), are never sent to the reference, and the device is held to the project's own
convention there -- convention() below."""
import functools
import struct

import numpy as np

EPS = 1e-10                      # spline.cc:51
P40 = ("p40", "p40a", "p40p3", "p40p4", "p40p6")       # the optimised-timings structures of tests/eval_matrix.py
N_IN_PHASE = (1, 2, 3, 4, 5, 6)
LENGTHS = tuple(range(1, 18)) + (31, 32, 63, 64)       # every remainder of the loop unrolled by 8, both host limits (32, 64)
N_UNIFORM = 16


def _bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def reaches(acc, t):
    """the reference's only decision (spline.cc:58)"""
    return acc >= t - EPS


def threshold(acc):
    """the largest double t with fl(t - EPS) <= acc, for acc >= 0 (the predicate is monotone in t: bisection on the bit
    patterns, which order non-negative doubles)"""
    lo, hi = _bits(acc + 0.0), _bits(acc + 4.0 * EPS + 4.0 * np.spacing(acc))
    assert reaches(acc, _from_bits(lo)) and not reaches(acc, _from_bits(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if reaches(acc, _from_bits(mid)):
            lo = mid
        else:
            hi = mid
    return _from_bits(lo)


def neighbours(v):
    """v and the doubles one and two ulp below and above (a negative neighbour of 0 is left out: t < 0 is not defined)"""
    out = [v]
    for towards in (-np.inf, np.inf):
        w = v
        for _ in range(2):
            w = float(np.nextafter(w, towards))
            out.append(w)
    return [w for w in out if w >= 0.0]


def sums(d):
    """A_i: the sequentially accumulated sums of the list"""
    acc, out = 0.0, []
    for v in d:
        acc += float(v)
        out.append(acc)
    return out


def convention(d, t):
    """(id, t_local, found) of the lookup as the project states it: the reference's where a segment is found; otherwise
    id = n - 1 and t_local = t minus the durations before the last one, subtracted one after the other"""
    n, acc, tl = len(d), 0.0, t
    for i in range(n):
        acc += float(d[i])
        if reaches(acc, t):
            return i, tl, True
        if i < n - 1:
            tl -= float(d[i])
    return n - 1, tl, False


def poly_durations(ph, first_constant, n_changing):
    """ConvertPhaseToPolyDurations (nodes_variables_phase_based.cc:38-84): one polynomial per constant phase, n_changing per
    changing phase, each phase / n_in_phase by one IEEE division"""
    out, constant = [], first_constant
    for p in ph:
        n = 1 if constant else n_changing
        out += [float(p) / n] * n
        constant = not constant
    return out


def set_variables(given, variables):
    """PhaseDurations::SetVariables (phase_durations.cc:77-103): the last duration fills up to the given total, both sums
    accumulated one after the other"""
    total = 0.0
    for v in given:
        total += float(v)
    s = 0.0
    for v in variables:
        s += float(v)
    return [float(v) for v in variables] + [total - s]


# ------------------------------------------------------------------------------------------------------------ lists
@functools.lru_cache(maxsize=None)
def structure_schedules():
    """[(structure name, foot, in contact at start, given durations, dt, T)] of the P40 structures, equal schedules once"""
    from . import eval_matrix as em

    out, seen = [], set()
    for name in P40:
        case = em.make_case(name)
        durs, contact = case.sched.durations(), case.sched.contact()
        T = sums(durs[0])[-1]
        for e, d in enumerate(durs):
            key = (tuple(float(v) for v in d), int(contact[e]), float(case.params.dt_dynamic))
            if key in seen:
                continue
            seen.add(key)
            out.append((name, e, bool(contact[e]), [float(v) for v in d], float(case.params.dt_dynamic), T))
    return out


@functools.lru_cache(maxsize=None)
def duration_cases():
    """The inputs of the conversion (mode `durations`): [(n_phases, contact, pps, ppf, given, variables)] -- every structure
    schedule at its given durations and at two +-10 % perturbations, for 1 .. 6 polynomials per changing phase; phases whose
    thirds do not sum back; 31 and 32 phases (up to 64 polynomials)."""
    cases = []
    for k, (_name, _e, contact, given, _dt, _T) in enumerate(structure_schedules()):
        rng = np.random.default_rng(900 + k)
        varsets = [given[:-1]] + [[v * (1.0 + 0.1 * u) for v, u in zip(given[:-1], rng.uniform(-1, 1, len(given) - 1))] for _ in range(2)]
        for variables in varsets:
            for n in N_IN_PHASE:
                cases.append((len(given), contact, n, n, given, variables))
    for d in (0.1, 0.7):
        given = [0.4, d, 0.4, d, 0.5]
        cases.append((5, True, 3, 3, given, given[:-1]))
        cases.append((5, False, 6, 5, given, given[:-1]))
    rng = np.random.default_rng(990)
    for n, contact, pps, ppf in ((31, True, 3, 3), (32, False, 3, 3)):
        given = [float(v) for v in rng.uniform(0.1, 0.5, n)]
        variables = [v * (1.0 + 0.1 * u) for v, u in zip(given[:-1], rng.uniform(-1, 1, n - 1))]
        cases.append((n, contact, pps, ppf, given, variables))
    for c in cases:
        assert sum(c[5]) < sum(c[4]) and min(c[5]) > 0.0
    return cases


def case_lists(case):
    """(phase, motion-polynomial, force-polynomial durations) of one duration case, computed in plain doubles"""
    n, contact, pps, ppf, given, variables = case
    ph = set_variables(given, variables)
    return ph, poly_durations(ph, contact, pps), poly_durations(ph, not contact, ppf)


@functools.lru_cache(maxsize=None)
def lists():
    """[(name, durations, grid times or None, foreign junction sums)]: every duration list the lookup is probed on.  The
    structure lists carry the time nodes of their structure's grid and -- the polynomial lists -- the junction sums of their
    PHASE list, which differ from their own by rounding (d/3 + d/3 + d/3 != d)."""
    out, seen = [], set()

    def add(name, d, grid=None, foreign=()):
        key = tuple(d)
        if key in seen:
            return
        seen.add(key)
        assert 1 <= len(d) <= 64 and min(d) >= 0.0
        out.append((name, np.array(d, dtype=np.float64), grid, tuple(foreign)))

    scheds = structure_schedules()
    per_sched = 3 * len(N_IN_PHASE)
    for k, (name, e, _contact, _given, dt, T) in enumerate(scheds):
        grid = grid_times(T, dt)
        for v in range(2):                                   # the given schedule and the first perturbation
            for n in N_IN_PHASE:
                ph, md, fd = case_lists(duration_cases()[k * per_sched + v * len(N_IN_PHASE) + n - 1])
                tag = "%s/ee%d/%s" % (name, e, "given" if v == 0 else "perturbed")
                add(tag + "/phase", ph, grid)
                add(tag + "/motion%d" % n, md, grid if n in (2, 3, 4, 6) else None, sums(ph))
                add(tag + "/force%d" % n, fd, grid if n == 3 else None, sums(ph))
    for case in duration_cases()[len(scheds) * per_sched:]:   # thirds that do not sum back, 31 and 32 phases
        ph, md, fd = case_lists(case)
        tag = "case%d_%d_%d" % (case[0], case[2], case[3])
        add(tag + "/phase", ph)
        if case[0] == 32:      # (the lists of 63 and 64 random durations below stand on the limit of the polynomials)
            continue
        if len(md) <= 64:
            add(tag + "/motion", md, None, sums(ph))
        if len(fd) <= 64:
            add(tag + "/force", fd, None, sums(ph))
    rng = np.random.default_rng(77)
    for n in LENGTHS:
        add("length%d" % n, [float(v) for v in rng.uniform(0.05, 0.5, n)])
    add("zero_inside", [0.3, 0.0, 0.2])
    add("zero_first", [0.0, 0.4])
    add("zeros_first", [0.0, 0.0, 0.5])
    add("zero_last", [0.4, 0.0])
    add("zero_only", [0.0])
    add("below_eps_inside", [0.3, 5e-11, 0.2])               # two junctions closer than EPS: the first must win
    add("below_eps_first", [3e-11, 3e-11, 0.5])
    add("below_eps_last", [0.25, 0.25, 9e-11])
    add("close_pair_mid", [0.1, 0.2, 2.0 ** -34, 0.3, 0.1])
    for d in (0.1, 0.7, 1.1):                                # equal durations whose thirds do not sum back
        add("thirds_%g" % d, [d / 3] * 3 + [0.2])
        add("sixths_%g" % d, [0.3] + [d / 6] * 6)
    return out


def grid_times(T, dt):
    """the time nodes of a structure's grid both ways: k * dt, and the accumulated t += dt the reference's
    TimeDiscretizationConstraint builds (time_discretization_constraint.cc:37-50), then T"""
    n = int(np.floor(T / dt))
    acc, t = [0.0], 0.0
    for _ in range(n):
        t += dt
        acc.append(t)
    return tuple(sorted(set([k * dt for k in range(n + 1)] + acc + [T])))


def time_nodes(T, dt):
    """the time nodes of a constraint grid (time_discretization_constraint.cc:37-50): t += dt floor(T / dt) times, then T"""
    t, out = 0.0, [0.0]
    for _ in range(int(np.floor(T / dt))):
        t += dt
        out.append(t)
    return out + [T]


def ulps_from_threshold(d, t):
    """how many doubles t lies from the nearest junction threshold of the list d (the last junction, the total, included)"""
    return min(abs(_bits(float(t)) - _bits(threshold(acc))) for acc in sums(d)) if t >= 0.0 else 1 << 62


def list_times(d, grid, foreign, rng):
    a = sums(d)
    times = [0.0, -0.0]
    for acc in list(a) + list(foreign):
        for v in (acc, threshold(acc)):
            times += neighbours(v)
    lo = 0.0
    for acc in a:
        times += [float(v) for v in rng.uniform(lo, acc, N_UNIFORM)]
        lo = acc
    if grid is not None:
        times += list(grid)
    total = a[-1]
    times += [total + 1e-5, total + 1.0, 2.0 * total + 1.0, threshold(total) + 1e-10]   # beyond: no segment is found
    return times


@functools.lru_cache(maxsize=None)
def points():
    """dict(list_start (L + 1), durations (sum of lengths), point_list (N) int32, point_t (N), defined (N) bool), the points
    ordered by list, then by the bit pattern of t (so -0 comes after every positive time), each (list, t) once"""
    ls = lists()
    start = np.concatenate([[0], np.cumsum([len(d) for _, d, _, _ in ls])]).astype(np.int32)
    pl, pt, df = [], [], []
    for k, (_name, d, grid, foreign) in enumerate(ls):
        rng = np.random.default_rng(5000 + k)
        bits = sorted(set(_bits(float(t)) & 0xFFFFFFFFFFFFFFFF for t in list_times(d, grid, foreign, rng)))
        total = sums(d)[-1]
        for b in bits:
            t = struct.unpack("<d", struct.pack("<Q", b))[0]
            pl.append(k), pt.append(t), df.append(bool(reaches(total, t)))
    out = dict(list_start=start, durations=np.concatenate([d for _, d, _, _ in ls]), point_list=np.array(pl, dtype=np.int32),
               point_t=np.array(pt, dtype=np.float64), defined=np.array(df, dtype=bool))
    for v in out.values():
        v.flags.writeable = False
    return out


def list_of(k):
    p = points()
    return p["durations"][p["list_start"][k]:p["list_start"][k + 1]]


@functools.lru_cache(maxsize=None)
def expected_convention():
    """(id (N) int32, t_local (N), found (N)) of convention() at every point"""
    p = points()
    ids, tls, found = [], [], []
    for k, t in zip(p["point_list"], p["point_t"]):
        i, tl, f = convention(list_of(int(k)), float(t))
        ids.append(i), tls.append(tl), found.append(f)
    return np.array(ids, dtype=np.int32), np.array(tls, dtype=np.float64), np.array(found, dtype=bool)
