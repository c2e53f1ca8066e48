"""The points at which the attitude of the base can be decided differently from the reference, and a numpy restatement of the
conversion they are meant for: quat_of_rotation (kernels/joints.h), sample_angular (kernels/sample.h) and base_frame_rotation /
base_frame (kernels/joints.h).  Seeded and deterministic, no GPU and no reference needed; tests/test_attitude_probe.py states what
the groups have to hold and asserts it, oracle/ref_golden.py --attitude records the reference at them (tests/golden/refattitude.npz),
tests/attitude_probe.hip runs the device functions on them.

points() returns three point sets, each with one group name per point:

quat   the input is R, 9 doubles row-major
  cube         the 24 rotation matrices with entries 0 and +-1: 8 have trace 0 and an all-zero diagonal (the trace boundary and a
               triple tie at once), 6 are half turns with two tied largest diagonal entries
  cube_ulp     each of them with one diagonal entry moved: +-1 and +-2 ulp for an entry +-1, +-5e-324 and +-1e-17 for an entry 0
  ties         R(q / |q|) of integer quaternions with w = 0 or small and x = y, y = z, x = z, x = y = z -- the entries are rational,
               n * R_ij an integer with n = |q|^2, divided exactly and rounded once -- and each with one diagonal entry moved +-1 ulp
  small_w      w = +-1e-8, +-1e-160, +-1e-170 (w^2 underflows) next to an axis (where R keeps w: m21 - m12 = 4 w x / n) and next to
               a general direction, exact and rounded once
  trace_order  matrices on which (m00 + m11) + m22 and m00 + (m11 + m22) differ: diag(1, 2^-53, -1) and its like, where the sign
               of the trace itself differs, and the matrices that the reference's formula gives for quarter-turn triples from
               correctly rounded sines and cosines wherever the two orders give other quaternion bits
  random       1024 rotations of random unit quaternions (exact, rounded once), 256 on each of the four branches
  skewed       rotations with every entry moved by up to 1e-12, and rotations times 2
  hostile      NaN, +-Inf and 1e300 in single entries of the identity and of a half turn

euler  the input is the state of base-ang, 9 doubles: angles, rates, accelerations (roll pitch yaw each).  These are the states
       WANTED; the reference is reached through a one-polynomial spline, and what that spline returns at t = 0 (angles and rates
       exactly, the acceleration to rounding) is what the fixture records and the probe is given.
  quarter      the 64 triples of k pi/2, k = 0 .. 3
  quarter_near each of them with one angle moved +-1 ulp and +-1e-9
  singular     pitch = +-pi/2 (M is singular) at random roll and yaw
  far          angles of 5e4 .. 3e5 with random sign, on both sides of the 1e5 switch of sincos_fast (Case.x_far)
  rates        zero rates and accelerations, and single non-zero ones of 1e-300, 1 and 1e6
  random       1024 states, angles uniform in (-pi, pi)
  A far or random state is kept only where the trace of the reference's matrix (from correctly rounded sines and cosines) is
  more than 1e-6 from 0 and, where it is <= 0, its two largest diagonal entries are more than 1e-6 apart: there the device's
  1.5 ulp trigonometry cannot take another branch.  euler_draws counts what was drawn.

frame  the input is q (w x y z), p_base, p_ee: 10 doubles
  unit         the restatement's quaternions of the quat groups (all but every fourth random one left out, no hostile ones)
  scaled       the same times 2^k, k in {-300, -1, 1, 300}
  negated      the same times -1
  nonunit      random quaternions of norm 1e-3 .. 1e3
  single       one non-zero component
  hostile      the zero quaternion, NaN or +-Inf components, 1e200 (the squares overflow), 1e-200 (they underflow to a norm of 0)
  The offset p_ee - p_base cycles through ordinary leg lengths (most), exactly 0, 1e-300 and 1e6."""
import functools
import itertools
from fractions import Fraction

import numpy as np

HALF_PI = float(np.pi / 2)
BRANCHES = ("trace", "i0", "i1", "i2")
QUAT_GROUPS = ("cube", "cube_ulp", "ties", "small_w", "trace_order", "random", "skewed", "hostile")
EULER_GROUPS = ("quarter", "quarter_near", "singular", "far", "rates", "random")
FRAME_GROUPS = ("unit", "scaled", "negated", "nonunit", "single", "hostile")
MARGIN = 1e-6           # the generator's distance from a branch boundary for far and random euler states
RATES0, ACC0 = (0.3, -0.7, 1.1), (0.5, 0.2, -0.9)


# ------------------------------------------------------------------ the conversion, restated
def quat_of_rotation(m, tie_ge=False, swap_qw=False, swap_jk=False, trace_right=False):
    """(q as x y z w, branch 0 .. 3) of quat_of_rotation (kernels/joints.h) = Eigen::Quaterniond(R) as this project states it, in
    the device's order of operations, every operation one rounded double operation.  The keyword arguments are the mutants of the
    negative controls: `>=` for the two strict comparisons of the diagonal, the operands of qw exchanged, qj and qk exchanged,
    the trace summed as m00 + (m11 + m22)."""
    m = np.asarray(m, dtype=np.float64).reshape(3, 3)
    q = np.empty(4)
    with np.errstate(all="ignore"):
        tr = m[0, 0] + (m[1, 1] + m[2, 2]) if trace_right else (m[0, 0] + m[1, 1]) + m[2, 2]
        if tr > 0:
            tr = np.sqrt(tr + 1.0)
            q[3] = 0.5 * tr
            tr = 0.5 / tr
            q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * tr, (m[0, 2] - m[2, 0]) * tr, (m[1, 0] - m[0, 1]) * tr
            return q, 0
        above = (lambda a, b: a >= b) if tie_ge else (lambda a, b: a > b)
        i = 0
        if above(m[1, 1], m[0, 0]):
            i = 1
        if above(m[2, 2], m[i, i]):
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        tr = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        qi = 0.5 * tr
        tr = 0.5 / tr
        qw = ((m[j, k] - m[k, j]) if swap_qw else (m[k, j] - m[j, k])) * tr
        qj, qk = (m[j, i] + m[i, j]) * tr, (m[k, i] + m[i, k]) * tr
        if swap_jk:
            qj, qk = qk, qj
        q[3], q[i], q[j], q[k] = qw, qi, qj, qk
        return q, 1 + i


def quats(R, **mutant):
    """(q (n, 4) x y z w, branch (n,)) of quat_of_rotation on R (n, 9)"""
    res = [quat_of_rotation(m, **mutant) for m in np.asarray(R, dtype=np.float64).reshape(-1, 9)]
    return np.array([r[0] for r in res]).reshape(-1, 4), np.array([r[1] for r in res], dtype=np.int64)


def rotation_of_quaternion(w, x, y, z):
    """R(q / |q|), 9 doubles: the entries are rational in the components, evaluated exactly and rounded once"""
    w, x, y, z = (Fraction(float(v)) for v in (w, x, y, z))
    n = w * w + x * x + y * y + z * z
    R = (n - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
         2 * (x * y + w * z), n - 2 * (x * x + z * z), 2 * (y * z - w * x),
         2 * (x * z - w * y), 2 * (y * z + w * x), n - 2 * (x * x + y * y))
    return np.array([float(e / n) for e in R])


@functools.lru_cache(maxsize=None)
def _sincos(x):
    import mpmath
    with mpmath.workprec(200):
        return float(mpmath.sin(mpmath.mpf(x))), float(mpmath.cos(mpmath.mpf(x)))


def reference_rotation(e):
    """GetRotationMatrixBaseToWorld (euler_converter.cc:207-221) in its own order of operations on correctly rounded sines and
    cosines (what a good libm returns in all but rare cases): 9 doubles"""
    (sx, cx), (sy, cy), (sz, cz) = (_sincos(float(v)) for v in e)
    return np.array([cy * cz, cz * sx * sy - cx * sz, sx * sz + cx * cz * sy,
                     cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx,
                     -sy, cy * sx, cx * cy])


def clear_of_branches(R):
    """the generator's rule for far and random euler states"""
    d = np.sort(np.asarray(R).reshape(3, 3).diagonal())
    tr = (R[0] + R[4]) + R[8]
    return abs(tr) > MARGIN and (tr > 0 or d[2] - d[1] > MARGIN)


def ulp_moves(v):
    """the neighbours an entry is moved to"""
    if v == 0.0:
        return [5e-324, -5e-324, 1e-17, -1e-17]
    up, down = np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
    return [float(up), float(down), float(np.nextafter(up, np.inf)), float(np.nextafter(down, -np.inf))]


def diagonal_moved(R, moves):
    """R (9,) with one diagonal entry replaced, for every diagonal entry and every move of it"""
    out = []
    for d in (0, 4, 8):
        for v in moves(float(R[d])):
            m = np.array(R, dtype=np.float64)
            m[d] = v
            out.append(m)
    return out


def cube_rotations():
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            m = np.zeros((3, 3))
            for r in range(3):
                m[r, perm[r]] = signs[r]
            if round(np.linalg.det(m)) == 1:
                out.append(m.ravel())
    assert len(out) == 24
    return out


TIE_QUATERNIONS = [(w, *v) for w in (0, 1) for v in ((2, 2, 1), (1, 2, 2), (2, 1, 2), (1, 1, 2), (2, 1, 1), (1, 2, 1), (1, 1, 1), (4, 4, 4),
                                                     (-2, 2, 1), (1, -2, 2), (2, 1, -2), (3, 3, 5), (5, 3, 3), (3, 5, 3))]


def _quat_points():
    rng = np.random.default_rng(20261)
    groups = {}
    groups["cube"] = cube_rotations()
    groups["cube_ulp"] = [m for R in groups["cube"] for m in diagonal_moved(R, ulp_moves)]
    ties = []
    for q in TIE_QUATERNIONS:
        R = rotation_of_quaternion(*q)
        ties += [R] + diagonal_moved(R, lambda v: ulp_moves(v)[:2])
    groups["ties"] = ties
    small = []
    for w in (1e-8, 1e-160, 1e-170):
        for s in (1.0, -1.0):
            for v in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0.6, 0.48, 0.64), (0.3, -0.9, 0.2), (-0.1, 0.2, 0.95)):
                small.append(rotation_of_quaternion(s * w, *v))
    groups["small_w"] = small
    order = []
    t = 2.0 ** -53
    for d in ((1, t, -1), (-1, t, 1), (1, -t, -1), (-1, -t, 1), (t, 1, -1), (t, -1, 1), (1, -1, t), (-1, 1, t)):
        order.append(np.diag(d).ravel().astype(np.float64))
    for k in itertools.product(range(-2, 3), repeat=3):
        R = reference_rotation([v * HALF_PI for v in k])
        if not np.array_equal(quat_of_rotation(R)[0].view(np.int64), quat_of_rotation(R, trace_right=True)[0].view(np.int64)):
            order.append(R)
    groups["trace_order"] = order
    per, rnd = [0, 0, 0, 0], [[], [], [], []]
    while min(per) < 256:
        q = rng.normal(size=4)
        R = rotation_of_quaternion(*(q / np.linalg.norm(q)))
        b = quat_of_rotation(R)[1]
        if per[b] < 256:
            per[b] += 1
            rnd[b].append(R)
    groups["random"] = [rnd[b][i] for i in range(256) for b in range(4)]
    skew = [R + rng.uniform(-1e-12, 1e-12, size=9) for R in groups["random"][:64]]
    skew += [2.0 * R for R in groups["random"][64:96]]
    groups["skewed"] = skew
    host = []
    for base in (np.eye(3).ravel(), np.diag([1.0, -1.0, -1.0]).ravel()):
        for at in range(9):
            for v in (np.nan, np.inf, -np.inf, 1e300):
                m = base.copy()
                m[at] = v
                host.append(m)
    groups["hostile"] = host
    return groups


def _euler_points():
    rng = np.random.default_rng(20262)
    groups = {}
    state = lambda e, r=RATES0, a=ACC0: np.concatenate([np.asarray(e, dtype=np.float64), r, a])
    triples = [tuple(v * HALF_PI for v in k) for k in itertools.product(range(4), repeat=3)]
    groups["quarter"] = [state(e) for e in triples]
    near = []
    for e in triples:
        for at in range(3):
            for v in (float(np.nextafter(e[at], np.inf)), float(np.nextafter(e[at], -np.inf)), e[at] + 1e-9, e[at] - 1e-9):
                m = list(e)
                m[at] = v
                near.append(state(m))
    groups["quarter_near"] = near
    groups["singular"] = [state([rng.uniform(-3, 3), s * HALF_PI, rng.uniform(-3, 3)], rng.normal(size=3), rng.normal(size=3))
                          for s in (1.0, -1.0) for _ in range(16)]
    draws = 0
    far = []
    while len(far) < 64:
        e = rng.uniform(5e4, 3e5, size=3) * rng.choice([-1.0, 1.0], size=3)
        draws += 1
        if clear_of_branches(reference_rotation(e)):
            far.append(state(e, rng.normal(size=3), rng.normal(size=3)))
    groups["far"] = far
    rates = []
    for e in ((0.0, 0.0, 0.0), (0.3, -0.4, 0.5), (2.0, 1.0, -2.5)):
        rates.append(state(e, (0, 0, 0), (0, 0, 0)))
        for slot in range(6):
            for v in (1e-300, 1.0, 1e6):
                ra = np.zeros(6)
                ra[slot] = v
                rates.append(state(e, ra[:3], ra[3:]))
    groups["rates"] = rates
    rnd = []
    while len(rnd) < 1024:
        e = rng.uniform(-np.pi, np.pi, size=3)
        draws += 1
        if clear_of_branches(reference_rotation(e)):
            rnd.append(state(e, rng.normal(size=3) * 2.0, rng.normal(size=3) * 5.0))
    groups["random"] = rnd
    return groups, draws


def _frame_points(quat_groups):
    rng = np.random.default_rng(20263)
    unit = []
    for name in QUAT_GROUPS[:-1]:
        R = quat_groups[name]
        if name == "random":
            R = R[::4]
        q = quats(np.array(R))[0]
        assert np.isfinite(q).all(), name
        unit += [v[[3, 0, 1, 2]] for v in q]
    groups = {"unit": unit}
    groups["scaled"] = [v * 2.0 ** k for k in (-300, -1, 1, 300) for v in unit]
    groups["negated"] = [-v for v in unit]
    groups["nonunit"] = [(lambda v: v / np.linalg.norm(v) * 10.0 ** rng.uniform(-3, 3))(rng.normal(size=4)) for _ in range(256)]
    single = []
    for at in range(4):
        for s in (1.0, -1.0, 0.5, -3.0, 1e-3, 1e3):
            v = np.zeros(4)
            v[at] = s
            single.append(v)
    groups["single"] = single
    ordinary = np.array([0.5, -0.5, 0.5, 0.5])
    host = [np.zeros(4), np.full(4, 1e200), np.full(4, -1e200), np.full(4, 1e-200), np.array([1e-200, 0, 0, -1e-200])]
    for at in range(4):
        for v in (np.nan, np.inf, -np.inf, 1e200, 1e-200):
            m = ordinary.copy()
            m[at] = v
            host.append(m)
        for v in (1e200, 1e-200, 1e-170):
            m = np.zeros(4)
            m[at] = v
            host.append(m)
    groups["hostile"] = host
    out = {}
    for name, qs in groups.items():
        rows = []
        for i, q in enumerate(qs):
            base = rng.normal(size=3) * np.array([1.0, 1.0, 0.3])
            kind = i % 8
            off = rng.uniform(-0.4, 0.4, size=3)
            if kind == 0:
                ee = base.copy()
            elif kind == 1:
                base = np.zeros(3)
                ee = off * 1e-300
            elif kind == 2:
                ee = base + off * 1e6
            else:
                ee = base + off
            rows.append(np.concatenate([q, base, ee]))
        out[name] = rows
    return out


def _stack(groups, names):
    data = np.array([row for name in names for row in groups[name]], dtype=np.float64)
    label = np.array([k for k, name in enumerate(names) for _ in groups[name]], dtype=np.uint8)
    data.flags.writeable = False
    label.flags.writeable = False
    return data, label


@functools.lru_cache(maxsize=None)
def points():
    """quat (n, 9), quat_group (n,) index into QUAT_GROUPS; euler (n, 9), euler_group, euler_draws; frame (n, 10), frame_group"""
    qg = _quat_points()
    eg, draws = _euler_points()
    fg = _frame_points(qg)
    out = {}
    out["quat"], out["quat_group"] = _stack(qg, QUAT_GROUPS)
    out["euler"], out["euler_group"] = _stack(eg, EULER_GROUPS)
    out["frame"], out["frame_group"] = _stack(fg, FRAME_GROUPS)
    out["euler_draws"] = draws
    return out


def group(which, name):
    """the rows of point set `which` that belong to group `name`, as a boolean mask"""
    names = {"quat": QUAT_GROUPS, "euler": EULER_GROUPS, "frame": FRAME_GROUPS}[which]
    return points()[which + "_group"] == names.index(name)


def spline_nodes(state):
    """the node values [p0 v0 p1 v1] (12) of a one-polynomial cubic Hermite spline of duration 1 whose state at t = 0 is `state`
    (9: p v a): a(0) = 2 c2 = -6 (p0 - p1) - 4 v0 - 2 v1 (polynomial.cc:100-103), so with v1 = 0, p1 = p0 + (a + 4 v0) / 6"""
    p, v, a = state[:3], state[3:6], state[6:9]
    return np.concatenate([p, v, p + (a + 4.0 * v) / 6.0, np.zeros(3)])
