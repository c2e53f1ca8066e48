"""The scenes and query points at which the nearest-plane lookup (kernels/planes.h: ring_side, ring_distance, nearest_plane) can
decide otherwise than fpowr's NearestPlaneLookup::GetNearestPlaneIndex over boost::geometry::distance(point, polygon).  Seeded
and deterministic; shared by tests/test_plane_probe.py, tests/test_planes_edges.py and oracle/ref_golden.py --planes (the recorded
reference).  Needs no GPU.

A scene is a list of planar regions (pose + local boundary ring) and query points.  Ring coordinates are multiples of 1/64 with
|coordinate| <= 4 (so float32, the message's format, holds them, and every product and sum of the side determinant and of c1, c2
is exact in double at a query point on the same grid: there the mathematically exact answer is the required one).  Kinds of
points (POINT_*): on the grid; the doubles 1 and 2 ulp next to a vertex or an edge midpoint; NaN / Inf / 1e300; off-grid points of
the collapse pairs; the grid points of the rotated scenes, whose world rings are off the grid.

Scenes
  ring/<class>/<name>   one identity region: every ring class of rings(), with ring_points() of it
  argmin/<name>         identity regions: none, one, two, 33 polygons, nested, overlapping, shared edge / vertex, exact ties, inside
                        a later polygon while an earlier one is near -- with the order of the polygons both ways
  collapse/<kind>       two one-point or two one-edge rings and off-grid points whose SQUARED distances to the two differ by 1 .. 4 ulp,
                        so that the rooted distances are equal or adjacent doubles (found by bisection in plain doubles, seeded);
                        the farther ring comes first for the points on one side and second for those on the other
  rotated/<k>           regions with random, non-unit, identity and half-turn quaternions at non-zero positions

float_side / float_distance / float_nearest restate the lookup in plain Python doubles (no operation can be contracted); `wrong`
names one deliberately wrong variant, which tests/test_plane_probe.py uses to show that the points catch it."""
import functools
import math
import struct

import numpy as np

G = 1.0 / 64
POINT_GRID, POINT_ULP, POINT_SPECIAL, POINT_COLLAPSE, POINT_ROTATED = 0, 1, 2, 3, 4
IDENTITY = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
DBL_MAX = 1.7976931348623157e308
SPECIAL = (float("nan"), float("inf"), -float("inf"), 1e300, -1e300)
# the deliberately wrong variants of float_*: `c1 <= 0` -> `<` and `c2 <= c1` -> `<` are one variant, because either alone computes
# the same distance (c1 == 0 gives b = 0 and q = a; c2 == c1 gives b = 1 and q = a + v = b exactly on the grid) -- only both
# together reach 0 / 0 on a zero-length edge.  "side_c_nonstrict" (`side * c > 0` -> `>= 0`) is the same function as the right one:
# side == 0 has returned before, so side * c is never 0; it is kept apart in UNOBSERVABLE
WRONG = ("vertical_touch_strict", "c1_c2_strict", "ring_min_3", "closing_edge", "sey_swapped", "weights_swapped", "argmin_nonstrict",
         "squared_compare", "fma_determinant")
UNOBSERVABLE = ("side_c_nonstrict",)


def _bits(v):
    return struct.unpack("<q", struct.pack("<d", v))[0]


def _step(v, k):
    """the double k ulp from v (k < 0: below)"""
    for _ in range(abs(k)):
        v = float(np.nextafter(v, math.inf if k > 0 else -math.inf))
    return v


# ------------------------------------------------------------------------------------------------ the lookup in plain doubles
def _fma(a, b, c):
    """fl(a * b + c) with one rounding, for finite doubles, by exact rational arithmetic"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def float_side(ring, px, py, wrong=None):
    """ring_side: 1 inside, 0 on the boundary, -1 outside"""
    n = len(ring)
    if wrong == "closing_edge" and n >= 1 and tuple(ring[0]) != tuple(ring[-1]):
        ring = list(ring) + [ring[0]]
        n += 1
    if n < (3 if wrong == "ring_min_3" else 4):
        return -1
    w1, w2 = (2, 1) if wrong == "weights_swapped" else (1, 2)
    count = 0
    for i in range(n - 1):
        s1x, s1y, s2x, s2y = float(ring[i][0]), float(ring[i][1]), float(ring[i + 1][0]), float(ring[i + 1][1])
        eq1, eq2 = s1x == px, s2x == px
        c = 0
        if eq1 and eq2:
            if wrong == "vertical_touch_strict":
                if (s1y < py and s2y > py) or (s2y < py and s1y > py):
                    return 0
            elif (s1y <= py and s2y >= py) or (s2y <= py and s1y >= py):
                return 0
        elif eq1:
            c = w1 if s2x > px else -w1
        elif eq2:
            c = -w1 if s1x > px else w1
        elif s1x < px and s2x > px:
            c = w2
        elif s2x < px and s1x > px:
            c = -w2
        if c != 0:
            if eq1 or eq2:
                sey = (s2y if eq1 else s1y) if wrong == "sey_swapped" else (s1y if eq1 else s2y)
                side = 0 if py == sey else (1 if py > sey else -1) * (1 if c > 0 else -1)      # (NaN: not on, not above)
            else:
                a, b = s2x - s1x, py - s1y
                if wrong == "fma_determinant":
                    det = _fma(a, b, -((s2y - s1y) * (px - s1x))) if all(map(math.isfinite, (a, b, s2y - s1y, px - s1x))) else a * b - (s2y - s1y) * (px - s1x)
                else:
                    det = a * b - (s2y - s1y) * (px - s1x)
                if det != det:                           # a NaN py: neither on the edge nor on a side of it
                    continue
                side = 1 if det > 0 else (-1 if det < 0 else 0)
            if side == 0:
                return 0
            if side * c > 0 or (wrong == "side_c_nonstrict" and side * c >= 0):
                count += c
    return -1 if count == 0 else 1


def float_comparable(ax, ay, bx, by, px, py, wrong=None):
    """the squared projected-point distance from (px, py) to the edge a b"""
    vx, vy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    c1 = wx * vx + wy * vy
    if (c1 < 0) if wrong == "c1_c2_strict" else (c1 <= 0):
        return wx * wx + wy * wy
    c2 = vx * vx + vy * vy
    if (c2 < c1) if wrong == "c1_c2_strict" else (c2 <= c1):
        return (px - bx) * (px - bx) + (py - by) * (py - by)
    # (c2 == 0 is reached by the wrong variant only: 0 / 0 is NaN in C)
    b = c1 / c2 if c2 != 0 else (math.nan if c1 == 0 or c1 != c1 else math.copysign(math.inf, c1))
    qx, qy = ax + b * vx, ay + b * vy
    return (px - qx) * (px - qx) + (py - qy) * (py - qy)


def float_squared_distance(ring, px, py, wrong=None):
    """the squared distance of ring_distance before its one square root (0.0 for the empty ring)"""
    n = len(ring)
    if wrong == "closing_edge" and n >= 2 and tuple(ring[0]) != tuple(ring[-1]):
        ring = list(ring) + [ring[0]]
        n += 1
    if n == 0:
        return 0.0
    e = lambda i, j: float_comparable(float(ring[i][0]), float(ring[i][1]), float(ring[j][0]), float(ring[j][1]), px, py, wrong)
    if n == 1:
        return e(0, 0)
    best = e(0, 1)
    for i in range(n - 1):
        c = e(i, i + 1)
        if c == 0.0:
            return 0.0
        if c < best:
            best = c
    return best


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan    # (v < 0 never happens; NaN stays NaN)


def float_distance(ring, px, py, wrong=None):
    """ring_distance"""
    return _sqrt(float_squared_distance(ring, px, py, wrong))


def float_nearest(rings, px, py, wrong=None):
    """nearest_plane: the first ring with the smallest bg::distance, -1 without one"""
    nearest, best = -1, DBL_MAX
    for i, ring in enumerate(rings):
        if float_side(ring, px, py, wrong) >= 0:
            d = 0.0
        elif wrong == "squared_compare":
            d = float_squared_distance(ring, px, py, wrong)
        else:
            d = float_distance(ring, px, py, wrong)
        if (d <= best) if wrong == "argmin_nonstrict" else (d < best):
            best, nearest = d, i
    return nearest


# ------------------------------------------------------------------------------------------------------------------ rings
def _q(a):
    return np.round(np.asarray(a, dtype=np.float64) * 64) / 64


@functools.lru_cache(maxsize=None)
def rings():
    """[(class, name, ring (n, 2))]"""
    out = []
    rng = np.random.default_rng(1871)
    for k in range(8):                                   # convex / star x cw / ccw x closed / open
        star, cw, closed = bool(k & 1), bool(k & 2), not (k & 4)
        n = int(rng.integers(5, 9))
        ang = (np.arange(n) + rng.uniform(0.1, 0.9, n)) * (2 * np.pi / n)
        rad = rng.uniform(0.2, 0.6, (n, 1)) if star else np.full((n, 1), rng.uniform(0.4, 0.6))
        centre = _q(rng.uniform(-1, 1, 2))
        pts = _q(np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad) + centre
        if cw:
            pts = pts[::-1]
        out.append(("star" if star else "convex", "%s_%s" % ("cw" if cw else "ccw", "closed" if closed else "open"),
                    np.concatenate([pts, pts[:1]]) if closed else pts.copy()))
    A = lambda v: np.array(v, dtype=np.float64)
    out += [
        ("empty", "empty", np.zeros((0, 2))),
        ("tiny", "one_point", A([[0.25, -0.5]])),
        ("tiny", "two_points", A([[0.0, 0.0], [1.0, 0.5]])),
        ("tiny", "three_points", A([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])),
        ("triangle", "closed", A([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.0]])),
        ("bowtie", "self_crossing", A([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])),
        ("vertical", "steps", A([[0.0, 0.0], [0.0, 1.0], [0.5, 1.0], [0.5, 0.5], [1.0, 0.5], [1.0, 0.0], [0.0, 0.0]])),
        ("horizontal", "hexagon", A([[-0.5, 0.0], [-0.25, 0.5], [0.25, 0.5], [0.5, 0.0], [0.25, -0.5], [-0.25, -0.5], [-0.5, 0.0]])),
        ("collinear", "mid_edge_vertices", A([[0.0, 0.0], [0.5, 0.25], [1.0, 0.5], [1.0, 1.0], [0.5, 1.0], [0.0, 1.0], [0.0, 0.5], [0.0, 0.0]])),
        ("repeated", "zero_length_edges", A([[0.0, 0.0], [0.0, 0.0], [1.0, 0.25], [1.0, 0.25], [0.5, 1.0], [0.5, 1.0], [0.0, 0.0]])),
        ("repeated", "unclosed", A([[-0.5, -0.5], [0.5, -0.5], [0.5, -0.5], [0.25, 0.5], [-0.5, 0.25]])),
        ("spike", "out_and_back", A([[0.0, 0.0], [1.0, 0.0], [1.0, 0.5], [1.75, 0.75], [1.0, 0.5], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0]])),
        ("spike", "vertical_out_and_back", A([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.5, 1.0], [0.5, 1.75], [0.5, 1.0], [0.0, 1.0], [0.0, 0.0]])),
        ("double", "twice_ccw", A([[0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.0, 0.0], [1.0, 0.0], [0.5, 1.0], [0.0, 0.0]])),
        ("double", "twice_cw_shifted", A([[0.0, 0.0], [0.5, 1.0], [1.0, 0.0], [0.25, 0.0], [0.5, 0.75], [0.75, 0.0], [0.0, 0.0]])),
        # a counter-clockwise square, then a clockwise one that overlaps it: the overlap has winding 0 -- outside
        ("opposite", "two_loops", A([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0], [0.0, 0.0], [0.5, 1.5], [1.5, 1.5], [1.5, 0.5], [0.5, 0.5],
                                      [0.0, 0.0]])),
        ("zero", "vertex_at_zero", A([[0.0, 0.0], [0.5, -0.5], [1.0, 0.0], [0.5, 0.75], [0.0, 0.0]])),
        ("zero", "edges_through_zero", A([[-0.5, 0.0], [0.0, -0.5], [0.5, 0.0], [0.0, 0.5], [-0.5, 0.0]])),
    ]
    for _, _, r in out:
        assert np.array_equal(r, _q(r)) and (np.abs(r).max() if len(r) else 0) <= 4
        r.flags.writeable = False
    return out


def _grid_box(lo, hi, step):
    xs = np.arange(math.floor(lo[0] / step), math.ceil(hi[0] / step) + 1) * step
    ys = np.arange(math.floor(lo[1] / step), math.ceil(hi[1] / step) + 1) * step
    return [(float(x), float(y)) for x in xs for y in ys]


def ring_points(ring, with_neighbours=True, step=0.125):
    """[(x, y, kind)] of one ring: the points the module's docstring lists, each once"""
    pts = []
    add = lambda x, y, kind=POINT_GRID: pts.append((float(x), float(y), kind))
    n = len(ring)
    sites = []
    for i in range(n):
        x, y = ring[i]
        add(x, y)
        sites.append((x, y))
        add(x, y + 0.75), add(x, y - 0.75)
        for j in range(n):                               # on the vertical through two vertices: between and beyond them
            if j != i and ring[j][0] == x and ring[j][1] != y:
                add(x, 0.5 * (y + ring[j][1])), add(x, 2 * ring[j][1] - y)
        if i + 1 < n:
            a, b = ring[i], ring[i + 1]
            for f in (0.25, 0.5, 0.75):
                add(a[0] + f * (b[0] - a[0]), a[1] + f * (b[1] - a[1]))
            sites.append((0.5 * (a[0] + b[0]), 0.5 * (a[1] + b[1])))
            add(2 * b[0] - a[0], 2 * b[1] - a[1]), add(2 * a[0] - b[0], 2 * a[1] - b[1])     # one edge-length beyond either end
    if n >= 2 and not np.array_equal(ring[0], ring[-1]):
        add(0.5 * (ring[0][0] + ring[-1][0]), 0.5 * (ring[0][1] + ring[-1][1]))               # on the closing edge that is not there
    lo, hi = (ring.min(axis=0) - 0.5, ring.max(axis=0) + 0.5) if n else (np.array([-0.5, -0.5]), np.array([0.5, 0.5]))
    for x, y in _grid_box(lo, hi, step):
        add(x, y)
    if with_neighbours:
        for x, y in sites:
            for k in (1, 2):
                for sx in (-1, 0, 1):
                    for sy in (-1, 0, 1):
                        if sx or sy:
                            add(_step(float(x), sx * k), _step(float(y), sy * k), POINT_ULP)
    cx, cy = (ring.mean(axis=0) if n else (0.0, 0.0))
    cx, cy = float(_q(cx)), float(_q(cy))
    for v in SPECIAL:
        add(v, cy, POINT_SPECIAL), add(cx, v, POINT_SPECIAL)
    if n and (ring == 0.0).any():                        # a coordinate at 0.0 queried at -0.0
        for x, y in list(ring) + [(0.5 * (ring[i][0] + ring[i + 1][0]), 0.5 * (ring[i][1] + ring[i + 1][1])) for i in range(n - 1)]:
            add(-0.0 if x == 0 else x, -0.0 if y == 0 else y)
    return _unique(pts)


def _unique(pts):
    seen, out = set(), []
    for x, y, kind in pts:
        key = (struct.pack("<d", x), struct.pack("<d", y))
        if key not in seen:
            seen.add(key)
            out.append((x, y, kind))
    return out


# ---------------------------------------------------------------------------------------------------------- collapse pairs
def collapse_points(ring_a, ring_b, seed, want=72):
    """off-grid points whose squared distances to the two rings differ by 1 .. 4 ulp: [(x, y)] with at least `want` whose rooted
    distances are equal and `want` whose rooted distances are adjacent doubles, half of each on either side of the bisector.
    ring_a lies left of ring_b and the bisector between x = 0.05 and 1.4; per random y the x of equal distance is found by
    bisection over the doubles, then its neighbours are taken."""
    rng = np.random.default_rng(seed)
    sq = lambda ring, x, y: float_squared_distance(ring, x, y)
    at = lambda b: struct.unpack("<d", struct.pack("<q", b))[0]
    cap = (want + 1) // 2
    kinds = {(0, True): [], (0, False): [], (1, True): [], (1, False): []}       # (root gap in ulp, a is farther) -> points
    while min(len(v) for v in kinds.values()) < cap:
        y = float(rng.uniform(-0.7, 0.7))
        lo, hi = _bits(0.05), _bits(1.4)                 # positive doubles: the bit patterns order them
        f = lambda b: sq(ring_a, at(b), y) - sq(ring_b, at(b), y)
        if not (f(lo) < 0 < f(hi)):
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if f(mid) < 0:
                lo = mid
            else:
                hi = mid
        for b in range(lo - 24, hi + 25):
            x = at(b)
            sa, sb = sq(ring_a, x, y), sq(ring_b, x, y)
            if 1 <= abs(_bits(sa) - _bits(sb)) <= 4:
                key = (abs(_bits(math.sqrt(sa)) - _bits(math.sqrt(sb))), sa > sb)
                if key in kinds and len(kinds[key]) < cap:
                    kinds[key].append((x, y))
    return [p for v in kinds.values() for p in v]


# ------------------------------------------------------------------------------------------------------------------ scenes
def _square(x0, y0, s, cw=False):
    r = np.array([[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s], [x0, y0]], dtype=np.float64)
    return r[::-1].copy() if cw else r


def _scene_points(ring_list, step, extra=(), neighbours=False):
    """the vertices, edge points and verticals of every ring (with their 1 and 2 ulp neighbours where asked), the `step` grid of
    their common box, the special values"""
    pts = []
    for r in ring_list:
        pts += [p for p in ring_points(r, with_neighbours=neighbours, step=step) if p[2] != POINT_SPECIAL]
    allp = np.concatenate([r for r in ring_list if len(r)]) if any(len(r) for r in ring_list) else np.zeros((1, 2))
    pts += [(x, y, POINT_GRID) for x, y in _grid_box(allp.min(axis=0) - 0.5, allp.max(axis=0) + 0.5, step)]
    pts += [(float(x), float(y), POINT_GRID) for x, y in extra]
    c = _q(allp.mean(axis=0))
    for v in SPECIAL:
        pts += [(v, float(c[1]), POINT_SPECIAL), (float(c[0]), v, POINT_SPECIAL)]
    return _unique(pts)


@functools.lru_cache(maxsize=None)
def scenes():
    """[dict(name, regions (n, 7), rings [local (k, 2)], points (m, 2), kind (m,) int8)]; `rings` are the world rings too
    wherever every region is IDENTITY"""
    out = []

    def add(name, ring_list, pts, regions=None):
        regions = np.array([IDENTITY] * len(ring_list) if regions is None else regions, dtype=np.float64).reshape(-1, 7)
        p = np.array([(x, y) for x, y, _ in pts], dtype=np.float64).reshape(-1, 2)
        k = np.array([kind for _, _, kind in pts], dtype=np.int8)
        for a in (regions, p, k):
            a.flags.writeable = False
        out.append(dict(name=name, regions=regions, rings=[np.asarray(r, dtype=np.float64) for r in ring_list], points=p, kind=k))

    for klass, name, ring in rings():
        add("ring/%s/%s" % (klass, name), [ring], ring_points(ring))
    box = [(-0.5, -0.5), (0.5, 0.5)]
    add("argmin/none", [], [(x, y, POINT_GRID) for x, y in _grid_box(box[0], box[1], 0.25)] + [(float("nan"), 0.0, POINT_SPECIAL)])
    a, b = _square(-1.0, -0.5, 1.0), _square(0.5, -0.25, 0.75, cw=True)
    add("argmin/one", [a], _scene_points([a], 0.25))
    add("argmin/two", [a, b], _scene_points([a, b], 0.25))
    many = [_square(-2.0 + 0.75 * (k % 6), -2.0 + 0.75 * (k // 6), 0.5, cw=bool(k & 1)) for k in range(33)]
    add("argmin/many33", many, [(x, y, POINT_GRID) for x, y in _grid_box((-2.5, -2.5), (2.5, 2.5), 0.5)]
        + [(-0.625, -1.0, POINT_GRID), (-0.625, -0.25, POINT_GRID), (-1.375, -1.75, POINT_GRID), (-1.75, -1.375, POINT_GRID)] + [(float("inf"), 0.0, POINT_SPECIAL), (0.0, 1e300, POINT_SPECIAL)])
    outer, inner = _square(-1.0, -1.0, 2.0), _square(-0.25, -0.25, 0.5, cw=True)
    add("argmin/nested_outer_first", [outer, inner], _scene_points([outer, inner], 0.25, neighbours=True))
    add("argmin/nested_inner_first", [inner, outer], _scene_points([inner, outer], 0.25, neighbours=True))
    o1, o2 = _square(-1.0, -0.5, 1.25), _square(-0.25, -0.25, 1.25)
    add("argmin/overlap", [o1, o2], _scene_points([o1, o2], 0.25))
    add("argmin/overlap_reversed", [o2, o1], _scene_points([o2, o1], 0.25))
    e1, e2 = _square(-1.0, 0.0, 1.0), _square(0.0, 0.0, 1.0, cw=True)
    add("argmin/shared_edge", [e1, e2], _scene_points([e1, e2], 0.25, neighbours=True))
    add("argmin/shared_edge_reversed", [e2, e1], _scene_points([e2, e1], 0.25, neighbours=True))
    v1, v2 = _square(-1.0, -1.0, 1.0), _square(0.0, 0.0, 1.0)
    add("argmin/shared_vertex", [v1, v2], _scene_points([v1, v2], 0.25, neighbours=True))
    add("argmin/shared_vertex_reversed", [v2, v1], _scene_points([v2, v1], 0.25, neighbours=True))
    t1, t2 = _square(-1.5, -0.5, 1.0), _square(0.5, -0.5, 1.0, cw=True)
    ties = [(0.0, y) for y in np.arange(-1.5, 1.51, 0.125)]                      # the axis of symmetry: equal non-zero distances
    add("argmin/tie", [t1, t2], _scene_points([t1, t2], 0.25, ties))
    add("argmin/tie_reversed", [t2, t1], _scene_points([t2, t1], 0.25, ties))
    near, far = _square(-1.0, 0.0, 0.5), _square(-0.375, 0.0, 1.0)               # inside the later one, 1/8 from the earlier
    add("argmin/inside_later", [near, far], _scene_points([near, far], 0.25, [(-0.25, 0.25), (-0.375, 0.25)]))
    pa, pb = np.array([[-0.25, 0.25]]), np.array([[1.25, -0.5]])
    add("collapse/points", [pa, pb], [(x, y, POINT_COLLAPSE) for x, y in collapse_points(pa, pb, 41)])
    ea, eb = np.array([[-0.5, -1.0], [-0.5, 1.0]]), np.array([[1.5, -1.0], [2.0, 1.0]])
    add("collapse/edges", [ea, eb], [(x, y, POINT_COLLAPSE) for x, y in collapse_points(ea, eb, 42)])
    rng = np.random.default_rng(97)
    for k in range(2):
        locals_ = [_square(-0.5, -0.5, 1.0), _q(np.array([[0.0, 0.0], [0.75, 0.25], [0.5, 1.0], [-0.25, 0.5], [0.0, 0.0]])),
                   _square(-0.25, -0.75, 0.75, cw=True), _q(np.array([[-0.5, 0.0], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.0]]))]
        quats = [rng.normal(size=4), rng.normal(size=4) * (3.0 if k else 0.2), np.array([0.0, 0.0, 0.0, 1.0]),
                 np.eye(4)[(k + 2) % 3] * 2.0]                                   # the last: a half turn about z (k = 0) or x (k = 1)
        quats[0] = quats[0] / np.sqrt((quats[0] ** 2).sum())
        regions = [np.concatenate([rng.uniform(-1.5, 1.5, 3), q]) for q in quats]
        add("rotated/%d" % k, locals_, [(x, y, POINT_ROTATED) for x, y in _grid_box((-2.5, -2.5), (2.5, 2.5), 0.5)], regions)
    return out


def scene(name):
    for s in scenes():
        if s["name"] == name:
            return s
    raise KeyError(name)


def is_identity(s):
    return all(tuple(r) == IDENTITY for r in s["regions"])


def n_pairs():
    return sum(len(s["points"]) * len(s["rings"]) for s in scenes())
