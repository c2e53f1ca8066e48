"""ring_side, ring_distance and nearest_plane (kernels/planes.h) on every polygon boundary and tie, against the reference's
recorded answers, the oracle and an exact computation.

tests/plane_probe.hip is a stand-alone program that includes kernels/planes.h and what it includes, nothing else of the product;
it is compiled here with the product's CXXFLAGS, started as a fresh child process per mode and fed the scenes of
tests/plane_points.py (that module's docstring lists the rings and the points).

References
  recorded   tests/golden/refplane.npz: fpowr::PlanarRegionsToPolygons and NearestPlaneLookup::GetNearestPlaneIndex themselves
             (oracle/ref_golden.py --planes through ref_dump --plane-points) over the stand-in boost::geometry of
             oracle/ref_dump/subset.  It pins the reference's loop (DBL_MAX start, strict <, -1, first wins) and the tf transform;
             the polygon geometry under them is the stand-in's, not Boost's: Boost is not executed anywhere.
  exact      exact_side / exact_squared / exact_scene below: fractions.Fraction on the exact values of the doubles, the root by
             mpmath at 50 digits.  They share no arithmetic with the device, the oracle or the stand-in: the side is a signed
             crossing count of the vertical through the point with the edge's height there by one exact division, the distance
             the clamped projection.
  oracle     orc_ring_side / orc_ring_distance / orc_nearest_plane (oracle/towr_oracle.cc).
Bounds
  side, index   equal.  On the 1/64 grid every product and sum of the determinant and of c1, c2 is exact, so the exact answer is
             the required one at every grid point; none is skipped.
  distance   oracle against the stand-in, device against the oracle: bit-equal (the same correctly rounded operations in the same
             order; neither CPU build can contract them -- test_checker_builds_cannot_contract).  Against the exact value D on
             grid points: |d - D| <= 2^-53 (C_D D + C_R R), C_D = 3, C_R = 4.5, R the largest |coordinate| and |edge component|
             of the ring.  Counting roundings u = 2^-53 to first order: on the grid v = b - a, w = p - a, c1 and c2 are exact.
             An end-point branch computes fl(fl(wx^2) + fl(wy^2)) = D^2 (1 + 2u) and one root: 2 u D.  The projection branch has
             b = fl(c1 / c2) in (0, 1) 1 rounding, fl(b vx) 2, qx = fl(ax + .) with |error| <= u |qx| + 2 u |b vx| <= 3 u R;
             dx = fl(px - qx) = Dx + ex with |ex| <= 3 u R + u |Dx|; so sqrt(dx^2 + dy^2) <= D (1 + u) + 3 sqrt(2) u R; the two
             squares and their sum add a factor (1 + 2u) under the root, i.e. (1 + u), and the root itself (1 + u): together
             3 u D + 4.243 u R, C_R rounded up to 4.5 for the second-order terms.  The minimum over the edges of values each within
             the bound is within the bound of the exact minimum.  (tests/test_ros_subset.py's 8 * 2^-53 * max(D, |coordinates|)
             is not implied by this count: an edge component reaches twice the largest coordinate, so R does, and 3 + 2 * 4.243
             exceeds 8; that test keeps its constant for its own rings, this one uses the derived form.)
  neighbours (the doubles 1 and 2 ulp from a vertex or an edge midpoint) the float side is the exact side or 0, never the
             opposite; the index is the exact one unless the exact margin between the two best distances is below the bound;
             those exceptions stay under 2 % of the neighbour points.

The tests print what they measured (run with -s); DESIGN section 5 "Nearest plane" quotes it."""
import functools
import os
import re
import tempfile
from fractions import Fraction

import numpy as np
import pytest

from oracle import binding as ob
from oracle import ref_golden, ref_run

from . import plane_points as pp
from .probe import GOLDEN, ROOT, Probe, bits, load_fixture

U = 2.0 ** -53
C_D, C_R = 3.0, 4.5          # the roundings of ring_distance relative to the distance and to the ring's scale (docstring)
MAX_ULP_DEVICE = 0           # the device's ring_distance against the oracle's, in ulp (sqrt and divide are correctly rounded)
NEIGHBOUR_CAP = 0.02
PROBE = Probe("plane_probe")


def fixture():
    return load_fixture("refplane")


@functools.lru_cache(maxsize=None)
def scene_refs():
    """per scene of pp.scenes(): (world rings [(k, 2)], index (m,), bg::distance (m, n)) as recorded"""
    f, out = fixture(), []
    for k, s in enumerate(pp.scenes()):
        r0, r1 = f["scene_region_start"][k], f["scene_region_start"][k + 1]
        world = [f["world_xy"][f["ring_start"][r]:f["ring_start"][r + 1]] for r in range(r0, r1)]
        p0, p1 = f["scene_point_start"][k], f["scene_point_start"][k + 1]
        d = f["distance"][f["scene_pair_start"][k]:f["scene_pair_start"][k + 1]].reshape(p1 - p0, r1 - r0)
        out.append((world, f["index"][p0:p1].astype(np.int32), d))
    return out


def probe_input():
    parts = [[float(len(pp.scenes()))]]
    for s, (world, _, _) in zip(pp.scenes(), scene_refs()):
        parts.append([float(len(world))])
        for w in world:
            parts += [[float(len(w))], w.ravel()]
        parts += [[float(len(s["points"]))], s["points"].ravel()]
    return np.concatenate([np.asarray(v, dtype=np.float64) for v in parts])


# ------------------------------------------------------------------------------------------------------ the exact reference
def _sign(v):
    return (v > 0) - (v < 0)


def exact_side(ring, px, py):
    """1 inside, 0 on an edge, -1 outside: the signed crossings of the vertical through p with the edges as given, an end on the
    vertical counting half, counted where p is strictly above; a ring of fewer than 4 points holds nothing"""
    if len(ring) < 4:
        return -1
    half_turns = 0
    for (ax, ay), (bx, by) in zip(ring[:-1], ring[1:]):
        sa, sb = _sign(ax - px), _sign(bx - px)
        if sa == 0 and sb == 0:
            if min(ay, by) <= py <= max(ay, by):
                return 0
            continue
        if sa == sb:
            continue
        y_at = ay + (px - ax) * (by - ay) / (bx - ax)
        if py == y_at:
            return 0
        if py > y_at:
            half_turns += sb - sa
    return 1 if half_turns else -1


def exact_squared(ring, px, py):
    """the squared distance from p to the ring's consecutive points (0 for the empty ring)"""
    if len(ring) == 0:
        return Fraction(0)
    best = None
    for (ax, ay), (bx, by) in (zip(ring[:-1], ring[1:]) if len(ring) > 1 else [(ring[0], ring[0])]):
        vx, vy, wx, wy = bx - ax, by - ay, px - ax, py - ay
        vv = vx * vx + vy * vy
        t = min(max((wx * vx + wy * vy) / vv, 0), 1) if vv else 0
        d = (wx - t * vx) ** 2 + (wy - t * vy) ** 2
        best = d if best is None or d < best else best
    return best


def _frac_ring(ring):
    return [(Fraction(float(x)), Fraction(float(y))) for x, y in ring]


@functools.lru_cache(maxsize=None)
def exact_scene(k):
    """(side (m, n) int, squared bg::distance as Fractions [[...]], index (m,)) of scene k at its finite points; rows of the
    special points hold side -2, None and -2"""
    s, (world, _, _) = pp.scenes()[k], scene_refs()[k]
    rings = [_frac_ring(w) for w in world]
    m, n = len(s["points"]), len(rings)
    side, sq, index = np.full((m, n), -2, dtype=np.int32), [None] * m, np.full(m, -2, dtype=np.int32)
    for i, (x, y) in enumerate(s["points"]):
        if s["kind"][i] == pp.POINT_SPECIAL:
            continue
        fx, fy = Fraction(float(x)), Fraction(float(y))
        row, best = [], -1
        for j, ring in enumerate(rings):
            side[i, j] = exact_side(ring, fx, fy)
            row.append(exact_squared(ring, fx, fy))
            bg = Fraction(0) if side[i, j] >= 0 else row[j]
            if best < 0 or bg < best_d:
                best, best_d = j, bg
        sq[i], index[i] = row, best
    return side, sq, index


def ring_scale(ring):
    """R of the distance bound: the largest |coordinate| and |edge component| of the ring"""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    return max([0.0] + ([float(np.abs(ring).max())] if len(ring) else []) + ([float(np.abs(np.diff(ring, axis=0)).max())] if len(ring) > 1 else []))


def _root(q):
    import mpmath
    mpmath.mp.dps = 50
    return mpmath.sqrt(mpmath.mpf(q.numerator) / mpmath.mpf(q.denominator))


def bound(d, scale):
    return U * (C_D * d + C_R * scale)


@functools.lru_cache(maxsize=None)
def oracle_scene(k):
    """(side (m, n), ring distance (m, n), index (m,)) of the oracle on the recorded world rings"""
    s, (world, _, _) = pp.scenes()[k], scene_refs()[k]
    m, n = len(s["points"]), len(world)
    side, dist = np.zeros((m, n), dtype=np.int32), np.zeros((m, n))
    for j, w in enumerate(world):
        side[:, j], dist[:, j] = ob.ring_side(w, s["points"]), ob.ring_distance(w, s["points"])
    start = np.concatenate([[0], np.cumsum([len(w) for w in world])]).astype(np.int32)
    xy = np.concatenate(list(world) + [np.zeros((0, 2))])
    index = np.array([ob.nearest_plane(xy, start, x, y) for x, y in s["points"]], dtype=np.int32)
    return side, dist, index


def _check_grid(k, side, dist, index, who):
    """`who`'s side, ring distance and index of scene k at its grid points against the exact reference; returns the worst
    distance error as a fraction of the bound"""
    import mpmath
    s, (world, _, _) = pp.scenes()[k], scene_refs()[k]
    es, esq, ei = exact_scene(k)
    worst = 0.0
    for i in np.nonzero(s["kind"] == pp.POINT_GRID)[0]:
        assert np.array_equal(side[i], es[i]), (who, s["name"], tuple(s["points"][i]), side[i], es[i])
        assert index[i] == ei[i], (who, s["name"], tuple(s["points"][i]), index[i], ei[i])
        for j, w in enumerate(world):
            D = _root(esq[i][j])
            b = bound(D, ring_scale(w))
            err = abs(mpmath.mpf(float(dist[i, j])) - D)
            if b == 0:
                assert err == 0
                continue
            assert err <= b, (who, s["name"], tuple(s["points"][i]), j, float(dist[i, j]), float(D), float(err / b))
            worst = max(worst, float(err / b))
    return worst


def _check_neighbours(k, side, index, who):
    """`who`'s side and index of scene k at its ulp-neighbour points: (points, exceptions)"""
    s, (world, _, _) = pp.scenes()[k], scene_refs()[k]
    es, esq, ei = exact_scene(k)
    scale = max([0.0] + [ring_scale(w) for w in world])
    rows = np.nonzero(s["kind"] == pp.POINT_ULP)[0]
    exceptions = 0
    for i in rows:
        assert np.all((side[i] == es[i]) | (side[i] == 0)), (who, s["name"], tuple(s["points"][i]), side[i], es[i])
        if index[i] != ei[i]:
            d = sorted(float(_root(Fraction(0) if es[i][j] >= 0 else esq[i][j])) for j in range(len(world)))
            assert d[1] - d[0] < bound(d[1], scale), (who, s["name"], tuple(s["points"][i]), index[i], ei[i], d[:2])
            exceptions += 1
    return len(rows), exceptions


def identity_scenes():
    return [k for k, s in enumerate(pp.scenes()) if pp.is_identity(s)]


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def test_probe_compiles_without_warning_and_refuses_malformed_input():
    """(CPU tier) hipcc compiles and links the probe for gfx950 with the product's flags, without a GPU and without a warning; the
    input parser refuses, on the host with exit 2, a file whose counts do not add up"""
    PROBE.refuses([], None, "usage")
    PROBE.refuses(["sides"], [1.0], "unknown mode")
    data = probe_input()
    for mode in ("side", "distance", "nearest"):
        PROBE.refuses([mode], data[:-1], "truncated")
    PROBE.refuses(["side"], np.concatenate([data, [0.0]]), "trailing data")
    PROBE.refuses(["nearest"], [0.0], "scene count")
    PROBE.refuses(["nearest"], [1.0, -1.0], "ring count")
    PROBE.refuses(["distance"], [1.0, 1.0, 4097.0], "ring length")
    PROBE.refuses(["distance"], [1.0, 1.0, -1.0], "ring length")
    PROBE.refuses(["side"], [1.0, 1.0, 2.0, 0.0, 0.0, 1.0, 1.0, float(2 ** 21)], "point count")
    PROBE.refuses(["side"], [1.0, 1.0, 2.0, 0.0, 0.0, 1.0], "truncated ring")


def test_fixture_holds_the_scenes():
    """(CPU tier) refplane.npz was recorded on exactly the scenes of tests/plane_points.py; the identity regions' world rings are
    the local rings bit for bit; the file is no larger than the largest ref*_*.npz"""
    f, scenes = fixture(), pp.scenes()
    assert np.array_equal(f["scene_region_start"], np.concatenate([[0], np.cumsum([len(s["rings"]) for s in scenes])]))
    assert np.array_equal(bits(f["regions"]), bits(np.concatenate([s["regions"] for s in scenes])))
    assert np.array_equal(bits(f["points"]), bits(np.concatenate([s["points"] for s in scenes])))
    local = np.concatenate([r.reshape(-1, 2) for s in scenes for r in s["rings"]])
    assert np.array_equal(f["local_xy"].astype(np.float64), local), "float32 holds every local boundary point"
    for s, (world, index, d) in zip(scenes, scene_refs()):
        assert [len(w) for w in world] == [len(r) for r in s["rings"]] and d.shape == (len(s["points"]), len(world))
        if pp.is_identity(s):
            for w, r in zip(world, s["rings"]):
                assert np.array_equal(bits(w), bits(r)), s["name"]
    assert 20000 <= pp.n_pairs() == len(f["distance"]) <= 30000
    largest = max(os.path.getsize(os.path.join(GOLDEN, n)) for n in os.listdir(GOLDEN) if re.match(r"ref.*_.*\.npz$", n))
    assert os.path.getsize(os.path.join(GOLDEN, "refplane.npz")) <= largest


def test_checker_builds_cannot_contract():
    """(CPU tier) neither the oracle's checker build nor ref_dump's is given -march or -ffp-contract: on plain x86-64 no fused
    multiply-add exists, so a * b + c * d is two rounded products and a rounded sum in both, as the bit equality below needs"""
    mk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1)
    assert "-march" not in flags and "-ffp-contract" not in flags and "-mfma" not in flags and "-Ofast" not in flags, flags
    for name in ("CMakeLists.txt", "build.sh"):
        text = open(os.path.join(ROOT, "oracle", "ref_dump", name)).read()
        code = "\n".join(line.split("#")[0] for line in text.split("\n"))
        for word in ("-march", "-ffp-contract", "-mfma", "-Ofast", "-ffast-math"):
            assert word not in code, (name, word)


def test_oracle_equals_the_fixture():
    """(CPU tier) at every point of every scene: the oracle's index is the recorded one, and its bg::distance (0 where covered, else
    the ring distance) has the stand-in's recorded bits -- NaN and Inf included; the plain-double restatement of
    tests/plane_points.py agrees with both"""
    for k, s in enumerate(pp.scenes()):
        _, index, d = scene_refs()[k]
        side, dist, oi = oracle_scene(k)
        assert np.array_equal(oi, index), (s["name"], np.nonzero(oi != index)[0][:5])
        bg = np.where(side >= 0, 0.0, dist)
        same = (bits(bg) == bits(d)) | (np.isnan(bg) & np.isnan(d))
        assert same.all(), (s["name"], [(tuple(s["points"][i]), j, bg[i, j], d[i, j]) for i, j in np.argwhere(~same)[:5]])
        world = scene_refs()[k][0]
        for i, (x, y) in enumerate(s["points"]):
            assert pp.float_nearest(world, float(x), float(y)) == index[i], (s["name"], x, y)


def test_exact_reference_on_grid_points():
    """(CPU tier) ring and point on the 1/64 grid: the oracle's side and index are the exact ones at every point, its ring distance
    within 2^-53 (C_D D + C_R R) of the 50-digit root of the exact squared distance"""
    worst, n = 0.0, 0
    for k in identity_scenes():
        side, dist, index = oracle_scene(k)
        worst = max(worst, _check_grid(k, side, dist, index, "oracle"))
        n += int((pp.scenes()[k]["kind"] == pp.POINT_GRID).sum())
    print("\nnearest plane, oracle on %d grid points: worst distance error %.3f of the bound" % (n, worst))
    assert n > 8000


def test_exact_reference_on_ulp_neighbours():
    """(CPU tier) the doubles 1 and 2 ulp from every vertex and edge midpoint: the oracle's side is the exact side or 0, its index
    (and the recorded one, which equals it) the exact one unless the two best exact distances are closer than the bound; such
    exceptions stay under 2 % of the neighbour points"""
    points = exceptions = 0
    for k in identity_scenes():
        side, _, index = oracle_scene(k)
        assert np.array_equal(index, scene_refs()[k][1])
        p, e = _check_neighbours(k, side, index, "oracle")
        points, exceptions = points + p, exceptions + e
    print("\nnearest plane, oracle on %d neighbour points: %d index exceptions (%.2f %%)" % (points, exceptions, 100.0 * exceptions / points))
    assert points > 5000 and exceptions < NEIGHBOUR_CAP * points


def _disagreements(wrong):
    """the (scene, point) at which the float restatement with one wrong variant leaves the recorded index or the recorded bits of
    bg::distance -- or, on the grid points, the exact side: a point ON the ring is at distance 0 whatever the side says, so the
    recorded distance alone cannot see a touch that is missed"""
    out = []
    for k, s in enumerate(pp.scenes()):
        world, index, d = scene_refs()[k]
        grid = pp.is_identity(s)
        for i, (x, y) in enumerate(s["points"]):
            x, y = float(x), float(y)
            if grid and s["kind"][i] == pp.POINT_GRID and any(pp.float_side(w, x, y, wrong) != exact_scene(k)[0][i, j] for j, w in enumerate(world)):
                out.append((s["name"], x, y, "side"))
                continue
            if pp.float_nearest(world, x, y, wrong) != index[i]:
                out.append((s["name"], x, y, "index"))
                continue
            if wrong in ("argmin_nonstrict", "squared_compare"):
                continue
            for j, w in enumerate(world):
                bg = 0.0 if pp.float_side(w, x, y, wrong) >= 0 else pp.float_distance(w, x, y, wrong)
                if not (bits([bg])[0] == bits([d[i, j]])[0] or (bg != bg and d[i, j] != d[i, j])):
                    out.append((s["name"], x, y, "distance to ring %d" % j))
                    break
    return out


@pytest.mark.parametrize("wrong", pp.WRONG)
def test_the_points_have_teeth(wrong):
    """(CPU tier) each wrong variant of the float algorithm, alone, disagrees with the fixture at a point of the set"""
    bad = _disagreements(wrong)
    print("\n%s: caught at %d points, first %r" % (wrong, len(bad), bad[:1]))
    assert len(bad) >= 1


def test_nonstrict_side_times_c_is_the_same_function():
    """(CPU tier) `side * c > 0` -> `>= 0` cannot be caught by any point: side == 0 has returned before, so the product is never
    0.  The variant is run to show that the set sees no difference, which is the most a test can say about it."""
    for wrong in pp.UNOBSERVABLE:
        assert _disagreements(wrong) == []


def test_the_regimes_were_all_hit():
    """(CPU tier) per ring class: points inside, on and outside; per argmin scene: exact ties and points covered by several polygons
    where the scene is built for them; the collapse pairs hold 64 of each kind in both orders"""
    import math
    by_class = {}
    for k, s in enumerate(pp.scenes()):
        if not s["name"].startswith("ring/"):
            continue
        klass = s["name"].split("/")[1]
        es = exact_scene(k)[0][:, 0]
        c = by_class.setdefault(klass, [0, 0, 0])
        for v, slot in ((1, 0), (0, 1), (-1, 2)):
            c[slot] += int((es == v).sum())
    print("\nring class: inside / on / outside")
    for klass, c in by_class.items():
        print("  %-12s %5d %5d %5d" % (klass, *c))
        if klass in ("empty", "tiny"):                       # fewer than 4 points hold nothing and have no boundary
            assert c[0] == 0 and c[1] == 0 and c[2] > 0, klass
        else:
            assert min(c) > 0, (klass, c)
    assert set(by_class) == {r[0] for r in pp.rings()}
    print("scene: exact ties / covered by several")
    total_ties = total_covered = 0
    for k, s in enumerate(pp.scenes()):
        if not s["name"].startswith("argmin/") or len(s["rings"]) < 2:
            continue
        es, esq, _ = exact_scene(k)
        ties = covered = 0
        for i in range(len(s["points"])):
            if esq[i] is None:
                continue
            bg = sorted(Fraction(0) if es[i, j] >= 0 else esq[i][j] for j in range(len(s["rings"])))
            ties += bg[0] == bg[1] and bg[0] > 0
            covered += int((es[i] >= 0).sum() >= 2)
        print("  %-32s %4d %4d" % (s["name"], ties, covered))
        total_ties, total_covered = total_ties + ties, total_covered + covered
        name = s["name"].split("/")[1]
        if name.startswith(("tie", "many33", "shared_vertex")):
            assert ties > 0, s["name"]
        if name.startswith(("nested", "overlap", "shared_edge", "shared_vertex")):
            assert covered > 0, s["name"]
        if name == "inside_later":                           # inside the second polygon only, the first one merely near
            assert int(((es[:, 1] >= 0) & (es[:, 0] == -1)).sum()) > 0
    assert total_ties > 0 and total_covered > 0
    for name in ("collapse/points", "collapse/edges"):
        k = [i for i, s in enumerate(pp.scenes()) if s["name"] == name][0]
        s, (world, index, _) = pp.scenes()[k], scene_refs()[k]
        dist = oracle_scene(k)[1]
        kinds = {}
        for i, (x, y) in enumerate(s["points"]):
            sq = [pp.float_squared_distance(w, float(x), float(y)) for w in world]
            assert sq[0] != sq[1] and [math.sqrt(v) for v in sq] == list(dist[i])
            gap = abs(int(bits([dist[i, 0]])[0]) - int(bits([dist[i, 1]])[0]))
            kinds[(gap, sq[0] > sq[1])] = kinds.get((gap, sq[0] > sq[1]), 0) + 1
            # equal roots: the first wins although the second is nearer; otherwise the nearer one
            assert index[i] == (0 if gap == 0 or sq[0] < sq[1] else 1)
        print("  %-32s %r" % (name, kinds))
        assert set(kinds) == {(0, True), (0, False), (1, True), (1, False)}
        assert kinds[(0, True)] + kinds[(0, False)] >= 64 and kinds[(1, True)] + kinds[(1, False)] >= 64 and min(kinds.values()) >= 32


def test_recorder_reproduces_the_fixture():
    """(CPU tier, where the reference is built) a fresh recording into a temporary directory equals the committed file"""
    if not ref_run.available():
        pytest.skip("oracle/_ref/ref_dump is not built on this box")
    with tempfile.TemporaryDirectory() as work:
        out, f = ref_golden.compute_planes(work), fixture()
        assert set(out) == set(f)
        for key in f:
            if key != "reference_deps":
                assert out[key].dtype == f[key].dtype and np.array_equal(out[key].view(np.uint8), f[key].view(np.uint8)), key


# ------------------------------------------------------------------------------------------------------------------ GPU tier
def _probe(mode):
    return PROBE.run(mode, probe_input())


def _split(raw, per_ring):
    """the probe's output per scene: (m, n) for the pair modes, (m,) for nearest"""
    out, at = [], 0
    for s in pp.scenes():
        m, n = len(s["points"]), len(s["rings"])
        size = m * n if per_ring else m
        out.append(raw[at:at + size].reshape((m, n) if per_ring else (m,)))
        at += size
    assert at == len(raw)
    return out


@pytest.mark.gpu
def test_ring_side_on_device():
    """ring_side, one thread per (ring, point): the oracle's side at every point of every scene, and with it the recorded
    bg::distance is 0 exactly where the device says inside or on (or where the ring distance itself is 0)"""
    raw = _probe("side")
    assert not np.isnan(raw).any()
    n = 0
    for k, got in enumerate(_split(raw, True)):
        s, (_, _, d) = pp.scenes()[k], scene_refs()[k]
        side = oracle_scene(k)[0]
        bad = np.argwhere(got.astype(np.int32) != side)
        assert len(bad) == 0, (s["name"], [(tuple(s["points"][i]), j, got[i, j], side[i, j]) for i, j in bad[:5]])
        assert np.all(d[got >= 0] == 0.0), s["name"]
        n += got.size
    print("\nring_side: %d (ring, point) pairs equal the oracle" % n)


@pytest.mark.gpu
def test_ring_distance_on_device():
    """ring_distance, one thread per (ring, point): the oracle's bits at every point (MAX_ULP_DEVICE = 0: the device's sqrt and
    divide are correctly rounded), the recorded bg::distance where the point is outside, and on the grid points within the derived
    bound of the exact distance"""
    raw = _probe("distance")
    worst_ulp, at, worst_frac, n = 0, None, 0.0, 0
    for k, got in enumerate(_split(raw, True)):
        s, (_, _, d) = pp.scenes()[k], scene_refs()[k]
        side, dist, index = oracle_scene(k)
        both_nan = np.isnan(got) & np.isnan(dist)
        assert np.array_equal(np.isnan(got), np.isnan(dist)), s["name"]
        ulp = np.where(both_nan, 0, np.abs(bits(got) - bits(dist)))
        if ulp.size and ulp.max() > worst_ulp:
            i, j = np.unravel_index(np.argmax(ulp), ulp.shape)
            worst_ulp, at = int(ulp.max()), (s["name"], tuple(s["points"][i]), int(j), float(got[i, j]), float(dist[i, j]))
        out = side < 0
        if MAX_ULP_DEVICE == 0:
            assert np.array_equal(bits(got[out & ~both_nan]), bits(d[out & ~both_nan])), s["name"]
        if pp.is_identity(s):
            worst_frac = max(worst_frac, _check_grid(k, side, got, index, "device"))
        n += got.size
    print("\nring_distance: %d pairs, worst difference from the oracle %d ulp %r; worst error %.3f of the bound on the grid points"
          % (n, worst_ulp, at, worst_frac))
    assert worst_ulp <= MAX_ULP_DEVICE, at


@pytest.mark.gpu
def test_nearest_plane_on_device():
    """nearest_plane, one thread per point: the recorded index and the oracle's at every point of every scene -- ties, collapse
    pairs, NaN / Inf / 1e300 and the rotated scenes included; on the neighbour points the exceptions from the exact index stay
    under the cap"""
    raw = _probe("nearest")
    assert not np.isnan(raw).any()
    n = points = exceptions = 0
    sides = _split(_probe("side"), True)
    for k, got in enumerate(_split(raw, False)):
        s, (_, index, _) = pp.scenes()[k], scene_refs()[k]
        got = got.astype(np.int32)
        bad = np.nonzero(got != index)[0]
        assert len(bad) == 0, (s["name"], [(tuple(s["points"][i]), got[i], index[i]) for i in bad[:5]])
        assert np.array_equal(got, oracle_scene(k)[2]), s["name"]
        n += len(got)
        if pp.is_identity(s):
            p, e = _check_neighbours(k, sides[k].astype(np.int32), got, "device")
            points, exceptions = points + p, exceptions + e
    print("\nnearest_plane: %d points equal the reference and the oracle; %d neighbour points, %d index exceptions (%.2f %%)"
          % (n, points, exceptions, 100.0 * exceptions / points))
    assert exceptions < NEIGHBOUR_CAP * points
