"""terrain_eval and force_core of kernels/terrain.h on every breakpoint, against the reference's recorded answers.

tests/terrain_probe.hip is a stand-alone program that includes that header and what it includes, nothing else of the product;
it is compiled here with the product's CXXFLAGS for kernels.o (so that floating-point contraction is the product's), started as
a fresh child process per mode and fed the points of tests/terrain_points.py: every breakpoint of the seven analytic maps as
the double the reference's constant expression yields, with the doubles one and two ulp on each side; for the CSV map every
cell edge, the slope-band thresholds fl(fl((c+1) res) - eps) and fl(fl(c res) + eps), their fused roundings where they differ,
the doubles at which the cell index steps, the negative and the outside points; for two `Grid` maps every cell centre and
border, the half-cell band along the map border, the points within eps of it (FLT_MAX samples), the corners and the outside.

References
  analytic maps, CSV   tests/golden/refterrain_*.npz: the reference's own classes, recorded by oracle/ref_golden.py --terrain
                       through ref_dump --terrain-points.  The oracle must equal them bit for bit (CPU tier).
  `Grid`               cannot be executed (grid_map is third party and absent): the oracle's GmAtPosition AND mp_ref's
                       independent GridMapTerrain, which must agree (CPU tier; the excepted points are listed with their reason
                       and stay below 1 %).
Bounds for the device
  CSV, `Grid`          h, hx, hy bit-equal: plainly rounded double and float operations on both sides.
  analytic maps        bit-equal on every piece that is one operation (so the branch is the reference's); where the device may
                       fuse -- Gap's a x^2 + b x + c and 2a x + b, Slope's hc - sl (x - xd) -- within 3 * 2^-53 * sum |terms| of
                       the mpmath value of the reference's formula on its own double constants: at most three roundings
                       against exact terms.  The branch there is pinned by hxx (Gap) and hx (Slope), which are bit-equal.
  force_core           mpmath at 60 digits on height_map.cc:62-148 and force_constraint.cc:62-171, fed the reference's
                       (hx, hy, hxx) at the point.  Per output C_FORCE * 2^-53 * sum_i |f_i| |dir_i| (derivative columns:
                       sum_i |f_i| |d dir_i|; the direction columns, which hold dir_i itself: |basis_i| + mu |normal_i|, the
                       two terms of dir_i).  C_FORCE = 20 counts the roundings of the longest chain of force_core, the
                       diagonal of the derivative column, an operation's count being those of its operands plus one: sq 3
                       (product, two sums), 1/sq 4, |v| = sqrt(sq) 4, 1/|v| = 1 / sqrt(sq) 5, the other two squares 3, their
                       product with 1/|v| 3 + 5 + 1 = 9, times 1/sq 9 + 4 + 1 = 14, times dv 15, times mu 16, the sum with the
                       other basis 17, times f 18, two additions 20.  (g5 alone would be 10.)  The bound is relative to the
                       exact |d dir_i|, so it only holds for a formula that does not cancel: the reference's own
                       |v| - v_dim^2 / |v| loses all but 1 / 145 of itself at Gap's edges (hx = -+12), and force_core written
                       that way missed this bound 6.3-fold there; it now sums the other two squares instead.

The GPU tests print the worst case they measured as a fraction of the bound (run with -s); DESIGN section 5 "Terrain
breakpoints" quotes them."""
import functools
import os

import numpy as np
import pytest

from oracle import binding as ob
from oracle import mp_ref, ref_golden

from . import terrain_points as tp
from .probe import GOLDEN, Probe, bits, load_fixture

U = 2.0 ** -53
C_FUSED = 3.0        # analytic pieces the device may fuse: at most three roundings against exact terms
C_FORCE = 20.0       # the roundings of the longest chain of force_core (the derivative column), counted in the docstring
GRID_EXCLUSION_CAP = 0.01
MIN_DIFFERING = 8    # thresholds per side and dimension at which the two roundings decide differently and the slope is not 0


def _mp():
    import mpmath
    mpmath.mp.dps = 60
    return mpmath.mp


def _same_bits(a, b):
    """element-wise: the same double, taking +0 and -0 for different"""
    return bits(a) == bits(b)


def fixture(name):
    return load_fixture("refterrain_%s" % name)


def fixture_rows(key):
    """the rows of its fixture that hold the points of terrain `key`"""
    name = "csv" if key == "csv" else "analytic"
    ids = fixture(name)["terrain_id"]
    return name, np.nonzero(ids == tp.TERRAIN_ID[key])[0]


@functools.lru_cache(maxsize=None)
def oracle_problem(key):
    """an oracle problem on terrain `key` (the robot and the schedule do not matter)"""
    kw = {}
    if key == "csv":
        kw["grid"] = tp.CSV_HEIGHTS
    if key.startswith("grid_map"):
        m = tp.GRID_MAPS[int(key[-1])]
        kw["grid_map"] = (tp.grid_elevation(m), m["res"], m["pos"])
    terrain = "grid_map" if key.startswith("grid_map") else key
    return ob.OracleProblem("monoped", terrain, [[0.4, 0.2, 0.4]], [1], **kw)


@functools.lru_cache(maxsize=None)
def oracle_values(key):
    """(n, 31) of OracleProblem.terrain_probe_full at every point of `key`"""
    P = oracle_problem(key)
    out = np.array([P.terrain_probe_full(x, y) for x, y in tp.points(key)])
    out.flags.writeable = False
    return out


@functools.lru_cache(maxsize=None)
def reference_values(key):
    """(n, 4) h, hx, hy, hxx the device is held to: the recorded reference, for `Grid` the oracle"""
    if key.startswith("grid_map"):
        return oracle_values(key)[:, :4]
    name, rows = fixture_rows(key)
    return fixture(name)["values"][rows]


# ------------------------------------------------------------------ running the probe (tests/probe.py)
PROBE = Probe("terrain_probe")


def _maps_block():
    rows, cols = tp.CSV_HEIGHTS.shape
    parts = [[3.0], [7.0, rows, cols, tp.CSV_RES, tp.CSV_EPS, 0.0, 0.0], tp.CSV_HEIGHTS.ravel()]
    for m in tp.GRID_MAPS:
        parts += [[8.0, m["size"][0], m["size"][1], m["res"], m["res"] / 6.0, m["pos"][0], m["pos"][1]],
                  tp.grid_elevation(m).ravel(order="F").astype(np.float64)]
    return parts


MAP_INDEX = {"csv": 0, "grid_map0": 1, "grid_map1": 2}


def _terrain_id(key):
    return 8 if key.startswith("grid_map") else tp.TERRAIN_ID[key]


@functools.lru_cache(maxsize=None)
def probe_input(mode):
    """(the input file's doubles, [(key, mu, index into points(key))] per group in order)"""
    parts, groups = _maps_block(), []
    if mode == "eval":
        for key in tp.terrain_keys():
            groups.append((key, 0.5, np.arange(len(tp.points(key)))))
    else:
        for key, (idx, _f, mu) in tp.force_subset().items():
            for m in tp.MUS:
                groups.append((key, m, np.nonzero(mu == m)[0]))
    parts.append([float(len(groups))])
    for key, mu, sel in groups:
        parts.append([_terrain_id(key), MAP_INDEX.get(key, -1), mu, 0.0, len(sel)])
        if mode == "eval":
            parts.append(tp.points(key)[sel].ravel())
        else:
            idx, f, _mu = tp.force_subset()[key]
            parts.append(np.column_stack([f[sel], tp.points(key)[idx[sel]]]).ravel())
    return np.concatenate([np.asarray(p, dtype=np.float64) for p in parts]), groups


@functools.lru_cache(maxsize=None)
def _probe(mode):
    """the probe's output for `mode`, from a child process of its own: key -> rows in the order of points(key) (eval) or of
    force_subset()[key] (force modes)"""
    data, groups = probe_input(mode)
    width = {"eval": 4, "force": 30, "force_g": 5}[mode]
    raw = PROBE.run(mode, data).reshape(-1, width)
    assert raw.shape[0] == sum(len(sel) for _, _, sel in groups)
    out, at = {}, 0
    for key, _mu, sel in groups:
        n_key = len(tp.points(key)) if mode == "eval" else len(tp.force_subset()[key][0])
        out.setdefault(key, np.full((n_key, width), np.nan))[sel] = raw[at:at + len(sel)]
        at += len(sel)
    for v in out.values():
        v.flags.writeable = False
    return out


# ------------------------------------------------------------------ CPU tier
def test_probe_compiles_without_warning():
    """(CPU tier) hipcc compiles and links the probe for gfx950 with the product's flags, without a GPU and without a warning;
    the input parser refuses a file whose counts do not add up before anything reaches a device"""
    PROBE.refuses([], None, "usage")
    PROBE.refuses(["eval"], probe_input("eval")[0][:-1], "truncated")


@pytest.mark.parametrize("name", ref_golden.TERRAIN_FIXTURES)
def test_points_are_the_recorded_ones(name):
    """(CPU tier) the generator yields, bit for bit, the points the reference was recorded at"""
    ids, xy, fi, heights = ref_golden.terrain_fixture_points(name)
    fx = fixture(name)
    assert np.array_equal(ids, fx["terrain_id"]) and _same_bits(xy, fx["xy"]).all() and np.array_equal(fi, fx["force_index"])
    assert fx["values"].shape == (len(ids), 4) and fx["basis"].shape == (len(fi), 27) and np.isfinite(fx["values"]).all()
    if heights is not None:
        assert _same_bits(heights, fx["csv_heights"]).all()
    assert os.path.getsize(os.path.join(GOLDEN, "refterrain_%s.npz" % name)) <= 1 << 20


def test_analytic_inputs_sit_on_every_breakpoint():
    """(CPU tier) every breakpoint with its neighbours, the shared points, every piece, +-0, +-10, 256 uniform points"""
    for key in tp.ANALYTIC:
        fam, p = tp.families(key), tp.points(key)
        assert np.isfinite(p).all()
        bx = tp.BREAKS_X[key]
        e = fam["break_x"][:, 0].reshape(-1, 5)
        assert e.shape[0] == len(bx) and np.all(np.diff(e, axis=1) > 0) and list(e[:, 2]) == list(bx)
        assert np.array_equal(e[:, 1], np.nextafter(e[:, 2], -np.inf)) and np.array_equal(e[:, 3], np.nextafter(e[:, 2], np.inf))
        if key in tp.SHARED:
            assert tp.SHARED[key] in e[:, 2]
        assert len(fam["mid"]) == len(bx) + 1 and len(fam["uniform"]) == tp.N_UNIFORM
        for lo, hi in zip((-np.inf,) + tuple(bx), tuple(bx) + (np.inf,)):    # a point strictly inside every piece
            assert ((fam["mid"][:, 0] > lo) & (fam["mid"][:, 0] < hi)).sum() == 1
        sp = fam["special"]
        for col in (0, 1):
            assert {(float(v), bool(np.signbit(v))) for v in sp[:, col]} >= {(0.0, False), (0.0, True), (10.0, False), (-10.0, True)}
        if key in tp.BREAKS_Y:
            ey = fam["break_y"]
            assert set(tp.BREAKS_Y[key]) <= set(ey[:, 1])
            for b in tp.BREAKS_Y[key]:      # on the sloped pieces, with neighbours
                on = ey[(ey[:, 1] >= np.nextafter(np.nextafter(b, -np.inf), -np.inf)) & (ey[:, 1] <= np.nextafter(np.nextafter(b, np.inf), np.inf))]
                assert len(np.unique(on[:, 1])) == 5 and len(np.unique(on[:, 0])) == len(bx) + 1
    ref = fixture("analytic")
    taken = {key: set(np.unique(ref["values"][fixture_rows(key)[1]][:, 0] != 0)) for key in tp.ANALYTIC[1:]}
    assert all(v == {False, True} for v in taken.values()), taken


def _csv_differing():
    """per (side, dimension): the points at which the reference's two-step threshold and the fused one decide differently
    and the neighbouring cell makes the slope non-zero -- from exact arithmetic"""
    sl, p = tp.family_slices("csv"), tp.points("csv")
    out = {}
    for side in ("end", "start"):
        for dim in "xy":
            idx = np.concatenate([np.arange(sl["%s%d_%s" % (side, k, dim)].start, sl["%s%d_%s" % (side, k, dim)].stop) for k in (2, 1)])
            hit = []
            for i in idx:
                two, one = tp.csv_expected(*p[i]), tp.csv_expected(*p[i], fused=True)
                col = 1 if dim == "x" else 2
                if two[col] != one[col] and (two[col] != 0.0 or one[col] != 0.0):
                    hit.append(i)
            out[(side, dim)] = np.array(hit, dtype=np.int64)
    return out


def test_csv_inputs_sit_on_both_roundings_of_the_thresholds():
    """(CPU tier) the CSV points: every edge, both slope-band thresholds in both roundings, the steps of the cell index, the
    negative and the outside points -- and, per side and dimension, at least MIN_DIFFERING points at which the fused and the
    two-step threshold decide differently with a non-zero slope, so that a fused threshold cannot pass"""
    rows, cols = tp.CSV_HEIGHTS.shape
    assert (rows, cols) == (7, 9)
    for a in (0, 1):             # every step between neighbouring lines of cells rises somewhere, falls somewhere, stays level somewhere
        d = np.sign(np.round(np.diff(tp.CSV_HEIGHTS, axis=a), 9))
        for line in (d if a == 0 else d.T):
            assert set(line) == {-1.0, 0.0, 1.0}
    fam = tp.families("csv")
    for dim, n in (("x", cols), ("y", rows)):
        col = 0 if dim == "x" else 1
        lines = tp.csv_line_values(n)
        assert list(lines["edge"][:, 2]) == [float(c) * tp.CSV_RES for c in range(n + 1)]
        assert list(lines["end2"][:, 2]) == [float(c + 1) * tp.CSV_RES - tp.CSV_EPS for c in range(n)]
        assert list(lines["start2"][:, 2]) == [float(c) * tp.CSV_RES + tp.CSV_EPS for c in range(n)]
        assert len(lines["end1"]) >= 1 and len(lines["start1"]) >= 1, "no cell of this map tells the roundings apart"
        for kind, vals in lines.items():
            assert set(vals.ravel()) == set(fam["%s_%s" % (kind, dim)][:, col]), kind
        for c, v in enumerate(lines["crossing"][:, 2]):
            assert v / tp.CSV_RES >= c and (v == 0.0 or np.nextafter(v, -np.inf) / tp.CSV_RES < c)
    neg = fam["negative_cell0"]
    assert ((neg > -tp.CSV_RES) & (neg < 0)).any(axis=1).all() and (tp.csv_cell(neg) >= 0).all()
    out = fam["outside"]
    cx, cy = tp.csv_cell(out[:, 0]), tp.csv_cell(out[:, 1])
    invalid = (cx < 0) | (cx >= cols) | (cy < 0) | (cy >= rows)
    assert (cx < 0).sum() >= 6 and (cy < 0).sum() >= 6 and (cx >= cols).sum() >= 6 and (cy >= rows).sum() >= 6
    # the only valid ones are the doubles just below cols res / rows res, the neighbours of the first invalid coordinate
    below = set(tp.neighbours([cols * tp.CSV_RES, rows * tp.CSV_RES])[:, :2].ravel())
    assert all(x in below or y in below for x, y in out[~invalid]) and (~invalid).sum() <= 4
    assert len(fam["uniform"]) == 2048
    differing = _csv_differing()
    assert all(len(v) >= MIN_DIFFERING for v in differing.values()), {k: len(v) for k, v in differing.items()}
    # the recorded reference takes the two-step side at every one of them
    ref = fixture("csv")["values"]
    for (side, dim), idx in differing.items():
        col = 1 if dim == "x" else 2
        want = np.array([tp.csv_expected(*tp.points("csv")[i])[col] for i in idx])
        assert _same_bits(ref[idx, col], want).all(), (side, dim)


def _grid_sample_state(m, p):
    """(inside the map, both +- eps samples in x inside, ... in y)"""
    res, eps = m["res"], m["res"] / 6.0
    ins = []
    for dx, dy in ((0, 0), (eps, 0), (-eps, 0), (0, eps), (0, -eps)):
        ok = True
        for a, d in ((0, dx), (1, dy)):
            t = m["pos"][a] + 0.5 * m["size"][a] * res - (p[a] + d)
            ok = ok and 0.0 <= t < m["size"][a] * res
        ins.append(ok)
    return ins


def test_grid_inputs_sit_on_centres_borders_and_the_flt_max_band():
    """(CPU tier) the `Grid` points: every centre and border with neighbours, the map borders, the half-cell band, points
    whose +- eps samples leave the map on one side or on both, the corners, the outside"""
    for k, m in enumerate(tp.GRID_MAPS):
        key, fam = "grid_map%d" % k, tp.families("grid_map%d" % k)
        for a, dim in ((0, "x"), (1, "y")):
            centres, borders = tp.grid_lines(m, a)
            assert len(centres) == m["size"][a] and len(borders) == m["size"][a] + 1
            for kind, vals in (("centre", centres), ("border", borders)):
                assert set(tp.neighbours(vals).ravel()) == set(fam["%s_%s" % (kind, dim)][:, a])
        ref = oracle_values(key)
        h, hx, hy = ref[:, 0], ref[:, 1], ref[:, 2]
        eps2 = 2 * (m["res"] / 6.0)
        big = tp.FLT_MAX / eps2 * 0.99
        assert (h == tp.FLT_MAX).sum() >= 200 and (h != tp.FLT_MAX).sum() >= 2000
        for s in (hx, hy):       # (FLT_MAX - h) / 2 eps, its negative, and exactly 0 with the point and both samples outside
            assert (s > big).sum() >= 20 and (s < -big).sum() >= 20 and ((s == 0.0) & (h == tp.FLT_MAX)).sum() >= 20
        state = np.array([_grid_sample_state(m, p) for p in tp.points(key)])
        assert (state[:, 0] & ~state[:, 1:].all(axis=1)).sum() >= 100, "inside, a sample outside"
        assert (~state[:, 0] & state[:, 1:].any(axis=1)).sum() >= 100, "outside, a sample inside"
        assert len(fam["corner"]) == 100 and len(fam["outside"]) == 12 and len(fam["uniform"]) == 2048


def test_force_subset_covers_every_terrain_and_the_steep_points():
    sub = tp.force_subset()
    assert sum(len(v[0]) for v in sub.values()) == tp.N_FORCE == 1024 and set(sub) == set(tp.terrain_keys())
    for key, (idx, f, mu) in sub.items():
        assert len(np.unique(idx)) == len(idx) and set(mu) == set(tp.MUS) and 0.5 in tp.MUS
        assert any((f == v).all(axis=1).any() for v in ([0.0, 0.0, 0.0],)) and sum((np.abs(f).sum(axis=1) == 1).astype(int)) >= 6
        assert np.abs(f).max() > 300.0
    ref = reference_values("csv")[sub["csv"][0]]
    assert (np.abs(ref[:, 1]) > 25).sum() >= 20 and (np.abs(ref[:, 2]) > 25).sum() >= 20, "CSV step slopes"
    ref = reference_values("gap")[sub["gap"][0]]
    assert (ref[:, 3] != 0).sum() >= 40 and (ref[:, 3] == 0).sum() >= 20, "Gap's hxx"
    for key in ("grid_map0", "grid_map1"):
        ref = reference_values(key)[sub[key][0]]
        assert (np.abs(ref[:, 1:3]) > 1e38).any(axis=1).sum() >= 20, "Grid slopes next to the border"


@pytest.mark.parametrize("key", tp.ANALYTIC + ("csv",))
def test_oracle_equals_the_recorded_reference_bit_for_bit(key):
    """(CPU tier) orc_terrain_height / orc_terrain_basis / orc_terrain_dbasis and OracleProblem.terrain_probe against the
    reference's classes at every point, bit for bit"""
    name, rows = fixture_rows(key)
    fx, p = fixture(name), tp.points(key)
    ref, got = fx["values"][rows], oracle_values(key)
    assert _same_bits(p, fx["xy"][rows]).all()
    bad = np.nonzero(~_same_bits(got[:, :4], ref).all(axis=1))[0]
    assert bad.size == 0, "%s: the oracle differs from the reference at %d points, first (x, y) %r: %r vs %r" % (
        key, bad.size, p[bad[0]].tolist(), got[bad[0], :4].tolist(), ref[bad[0]].tolist())
    P = oracle_problem(key)
    for i in range(0, len(p), 7):
        assert _same_bits(P.terrain_probe(*p[i]), ref[i, :3]).all()
    pos = {int(r): k for k, r in enumerate(fx["force_index"])}
    sel = [(i, pos[int(r)]) for i, r in enumerate(rows) if int(r) in pos]
    assert len(sel) == len(tp.force_subset()[key][0])
    for i, k in sel:
        assert _same_bits(got[i, 4:], fx["basis"][k]).all(), "%s: basis at %r" % (key, p[i].tolist())
        if key == "csv":
            continue
        x, y = p[i]
        assert _same_bits(ob.terrain_height(key, x, y), ref[i, 0]).all()
        for b in range(3):
            assert _same_bits(ob.terrain_basis(key, b, x, y), fx["basis"][k][3 * b:3 * b + 3]).all()
            for dim in range(2):
                o = 9 + 3 * (2 * b + dim)
                assert _same_bits(ob.terrain_dbasis(key, b, dim, x, y), fx["basis"][k][o:o + 3]).all()


TIE = 2.0 ** -20     # of a float ulp: how close to a float rounding midpoint an exact sample must lie to be called a tie


@pytest.mark.parametrize("k", range(len(tp.GRID_MAPS)))
def test_grid_oracle_agrees_with_the_independent_mpmath_model(k):
    """(CPU tier) `Grid` has no executable reference: the oracle's GmAtPosition and mp_ref's GridMapTerrain, written
    independently from grid_height_map.h and grid_map's published algorithm, must give the same h, hx, hy at every point.
    One kind of point is excepted, listed, and kept below 1 %: a TIE.  On a cell centre line the +- res / 6 samples have
    bilinear weights 1/6 and 5/6, so the exact value is a multiple of a sixth of a float ulp and sits on a float rounding
    midpoint once in six; mp_ref rounds the exact value once, grid_map and the oracle round each product and sum to double
    first, and which neighbour wins is decided by rounding noise.  Every excepted point must have a sample whose exact value
    lies within TIE of a midpoint, with the two models on the two floats either side of it."""
    mp = _mp()
    m = tp.GRID_MAPS[k]
    key = "grid_map%d" % k
    T = mp_ref.GridMapTerrain(tp.grid_elevation(m), m["res"], m["pos"])
    P = oracle_problem(key)
    ref, p = oracle_values(key), tp.points(key)
    eps = m["res"] / 6.0
    listed = []
    for i, (x, y) in enumerate(p):
        got = np.array([float(v) for v in T.h_hx_hy(x, y)])
        if _same_bits(got, ref[i, :3]).all():
            continue
        ties = 0
        for sx, sy in ((x, y), (x + eps, y), (x - eps, y), (x, y + eps), (x, y - eps)):
            a, b = np.float32(T.height(sx, sy)), np.float32(P.terrain_probe(sx, sy)[0])
            if a == b:
                continue
            exact = T.at_position_exact(sx, sy)
            lo, hi = min(a, b), max(a, b)
            assert exact is not None and not isinstance(exact, np.float32) and np.nextafter(lo, np.float32(np.inf)) == hi, (
                "%s: the two models differ at (%r, %r) by more than a tie: %r vs %r" % (key, sx, sy, a, b))
            mid = (mp.mpf(float(lo)) + mp.mpf(float(hi))) / 2
            assert abs(exact - mid) <= TIE * (float(hi) - float(lo)), "%s: (%r, %r) is no tie: %r vs %r" % (key, sx, sy, a, b)
            ties += 1
        assert ties, "%s: (%r, %r) differs without a differing sample" % (key, x, y)
        listed.append((float(x), float(y), "a sample's exact value on a float rounding midpoint"))
    print("\n%s: %d of %d points excepted as ties (cap %d), e.g. %r" % (key, len(listed), len(p), int(GRID_EXCLUSION_CAP * len(p)), listed[:3]))
    assert len(listed) < GRID_EXCLUSION_CAP * len(p), listed[:5]


# ------------------------------------------------------------------ GPU tier
def _report_bits(key, got, ref, cols, what):
    p = tp.points(key)
    bad = np.nonzero(~_same_bits(got[:, cols], ref[:, cols]).all(axis=1))[0]
    sl = tp.family_slices(key)
    by_family = {name: int(((bad >= s.start) & (bad < s.stop)).sum()) for name, s in sl.items()}
    by_family = {k: v for k, v in by_family.items() if v}
    assert bad.size == 0, "%s %s: %d of %d points differ from the reference (by family %r), first (x, y) = %r: device %r, reference %r" % (
        key, what, bad.size, len(p), by_family, p[bad[0]].tolist(), got[bad[0]].tolist(), ref[bad[0]].tolist())


@pytest.mark.gpu
def test_csv_map_bit_equal_to_the_reference():
    """h, hx, hy (and the zero hxx) of grid_eval at every point, the thresholds in both roundings included"""
    got = _probe("eval")["csv"]
    ref = reference_values("csv")
    differing = _csv_differing()
    print("\ncsv: %d points, of them %s decide differently under a fused threshold" % (len(got), {k: len(v) for k, v in differing.items()}))
    _report_bits("csv", got, ref, [0, 1, 2, 3], "grid_eval")


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(tp.GRID_MAPS)))
def test_grid_map_bit_equal_to_the_oracle(k):
    """h, hx, hy of gridmap_eval at every point: centres, borders, the nearest-cell band, FLT_MAX samples"""
    key = "grid_map%d" % k
    got = _probe("eval")[key]
    _report_bits(key, got, reference_values(key), [0, 1, 2, 3], "gridmap_eval")


def _fused_pieces(key, p):
    """rows of the analytic map `key` on a piece whose formula the device may fuse, with (mpmath value, sum |terms|) per
    column that may differ: {row: {column: (value, magnitude)}}"""
    mp = _mp()
    out = {}
    if key == "gap":
        gs, w, hh = 1.0, 0.5, 1.5
        xc, ge = gs + w / 2.0, gs + w
        a, b, c = (4 * hh) / (w * w), -(8 * hh * xc) / (w * w), -(hh * (w - 2 * xc) * (w + 2 * xc)) / (w * w)
        for i, (x, _y) in enumerate(p):
            if gs <= x <= ge:
                X = mp.mpf(float(x))
                out[i] = {0: (a * X * X + b * X + c, abs(a * X * X) + abs(b * X) + abs(c)), 1: (2 * mp.mpf(a) * X + b, abs(2 * a * X) + abs(b))}
    if key == "slope":
        ss, up, dn, hc = 1.0, 1.0, 1.0, 0.7
        xd = ss + up
        xf, sl = xd + dn, hc / up
        for i, (x, _y) in enumerate(p):
            if xd <= x < xf:
                X = mp.mpf(float(x))
                out[i] = {0: (hc - mp.mpf(sl) * (X - xd), abs(mp.mpf(hc)) + abs(mp.mpf(sl) * (X - xd)))}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("key", tp.ANALYTIC)
def test_analytic_map_takes_the_reference_branch(key):
    mp = _mp()
    got, ref, p = _probe("eval")[key], reference_values(key), tp.points(key)
    fused = _fused_pieces(key, p)
    exact = np.ones(got.shape, dtype=bool)
    worst = 0.0
    for i, cols in fused.items():
        for col, (val, mag) in cols.items():
            exact[i, col] = False
            err = abs(mp.mpf(float(got[i, col])) - val)
            bound = C_FUSED * U * mag
            worst = max(worst, float(err / bound))
            assert err <= bound, "%s column %d at x = %r: device %r, mpmath %s, error %.3g x the bound" % (
                key, col, float(p[i, 0]), float(got[i, col]), mp.nstr(val, 20), float(err / bound))
            assert abs(mp.mpf(float(ref[i, col])) - val) <= bound, "the recorded reference itself lies within the bound"
    same = _same_bits(got, ref) | ~exact
    bad = np.nonzero(~same.all(axis=1))[0]
    print("\n%s: %d points, %d on fused pieces, worst fused error %.3f of the bound" % (key, len(p), len(fused), worst))
    assert bad.size == 0, "%s: %d points differ from the reference, first (x, y) = %r: device %r, reference %r" % (
        key, bad.size, p[bad[0]].tolist(), got[bad[0]].tolist(), ref[bad[0]].tolist())


def force_reference(hx, hy, hxx, f, mu):
    """(value[30], magnitude[30]) as mpf: g5 then st25 of ForceConstraint on one node (force_constraint.cc:62-171) with the
    terrain basis and its derivative per height_map.cc:62-148, and per output the magnitude its bound scales with"""
    mp = _mp()
    hx, hy, hxx, mu = mp.mpf(float(hx)), mp.mpf(float(hy)), mp.mpf(float(hxx)), mp.mpf(float(mu))
    f = [mp.mpf(float(v)) for v in f]
    vb = [[-hx, -hy, mp.mpf(1)], [mp.mpf(1), mp.mpf(0), hx], [mp.mpf(0), mp.mpf(1), hy]]
    sq = [sum(c * c for c in v) for v in vb]
    nr = [mp.sqrt(s) for s in sq]
    nb = [[c / n for c in v] for v, n in zip(vb, nr)]
    pairs = [(0, 0.0), (1, -1.0), (1, 1.0), (2, -1.0), (2, 1.0)]     # row = basis + sign * mu * normal
    rowv = [[nb[b][i] + s * mu * nb[0][i] if b else nb[0][i] for i in range(3)] for b, s in pairs]
    rowm = [[abs(nb[b][i]) + mu * abs(nb[0][i]) if b else abs(nb[0][i]) for i in range(3)] for b, s in pairs]
    val, mag = [mp.mpf(0)] * 30, [mp.mpf(0)] * 30
    for r in range(5):
        val[r] = sum(f[i] * rowv[r][i] for i in range(3))
        mag[r] = sum(abs(f[i]) * abs(rowv[r][i]) for i in range(3))
    for dim in range(2):
        hx_d = hxx if dim == 0 else mp.mpf(0)
        dv = [[-hx_d, mp.mpf(0), mp.mpf(0)], [mp.mpf(0), mp.mpf(0), hx_d], [mp.mpf(0)] * 3]
        db = [[(1 / sq[b]) * (nr[b] * (1 if i == dim else 0) - vb[b][dim] * nb[b][i]) * dv[b][i] for i in range(3)] for b in range(3)]
        dr = [[db[b][i] + s * mu * db[0][i] if b else db[0][i] for i in range(3)] for b, s in pairs]
        for r in range(5):
            val[5 + 5 * r + dim] = sum(f[i] * dr[r][i] for i in range(3))
            mag[5 + 5 * r + dim] = sum(abs(f[i]) * abs(dr[r][i]) for i in range(3))
    for r in range(5):
        for i in range(3):
            val[5 + 5 * r + 2 + i] = rowv[r][i]
            mag[5 + 5 * r + 2 + i] = rowm[r][i]
    return val, mag


def check_force(key, got):
    """holds the (k, 30) outputs `got` at the force subset of `key` to the bound; returns the worst error / bound per kind"""
    mp = _mp()
    idx, f, mu = tp.force_subset()[key]
    ref = reference_values(key)[idx]
    p = tp.points(key)[idx]
    worst = {"g5": 0.0, "derivative": 0.0, "direction": 0.0}
    kind = ["g5"] * 5 + [("derivative" if c < 2 else "direction") for _r in range(5) for c in range(5)]
    bad = []
    for k in range(len(idx)):
        val, mag = force_reference(ref[k, 1], ref[k, 2], ref[k, 3], f[k], mu[k])
        for o in range(30):
            g = float(got[k, o])
            err = abs(mp.mpf(g) - val[o]) if np.isfinite(g) else mp.inf
            bound = C_FORCE * U * mag[o]
            if bound:
                worst[kind[o]] = max(worst[kind[o]], float(err / bound))
            if err > bound:
                bad.append((key, p[k].tolist(), o, g, mp.nstr(val[o], 20), float(err / bound) if bound else float("inf")))
    return worst, bad


@pytest.mark.gpu
def test_force_core_against_mpmath():
    got = _probe("force")
    worst, bad = {"g5": 0.0, "derivative": 0.0, "direction": 0.0}, []
    for key in tp.terrain_keys():
        w, b = check_force(key, got[key])
        print("\nforce_core on %-10s worst error / bound: %s" % (key, ", ".join("%s %.3f" % kv for kv in w.items())), end="")
        worst = {k: max(worst[k], w[k]) for k in worst}
        bad += b
    print("\nforce_core, all %d nodes: worst error / bound (C = %g): %s" % (tp.N_FORCE, C_FORCE, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert not bad, "%d outputs beyond the bound, e.g. (terrain, (x, y), output, device, mpmath, error / bound) %r" % (len(bad), bad[:5])


@pytest.mark.gpu
def test_force_core_values_do_not_depend_on_want_j():
    """g5 with want_j off has the bits of g5 with it on"""
    both, only_g = _probe("force"), _probe("force_g")
    for key in tp.terrain_keys():
        differ = np.nonzero(~_same_bits(both[key][:, :5], only_g[key]).all(axis=1))[0]
        assert differ.size == 0, "%s: g5 of %d nodes depends on want_j" % (key, differ.size)
