"""The points at which a terrain of kernels/terrain.h can take another branch than the reference: every breakpoint as the
double the reference's own constant expression yields, the doubles next to it, the slope-band thresholds of a CSV step in
both of their roundings, the cell centres and borders of a `Grid` map.  Seeded and deterministic; shared by
tests/test_terrain_probe.py (the device probe), oracle/ref_golden.py --terrain (the recorded reference) and Case.x_edges.

Point sets are (n, 2) arrays of (x, y).  "With neighbours" = the double itself and the doubles one and two ulp on each side."""
import functools
from fractions import Fraction

import numpy as np

ANALYTIC = ("flat", "block", "stairs", "gap", "slope", "chimney", "chimney_lr")
TERRAIN_ID = {"flat": 0, "block": 1, "stairs": 2, "gap": 3, "slope": 4, "chimney": 5, "chimney_lr": 6, "csv": 7, "grid_map": 8}
# breakpoints in x, as the reference's member initialisers compute them (height_map_examples.h:63-165)
BREAKS_X = {
    "flat": (),
    "block": (0.7, 0.7 + 0.03, 0.7 + 3.5),               # block_start, block_start + eps_, block_start + length_
    "stairs": (1.0, 1.0 + 0.4, 1.0 + 0.4 + 1.0),         # first_step_start_, + first_step_width_, + width_top
    "gap": (1.0, 1.0 + 0.5),                             # gap_start_, gap_end_x
    "slope": (1.0, 1.0 + 1.0, (1.0 + 1.0) + 1.0),        # slope_start_, x_down_start_, x_flat_start_
    "chimney": (1.0, 1.0 + 1.5),                         # x_start_, x_end_
    "chimney_lr": (0.5, 0.5 + 1.0, 0.5 + 2 * 1.0),       # x_start_, x_end1_, x_end2_
}
BREAKS_Y = {"chimney": (0.5,), "chimney_lr": (0.5, -0.5)}   # where the chimneys' heights cross zero (y_start_)
SHARED = {"block": 0.7 + 0.03, "chimney_lr": 0.5 + 1.0}      # the point two closed intervals share: the second `if` wins
N_UNIFORM = 256

CSV_RES = 0.17
CSV_EPS = CSV_RES / 50                                       # height_map_from_csv.h:112-115
# heights[y_cell, x_cell], 7 x 9: along every column step and every row step some line rises, some falls, some stays level
CSV_HEIGHTS = 0.1 * np.array([[1, 3, 3, 1, 0, 2, 2, 3, 2],
                              [2, 3, 3, 3, 3, 2, 3, 0, 0],
                              [3, 1, 2, 1, 3, 0, 2, 0, 0],
                              [3, 1, 3, 1, 3, 3, 1, 3, 2],
                              [3, 1, 2, 2, 3, 1, 1, 3, 3],
                              [3, 0, 3, 0, 3, 3, 3, 3, 2],
                              [2, 2, 0, 3, 3, 0, 2, 1, 2]], dtype=np.float64)

GRID_MAPS = (dict(size=(9, 7), res=0.05, pos=(1.0, 0.1), seed=31), dict(size=(6, 11), res=0.07, pos=(-0.3, 0.45), seed=32))
FLT_MAX = float(np.finfo(np.float32).max)


def neighbours(v):
    """v and the doubles one and two ulp below and above, (n, 5) in rising order"""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    up1, dn1 = np.nextafter(v, np.inf), np.nextafter(v, -np.inf)
    return np.stack([np.nextafter(dn1, -np.inf), dn1, v, up1, np.nextafter(up1, np.inf)], axis=1)


def _pair(xs, ys):
    return np.stack([np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)], axis=1)


# --------------------------------------------------------------------------------------------------- analytic maps
def analytic_families(name):
    """family -> (n, 2) points of one analytic map"""
    rng = np.random.default_rng(100 + TERRAIN_ID[name])
    bx = BREAKS_X[name]
    fam = {}
    edge = neighbours(bx).ravel() if bx else np.zeros(0)
    fam["break_x"] = _pair(edge, rng.uniform(-1.0, 1.0, edge.size))
    cuts = (-0.5,) + tuple(bx) + ((bx[-1] if bx else 0.0) + 0.5,)
    mid = np.array([0.5 * (a + b) for a, b in zip(cuts[:-1], cuts[1:])])
    fam["mid"] = _pair(mid, rng.uniform(-1.0, 1.0, mid.size))
    inside = [0.5 * (bx[0] + bx[-1])] if bx else [0.0]
    pieces = np.concatenate([rng.uniform(a, b, 24) for a, b in zip(bx[:-1], bx[1:])]) if bx else rng.uniform(-0.5, 0.5, 24)
    fam["pieces"] = _pair(pieces, rng.uniform(-1.0, 1.0, pieces.size))     # inside every bounded piece
    if name in BREAKS_Y:
        edge_y = neighbours(BREAKS_Y[name]).ravel()
        # once in every piece of x: the chimneys' height changes sign at y_start on the piece that has a slope
        xs = np.concatenate([np.full(edge_y.size, m) for m in mid])
        fam["break_y"] = _pair(xs, np.tile(edge_y, mid.size))
    special = np.array([0.0, -0.0, 10.0, -10.0])
    fam["special"] = np.concatenate([_pair(special, rng.uniform(-1.0, 1.0, 4)), _pair(np.full(4, inside[0]), special)])
    fam["uniform"] = _pair(rng.uniform(-0.5, 4.7, N_UNIFORM), rng.uniform(-1.0, 1.0, N_UNIFORM))
    return fam


# --------------------------------------------------------------------------------------------------------- CSV map
def _f(v):
    return Fraction(float(v))


def csv_thresholds(c, res=CSV_RES, eps=CSV_EPS):
    """The slope-band thresholds of cell index c as the reference rounds them (two operations) and as one fused
    multiply-add rounds them: dict(edge = fl(c res), end2 = fl(fl((c+1) res) - eps), end1 = fl((c+1) res - eps),
    start2 = fl(fl(c res) + eps), start1 = fl(c res + eps))"""
    return dict(edge=float(c) * res, end2=float(c + 1) * res - eps, end1=float((c + 1) * _f(res) - _f(eps)),
                start2=float(c) * res + eps, start1=float(c * _f(res) + _f(eps)))


def cell_crossing(c, res=CSV_RES):
    """the smallest double v >= 0 with fl(v / res) >= c: where the truncated cell index becomes c"""
    v = float(c) * res
    while v / res >= c and v > 0.0:
        v = np.nextafter(v, -np.inf)
    while v / res < c:
        v = np.nextafter(v, np.inf)
    return float(v)


def csv_line_values(n):
    """the coordinates that matter along one dimension with n cells, each with neighbours: name -> (k, 5)"""
    out = {k: [] for k in ("edge", "end2", "end1", "start2", "start1", "crossing")}
    for c in range(n + 1):
        t = csv_thresholds(c)
        out["edge"].append(t["edge"])
        out["crossing"].append(cell_crossing(c))
        if c < n:
            out["end2"].append(t["end2"])
            out["start2"].append(t["start2"])
            if t["end1"] != t["end2"]:
                out["end1"].append(t["end1"])
            if t["start1"] != t["start2"]:
                out["start1"].append(t["start1"])
    return {k: neighbours(v) if v else np.zeros((0, 5)) for k, v in out.items()}


def csv_cell(v, res=CSV_RES):
    """the reference's cell index: static_cast<size_t>(v / res), -1 for what wraps to an invalid index"""
    q = np.asarray(v, dtype=np.float64) / res
    return np.where(q <= -1.0, -1, np.trunc(q)).astype(np.int64)


def csv_families():
    """family -> (n, 2) points of the CSV map CSV_HEIGHTS"""
    rows, cols = CSV_HEIGHTS.shape
    rng = np.random.default_rng(107)
    fam = {}
    for dim, n, n_other in ((0, cols, rows), (1, rows, cols)):
        for kind, vals in csv_line_values(n).items():
            v = vals.ravel()
            # every line of cells of the other dimension, at its centre and at four other places outside its slope bands
            other = np.concatenate([(np.arange(n_other) + o) * CSV_RES for o in (0.5, 0.31, 0.77, 0.12, 0.9)])
            vv, oo = np.repeat(v, other.size), np.tile(other, v.size)
            fam["%s_%s" % (kind, "xy"[dim])] = _pair(vv, oo) if dim == 0 else _pair(oo, vv)
    # both coordinates on a threshold at once
    lx, ly = csv_line_values(cols), csv_line_values(rows)
    cx = np.concatenate([lx[k][:, 2] for k in ("edge", "end2", "start2")])
    cy = np.concatenate([ly[k][:, 2] for k in ("edge", "end2", "start2")])
    fam["corner"] = _pair(np.repeat(cx, cy.size), np.tile(cy, cx.size))
    neg = -CSV_RES * np.array([1e-300, 1e-9, 0.25, 0.5, 0.999, float(np.nextafter(1.0, 0.0))])
    fam["negative_cell0"] = np.concatenate([_pair(neg, rng.uniform(0.0, rows * CSV_RES, neg.size)), _pair(rng.uniform(0.0, cols * CSV_RES, neg.size), neg)])
    below = np.concatenate([neighbours(-CSV_RES).ravel()[:3], [-0.2, -1.0, -10.0]])
    above_x = np.concatenate([neighbours(cols * CSV_RES).ravel(), [cell_crossing(cols), cols * CSV_RES + 0.001, cols * CSV_RES + 1.0]])
    above_y = np.concatenate([neighbours(rows * CSV_RES).ravel(), [cell_crossing(rows), rows * CSV_RES + 0.001, rows * CSV_RES + 1.0]])
    fam["outside"] = np.concatenate([_pair(below, rng.uniform(0.0, rows * CSV_RES, below.size)), _pair(rng.uniform(0.0, cols * CSV_RES, below.size), below),
                                     _pair(above_x, rng.uniform(0.0, rows * CSV_RES, above_x.size)), _pair(rng.uniform(0.0, cols * CSV_RES, above_y.size), above_y)])
    fam["uniform"] = _pair(rng.uniform(0.0, cols * CSV_RES, 2048), rng.uniform(0.0, rows * CSV_RES, 2048))
    return fam


def csv_expected(x, y, fused=False, heights=CSV_HEIGHTS, res=CSV_RES, eps=CSV_EPS):
    """(h, hx, hy) of HeightMapFromCSV at one point from exact rational arithmetic on the reference's rounded thresholds
    (fused = True: on the thresholds one fused multiply-add yields instead) -- for the conditions on the inputs only"""
    rows, cols = heights.shape
    xc, yc = int(csv_cell(x, res)), int(csv_cell(y, res))
    if xc < 0 or yc < 0 or xc >= cols or yc >= rows:
        return 0.0, 0.0, 0.0
    h0 = heights[yc, xc]
    out = [h0]
    for v, c, n, nxt, prv in ((x, xc, cols, (yc, xc + 1), (yc, xc - 1)), (y, yc, rows, (yc + 1, xc), (yc - 1, xc))):
        t = csv_thresholds(c, res, eps)
        d = 0.0
        done = False
        if c + 1 < n:
            diff = heights[nxt] - h0
            if diff > 0 and v <= float(c + 1) * res and v >= (t["end1"] if fused else t["end2"]):
                d, done = diff / eps, True
        if not done and c - 1 >= 0:
            diff = h0 - heights[prv]
            if diff < 0 and v >= t["edge"] and v <= (t["start1"] if fused else t["start2"]):
                d = diff / eps
        out.append(d)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------- `Grid` maps
def grid_elevation(m):
    rng = np.random.default_rng(m["seed"])
    return rng.uniform(-0.05, 0.3, size=m["size"]).astype(np.float32)


def grid_lines(m, a):
    """(centres, borders) of map m along axis a, as grid_map's getPositionFromIndex rounds them"""
    n, res, p = m["size"][a], m["res"], m["pos"][a]
    length = n * res
    centres = np.array([p + 0.5 * length - 0.5 * res - res * float(i) for i in range(n)])
    borders = np.array([p + 0.5 * length - res * float(i) for i in range(n + 1)])
    return centres, borders


def grid_families(m):
    """family -> (n, 2) points of one `Grid` map"""
    rng = np.random.default_rng(200 + m["seed"])
    res, eps = m["res"], m["res"] / 6.0
    lo = [m["pos"][a] + 0.5 * m["size"][a] * res - m["size"][a] * res for a in (0, 1)]    # tx = lx: the excluded border
    hi = [m["pos"][a] + 0.5 * m["size"][a] * res for a in (0, 1)]                            # tx = 0: the included border
    lines = [grid_lines(m, a) for a in (0, 1)]
    fam = {}
    for a in (0, 1):
        o = 1 - a
        for kind, vals in (("centre", lines[a][0]), ("border", lines[a][1])):
            v = neighbours(vals).ravel()
            other = np.concatenate([lines[o][0][[0, len(lines[o][0]) // 2]], rng.uniform(lo[o], hi[o], 5), [lo[o] + 0.3 * eps, hi[o] - 0.3 * eps]])
            vv, oo = np.repeat(v, other.size), np.tile(other, v.size)
            fam["%s_%s" % (kind, "xy"[a])] = _pair(vv, oo) if a == 0 else _pair(oo, vv)
        n = 48
        for side, base, sgn in (("lo", lo[a], 1.0), ("hi", hi[a], -1.0)):
            band = base + sgn * rng.uniform(0.0, 0.5 * res, n)            # the 2 x 2 stencil leaves the map: nearest cell
            near_in = base + sgn * rng.uniform(0.0, eps, n)               # one of the +- eps samples is outside
            near_out = base - sgn * rng.uniform(0.0, eps, n)              # the point is outside, one sample inside
            far_out = base - sgn * rng.uniform(eps, 3 * eps, n)           # the point and both samples outside: slope exactly 0
            v = np.concatenate([band, near_in, near_out, far_out])
            w = rng.uniform(lo[o] - eps, hi[o] + eps, v.size)
            fam["band_%s_%s" % (side, "xy"[a])] = _pair(v, w) if a == 0 else _pair(w, v)
    cx, cy = neighbours([lo[0], hi[0]]).ravel(), neighbours([lo[1], hi[1]]).ravel()
    fam["corner"] = _pair(np.repeat(cx, cy.size), np.tile(cy, cx.size))
    out = []
    for a in (0, 1):
        for base, sgn in ((lo[a], -1.0), (hi[a], 1.0)):
            for d in (0.001, 1.0):
                out.append((a, base + sgn * d))
            out.append((a, float(np.nextafter(base, sgn * np.inf))))
    w = [rng.uniform(lo[1 - a], hi[1 - a]) for a, _ in out]
    fam["outside"] = np.array([(v, u) if a == 0 else (u, v) for (a, v), u in zip(out, w)])
    fam["uniform"] = _pair(rng.uniform(lo[0] - 2 * res, hi[0] + 2 * res, 2048), rng.uniform(lo[1] - 2 * res, hi[1] + 2 * res, 2048))
    return fam


# ----------------------------------------------------------------------------------------------------------- the set
def terrain_keys():
    """the terrains of the probe in order: the seven analytic maps, the CSV map, the two `Grid` maps"""
    return ANALYTIC + ("csv", "grid_map0", "grid_map1")


@functools.lru_cache(maxsize=None)
def families(key):
    if key in ANALYTIC:
        return analytic_families(key)
    if key == "csv":
        return csv_families()
    return grid_families(GRID_MAPS[int(key[-1])])


@functools.lru_cache(maxsize=None)
def points(key):
    """every point of one terrain, (n, 2), families in order; read-only"""
    p = np.ascontiguousarray(np.concatenate(list(families(key).values())))
    p.flags.writeable = False
    return p


def family_slices(key):
    out, at = {}, 0
    for name, v in families(key).items():
        out[name] = slice(at, at + len(v))
        at += len(v)
    return out


N_FORCE = 1024
MUS = (0.5, 0.85)


@functools.lru_cache(maxsize=None)
def force_subset():
    """The force_core inputs: dict(key -> (index into points(key), force (k, 3), mu (k,))), N_FORCE in all.  Every terrain;
    the steep points always: the CSV slope-band thresholds, the `Grid` points next to a border, the Gap's edges and pieces."""
    rng = np.random.default_rng(4242)
    keys = terrain_keys()
    share = {k: 40 for k in ANALYTIC}
    share["gap"] = 144
    share["csv"] = 300
    share["grid_map0"] = share["grid_map1"] = (N_FORCE - 6 * 40 - 144 - 300) // 2
    out = {}
    for key in keys:
        sl, n = family_slices(key), share[key]
        steep = []
        if key == "gap":
            steep = [i for name in ("break_x", "mid", "pieces") for i in range(sl[name].start, sl[name].stop)]
        elif key == "csv":
            for name in ("end2_x", "end1_x", "start2_x", "start1_x", "end2_y", "end1_y", "start2_y", "start1_y", "corner"):
                idx = np.arange(sl[name].start, sl[name].stop)
                steep += list(rng.choice(idx, min(len(idx), 24), replace=False))
        elif key.startswith("grid_map"):
            for name in sl:
                if name.startswith(("band_", "border_", "corner")):
                    idx = np.arange(sl[name].start, sl[name].stop)
                    steep += list(rng.choice(idx, min(len(idx), 18), replace=False))
        steep = sorted(set(int(i) for i in steep))[:n]
        rest = np.setdiff1d(np.arange(len(points(key))), steep)
        idx = np.concatenate([np.array(steep, dtype=np.int64), rng.choice(rest, n - len(steep), replace=False)])
        f = rng.normal(size=(n, 3)) * 300.0
        f[:7] = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 0]]
        f = np.roll(f, n // 2, axis=0)                   # (the unit and zero forces land on points of both kinds)
        mu = np.where(np.arange(n) % 2 == 0, MUS[0], MUS[1])
        for a in (idx, f, mu):
            a.flags.writeable = False
        out[key] = (idx, f, mu)
    assert sum(len(v[0]) for v in out.values()) == N_FORCE
    return out


# ------------------------------------------------------------------------------------ footholds of whole problems
def map_lines(size, res, pos, a):
    """(centres, borders) along axis a of a `Grid` map of `size` cells, as getPositionFromIndex rounds them"""
    return grid_lines(dict(size=size, res=res, pos=pos), a)


def breakpoint_lines(terrain, heights=None, grid_map=None):
    """(the x coordinates, the y coordinates) at which `terrain` changes branch: the analytic maps' breakpoints, the cell
    edges fl(c res) of a CSV map heights[y_cell, x_cell], the cell borders of a `Grid` map (elevation, res, pos)"""
    if terrain == "csv":
        rows, cols = heights.shape
        return np.array([float(c) * CSV_RES for c in range(cols + 1)]), np.array([float(c) * CSV_RES for c in range(rows + 1)])
    if terrain == "grid_map":
        el, res, pos = grid_map
        return map_lines(el.shape, res, pos, 0)[1], map_lines(el.shape, res, pos, 1)[1]
    return np.array(BREAKS_X[terrain], dtype=np.float64), np.array(BREAKS_Y.get(terrain, ()), dtype=np.float64)


def on_breakpoint(terrain, xy, heights=None, grid_map=None):
    """per point: x or y is a breakpoint of the terrain or one of its two neighbouring doubles"""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    out = np.zeros(len(xy), dtype=bool)
    for a, lines in enumerate(breakpoint_lines(terrain, heights, grid_map)):
        if len(lines):
            near = neighbours(lines)[:, 1:4].ravel()
            out |= np.isin(xy[:, a], near)
    return out


def edge_footholds(terrain, n, seed, heights=None, grid_map=None):
    """n footholds (n, 2) for a problem on `terrain`, foothold k of kind (n - 1 - k + seed) % 4 (counted from the last one, whose
    stance phase fills the partial last chunk of the force nodes):
      0 on a breakpoint, 1 on the double next to one (up or down), 2 on a slope-band threshold in either rounding (CSV), a
      cell centre (`Grid`) or the double two steps from a breakpoint (analytic maps), 3 anywhere inside a piece.
    Which breakpoint, which coordinate carries it and which way the neighbour lies cycle with k and seed.  On a CSV map the
    other coordinate is the centre of a line of cells along which the step at that threshold is a slope, where there is one."""
    rng = np.random.default_rng(9000 + seed)
    out = np.empty((n, 2))
    lines = breakpoint_lines(terrain, heights, grid_map)
    for k in range(n):
        j = k + 7 * seed
        kind, q = (n - 1 - k + seed) % 4, j // 4
        up = np.inf if (q // 2) % 2 else -np.inf
        if terrain == "csv":
            rows, cols = heights.shape
            a = q % 2                                     # the coordinate on the line: 0 = x
            nc, no = (cols, rows) if a == 0 else (rows, cols)
            c = 1 + (q // 2) % (nc - 1)                   # an interior edge: cells c - 1 and c meet at fl(c res)
            t = csv_thresholds(c)
            step = (heights[:, c] - heights[:, c - 1]) if a == 0 else (heights[c, :] - heights[c - 1, :])   # per line of the other axis
            side = (q // 4) % 2                           # kind 2: 0 = the band below the edge (cell c - 1), 1 = above it (cell c)
            if kind == 2 and side == 0:
                tb = csv_thresholds(c - 1)
                v = tb["end1"] if (q // 8) % 2 else tb["end2"]
                active = np.nonzero(step > 0)[0]
            elif kind == 2:
                v = t["start1"] if (q // 8) % 2 else t["start2"]
                active = np.nonzero(step < 0)[0]
            else:
                v = t["edge"] if kind == 0 else float(np.nextafter(t["edge"], up)) if kind == 1 else rng.uniform(0.0, nc * CSV_RES)
                active = np.nonzero(step != 0)[0]
            line = active[j % len(active)] if len(active) else j % no
            w = (line + 0.5) * CSV_RES if kind != 3 else rng.uniform(0.0, no * CSV_RES)
            out[k] = (v, w) if a == 0 else (w, v)
        elif terrain == "grid_map":
            el, res, pos = grid_map
            a = q % 2
            centres, borders = map_lines(el.shape, res, pos, a)
            lo, hi = [pos[b] - 0.5 * el.shape[b] * res for b in (0, 1)], [pos[b] + 0.5 * el.shape[b] * res for b in (0, 1)]
            borders = np.concatenate([borders, borders[[0, -1]]])    # the map's own borders twice: an FLT_MAX sample
            b = borders[(q // 2) % len(borders)]
            v = b if kind == 0 else float(np.nextafter(b, up)) if kind == 1 else centres[(q // 2) % len(centres)] if kind == 2 else rng.uniform(lo[a], hi[a])
            w = rng.uniform(lo[1 - a], hi[1 - a])
            out[k] = (v, w) if a == 0 else (w, v)
        else:
            bx, by = lines
            b = bx[q % len(bx)]
            x = b if kind == 0 else float(np.nextafter(b, up)) if kind == 1 else float(np.nextafter(np.nextafter(b, up), up)) if kind == 2 else rng.uniform(-0.5, bx[-1] + 0.5)
            y = rng.uniform(-1.0, 1.0)
            if len(by) and (q // len(bx)) % 2:            # the chimneys: the zero crossing of the height in y as well
                y = by[q % len(by)] if kind != 1 else float(np.nextafter(by[q % len(by)], up))
            out[k] = (x, y)
    return out
