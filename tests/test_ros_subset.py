"""oracle/ref_dump/subset/fpowr_deps holds the stand-ins for ROS, xpp, tf and boost::geometry on which the reference's
fpowr extractors compile where those packages are absent (oracle/ref_dump/CMakeLists.txt).  They are test
infrastructure, and they are tested here on their own, without the reference: tests/ros_subset_driver.cc applies them to
the cases this module writes, and this module redoes each with numpy.

  * tf::Matrix3x3(q) * v + position against the rotation matrix of the normalised quaternion (numpy, extended precision);
  * boost::geometry::distance(point, polygon) against a brute-force point-to-segment / winding computation over the
    ring's consecutive points as given -- convex and non-convex rings, closed and unclosed, clockwise and
    counter-clockwise, rings of fewer than four points, queries on a vertex and on an edge;
  * xpp's Endeffectors ordering, the foot enumerations and the initial contact flags."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSET = os.path.join(ROOT, "oracle", "ref_dump", "subset")
L = np.longdouble


def ring_side(ring, p):
    """+1 inside, 0 on an edge, -1 outside, by the winding of the GIVEN consecutive points (no closing edge is added)
    seen along the vertical through p: an edge below p turns by the change of sign(x - p.x) over it, in half turns.
    A ring of fewer than four points holds nothing (the minimum of a closed ring)."""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    if len(ring) < 4:
        return -1
    a, b = ring[:-1], ring[1:]
    cross = (b[:, 0] - a[:, 0]) * (p[1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (p[0] - a[:, 0])
    box = (np.minimum(a, b) <= p).all(axis=1) & (p <= np.maximum(a, b)).all(axis=1)
    if np.any((cross == 0) & box):
        return 0
    sa, sb = np.sign(a[:, 0] - p[0]), np.sign(b[:, 0] - p[0])
    above = cross * (b[:, 0] - a[:, 0]) > 0        # p on the upper side of the edge
    return 1 if int(((sb - sa) * above).sum()) != 0 else -1


def segment_distance(a, b, p):
    """distance from p to the segment a b: plain projection, clamped to the segment"""
    v, w = b - a, p - a
    vv = float(v @ v)
    f = 0.0 if vv == 0.0 else min(1.0, max(0.0, float(w @ v) / vv))
    return float(np.hypot(*(p - (a + f * v))))


def ring_distance(ring, p):
    """boost::geometry::distance(point, polygon) for an outer ring walked as given: 0 inside or on it, else the distance
    to the nearest given edge (an empty ring is at distance 0, a single point is its own edge)"""
    ring = np.asarray(ring, dtype=np.float64).reshape(-1, 2)
    p = np.asarray(p, dtype=np.float64)
    if len(ring) == 0 or ring_side(ring, p) >= 0:
        return 0.0
    if len(ring) == 1:
        return float(np.hypot(*(p - ring[0])))
    return min(segment_distance(ring[i], ring[i + 1], p) for i in range(len(ring) - 1))


def _rings(rng):
    """(name, ring) pairs; coordinates are multiples of 1/64, so that side determinants and midpoints are exact"""
    out = []
    for k in range(24):
        n = int(rng.integers(4, 10))
        ang = (np.arange(n) + rng.uniform(0.1, 0.9, n)) * (2 * np.pi / n)    # spread all round: the centre lies inside
        rad = rng.uniform(0.3, 1.0, (n, 1)) if k % 2 else np.full((n, 1), rng.uniform(0.4, 1.0))   # star-shaped non-convex / convex
        centre = np.round(rng.uniform(-1, 1, 2) * 64) / 64
        pts = np.round(np.stack([np.cos(ang), np.sin(ang)], axis=1) * rad * 64) / 64 + centre
        if k % 3 == 0:
            pts = pts[::-1]                                   # clockwise (the angles ascend counter-clockwise)
        closed = k % 4 != 1
        out.append(("ring%d_%s_%s_%s" % (k, "nonconvex" if k % 2 else "convex", "cw" if k % 3 == 0 else "ccw", "closed" if closed else "open"),
                    np.concatenate([pts, pts[:1]]) if closed else pts.copy(), centre))
    out.append(("empty", np.zeros((0, 2))))
    out.append(("one_point", np.array([[0.25, -0.5]])))
    out.append(("two_points", np.array([[0.0, 0.0], [1.0, 0.5]])))
    out.append(("three_points", np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])))                 # an unclosed triangle: holds nothing
    out.append(("closed_triangle", np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 0.0], [0.0, 0.0]])))
    out.append(("self_crossing", np.array([[0.0, 0.0], [1.0, 1.0], [1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])))
    out.append(("vertical_edges", np.array([[0.0, 0.0], [0.0, 1.0], [0.5, 1.0], [0.5, 0.5], [1.0, 0.5], [1.0, 0.0], [0.0, 0.0]])))
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    work = tmp_path_factory.mktemp("ros_subset")
    exe = str(work / "driver")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", "-I" + SUBSET, "-I" + os.path.join(SUBSET, "fpowr_deps"),
                           os.path.join(ROOT, "tests", "ros_subset_driver.cc"), "-o", exe])
    rng = np.random.default_rng(17)
    cases, lines = [], []
    fmt = lambda v: " ".join(float(a).hex() for a in np.asarray(v, dtype=np.float64).reshape(-1))
    for k in range(40):                       # rotations: random, unnormalised, identity, half turns
        q = rng.normal(size=4) * rng.uniform(0.2, 3.0)
        if k == 0:
            q = np.array([0.0, 0.0, 0.0, 1.0])
        if k in (1, 2, 3):
            q = np.eye(4)[k - 1] * 2.0
        pos, loc = rng.uniform(-2, 2, 3), rng.uniform(-1, 1, 2)
        cases.append(("R", q, pos, loc))
        lines.append("R %s %s %s" % (fmt(q), fmt(pos), fmt(loc)))
    for name, ring, *centre in _rings(rng):
        queries = [rng.uniform(-1.6, 1.6, 2) for _ in range(40)]
        queries += [centre[0] + rng.uniform(-0.3, 0.3, 2) for _ in range(12 if centre else 0)]   # around the centre of the star
        queries += [np.round(rng.uniform(-1.2, 1.2, 2) * 64) / 64 for _ in range(10)]    # on the grid of the vertices: ends on the vertical
        for i in range(len(ring)):
            queries.append(ring[i].copy())                                             # on a vertex
            if i + 1 < len(ring):
                queries.append(0.5 * (ring[i] + ring[i + 1]))                          # on an edge (exact midpoint)
                queries.append(np.array([ring[i][0], ring[i][1] + 0.75]))              # above a vertex: one end on the vertical
                queries.append(np.array([ring[i][0], ring[i][1] - 0.75]))
        if len(ring) >= 2 and not np.array_equal(ring[0], ring[-1]):
            queries.append(0.5 * (ring[0] + ring[-1]))                                  # on the closing edge that is NOT there
        for p in queries:
            cases.append(("D", name, ring, p))
            lines.append("D %d %s %s" % (len(ring), fmt(ring), fmt(p)))
    for n in (1, 2, 4):
        cases.append(("E", n))
        lines.append("E %d" % n)
    (work / "cases.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(work / "cases.txt")], capture_output=True, text=True, timeout=120, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    return list(zip(cases, [ln.split() for ln in out]))


def test_tf_rotation_against_numpy(results):
    n = 0
    for case, out in results:
        if case[0] != "R":
            continue
        _, q, pos, loc = case
        x, y, z, w = (q.astype(L) / np.sqrt((q.astype(L) ** 2).sum()))
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=L)
        want = R @ np.array([loc[0], loc[1], 0.0], dtype=L) + pos.astype(L)
        got = np.array([float.fromhex(v) for v in out[1:]])
        # a dozen roundings on numbers of magnitude <= |loc| + |pos|
        assert np.all(np.abs(got.astype(L) - want) <= 16 * 2.0 ** -53 * (np.abs(loc).sum() + np.abs(pos).max())), (q, got, want)
        n += 1
    assert n == 40
    ident = [o for c, o in results if c[0] == "R"][0]
    c0 = [c for c, o in results if c[0] == "R"][0]
    assert np.array_equal([float.fromhex(v) for v in ident[1:]], [c0[3][0] + c0[2][0], c0[3][1] + c0[2][1], c0[2][2]])   # identity: exact


def test_polygon_distance_against_brute_force(results):
    seen = {}
    for case, out in results:
        if case[0] != "D":
            continue
        _, name, ring, p = case
        got, want = float.fromhex(out[1]), ring_distance(ring, p)
        side = ring_side(ring, p) if len(ring) else 1
        st = seen.setdefault(name, dict(inside=0, on=0, outside=0))
        st["inside" if side > 0 else "on" if side == 0 else "outside"] += 1
        if want == 0.0:
            assert got == 0.0, (name, p, got)
        else:
            assert abs(got - want) <= 8 * 2.0 ** -53 * max(want, np.abs(ring).max(), np.abs(p).max()), (name, p, got, want)
    assert len(seen) == 31
    for name, st in seen.items():
        if name.startswith("ring"):
            assert st["inside"] > 0 and st["on"] > 0 and st["outside"] > 0, (name, st)   # every regime on every random ring
        if name in ("one_point", "two_points", "three_points"):
            assert st["inside"] == 0 and st["on"] == 0, (name, st)                        # fewer than four points hold nothing
    assert any("_open" in n and "_cw_" in n for n in seen) and any("_open" in n and "_ccw_" in n for n in seen)
    assert any("_closed" in n and "_ccw_" in n and "nonconvex" in n for n in seen)
    # known answers: the unclosed square has no fourth edge, so the point next to the missing edge is farther than from the closed one
    sq = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [1.0, 0.0]])
    assert ring_distance(np.concatenate([sq, sq[:1]]), [0.5, -0.25]) == 0.25
    assert ring_distance(sq, [0.5, -0.25]) == np.hypot(0.5, 0.25)
    assert ring_distance(sq[:3], [0.5, 0.5]) == 0.5 and ring_distance(np.concatenate([sq, sq[:1]]), [0.5, 0.5]) == 0.0


def test_xpp_endeffectors(results):
    rows = {c[1]: o for c, o in results if c[0] == "E"}
    for n in (1, 2, 4):
        o = rows[n]
        assert int(o[1]) == n
        assert [int(v) for v in o[2:2 + n]] == list(range(n))                         # GetEEsOrdered: 0 .. n - 1 in order
        assert [float(v) for v in o[2 + n:2 + 2 * n]] == [10.0 + i for i in range(n)]   # at(id) addresses that order
        rest = o[2 + 2 * n:]
        # at(n) throws; EndeffectorsContact starts false; RobotStateCartesian sizes its sets and starts in contact; a flag
        # can be cleared through at(); StateLin3d takes a StateLinXd; then the foot enumerations
        assert rest == ["1", "1", "1", "0", "3", "4", "8", "0", "1", "0", "1", "2", "3"], rest
