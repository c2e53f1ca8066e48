"""What the tests of the request start (tests/test_start_host.py on the CPU, tests/test_start_device.py on the GPU) share:
the terrains, the structures, the request records and the bit comparison."""
import numpy as np

import towr_amd as ta

HALF_PI = 1.5707963267948966          # pi / 2 rounded to double
YAWS = (0.0, 0.3, -2.0, HALF_PI)
TIMINGS = 27 | ta.SET_TOTAL_TIME      # the default sets with optimised phase durations


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """equal as uint64 views: -0.0 != 0.0, 1e20 == 1e20, NaN == the same NaN"""
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def csv_heights():
    """HeightMapFromCSV: heights[y_cell, x_cell] of 0.17 m cells, x up to 3.4 m, y up to 2.0 m"""
    return np.round(np.random.default_rng(11).uniform(0.0, 0.25, size=(12, 20)), 2)


def grid_map(size, seed=5, resolution=0.1, position=(1.0, 0.05)):
    """(elevation[size_x, size_y] float32, resolution, centre) of a `Grid` map"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-0.05, 0.3, size=size).astype(np.float32), resolution, position)


def terrain_grid(terrain, size=(47, 37)):
    """the grid argument of tests.common.Case / ta.Structure for `terrain` (None for an analytic one)"""
    if terrain == "csv":
        return ta.TerrainGrid(csv_heights())
    if terrain == "grid_map":
        return ta.GridMap(*grid_map(size))
    return None


def goals(terrain, grid=None):
    """(x, y) of goals on and off the breakpoints of `terrain`"""
    below, above = lambda v: float(np.nextafter(v, -np.inf)), lambda v: float(np.nextafter(v, np.inf))
    pts = [(0.77, 0.13), (-0.3, -0.2), (2.05, 0.31)]
    if terrain == "stairs":
        pts += [(1.0, 0.0), (below(1.0), 0.1), (above(1.0), 0.1), (1.4, -0.2), (below(1.4), 0.0), (above(1.4), 0.0), (2.4, 0.0), (below(2.4), 0.0)]
    elif terrain == "gap":
        pts += [(1.0, 0.0), (below(1.0), 0.0), (1.5, 0.1), (above(1.5), 0.1), (1.31, 0.0)]
    elif terrain == "slope":
        pts += [(1.0, 0.0), (below(1.0), 0.0), (2.0, 0.1), (below(2.0), 0.1), (3.0, 0.0), (below(3.0), 0.0)]
    elif terrain == "csv":
        pts += [(0.17 * 3, 0.17 * 2), (below(0.17 * 3), 0.17 * 2), (0.17 * 5, above(0.17 * 4)), (3.4, 0.3), (0.3, 2.04)]
    elif terrain == "grid_map":
        sx, sy = grid.elevation.shape
        res, (px, py) = grid.resolution, grid.position
        edge_x, edge_y = px + 0.5 * sx * res, py + 0.5 * sy * res          # the map's upper borders
        centre_x, centre_y = edge_x - 0.5 * res - 3 * res, edge_y - 0.5 * res - 5 * res   # a cell centre (a bilinear breakpoint)
        pts += [(centre_x, centre_y), (below(centre_x), centre_y), (centre_x, above(centre_y)), (edge_x - 4 * res, py), (edge_x, py),
                (above(edge_x), py), (px, edge_y - 0.2 * res), (px - 0.5 * sx * res + 0.3 * res, py)]
    return pts


def request(S, goal, yaw, seed=0):
    """a request record for structure S: start at the nominal stance with NON-ZERO velocities and a small start attitude, the
    goal at `goal` with final yaw `yaw`, the feet next to their nominal positions"""
    rng = np.random.default_rng(100 + seed)
    m = S.model
    z = -m.nominal_stance[0][2]
    init = np.concatenate([[0.01, -0.02, z], rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.2, 0.2, 3)])
    final = np.concatenate([[goal[0], goal[1], z], rng.uniform(-0.1, 0.1, 3), [0.02, -0.01, yaw], rng.uniform(-0.1, 0.1, 3)])
    ee = np.array([[m.nominal_stance[e][0] + 0.01 * e, m.nominal_stance[e][1] - 0.005 * e, 0.0] for e in range(m.n_ee)])
    return ta.start_request(init, final, ee)


def host_start(S, rq):
    """(x0, x_l, x_u) of the EXISTING host functions for record rq: the yardstick"""
    ee = rq[24:24 + 3 * S.n_ee]
    x = S.initial_guess(rq[0:3], rq[6:9], rq[12:15], rq[18:21], ee)
    lo, up = S.variable_bounds(rq[0:12], rq[12:24], ee)
    return x, lo, up
