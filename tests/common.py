"""Shared helpers of the parity tests: case construction and the parity bar.

Parity bar (BASELINE.json north_star: <= 1e-9 relative on constraint values and Jacobian
non-zeros).  g is a residual and many Jacobian entries are sums with cancellation, so a pure
relative test is ill-posed at (near-)zeros; every comparison therefore uses
    |got - ref| <= RTOL*|ref| + FLOOR*scale
with RTOL = 1e-9 and FLOOR = 1e-12 (1000x tighter than 1e-9) times the magnitude `scale` of
the row the entry belongs to (max |ref| in that Jacobian row / in that constraint set for g).
The linear sets (splineacc-*, swing-*: g = J x exactly) vanish identically on e.g. the linearly
interpolated initial guess, so for their rows the scale of g is the magnitude of the terms that
cancel, sum_k |J_rk x_k| (needs x), when that is larger than the set maximum.
"""
from fractions import Fraction

import numpy as np

import towr_amd as ta
from oracle import binding as ob

RTOL = 1e-9
FLOOR = 1e-12


def row_scale(row_ptr, ref_vals):
    m = len(row_ptr) - 1
    sc = np.zeros(m)
    absv = np.abs(ref_vals)
    nz = row_ptr[1:] > row_ptr[:-1]
    sc[nz] = np.maximum.reduceat(absv, row_ptr[:-1][nz])
    return np.repeat(sc, np.diff(row_ptr))


def set_scale(con_sets, ref_g):
    sc = np.zeros_like(ref_g)
    for s in con_sets:
        a, b = s["offset"], s["offset"] + s["size"]
        if b > a:
            sc[a:b] = np.abs(ref_g[a:b]).max()
    return sc


def parity_violations(got, ref, scale):
    err = np.abs(got - ref)
    tol = RTOL * np.abs(ref) + FLOOR * scale
    return np.nonzero(~(err <= tol))[0], err


def linear_row_scale(S, ref_j, x):
    sc = np.zeros(S.m)
    terms = np.abs(ref_j * x[S.col_idx])
    for s in S.con_sets:
        if s["name"].startswith(("splineacc-", "swing-", "baseMotion", "totalduration-")):
            for r in range(s["offset"], s["offset"] + s["size"]):
                sc[r] = terms[S.row_ptr[r]:S.row_ptr[r + 1]].sum()
    return sc


def assert_parity(S, got_g, got_j, ref_g, ref_j, what="", x=None):
    gscale = set_scale(S.con_sets, ref_g)
    if x is not None:
        gscale = np.maximum(gscale, linear_row_scale(S, ref_j, np.asarray(x)))
    bad, err = parity_violations(got_g, ref_g, gscale)
    assert bad.size == 0, "%s: %d constraint values off, worst |err| %.3e at row %d" % (what, bad.size, err[bad].max(), bad[err[bad].argmax()])
    bad, err = parity_violations(got_j, ref_j, row_scale(S.row_ptr, ref_j))
    assert bad.size == 0, "%s: %d Jacobian values off, worst |err| %.3e at nz %d" % (what, bad.size, err[bad].max(), bad[err[bad].argmax()])


class Case:
    """One problem description realised both in the product (Structure) and in the oracle."""

    def __init__(self, robot, terrain, sched, grid=None, **params):
        self.robot, self.terrain = robot, terrain
        self.sched = sched
        self.params = ta.params_default(**params)
        self.model = ta.model_preset(robot, terrain)
        # gridded terrain (HeightMapFromCSV): `grid` is heights[y_cell, x_cell] or an existing ta.TerrainGrid
        if isinstance(grid, tuple):       # (elevation[size_x, size_y], resolution, (pos_x, pos_y)): the `Grid` terrain
            grid = ta.GridMap(*grid)
        self.grid = ta.TerrainGrid(grid) if isinstance(grid, np.ndarray) else grid
        self.S = ta.Structure(self.model, sched, self.params, grid=self.grid)
        p = self.params
        self.P = ob.OracleProblem(robot, terrain, sched.durations(), sched.contact(), dt_dynamic=p.dt_dynamic,
                                  dt_rom=p.dt_rom, duration_base_poly=p.duration_base_poly,
                                  polys_per_swing=p.polys_per_swing, polys_per_stance_force=p.polys_per_stance_force,
                                  constraint_sets=p.constraint_sets, dt_base_motion=p.dt_base_motion,
                                  base_z_init=p.base_z_init,
                                  grid=None if self.grid is None else self.grid.heights,
                                  grid_map=(self.grid.elevation, self.grid.resolution, self.grid.position)
                                  if isinstance(self.grid, ta.GridMap) else None)

    def nominal_start(self):
        m = self.model
        ee = [[m.nominal_stance[e][0], m.nominal_stance[e][1], 0.0] for e in range(m.n_ee)]
        z = -m.nominal_stance[0][2]
        return [0.0, 0.0, z], ee

    def x_guess(self, goal_x=1.0):
        lin0, ee = self.nominal_start()
        return self.S.initial_guess(lin0, [0, 0, 0], [goal_x, 0.0, lin0[2]], [0, 0, 0], ee)

    def x_perturbed(self, seed, goal_x=1.0, sigma=0.05):
        """x0 + sigma*N(0,1)*scale (pos 0.1 m, vel 0.5 m/s, euler 0.2 rad, force 50 N)."""
        x = self.x_guess(goal_x)
        rng = np.random.default_rng(1234 + seed)
        scale = np.ones(self.S.n)
        for vs in self.S.var_sets:
            a, b = vs["offset"], vs["offset"] + vs["size"]
            if vs["name"] == "base-lin":
                s = np.tile([0.1] * 3 + [0.5] * 3, vs["size"] // 6)
            elif vs["name"] == "base-ang":
                s = np.tile([0.2] * 3 + [0.5] * 3, vs["size"] // 6)
            elif vs["name"].startswith("ee-motion"):
                s = np.full(vs["size"], 0.1)
            elif vs["name"].startswith("ee-schedule"):
                s = np.full(vs["size"], 0.3)      # phase durations: +-15 ms at sigma = 0.05
            else:
                s = np.full(vs["size"], 50.0)
            scale[a:b] = s
        return x + sigma * rng.normal(size=self.S.n) * scale

    def x_wild(self, seed):
        """Far-from-feasible point: large angles, footholds spread over the terrain features."""
        rng = np.random.default_rng(99 + seed)
        x = rng.normal(size=self.S.n) * 0.5
        for vs in self.S.var_sets:
            a, b = vs["offset"], vs["offset"] + vs["size"]
            if vs["name"].startswith("ee-motion"):
                x[a:b] = rng.uniform(-0.5, 3.0, size=b - a)
            if vs["name"].startswith("ee-force"):
                x[a:b] = rng.normal(size=b - a) * 150.0
            if vs["name"].startswith("ee-schedule"):   # the given phase durations +-10 % (sum stays below T)
                e = int(vs["name"][len("ee-schedule"):])
                x[a:b] = np.asarray(self.sched.durations()[e][:-1]) * (1.0 + 0.1 * rng.uniform(-1, 1, size=b - a))
        return x

    def euler_positions(self):
        """indices into x of the Euler angles of base-ang, [node, axis] (the first three of each node's six values)"""
        vs = [v for v in self.S.var_sets if v["name"] == "base-ang"][0]
        assert vs["size"] % 6 == 0
        return vs["offset"] + 6 * np.arange(vs["size"] // 6)[:, None] + np.arange(3)[None, :]

    def x_turned(self, seed):
        """x_perturbed(seed) with every Euler angle turned into another quadrant: theta = k*pi/2 + delta, k cycling through
        -6 .. 6 with node, axis and seed.  A quarter of the angles are the double nearest k*pi/2 (delta = 0), a quarter that
        double's neighbour one ulp up or down, the rest have delta uniform in (-0.7, 0.7)."""
        x = self.x_perturbed(seed)
        idx = self.euler_positions()
        rng = np.random.default_rng(4321 + seed)
        node, axis = np.indices(idx.shape)
        k = (node + 4 * axis + 5 * seed) % 13 - 6
        theta = np.array([[nearest_quarter_turn(int(kk)) for kk in row] for row in k])
        kind = rng.integers(4, size=idx.shape)       # 0: the multiple itself, 1: a neighbour, 2 and 3: anywhere in the quadrant
        towards = np.where(rng.integers(2, size=idx.shape) == 1, np.inf, -np.inf)
        delta = rng.uniform(-0.7, 0.7, size=idx.shape)
        theta = np.where(kind == 1, np.nextafter(theta, towards), np.where(kind >= 2, theta + delta, theta))
        x[idx] = theta
        return x

    def x_far(self, seed):
        """x_perturbed(seed) with Euler angles on both sides of the 1e5 switch of sincos_fast: |theta| uniform in
        [5e4, 1e5) where node + axis is even and in [1e5, 3e5] where it is odd, with random sign."""
        x = self.x_perturbed(seed)
        idx = self.euler_positions()
        rng = np.random.default_rng(8765 + seed)
        node, axis = np.indices(idx.shape)
        below = np.minimum(rng.uniform(5e4, 1e5, size=idx.shape), np.nextafter(1e5, 0.0))
        above = rng.uniform(1e5, 3e5, size=idx.shape)
        x[idx] = rng.choice([-1.0, 1.0], size=idx.shape) * np.where((node + axis) % 2 == 0, below, above)
        return x

    def footholds(self):
        """indices into x of the (x, y) of every ee-motion node, one row per node, in the order of the terrain rows: a terrain
        row's Jacobian entries are (-hx, -hy, 1) at the node's x, y and z (the nodes of a stance phase share their variables)"""
        S = self.S
        pairs = []
        for cs in S.con_sets:
            if cs["name"].startswith("terrain-"):
                for r in range(cs["offset"], cs["offset"] + cs["size"]):
                    cols = S.col_idx[S.row_ptr[r]:S.row_ptr[r + 1]]
                    assert len(cols) == 3   # (a swing node's velocities lie between its coordinates)
                    pairs.append((int(cols[0]), int(cols[1])))
        return np.array(list(dict.fromkeys(pairs)), dtype=np.int64).reshape(-1, 2)

    def x_edges(self, seed):
        """x_perturbed(seed) with the x and y of every ee-motion node on the breakpoints of the case's own terrain
        (tests/terrain_points.py edge_footholds): a quarter on a breakpoint, a quarter on a neighbouring double, a quarter on a
        slope-band threshold in either rounding (CSV), a cell centre (`Grid`) or two doubles from a breakpoint, the rest
        inside a piece; which one cycles with node, foot and seed."""
        from tests import terrain_points as tp
        x = self.x_perturbed(seed)
        idx = self.footholds()
        grid_map = (self.grid.elevation, self.grid.resolution, self.grid.position) if isinstance(self.grid, ta.GridMap) else None
        heights = self.grid.heights if self.grid is not None and grid_map is None else None
        x[idx] = tp.edge_footholds(self.terrain, len(idx), seed, heights=heights, grid_map=grid_map)
        return x

    def x_junctions(self, seed, times=None):
        """x_perturbed(seed) with the ee-schedule variables re-solved foot by foot, phase after phase, so that accumulated sums
        of durations land on chosen doubles next to a time node: of the dynamic grid or of the range-of-motion grid in turn, or
        of `times` when given.  With t the time node nearest to where the perturbed junction lies and fl(t - 1e-10) the sum
        that just reaches it (t is then the threshold double of tests/segment_points.py), the kind cycles with phase, foot and
        seed: 0 the end of the phase on fl(t - 1e-10); 1 on the double one ulp below or above it; 2 on t itself or a neighbour;
        3 a polynomial junction INSIDE the phase on fl(t' - 1e-10) of its own nearest node t', through the ee-motion
        accumulation where the phase has several ee-motion polynomials and through the ee-force accumulation otherwise (the
        phase's end then stays where the solved duration puts it; the junction chosen is the one that moves the duration least,
        and a phase whose duration would move by more than 40 ms, or with one polynomial in both lists, stays as perturbed).
        The end of a phase is aimed through the phase, the ee-motion or the ee-force accumulation in turn: their sums differ by
        rounding.  A duration d_j = (target - acc) * n / j is searched 16 ulp either way for fl(acc + d_j/n + ... ) == target;
        a target that cannot be met, or would leave a duration below 20 ms (the last phase: below 5 ms), stays as perturbed."""
        from tests import segment_points as sp
        x = self.x_perturbed(seed)
        perturbed = x.copy()
        p = self.params
        durs, contact = self.sched.durations(), self.sched.contact()
        T = sp.sums(durs[0])[-1]
        if times is not None:
            grids = [np.sort(np.asarray(times, dtype=np.float64))]
        else:
            grids = [np.array(sp.time_nodes(T, p.dt_dynamic)), np.array(sp.time_nodes(T, p.dt_rom))]

        def end_of(acc, d, n, j):
            h = d / n
            for _ in range(j):
                acc += h
            return acc

        def solve(acc, n, j, target):
            d0 = (target - acc) * n / j
            for towards in (np.inf, -np.inf):
                d = d0
                for _ in range(17):
                    if end_of(acc, d, n, j) == target:
                        return d
                    d = float(np.nextafter(d, towards))
            return None

        for vs in self.S.var_sets:
            if not vs["name"].startswith("ee-schedule"):
                continue
            e = int(vs["name"][len("ee-schedule"):])
            a = vs["offset"]
            acc = {"phase": 0.0, "motion": 0.0, "force": 0.0}
            for i in range(vs["size"]):
                stance = bool(contact[e]) == (i % 2 == 0)
                count = {"phase": 1, "motion": 1 if stance else p.polys_per_swing, "force": p.polys_per_stance_force if stance else 1}
                d = float(x[a + i])
                kind = (i + e + seed) % 4
                grid = grids[(i + seed) % len(grids)]
                nearest = lambda v: float(grid[np.argmin(np.abs(grid - v))])
                new = None
                if kind == 3:
                    which = "motion" if count["motion"] > 1 else "force"
                    n = count[which]
                    # (moving junction j of n by delta moves the duration by delta * n / j: the j that moves it least)
                    found = [solve(acc[which], n, j, nearest(end_of(acc[which], d, n, j)) - sp.EPS) for j in range(1, n)]
                    found = [v for v in found if v is not None and abs(v - d) <= 0.04]
                    if found:
                        new = min(found, key=lambda v: abs(v - d))
                else:
                    which = ("phase", "motion", "force")[(i // 4 + e + seed) % 3]
                    t = nearest(acc["phase"] + d)
                    side = np.inf if (i // 4 + seed) % 2 else -np.inf
                    target = (t - sp.EPS, float(np.nextafter(t - sp.EPS, side)), t if (i // 2 + seed) % 2 else float(np.nextafter(t, side)))[kind]
                    new = solve(acc[which], count[which], count[which], target)
                if new is not None and new >= 0.02 and (i < vs["size"] - 1 or T - (acc["phase"] + new) >= 0.005):
                    d = new
                x[a + i] = d
                for name in acc:
                    acc[name] = end_of(acc[name], d, count[name], count[name])
            if T - acc["phase"] < 0.005:      # the moves added up to more than the last phase holds: this foot stays as perturbed
                x[a:a + vs["size"]] = perturbed[a:a + vs["size"]]
            assert T - sp.sums(x[a:a + vs["size"]])[-1] > 0.0, "the last phase keeps a positive duration"
        return x

    def nudged(self, x, direction):
        """x with every base-ang variable moved one ulp up (direction > 0) or down: how far the reference's own output moves
        under it is the yardstick for points where the parity bar alone is below the conditioning of the problem"""
        vs = [v for v in self.S.var_sets if v["name"] == "base-ang"][0]
        y = np.array(x, dtype=np.float64)
        seg = slice(vs["offset"], vs["offset"] + vs["size"])
        y[seg] = np.nextafter(y[seg], np.inf if direction > 0 else -np.inf)
        return y


_HALF_PI = Fraction(1.5707963267948966) + Fraction(6.123233995736766e-17)   # pi/2 to 1e-33


def nearest_quarter_turn(k):
    """the double nearest k * pi/2 (the exact rational product, rounded once)"""
    return float(k * _HALF_PI)


def hopper_schedule():
    return ta.schedule([[0.4, 0.2, 0.4, 0.2, 0.4, 0.2, 0.2]], [1])  # towr/test/hopper_example.cc:67-68


def k_params(T, K):
    """BASELINE: choose dt = T/(K-1.5) so that the reference rule floor(T/dt)+2 yields K nodes."""
    dt = T / (K - 1.5)
    return dict(dt_dynamic=dt, dt_rom=dt)


ALL_SETS = dict(constraint_sets=63)  # TWR_SETS_TOWR_DEFAULT: + splineacc-base-*, swing-* (parameters.cc:55-60)


def baseline_cases():
    """The five BASELINE.json configs at sizes the oracle handles in seconds."""
    return {
        "C1_hopper": lambda: Case("monoped", "flat", hopper_schedule()),
        "C2_biped_K100": lambda: Case("biped", "flat", ta.gait_combo(2, 0, 2.0), **k_params(2.0, 100)),
        "C3_anymal_trot_K200": lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200)),
        "C4_anymal_gap_K200": lambda: Case("anymal", "gap", ta.gait_combo(4, 2, 1.8, 0.9), **k_params(1.8, 200)),
        "C4_anymal_stairs_K200": lambda: Case("anymal", "stairs", ta.gait_combo(4, 0, 2.4, 1.1), **k_params(2.4, 200)),
    }


def random_case(seed):
    """Seeded random problem: robot, terrain, per-foot schedules with random phase counts and durations
    (same total time), polynomial counts, time steps and constraint-set mask."""
    rng = np.random.default_rng(seed)
    robot = ["monoped", "biped", "hyq", "anymal", "go1"][rng.integers(5)]
    terrain = list(ta.TERRAINS)[rng.integers(len(ta.TERRAINS))]
    grid = np.round(rng.uniform(0.0, 0.25, size=(int(rng.integers(3, 25)), int(rng.integers(3, 25)))), 2) if terrain == "csv" else None
    if terrain == "grid_map":   # a perception-like elevation patch; small enough that wild footholds also leave it
        sx, sy = int(rng.integers(8, 60)), int(rng.integers(8, 40))
        grid = (rng.uniform(-0.05, 0.3, size=(sx, sy)).astype(np.float32), float(rng.uniform(0.03, 0.12)),
                (float(rng.uniform(0.5, 1.5)), float(rng.uniform(-0.3, 0.3))))
    n_ee = ta.model_preset(robot, terrain).n_ee
    T = float(rng.uniform(0.9, 3.0))
    mask = int(rng.integers(1, 256))
    durs, contact = [], []
    for _ in range(n_ee):
        n_ph = int(rng.integers(1, 9))
        start_contact = bool(rng.integers(2))
        if mask & 32:            # swing set: schedules must start and end in stance
            start_contact = True
            n_ph = n_ph | 1
        if mask & 64:            # optimised timings: at least two phases
            n_ph = max(n_ph, 3 if mask & 32 else 2)
        d = rng.uniform(0.15, 0.6, size=n_ph)
        durs.append(d * (T / d.sum()))
        contact.append(int(start_contact))
    params = dict(constraint_sets=mask, dt_dynamic=float(rng.uniform(0.03, 0.3)), dt_rom=float(rng.uniform(0.03, 0.3)),
                  duration_base_poly=float(rng.uniform(0.05, 0.25)), polys_per_swing=int(rng.integers(1, 4)),
                  polys_per_stance_force=int(rng.integers(1, 5)), dt_base_motion=float(rng.uniform(0.02, 0.2)),
                  base_z_init=float(rng.uniform(0.3, 0.7)))
    return Case(robot, terrain, ta.schedule(durs, contact), grid=grid, **params)
