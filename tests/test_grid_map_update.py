"""A new grid_map elevation layer for a live handle and a live batch: twr_terrain_grid_map_update (host),
twr_batch_grid_map_sync and twr_batch_grid_map_update_device (device), through towr_amd.GridMap.update, Batch.sync_grid_map and
Batch.update_grid_map_device.

The yardstick is never the code under test: what an updated handle or batch computes is compared, bit for bit (integer views, so
NaN and FLT_MAX rows count), with what the create path computes on the UNROLLED layer np.roll(buf, (-start_x, -start_y), (0, 1))
-- a fresh GridMap, fresh structures, a fresh batch -- and, to the parity bar of tests/common.py, with the CPU oracle on that
same unrolled layer.

Maps: 47 x 37 cells (not square, both sizes odd, neither a multiple of 4 or 64: a transposed index, a tail lane or a misaligned
column shows) and 5 x 3 cells (a wrap run shorter than a wave).  Start indices: none, inside, the last cell in both dimensions,
the last cell in one."""
import ctypes as C
import functools

import numpy as np
import pytest

import towr_amd as ta
from tests.common import Case, assert_parity, hopper_schedule

BIG, SMALL = (47, 37), (5, 3)
STARTS = {BIG: ((0, 0), (17, 5), (46, 36), (46, 0)), SMALL: ((0, 0), (2, 1), (4, 2), (4, 0))}
RES = {BIG: 0.05, SMALL: 0.45}                      # 2.35 m x 1.85 m and 2.25 m x 1.35 m: the robot's 1.6 m walk fits, x_wild leaves
POS_A, POS_B = (1.0, 0.1), (0.85, -0.05)            # the map centre moves with the update
FLT_MAX = float(np.finfo(np.float32).max)


def layer(size, seed):
    """A perception-like patch: a ramp along x plus noise, float32 [size_x, size_y]."""
    rng = np.random.default_rng(seed)
    return (0.03 * np.arange(size[0])[:, None] * RES[size] + rng.uniform(-0.05, 0.25, size=size)).astype(np.float32)


def rolled(a, start):
    """The circular buffer grid_map holds for layer `a` after a move to start index `start`: rolled(a, s)[(i + sx) % n] = a[i]."""
    return np.asfortranarray(np.roll(a, start, axis=(0, 1)))


def unrolled(buf, start):
    return np.asfortranarray(np.roll(buf, (-start[0], -start[1]), axis=(0, 1)))


def u32(a):
    return np.asfortranarray(a, dtype=np.float32).view(np.uint32)


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u64(a), u64(b))


def grid_info(gm):
    """(layer [size_x, size_y] as the handle stores it, (pos_x, pos_y)) straight from twr_terrain_grid_info."""
    kind, sx, sy = C.c_int32(), C.c_int32(), C.c_int32()
    res, px, py, data = C.c_double(), C.c_double(), C.c_double(), C.c_void_p()
    rc = ta.lib().twr_terrain_grid_info(gm._h, C.byref(kind), C.byref(sx), C.byref(sy), C.byref(res), C.byref(px), C.byref(py), C.byref(data))
    assert rc == 0 and kind.value == 1
    flat = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_float)), shape=(sx.value * sy.value,)).copy()
    return flat.reshape((sx.value, sy.value), order="F"), (px.value, py.value), res.value


def where_footholds_fall(case, xs, size, pos):
    """How many footholds of xs lie in the interior of the map (bilinear over four cells), in its half-cell border band (nearest
    cell) and outside it (FLT_MAX), by grid_map's published rule for a map of `size` cells centred on `pos`."""
    idx = case.footholds()
    res = RES[size]
    n = dict(interior=0, border=0, outside=0)
    for x in xs:
        fx, fy = x[idx[:, 0]], x[idx[:, 1]]
        tx, ty = pos[0] + 0.5 * size[0] * res - fx, pos[1] + 0.5 * size[1] * res - fy
        inside = (tx >= 0) & (ty >= 0) & (tx < size[0] * res) & (ty < size[1] * res)
        edge = np.minimum(np.minimum(tx, size[0] * res - tx), np.minimum(ty, size[1] * res - ty))
        n["outside"] += int((~inside).sum())
        n["border"] += int((inside & (edge < 0.5 * res)).sum())
        n["interior"] += int((inside & (edge > 0.5 * res)).sum())
    return n


# robot, map size, constraint sets, gait, and the x_wild seeds: those whose footholds also fall into the half-cell border band of
# the map at both centres (2.5 cm wide on the larger map; Live asserts what is hit)
CASES = {"go1_47x37": ("go1", BIG, 127, 1, (5, 20)), "go1_5x3": ("go1", SMALL, 127, 1, (1, 7)), "anymal_47x37": ("anymal", BIG, 27, 0, (23, 0))}


class Live:
    """A structure on a GridMap handle holding map A, the inputs every test evaluates, and the maps it moves between."""

    def __init__(self, name):
        robot, self.size, self.sets, combo, wild = CASES[name]
        self.robot, self.sched = robot, ta.gait_combo(4, combo, 2.0)
        self.A, self.B = layer(self.size, 1), layer(self.size, 2)
        self.gm = ta.GridMap(self.A, RES[self.size], POS_A)
        self.case = Case(robot, "grid_map", self.sched, grid=self.gm, constraint_sets=self.sets)
        c = self.case
        self.xs = [c.x_guess(1.6), c.x_perturbed(0, 1.6), c.x_perturbed(1, 1.2)] + [c.x_wild(seed) for seed in wild]
        for pos in (POS_A, POS_B):
            hit = where_footholds_fall(c, self.xs, self.size, pos)
            assert min(hit.values()) > 0, "interior, border band and the FLT_MAX outside must all be hit: %r" % (hit,)

    def fresh(self, elev, pos):
        """The create path on a layer with start index (0,0): a new handle, a new structure, the oracle on the same map."""
        return Case(self.robot, "grid_map", self.sched, grid=(elev, RES[self.size], pos), constraint_sets=self.sets)


@functools.lru_cache(maxsize=None)
def live(name):
    return Live(name)


# ---------------------------------------------------------------- host: twr_terrain_grid_map_update

@pytest.mark.parametrize("size", [BIG, SMALL], ids=["47x37", "5x3"])
def test_host_update_unrolls_the_buffer_bit_for_bit_and_structures_follow(size):
    """1. For each start index the handle holds the unrolled layer bit for bit (a NaN with a payload, FLT_MAX and -0.0 included) and
    the new centre, and a structure built BEFORE the update gives the initial guess and the variable bounds of a structure built
    on the new map."""
    model = ta.model_preset("go1", "grid_map")
    sched = ta.gait_combo(4, 1, 2.0)
    gm = ta.GridMap(layer(size, 1), RES[size], POS_A)
    S = ta.Structure(model, sched, ta.params_default(constraint_sets=127), grid=gm)
    ee = [[model.nominal_stance[e][0], model.nominal_stance[e][1], 0.0] for e in range(4)]
    init, final = [0, 0, 0.3] + [0.0] * 9, [1.6, 0, 0.3] + [0.0] * 9
    for k, start in enumerate(STARTS[size]):
        new = layer(size, 10 + k)
        special = new.view(np.uint32)
        special[1, 1], special[size[0] - 1, size[1] - 1], special[0, 2] = 0x7FC12345, 0x7F7FFFFF, 0x80000000
        buf, pos = rolled(new, start), (0.9 + 0.01 * k, -0.1 * k)
        gm.update(buf, pos, start)
        stored, centre, res = grid_info(gm)
        assert np.array_equal(u32(stored), u32(unrolled(buf, start))) and np.array_equal(u32(stored), u32(new)), start
        assert centre == pos and gm.position == pos and res == RES[size]
        assert np.array_equal(u32(gm.elevation), u32(new)) and gm.elevation.flags.f_contiguous
        # (the structure calls read cells: take the NaN out again, keep the rest)
        new[1, 1] = 0.125
        buf = rolled(new, start)
        gm.update(buf, pos, start)
        ref = ta.Structure(model, sched, ta.params_default(constraint_sets=127), grid=ta.GridMap(new, RES[size], pos))
        a, b = S.initial_guess([0, 0, 0.3], [0, 0, 0], [1.6, 0, 0.3], [0, 0, 0], ee), ref.initial_guess([0, 0, 0.3], [0, 0, 0], [1.6, 0, 0.3], [0, 0, 0], ee)
        assert same_bits(a, b), start
        for got, want in zip(S.variable_bounds(init, final, ee), ref.variable_bounds(init, final, ee)):
            assert same_bits(got, want), start
    assert not same_bits(a, ta.Structure(model, sched, ta.params_default(constraint_sets=127),
                                         grid=ta.GridMap(layer(size, 1), RES[size], POS_A)).initial_guess(
                                             [0, 0, 0.3], [0, 0, 0], [1.6, 0, 0.3], [0, 0, 0], ee)), "the guess must depend on the map"


def test_host_update_refuses_bad_arguments_and_leaves_the_handle_alone():
    """2. Every bad argument is TWR_ERR_INVALID with a message that names it, and the handle is as before."""
    L = ta.lib()
    a = layer(BIG, 3)
    gm = ta.GridMap(a, RES[BIG], POS_A)
    csv = ta.TerrainGrid(np.zeros((4, 5)))
    new = rolled(layer(BIG, 4), (3, 3))
    p = new.ctypes.data
    nan, inf = float("nan"), float("inf")
    bad = [((None, p, 0, 0, 0.0, 0.0), "g"), ((gm._h, None, 0, 0, 0.0, 0.0), "elevation"), ((gm._h, p + 2, 0, 0, 0.0, 0.0), "elevation"),
           ((csv._h, p, 0, 0, 0.0, 0.0), "g"), ((gm._h, p, -1, 0, 0.0, 0.0), "start_x"), ((gm._h, p, BIG[0], 0, 0.0, 0.0), "start_x"),
           ((gm._h, p, 0, -1, 0.0, 0.0), "start_y"), ((gm._h, p, 0, BIG[1], 0.0, 0.0), "start_y"), ((gm._h, p, 0, 0, nan, 0.0), "pos_x"),
           ((gm._h, p, 0, 0, 0.0, inf), "pos_y"), ((gm._h, p, 0, 0, -inf, 0.0), "pos_x")]
    for args, name in bad:
        assert L.twr_terrain_grid_map_update(*args) == -1, args[2:]
        assert name in L.twr_last_error().decode().split(), (args[2:], L.twr_last_error())
        stored, centre, _ = grid_info(gm)
        assert np.array_equal(u32(stored), u32(a)) and centre == POS_A
    with pytest.raises(ta.TowrError, match="another size"):
        gm.update(layer(SMALL, 1), POS_A)
    assert L.twr_terrain_grid_map_update(gm._h, p, 3, 3, 0.5, 0.25) == 0     # and the same arguments, well-formed, are taken
    stored, centre, _ = grid_info(gm)
    assert np.array_equal(u32(stored), u32(unrolled(new, (3, 3)))) and centre == (0.5, 0.25)


# ---------------------------------------------------------------- device

def torch_ctx():
    import torch

    return torch, torch.device("cuda", 0)


def dev_layer(buf):
    """A layer on the device in grid_map's storage order: a [size_x, size_y] tensor with stride (1, size_x)."""
    torch, dev = torch_ctx()
    return torch.from_numpy(np.ascontiguousarray(np.asfortranarray(buf, dtype=np.float32).T)).to(dev).t()


class Runner:
    """A batch with x on the device and one set of output buffers per request; run() enqueues all three requests on `stream`."""

    def __init__(self, structs, order, xs):
        torch, dev = torch_ctx()
        self.batch = ta.Batch(structs, order, device=0)
        self.x = torch.from_numpy(np.concatenate(xs)).to(dev)
        new = lambda n: torch.full((max(1, int(n)),), 7.0, dtype=torch.float64, device=dev)
        b = self.batch
        self.new_out = lambda: dict(g=new(b.g_off[-1]), j=new(b.jac_off[-1]), gv=new(b.g_off[-1]), gs=new(b.g_off[-1]), s=new(16 * b.n_problems))
        self.out = self.new_out()

    def run(self, stream=0, out=None):
        o, b, x = out or self.out, self.batch, self.x.data_ptr()
        b.eval_device(x, o["g"].data_ptr(), o["j"].data_ptr(), ta.EVAL_BOTH, stream)
        b.eval_device(x, o["gv"].data_ptr(), 0, ta.EVAL_VALUES, stream)
        b.eval_scores_device(x, o["s"].data_ptr(), d_g=o["gs"].data_ptr(), stream=stream)

    def read(self, out=None):
        torch, _ = torch_ctx()
        torch.cuda.synchronize()
        o = out or self.out
        return {k: o[k].cpu().numpy().copy() for k in ("g", "j", "gv", "s")}

    def __call__(self):
        self.run()
        return self.read()


def assert_same(got, want, what):
    for k in ("g", "j", "gv", "s"):
        assert same_bits(got[k], want[k]), "%s: %s differs in %d places" % (what, k, int((u64(got[k]) != u64(want[k])).sum()))


def assert_differs(a, b):
    assert not same_bits(a["g"], b["g"]) and not same_bits(a["j"], b["j"]) and not same_bits(a["s"], b["s"])


@functools.lru_cache(maxsize=None)
def fresh_bits(name, which):
    """What the create path gives for the inputs of live(name) on map A / B (start index (0,0)): the yardstick, computed once."""
    lv = live(name)
    elev, pos = (lv.A, POS_A) if which == "A" else (lv.B, POS_B)
    c = lv.fresh(elev, pos)
    return c, Runner([c.S], [0] * len(lv.xs), lv.xs)()


def set_map(lv, run, how, elev, pos, start, stream=None):
    """Brings lv's handle and / or the batch of `run` to layer elev (start index (0,0)) through a buffer rolled to `start`."""
    buf = rolled(elev, start)
    if how == "sync":
        lv.gm.update(buf, pos, start)
        run.batch.sync_grid_map(lv.gm, stream)
    else:
        d = dev_layer(buf)
        run.batch.update_grid_map_device(lv.gm, d, start, pos, stream)
        return d   # (the launch reads it when it runs: the caller keeps it)


LIVE_STARTS = [(n, s) for n in ("go1_47x37", "go1_5x3") for s in STARTS[CASES[n][1]]] + [("anymal_47x37", (17, 5))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,start", LIVE_STARTS, ids=["%s-start%d_%d" % (n, s[0], s[1]) for n, s in LIVE_STARTS])
def test_updated_batch_equals_a_fresh_batch_on_the_unrolled_map(name, start):
    """3. A batch built on A, evaluated, updated to B (other values, another centre, a rolled buffer) through sync and through
    update_device: g and the Jacobian values of EVAL_BOTH, g of EVAL_VALUES alone and the eval_scores table have the bits of a
    fresh batch built on unrolled B, and meet the oracle on B; updated back to A they have the first evaluation's bits."""
    lv = live(name)
    try:
        run = Runner([lv.case.S], [0] * len(lv.xs), lv.xs)
        first = run()
        (_, bits_a), (case_b, bits_b) = fresh_bits(name, "A"), fresh_bits(name, "B")
        assert_same(first, bits_a, "before any update")
        assert_differs(bits_a, bits_b)
        outside = False
        for how in ("sync", "device"):
            keep = set_map(lv, run, how, lv.B, POS_B, start)
            got = run()
            assert_same(got, bits_b, "%s to B" % how)
            for p, x in enumerate(lv.xs):
                rg, _, _, rj = case_b.P.eval(x)
                b = run.batch
                assert_parity(case_b.S, got["g"][b.g_off[p]:b.g_off[p + 1]], got["j"][b.jac_off[p]:b.jac_off[p + 1]], rg, rj,
                              "%s %s to B x[%d]" % (name, how, p), x=x)
                outside |= bool((np.abs(rg) > 1e37).any())
            keep = set_map(lv, run, how, lv.A, POS_A, start)
            assert_same(run(), first, "%s back to A" % how)
            del keep
        assert outside, "the out-of-range branch (FLT_MAX) must be exercised"
    finally:
        lv.gm.update(lv.A, POS_A)   # live(name) is shared: the handle goes back to A whatever happened


@pytest.mark.gpu
def test_only_the_structures_of_the_updated_map_follow():
    """4. Two structures share map M, one is on map N, problems [0, 1, 2, 1].  After M alone is updated, problem 2 has exactly its
    earlier bits and the others those of a fresh batch on the new M; an update that names a handle the batch does not hold is
    refused and changes nothing."""
    M0, M1, N = layer(BIG, 21), layer(BIG, 22), layer(BIG, 23)
    order = [0, 1, 2, 1]

    def build(m_layer, m_pos):
        c1 = Case("anymal", "grid_map", ta.gait_combo(4, 0, 1.6), grid=(m_layer, RES[BIG], m_pos))
        c2 = Case("anymal", "grid_map", ta.gait_combo(4, 2, 2.2), grid=c1.grid)
        c3 = Case("anymal", "grid_map", ta.gait_combo(4, 1, 2.0), grid=(N, RES[BIG], POS_A))
        return [c1, c2, c3]

    cases = build(M0, POS_A)
    xs = [cases[s].x_perturbed(7 + i, 1.5) for i, s in enumerate(order)]
    run = Runner([c.S for c in cases], order, xs)
    before = run()
    stranger = ta.GridMap(M1, RES[BIG], POS_B)
    for call in (lambda: run.batch.sync_grid_map(stranger), lambda: run.batch.update_grid_map_device(stranger, dev_layer(M1), (0, 0), POS_B)):
        with pytest.raises(ta.TowrError, match=r"error -1: g is not a map of this batch"):
            call()
    assert_same(run(), before, "after the refused updates")
    start = (46, 36)
    cases[0].grid.update(rolled(M1, start), POS_B, start)
    run.batch.sync_grid_map(cases[0].grid)
    after = run()
    ref_cases = build(M1, POS_B)
    ref = Runner([c.S for c in ref_cases], order, xs)()
    assert_same(after, ref, "M updated")
    b = run.batch
    for k, off in (("g", b.g_off), ("gv", b.g_off), ("j", b.jac_off)):
        assert same_bits(after[k][off[2]:off[3]], before[k][off[2]:off[3]]), "problem 2 is on map N"
        for p in (0, 1, 3):
            assert not same_bits(after[k][off[p]:off[p + 1]], before[k][off[p]:off[p + 1]]), "problem %d is on map M" % p
    assert same_bits(after["s"][32:48], before["s"][32:48])
    for p, s in enumerate(order):
        rg, _, _, rj = ref_cases[s].P.eval(xs[p])
        assert_parity(ref_cases[s].S, after["g"][b.g_off[p]:b.g_off[p + 1]], after["j"][b.jac_off[p]:b.jac_off[p + 1]], rg, rj, "problem %d" % p)


@pytest.mark.gpu
def test_batch_update_refuses_bad_arguments_before_it_touches_the_device():
    """Every bad argument of the two batch calls is TWR_ERR_INVALID with a message that names it; the batch computes what it did."""
    L = ta.lib()
    lv = live("go1_5x3")
    run = Runner([lv.case.S], [0] * len(lv.xs), lv.xs)
    first = run()
    d = dev_layer(lv.B)
    p, b, g = d.data_ptr(), run.batch._h, lv.gm._h
    csv = ta.TerrainGrid(np.zeros((4, 5)))
    nan, inf = float("nan"), float("inf")
    for args, name in (((None, g, None), "b"), ((b, None, None), "g"), ((b, csv._h, None), "g")):
        assert L.twr_batch_grid_map_sync(*args) == -1
        assert name in L.twr_last_error().decode().split(), L.twr_last_error()
    for args, name in (((None, g, p, 0, 0, 0.0, 0.0), "b"), ((b, None, p, 0, 0, 0.0, 0.0), "g"), ((b, csv._h, p, 0, 0, 0.0, 0.0), "g"),
                       ((b, g, None, 0, 0, 0.0, 0.0), "d_elevation"), ((b, g, p + 2, 0, 0, 0.0, 0.0), "d_elevation"),
                       ((b, g, p, -1, 0, 0.0, 0.0), "start_x"), ((b, g, p, SMALL[0], 0, 0.0, 0.0), "start_x"),
                       ((b, g, p, 0, -1, 0.0, 0.0), "start_y"), ((b, g, p, 0, SMALL[1], 0.0, 0.0), "start_y"),
                       ((b, g, p, 0, 0, nan, 0.0), "pos_x"), ((b, g, p, 0, 0, 0.0, -inf), "pos_y")):
        assert L.twr_batch_grid_map_update_device(*args, None) == -1, args[3:]
        assert name in L.twr_last_error().decode().split(), (args[3:], L.twr_last_error())
    torch, _ = torch_ctx()
    with pytest.raises(ta.TowrError, match="column-major"):
        run.batch.update_grid_map_device(lv.gm, torch.zeros(SMALL, dtype=torch.float32, device=d.device), (0, 0), POS_A)   # row-major
    with pytest.raises(ta.TowrError, match="column-major"):
        run.batch.update_grid_map_device(lv.gm, d.double(), (0, 0), POS_A)
    assert_same(run(), first, "after the refused updates")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["device", "sync"])
def test_updates_and_evaluations_are_ordered_on_one_stream(how):
    """5. On one non-default stream: update to B, evaluate, update to A, evaluate, without a host synchronisation in between.  Each
    evaluation sees its own map."""
    torch, _ = torch_ctx()
    name, start = "go1_47x37", (17, 5)
    lv = live(name)
    try:
        run = Runner([lv.case.S], [0] * len(lv.xs), lv.xs)
        run()                                     # (module load and first-use allocations stay out of the ordered part)
        second = run.new_out()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        keep = [set_map(lv, run, how, lv.B, POS_B, start, s.cuda_stream)]
        run.run(s.cuda_stream)
        keep.append(set_map(lv, run, how, lv.A, POS_A, start, s.cuda_stream))
        run.run(s.cuda_stream, second)
        s.synchronize()
        assert_same(run.read(), fresh_bits(name, "B")[1], "the evaluation behind the update to B")
        assert_same(run.read(second), fresh_bits(name, "A")[1], "the evaluation behind the update to A")
    finally:
        lv.gm.update(lv.A, POS_A)


@pytest.mark.gpu
def test_a_captured_evaluation_sees_the_updated_map_and_an_update_can_be_captured():
    """6. (a) An evaluation captured on A, an update outside the graph, a replay: the bits of B (the map's address is stable).
    (b) update_device and the evaluation captured as one linear graph, the caller's layer changed, a replay: the bits of a fresh
    batch on the changed layer."""
    from tests.jac_device import capture

    torch, _ = torch_ctx()
    name, start = "go1_47x37", (46, 0)
    lv = live(name)
    try:
        run = Runner([lv.case.S], [0] * len(lv.xs), lv.xs)
        graph = capture(run.run)
        graph.replay()
        assert_same(run.read(), fresh_bits(name, "A")[1], "replay on A")
        for how in ("sync", "device"):
            keep = set_map(lv, run, how, lv.B, POS_B, start)
            graph.replay()
            assert_same(run.read(), fresh_bits(name, "B")[1], "replay after %s to B" % how)
            keep = set_map(lv, run, how, lv.A, POS_A, start)
            graph.replay()
            assert_same(run.read(), fresh_bits(name, "A")[1], "replay after %s back to A" % how)
            del keep
        # (b) start index and centre are arguments of the captured launch; the layer is read at every replay
        d = dev_layer(rolled(lv.A, start))

        def step(stream):
            run.batch.update_grid_map_device(lv.gm, d, start, POS_B, stream)
            run.run(stream)

        both = capture(step)
        d.copy_(dev_layer(rolled(lv.B, start)))
        assert d.t().is_contiguous()
        both.replay()
        assert_same(run.read(), fresh_bits(name, "B")[1], "replay of update + evaluation on the changed layer")
    finally:
        lv.gm.update(lv.A, POS_A)


@pytest.mark.gpu
def test_lm_driver_bound_to_an_updated_batch_steps_like_one_on_a_fresh_batch():
    """7. The LM driver is bound to its batch: after the batch's map went from A to B, a start and one twr_jac_lm_step give the x and
    the state records of a driver on a fresh batch built on B, bit for bit (the hopper of tests/jac_ref.py, on the `Grid` terrain)."""
    from tests import jac_ref
    from tests.jac_device import JacBatch, dev, nan

    lm_box_cpu = jac_ref._lm_box_cpu()
    torch, _ = torch_ctx()
    st = torch.cuda.current_stream().cuda_stream
    A, B, start = layer(BIG, 31), layer(BIG, 32), (17, 5)

    def hopper(elev, pos):
        return Case("monoped", "grid_map", hopper_schedule(), grid=(elev, RES[BIG], pos), constraint_sets=ta.SETS_ALL)

    fresh = hopper(B, POS_B)
    lo, up = lm_box_cpu.case_bounds(fresh)
    x0 = np.concatenate([fresh.x_perturbed(seed) for seed in (0, 1)])
    lo, up = np.tile(lo, 2), np.tile(up, 2)

    def one_step(case, between=None):
        jb = JacBatch([case.S], [0, 0], make=("batch", "ops", "lsq"))
        lm = ta.JacLm(jb.batch, jb.lsq)
        g, jac, rec = nan(jb.G), nan(jb.J), nan(ta.JacLm.REC * jb.P)
        x, d_lo, d_up = dev(x0), dev(lo), dev(up)
        if between:   # the driver has already run on the old map
            x_old = dev(x0)
            lm.start_device(x_old.data_ptr(), d_lo.data_ptr(), d_up.data_ptr(), g.data_ptr(), jac.data_ptr(), st)
            lm.step_device(st)
            between(jb.batch)
        lm.start_device(x.data_ptr(), d_lo.data_ptr(), d_up.data_ptr(), g.data_ptr(), jac.data_ptr(), st)
        lm.step_device(st)
        lm.state_device(rec.data_ptr(), st)
        torch.cuda.synchronize()
        return x.cpu().numpy(), rec.cpu().numpy(), g.cpu().numpy(), jac.cpu().numpy()

    want = one_step(fresh)
    live_case = hopper(A, POS_A)

    def to_b(batch):
        live_case.grid.update(rolled(B, start), POS_B, start)
        batch.sync_grid_map(live_case.grid, st)

    got = one_step(live_case, to_b)
    stale = one_step(hopper(A, POS_A))
    for a, b, c, what in zip(got, want, stale, ("x", "state records", "g", "Jacobian values")):
        assert same_bits(a, b), what
    assert not same_bits(stale[0], want[0]), "the step must depend on the map"
    assert np.isfinite(want[0]).all() and not same_bits(want[0], x0), "the step must move x"
