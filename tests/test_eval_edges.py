"""Breakpoint footholds through every kernel that evaluates a terrain, against the oracle.

The other tests reach kernels/terrain.h with random footholds, which never land on a breakpoint.  Here small problems, one per
terrain (Block, Stairs, Gap, Slope, Chimney, ChimneyLR, a CSV map, a `Grid` map), run at Case.x_edges: x_perturbed with the x
and y of every ee-motion node on the breakpoints of the problem's own terrain -- a quarter on a breakpoint, a quarter on a
neighbouring double, a quarter on a slope-band threshold in either rounding (CSV), a cell centre (`Grid`) or two doubles from a
breakpoint, the rest inside a piece.  The rows of EDGE_MATRIX (the format of tests/eval_matrix.py) are the smallest batches for
which the planner picks each of node_kernel, node_kernel2, node_chunk_kernel<G | J | GJ>, the node role of eval_fused_kernel,
eval_values_kernel and eval_scores_kernel; one structure has more than 64 terrain rows and more than 64 force nodes, so the
last, partial chunk of 64 of node_body holds breakpoint footholds too.

Per row, for EVAL_BOTH, EVAL_VALUES and EVAL_JACOBIAN, without and with per-kernel events: parity with the oracle at the bar of
tests/common.py; on CSV and `Grid` the terrain rows (g = z - h and the Jacobian values -hx, -hy, 1) bit-equal to the oracle's;
the same bits from the fused and the separate launches; every problem bit for bit its one-problem batch; scores and arg-min
against numpy on the oracle's g."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import towr_amd as ta
from tests import eval_matrix
from tests import terrain_points as tp
from tests.common import Case, assert_parity, k_params
from tests.test_eval_scores import _oracle_scores

EDGE_MATRIX = """
struct e_block  K=16 terrain=block sets=27
struct e_stairs K=16 terrain=stairs sets=63 combo=0 T=2.4 swing=1.1
struct e_gap    K=24 terrain=gap sets=127 combo=2 T=1.8 swing=0.9
struct e_slope  K=16 terrain=slope sets=27
struct e_chim   K=16 terrain=chimney sets=63
struct e_chlr   K=16 terrain=chimney_lr sets=27
struct e_csv    K=16 terrain=csv sets=63
struct e_grid   K=16 terrain=grid_map sets=27
struct e_long   K=12 terrain=csv sets=27 combo=0 T=2.4 pps=4 ppf=5
struct c_csv    K=12 terrain=csv sets=63
struct c_grid   K=12 terrain=grid_map sets=63
struct c_gap    K=12 terrain=gap sets=63 combo=2 T=1.8
row edge_27    kind=cheap structs=e_block,e_slope,e_chlr,e_grid order=0,1,2,3,3 val_off=eval_values_kernel<3> val_on=eval_values_kernel<3>;node_kernel2 jac_off=eval_fused_kernel<34,xc4,*> jac_on=node_kernel2 scores=eval_scores_kernel<3>;score_fold_kernel
row edge_63    kind=cheap structs=e_stairs,e_chim,e_csv order=0,1,2,2 val_off=eval_values_kernel<3> val_on=eval_values_kernel<3>;node_kernel jac_off=eval_fused_kernel<34,xc4,*> jac_on=node_kernel scores=eval_scores_kernel<3>;score_fold_kernel
row edge_127   kind=cheap structs=e_gap,e_csv order=0,1,0 val_off=node_kernel val_on=node_kernel jac_off=node_kernel jac_on=node_kernel scores=node_kernel;score_kernel
row edge_long  kind=cheap structs=e_long order=0,0 val_off=eval_values_kernel<5> val_on=eval_values_kernel<5>;node_kernel2 jac_off=eval_fused_kernel<34,xc4,*> jac_on=node_kernel2 scores=eval_scores_kernel<5>;score_fold_kernel
row edge_chunk kind=chunk structs=c_csv,c_grid,c_gap order=cycle:2051 val_off=eval_values_kernel<3>;node_chunk_kernel<*> val_on=eval_values_kernel<3>;node_chunk_kernel<*> jac_off=eval_fused_kernel<34,xc4,*> jac_on=node_chunk_kernel<*> scores=eval_scores_kernel<3>;score_fold_kernel
"""
STRUCT_FIELDS, ROWS, _ = eval_matrix.parse(EDGE_MATRIX)
POOL = 2                      # distinct points per structure
LONG = "e_long"
GRIDDED = ("csv", "grid_map")
MIN_ON_BREAKPOINT = 0.2       # of the terrain rows of a batch
MIN_STEEP = 5                 # terrain rows of a batch with a non-zero slope-band slope (CSV) or an FLT_MAX sample (`Grid`)
COMPARED = 18                 # problems of the chunk row held to the oracle (all of them to their one-problem batch)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The Case of a `struct` line of EDGE_MATRIX: the formulas of eval_matrix.make_case, plus the CSV and `Grid` maps of
    tests/terrain_points.py"""
    f = STRUCT_FIELDS[name]
    terrain = f["terrain"]
    T, K = float(f.get("T", 2.0)), int(f.get("K", 40))
    model = ta.model_preset("anymal", terrain)
    grid = None
    if terrain == "csv":
        grid = tp.CSV_HEIGHTS
    if terrain == "grid_map":
        m = tp.GRID_MAPS[0]
        grid = (tp.grid_elevation(m), m["res"], m["pos"])
    return Case("anymal", terrain, ta.gait_combo(model.n_ee, int(f.get("combo", 1)), T, float(f.get("swing", 1.0))), grid=grid,
                duration_base_poly=0.1, polys_per_swing=int(f.get("pps", 2)), polys_per_stance_force=int(f.get("ppf", 3)),
                constraint_sets=int(f.get("sets", 27)), dt_base_motion=0.025, base_z_init=-model.nominal_stance[0][2], **k_params(T, K))


@functools.lru_cache(maxsize=None)
def _x(name, i):
    x = make_case(name).x_edges(i)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def _ref(name, i):
    rg, _, _, rj = make_case(name).P.eval(_x(name, i))
    return rg, rj


def _keys(row):
    """(structure name, point) of every problem of a row: the points of a structure cycle through its pool"""
    names = [row["structs"][s] for s in row["order"]]
    seen, key = {}, []
    for nm in names:
        key.append((nm, seen.get(nm, 0) % POOL))
        seen[nm] = seen.get(nm, 0) + 1
    return key


def _maps(case):
    grid_map = (case.grid.elevation, case.grid.resolution, case.grid.position) if case.terrain == "grid_map" else None
    return (case.grid.heights if case.terrain == "csv" else None), grid_map


def _rows_of(S, prefix):
    return np.concatenate([np.arange(cs["offset"], cs["offset"] + cs["size"]) for cs in S.con_sets if cs["name"].startswith(prefix)] or
                          [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def _terrain_row_footholds(case, x):
    """(x, y) of the foothold of every terrain row, in row order"""
    S = case.S
    rows = _rows_of(S, "terrain-")
    cols = np.array([S.col_idx[S.row_ptr[r]:S.row_ptr[r] + 2] for r in rows])
    return x[cols]


def _steep(case, xy):
    """per foothold: a non-zero slope of a CSV step, or an FLT_MAX sample of a `Grid` map (the height itself or a slope)"""
    out = np.zeros(len(xy), dtype=bool)
    for k, (px, py) in enumerate(xy):
        h, hx, hy = case.P.terrain_probe(px, py)
        out[k] = (hx != 0 or hy != 0) if case.terrain == "csv" else (h == tp.FLT_MAX or abs(hx) > 1e38 or abs(hy) > 1e38)
    return out


# ------------------------------------------------------------------ CPU tier
def test_rows_reach_every_kernel_that_evaluates_a_terrain():
    """(CPU tier) the product's planner, on the host, plans for every row what the row claims; between them the rows claim
    every kernel through which a terrain is evaluated"""
    from tests.host_build import plan_driver
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "edges.txt")
        with open(path, "w") as f:
            f.write(EDGE_MATRIX)
        r = subprocess.run([plan_driver("eval_matrix_driver"), path, "--partial"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "%d rows" % len(ROWS) in r.stdout and ", 0 failures" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr
    claimed = set()
    for row in ROWS:
        for flags in (ta.EVAL_VALUES, ta.EVAL_JACOBIAN, ta.EVAL_BOTH):
            for events in (False, True):
                claimed |= set(eval_matrix.claims_of(row, flags, events))
        claimed |= set(row["claims"]["scores"])
    for kernel in ("node_kernel", "node_kernel2", "node_chunk_kernel<G>", "node_chunk_kernel<J>", "node_chunk_kernel<GJ>"):
        assert kernel in claimed, "no row claims %s" % kernel
    for family in ("eval_fused_kernel<", "eval_values_kernel<", "eval_scores_kernel<"):
        assert any(c.startswith(family) for c in claimed), "no row claims %s...>" % family


def test_cases_are_small_and_one_per_terrain():
    terrains, masks = set(), set()
    for name, f in STRUCT_FIELDS.items():
        S = make_case(name).S
        assert int(f["K"]) <= 24 and ta.model_preset("anymal", f["terrain"]).n_ee == 4 and S.n < 1200, name
        terrains.add(f["terrain"]), masks.add(int(f["sets"]))
    assert terrains == {"block", "stairs", "gap", "slope", "chimney", "chimney_lr", "csv", "grid_map"} and masks == {27, 63, 127}
    assert [n for n, f in STRUCT_FIELDS.items() if int(f["sets"]) == 127] == ["e_gap"]
    for row in ROWS:
        assert row["kind"] == "chunk" or len(row["order"]) <= 5
        assert any(STRUCT_FIELDS[s]["terrain"] in GRIDDED for s in row["structs"]), row["name"]


def test_long_structure_has_breakpoint_footholds_in_its_last_partial_chunk():
    """more than 64 terrain rows and more than 64 force nodes, neither a multiple of 64, and rows beyond the 64th whose foothold
    sits on a breakpoint: the rows[min(r0 + lane, nr - 1)] tail of node_body"""
    case = make_case(LONG)
    S = case.S
    heights, grid_map = _maps(case)
    t_rows, f_rows = _rows_of(S, "terrain-"), _rows_of(S, "force-")
    assert len(f_rows) % 5 == 0
    n_t, n_f = len(t_rows), len(f_rows) // 5
    assert 64 < n_t < 128 and 64 < n_f < 128 and n_t % 64 and n_f % 64, (n_t, n_f)
    for i in range(POOL):
        x = _x(LONG, i)
        xy = _terrain_row_footholds(case, x)
        assert tp.on_breakpoint("csv", xy[64:], heights, grid_map).sum() >= 5 and _steep(case, xy[64:]).sum() >= 3
        nodes = f_rows[::5][64:]                 # the foothold of a force node: the first two columns of its rows
        fxy = x[np.array([S.col_idx[S.row_ptr[r]:S.row_ptr[r] + 2] for r in nodes])]
        # (the last force nodes belong to the last stance phases of the last foot: three footholds between them)
        assert (tp.on_breakpoint("csv", fxy, heights, grid_map) | _steep(case, fxy)).sum() >= 5, i


def test_edge_points_sit_on_the_breakpoints_of_their_own_terrain():
    """(CPU tier) only footholds change; the four kinds come in quarters; in every batch at least 20 % of the terrain rows sit
    on a breakpoint or a neighbouring double and at least five carry a CSV step slope or an FLT_MAX sample"""
    for name in STRUCT_FIELDS:
        case = make_case(name)
        heights, grid_map = _maps(case)
        idx = case.footholds()
        for i in range(POOL):
            x, base = _x(name, i), case.x_perturbed(i)
            rest = np.ones(x.size, dtype=bool)
            rest[idx.ravel()] = False
            assert np.array_equal(x[rest], base[rest]) and np.isfinite(x).all(), name
            on = tp.on_breakpoint(case.terrain, x[idx], heights, grid_map)
            assert 0.4 <= on.mean() <= 0.8, (name, i, on.mean())          # kinds 0 and 1 (a chimney's y adds some)
            lines = tp.breakpoint_lines(case.terrain, heights, grid_map)
            exact = np.isin(x[idx][:, 0], lines[0]) | (np.isin(x[idx][:, 1], lines[1]) if len(lines[1]) else False)
            assert 0.2 <= exact.mean() and 0.2 <= (on & ~exact).mean(), (name, i, exact.mean(), (on & ~exact).mean())
    for row in ROWS:
        keys = _keys(row)
        if row["kind"] == "chunk":
            keys = keys[:len(row["structs"]) * POOL]        # the batch tiles these
        on, steep, total = 0, 0, 0
        for nm, i in keys:
            case = make_case(nm)
            heights, grid_map = _maps(case)
            xy = _terrain_row_footholds(case, _x(nm, i))
            on += tp.on_breakpoint(case.terrain, xy, heights, grid_map).sum()
            total += len(xy)
            if case.terrain in GRIDDED:
                steep += _steep(case, xy).sum()
        assert on >= MIN_ON_BREAKPOINT * total and steep >= MIN_STEEP, (row["name"], on, total, steep)


def test_oracle_is_finite_at_the_edge_points():
    for name in STRUCT_FIELDS:
        for i in range(POOL):
            rg, rj = _ref(name, i)
            assert np.isfinite(rg).all() and np.isfinite(rj).all(), name


# ------------------------------------------------------------------ GPU tier
def _terrain_entries(S):
    """(rows of the terrain sets, positions of their Jacobian values)"""
    rows = _rows_of(S, "terrain-")
    nz = np.concatenate([np.arange(S.row_ptr[r], S.row_ptr[r + 1]) for r in rows])
    return rows, nz


@functools.lru_cache(maxsize=None)
def _solo(name, i):
    """EVAL_BOTH of one problem alone in a batch, as device tensors"""
    import torch
    from tests.test_eval_matrix import _run
    batch = ta.Batch([make_case(name).S], [0], device=0)
    g, j = _run(batch, torch.from_numpy(np.array(_x(name, i))).cuda(), ta.EVAL_BOTH, False, "%s alone" % name)
    return g.clone(), j.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_row_at_breakpoint_footholds(row):
    import torch
    from tests.test_eval_matrix import _run, _same_bits
    key = _keys(row)
    n = len(key)
    cases = [make_case(nm) for nm in row["structs"]]
    batch = ta.Batch([c.S for c in cases], row["order"], device=0)
    d_x = torch.from_numpy(np.concatenate([_x(*k) for k in key])).cuda()
    compared = list(range(n)) if n <= COMPARED else sorted(set(list(range(COMPARED - 6)) + list(range(n - 6, n))))
    for flags in (ta.EVAL_BOTH, ta.EVAL_VALUES, ta.EVAL_JACOBIAN):
        out = {}
        for events in (False, True):
            what = "%s flags %d events %d" % (row["name"], flags, events)
            planned = {s["instantiation"] for s in batch.eval_plan(flags, events)}
            missing = set(eval_matrix.claims_of(row, flags, events)) - planned
            assert not missing, "%s: the device plans %s, the row claims %s as well" % (what, sorted(planned), sorted(missing))
            out[events] = _run(batch, d_x, flags, events, what)
            for p in compared:
                case = cases[row["order"][p]]
                S = case.S
                rg, rj = _ref(*key[p])
                g = out[events][0][batch.g_off[p]:batch.g_off[p + 1]].cpu().numpy() if flags & ta.EVAL_VALUES else rg
                j = out[events][1][batch.jac_off[p]:batch.jac_off[p + 1]].cpu().numpy() if flags & ta.EVAL_JACOBIAN else rj
                where = "%s problem %d (%s, point %d)" % ((what, p) + key[p])
                assert_parity(S, g, j, rg, rj, where, x=_x(*key[p]))
                if case.terrain in GRIDDED:
                    rows, nz = _terrain_entries(S)
                    bad = np.nonzero(g[rows].view(np.int64) != rg[rows].view(np.int64))[0]
                    assert bad.size == 0, "%s: %d terrain values differ in their bits from the oracle's, first row %d: %r vs %r" % (
                        where, bad.size, rows[bad[0]], g[rows[bad[0]]], rg[rows[bad[0]]])
                    bad = np.nonzero(j[nz].view(np.int64) != rj[nz].view(np.int64))[0]
                    assert bad.size == 0, "%s: %d terrain Jacobian values differ in their bits from the oracle's, first %d: %r vs %r" % (
                        where, bad.size, nz[bad[0]], j[nz[bad[0]]], rj[nz[bad[0]]])
            if flags == ta.EVAL_BOTH and not events:   # every problem: the same bits as alone in a batch
                for p in range(n):
                    sg, sj = _solo(*key[p])
                    assert _same_bits(out[events][0][batch.g_off[p]:batch.g_off[p + 1]], sg), "%s problem %d: g differs from the one-problem batch" % (what, p)
                    assert _same_bits(out[events][1][batch.jac_off[p]:batch.jac_off[p + 1]], sj), "%s problem %d: jac differs from the one-problem batch" % (what, p)
        if flags & ta.EVAL_VALUES:
            assert _same_bits(out[False][0], out[True][0]), "%s flags %d: g differs between the fused and the separate launches" % (row["name"], flags)
        if flags & ta.EVAL_JACOBIAN:
            assert _same_bits(out[False][1], out[True][1]), "%s flags %d: jac differs between the fused and the separate launches" % (row["name"], flags)
        del out
    _check_scores(row, batch, cases, key, d_x)


def _check_scores(row, batch, cases, key, d_x):
    """eval_scores_device against numpy on the oracle's g (tests/test_eval_scores.py _oracle_scores), and the arg-min of
    eval_score_best_device against towr_amd.dist.best_candidate, as tests/test_eval_matrix.py does"""
    import torch
    from tests.test_eval_matrix import _Out
    from towr_amd.dist import best_candidate
    n, st = batch.n_problems, torch.cuda.current_stream().cuda_stream
    for request in ("scores", "score_best"):
        planned = {s["instantiation"] for s in batch.eval_plan(request=request)}
        claimed = set(row["claims"]["scores"]) | ({"best_kernel"} if request == "score_best" else set())
        assert claimed <= planned, "%s %s: the device plans %s" % (row["name"], request, sorted(planned))
    g = _Out(int(batch.g_off[-1]))
    scores = torch.full((n, 16), -1.0, dtype=torch.float64, device="cuda")
    batch.eval_scores_device(d_x.data_ptr(), scores.data_ptr(), d_g=0 if batch.scores_without_g else g.ptr(), stream=st)
    torch.cuda.synchronize()
    assert g.guards_intact() and (g.untouched() if batch.scores_without_g else g.fully_written())
    table = scores.cpu().numpy()
    want = {k: _oracle_scores(make_case(k[0]), _x(*k)) for k in set(key)}
    for p in range(n):
        got = table[p].reshape(8, 2)
        assert not np.isnan(got).any() and not np.isnan(want[key[p]]).any(), (row["name"], p)
        assert np.all(np.abs(got - want[key[p]]) <= 1e-9 * np.abs(want[key[p]]) + 1e-9), (row["name"], p, key[p], got, want[key[p]])
    best = torch.zeros(2, dtype=torch.float64, device="cuda")
    again = torch.full((n, 16), -1.0, dtype=torch.float64, device="cuda")
    for fam, off in (((0, 1, 3, 4), 0), ((1, 4), 1000)):
        batch.eval_score_best_device(d_x.data_ptr(), again.data_ptr(), best.data_ptr(), families=fam, index_offset=off,
                                     d_g=0 if batch.scores_without_g else g.ptr(), stream=st)
        torch.cuda.synchronize()
        assert torch.equal(again, scores), "%s: the two scoring entry points give different tables" % row["name"]
        idx, total = best_candidate(again, families=fam)
        assert (int(best[0]), float(best[1])) == (off + idx, total), (row["name"], fam, best.cpu(), idx, total)
