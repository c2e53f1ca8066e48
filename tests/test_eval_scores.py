"""twr_batch_eval_scores / twr_batch_eval_score_best: the planner's score table straight from x, without g where every problem
takes the values-only path (fixed timings, at most 2046 variables), else through g (values evaluation + score_kernel)."""
import numpy as np
import pytest

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def _scores(batch, xs, d_g=None):
    """(eval_scores table, eval + score_kernel table, the g of that evaluation) for the inputs xs."""
    torch, dev, st = _torch()
    n = batch.n_problems
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    got = torch.full((n, 16), -1.0, dtype=torch.float64, device=dev)
    batch.eval_scores_device(x.data_ptr(), got.data_ptr(), d_g=0 if d_g is None else d_g.data_ptr(), stream=st)
    g = torch.empty(max(1, int(batch.g_off[-1])), dtype=torch.float64, device=dev)
    ref = torch.full((n, 16), -1.0, dtype=torch.float64, device=dev)
    batch.eval_device(x.data_ptr(), g.data_ptr(), 0, ta.EVAL_VALUES, st)
    batch.score_device(g.data_ptr(), ref.data_ptr(), st)
    torch.cuda.synchronize()
    return got.cpu().numpy(), ref.cpu().numpy(), g.cpu().numpy()


def _assert_matches_score_kernel(got, ref, what=""):
    """inf-norms bit for bit, 1-norms to 1e-12 relative, the same NaN pattern."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[:, 0::2], ref[:, 0::2], equal_nan=True), what
    a, b = got[:, 1::2], ref[:, 1::2]
    ok = ~np.isnan(b)
    assert np.all(np.abs(a[ok] - b[ok]) <= 1e-12 * np.abs(b[ok])), (what, np.abs(a[ok] - b[ok]).max())


def _oracle_scores(case, x):
    rg = case.P.values(x)
    lo, up = case.P.bounds()
    viol = np.maximum(np.maximum(lo - rg, rg - up), 0.0)
    viol[np.isnan(rg)] = np.nan
    want = np.zeros((8, 2))
    for cs in case.S.con_sets:
        fam = [i for i, f in enumerate(ta.FAMILIES) if cs["name"].startswith(f)][0]
        v = viol[cs["offset"]:cs["offset"] + cs["size"]]
        want[fam, 0] = np.nan if (np.isnan(v).any() or np.isnan(want[fam, 0])) else max(want[fam, 0], v.max(initial=0.0))
        want[fam, 1] += v.sum()
    return want


def _ragged_fixed():
    cases = [Case("anymal", "stairs", ta.gait_combo(4, 1, 2.0), constraint_sets=63),
             Case("anymal", "gap", ta.gait_combo(4, 0, 2.4, 0.9), constraint_sets=191, base_z_init=0.42),
             Case("go1", "flat", ta.gait_combo(4, 4, 1.8), constraint_sets=63),
             Case("anymal", "block", ta.gait_combo(4, 3, 2.2), constraint_sets=27)]
    order = [0, 1, 2, 3, 2, 0, 1]
    xs = [cases[s].x_perturbed(i, 1.5) if i % 2 else cases[s].x_wild(i) for i, s in enumerate(order)]
    return cases, order, xs


def test_oracle_parity_without_g():
    cases, order, xs = _ragged_fixed()
    batch = ta.Batch([c.S for c in cases], order, device=0)
    assert batch.scores_without_g
    clean = [x.copy() for x in xs]
    xs[4][cases[2].S.var_sets[0]["offset"] + 2] = float("nan")   # one problem with a poisoned base height
    got, ref, _ = _scores(batch, xs)
    for p, s in enumerate(order):
        want = _oracle_scores(cases[s], xs[p])
        g = got[p].reshape(8, 2)
        assert np.array_equal(np.isnan(g), np.isnan(want)), (p, g, want)
        ok = ~np.isnan(want)
        assert np.all(np.abs(g[ok] - want[ok]) <= 1e-9 * np.abs(want[ok]) + 1e-9), (p, g, want)
    assert np.isnan(got[4]).any() and not np.isnan(np.delete(got, 4, axis=0)).any()
    _assert_matches_score_kernel(got, ref)
    got_clean, _, _ = _scores(batch, clean)
    others = [p for p in range(len(order)) if p != 4]
    assert np.array_equal(got[others], got_clean[others])


@pytest.mark.parametrize("name", list(baseline_cases()))
def test_matches_score_kernel_baseline(name):
    case = baseline_cases()[name]()
    batch = ta.Batch([case.S], [0, 0, 0], device=0)
    assert batch.scores_without_g
    got, ref, _ = _scores(batch, [case.x_perturbed(i) if i else case.x_wild(7) for i in range(3)])
    _assert_matches_score_kernel(got, ref, name)


def _c5_sweep():
    from towr_amd import sweep

    m5 = ta.model_preset("anymal", "stairs")
    cands = sweep.enumerate_candidates(1024)
    return m5, sweep.candidate_structures(m5, cands, threads=8)


def _x_of(S, model, seed):
    ee = [[model.nominal_stance[e][0], model.nominal_stance[e][1], 0.0] for e in range(model.n_ee)]
    z = -model.nominal_stance[0][2]
    x0 = S.initial_guess([0, 0, z], [0, 0, 0], [1.0, 0, z], [0, 0, 0], ee)
    return x0 + 0.05 * np.random.default_rng(seed).normal(size=S.n)


def test_matches_score_kernel_c5_sweep_and_determinism():
    torch, dev, st = _torch()
    m5, structs = _c5_sweep()
    n = len(structs)
    assert n == 1024
    batch = ta.Batch(structs, list(range(n)), device=0)
    assert batch.scores_without_g
    xs = [_x_of(S, m5, i) for i, S in enumerate(structs)]
    sentinel = torch.full((int(batch.g_off[-1]),), 1234.5, dtype=torch.float64, device=dev)
    got, ref, _ = _scores(batch, xs, d_g=sentinel)
    _assert_matches_score_kernel(got, ref, "C5")
    assert bool((sentinel == 1234.5).all())   # d_g given on the fused path: untouched
    # repeated calls: bit for bit
    again, _, _ = _scores(batch, xs)
    assert np.array_equal(got, again, equal_nan=True)
    # the same candidates at permuted positions of one batch
    perm = np.random.default_rng(3).permutation(n)[:300]
    b2 = ta.Batch(structs, [int(i) for i in perm], device=0)
    got2, _, _ = _scores(b2, [xs[i] for i in perm])
    assert np.array_equal(got2, got[perm], equal_nan=True)


def test_matches_score_kernel_c3_8192():
    """8192 problems of towr's default list: the values path hands the node sets to node_chunk_kernel; the scoring launch
    keeps them."""
    case = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), constraint_sets=63, **k_params(2.0, 200))
    n = 8192
    batch = ta.Batch([case.S], [0] * n, device=0)
    assert batch.scores_without_g
    base = case.x_perturbed(1)
    rng = np.random.default_rng(5)
    xs = [base + 0.01 * rng.normal(size=case.S.n) for _ in range(n)]
    got, ref, _ = _scores(batch, xs)
    _assert_matches_score_kernel(got, ref, "C3 x 8192")
    # the position of a problem does not change its bits
    b1 = ta.Batch([case.S], [0] * 3, device=0)
    one, _, _ = _scores(b1, [xs[8000], xs[17], xs[4095]])
    assert np.array_equal(one, got[[8000, 17, 4095]], equal_nan=True)


def _fallback_batches():
    opt = Case("anymal", "gap", ta.gait_combo(4, 0, 2.4, 0.9), constraint_sets=255, base_z_init=0.42)
    fixed = Case("anymal", "stairs", ta.gait_combo(4, 1, 2.0), constraint_sets=63)
    big = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200), duration_base_poly=0.01)   # 2800 variables
    return [("optimised timings", [opt], [0, 0]), ("mixed", [fixed, opt], [0, 1, 0]), ("over 2046 variables", [big, fixed], [0, 1])]


def test_fallback_through_g():
    torch, dev, st = _torch()
    for what, cases, order in _fallback_batches():
        if what == "over 2046 variables":
            assert cases[0].S.n > 2046, cases[0].S.n
        batch = ta.Batch([c.S for c in cases], order, device=0)
        assert not batch.scores_without_g, what
        xs = [cases[s].x_perturbed(i) for i, s in enumerate(order)]
        g = torch.empty(int(batch.g_off[-1]), dtype=torch.float64, device=dev)
        got, ref, g_ref = _scores(batch, xs, d_g=g)
        assert np.array_equal(got, ref, equal_nan=True), what
        assert np.array_equal(g.cpu().numpy(), g_ref, equal_nan=True), what
        x = torch.from_numpy(np.concatenate(xs)).to(dev)
        s = torch.empty((len(order), 16), dtype=torch.float64, device=dev)
        with pytest.raises(ta.TowrError):
            batch.eval_scores_device(x.data_ptr(), s.data_ptr(), stream=st)
        best = torch.zeros(2, dtype=torch.float64, device=dev)
        with pytest.raises(ta.TowrError):
            batch.eval_score_best_device(x.data_ptr(), s.data_ptr(), best.data_ptr(), stream=st)


def test_eval_score_best():
    from towr_amd.dist import best_candidate

    torch, dev, st = _torch()
    cases, order, xs = _ragged_fixed()
    order = order + [order[2]]
    xs = xs + [xs[2].copy()]   # a duplicate of candidate 2: the tie goes to the first index
    xs[5] = np.full_like(xs[5], np.nan)   # an all-NaN candidate loses
    batch = ta.Batch([c.S for c in cases], order, device=0)
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    scores = torch.full((len(order), 16), -1.0, dtype=torch.float64, device=dev)
    best = torch.zeros(2, dtype=torch.float64, device=dev)
    for fam, off in (((0, 1, 3, 4), 0), ((1, 4), 1000)):
        batch.eval_score_best_device(x.data_ptr(), scores.data_ptr(), best.data_ptr(), families=fam, index_offset=off, stream=st)
        torch.cuda.synchronize()
        idx, total = best_candidate(scores, families=fam)
        assert (int(best[0]), float(best[1])) == (off + idx, total), (fam, best.cpu(), idx, total)
        assert idx != 5 and idx != len(order) - 1
        table = scores.cpu().numpy()
        assert np.isnan(table[5]).any()
        assert np.array_equal(table[2], table[-1])
    # a tie between the duplicated pair when it is the winner
    dup = ta.Batch([cases[2].S], [0, 0], device=0)
    x2 = torch.from_numpy(np.concatenate([xs[2], xs[2]])).to(dev)
    s2 = torch.empty((2, 16), dtype=torch.float64, device=dev)
    batch_best = torch.zeros(2, dtype=torch.float64, device=dev)
    dup.eval_score_best_device(x2.data_ptr(), s2.data_ptr(), batch_best.data_ptr(), index_offset=7, stream=st)
    torch.cuda.synchronize()
    assert int(batch_best[0]) == 7


def test_edge_cases():
    case = random_case(5111)   # no rows at all
    assert case.S.m == 0
    batch = ta.Batch([case.S], [0, 0, 0], device=0)
    assert batch.scores_without_g
    got, ref, _ = _scores(batch, [case.x_wild(i) for i in range(3)])
    assert np.array_equal(got, np.zeros((3, 16))) and np.array_equal(ref, got)
    # more than 4096 rows on the fused path
    big = Case("hyq", "slope", ta.gait_combo(4, 2, 2.0), constraint_sets=63, **k_params(2.0, 460))
    assert big.S.m > 4096 and big.S.n <= 2046, (big.S.m, big.S.n)
    b = ta.Batch([big.S], [0, 0], device=0)
    assert b.scores_without_g
    xs = [big.x_perturbed(1), big.x_wild(2)]
    got, ref, _ = _scores(b, xs)
    _assert_matches_score_kernel(got, ref, "> 4096 rows")
    for p in range(2):
        want = _oracle_scores(big, xs[p])
        ok = ~np.isnan(want)
        assert np.all(np.abs(got[p].reshape(8, 2)[ok] - want[ok]) <= 1e-9 * np.abs(want[ok]) + 1e-9)


def test_graph_capture():
    torch, dev, _ = _torch()
    cases, order, xs = _ragged_fixed()
    batch = ta.Batch([c.S for c in cases], order, device=0)
    x = torch.from_numpy(np.concatenate(xs)).to(dev)
    scores = torch.zeros((len(order), 16), dtype=torch.float64, device=dev)
    best = torch.zeros(2, dtype=torch.float64, device=dev)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # (warm-up off the capture)
        batch.eval_score_best_device(x.data_ptr(), scores.data_ptr(), best.data_ptr(), stream=s.cuda_stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.eval_score_best_device(x.data_ptr(), scores.data_ptr(), best.data_ptr(),
                                     stream=torch.cuda.current_stream().cuda_stream)
    xs2 = [cases[s_].x_perturbed(100 + i, 1.2) for i, s_ in enumerate(order)]
    x.copy_(torch.from_numpy(np.concatenate(xs2)))
    graph.replay()
    torch.cuda.synchronize()
    got_s, got_b = scores.clone(), best.clone()
    eager_s = torch.zeros_like(scores)
    eager_b = torch.zeros_like(best)
    st = torch.cuda.current_stream().cuda_stream
    batch.eval_score_best_device(x.data_ptr(), eager_s.data_ptr(), eager_b.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert torch.equal(got_s, eager_s) and torch.equal(got_b, eager_b)
