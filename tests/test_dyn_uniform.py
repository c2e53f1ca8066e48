"""dyn_uniform_kernel against dyn_kernel, bit for bit.  A batch whose problems all reference ONE structure is uniform: with
per-kernel launches its "dynamic" rows are evaluated by waves that own one slice kind and load its records once.  The same
x evaluated as [S, S2] alternating -- S2 a separately built equal structure -- takes the general kernel.  Both runs record
per-kernel events, so that batches of these sizes take the three launches instead of the fused one.  g and jac must be the
same bits for EVAL_BOTH, EVAL_JACOBIAN and EVAL_VALUES, every element written, and three sampled problems match the oracle.
Shapes: K = 200, 400 problems (two-chunk staging maps, 16 kinds, three full iterations and a ragged fourth); K = 52, 1603
problems (four-chunk maps, 5 kinds on the trimmed grid, not a multiple of 8); K = 40, 5 problems (fewer slices than waves)."""
import functools

import numpy as np
import pytest

import towr_amd as ta
from tests.common import Case, assert_parity, k_params

pytestmark = pytest.mark.gpu

SENTINEL = 1.2345e300   # what the outputs hold before an evaluation: none may be left


@functools.lru_cache(maxsize=None)
def _case(K):
    mk = lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, K))
    a, b = mk(), mk()
    xs = [a.x_guess()] + [a.x_perturbed(i) for i in range(4)] + [a.x_wild(i) for i in range(3)]
    return a, b, xs


def _run(batch, x, flags):
    import torch
    d_x = torch.from_numpy(x).cuda()
    g = torch.full((int(batch.g_off[-1]),), SENTINEL, dtype=torch.float64, device="cuda")
    j = torch.full((int(batch.jac_off[-1]),), SENTINEL, dtype=torch.float64, device="cuda")
    batch.profile_begin(1)
    batch.eval_device(d_x.data_ptr(), g.data_ptr(), j.data_ptr(), flags, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    batch.profile_end()
    return g.cpu().numpy(), j.cpu().numpy()


def _both_ways(K, B, kinds, xs):
    a, b, _ = _case(K)
    uni = ta.Batch([a.S], [0] * B, device=0)
    gen = ta.Batch([a.S, b.S], [p & 1 for p in range(B)], device=0)
    assert uni.dyn_uniform_kinds() == kinds and gen.dyn_uniform_kinds() == 0
    assert np.array_equal(uni.g_off, gen.g_off) and np.array_equal(uni.jac_off, gen.jac_off)
    x = np.concatenate(xs)
    out = {}
    for flags in (ta.EVAL_BOTH, ta.EVAL_JACOBIAN, ta.EVAL_VALUES):
        gu, ju = _run(uni, x, flags)
        gg, jg = _run(gen, x, flags)
        if flags & ta.EVAL_VALUES:
            assert not (gu == SENTINEL).any(), "flags %d: constraint values left unwritten" % flags
            assert np.array_equal(gu.view(np.int64), gg.view(np.int64)), "flags %d: g differs between the uniform and the general path" % flags
        if flags & ta.EVAL_JACOBIAN:
            assert not (ju == SENTINEL).any(), "flags %d: Jacobian values left unwritten" % flags
            assert np.array_equal(ju.view(np.int64), jg.view(np.int64)), "flags %d: jac differs between the uniform and the general path" % flags
        out[flags] = (gu, ju)
    return uni, out


@pytest.mark.parametrize("K,B,kinds", [(200, 400, 16), (52, 1603, 5), (40, 5, 4)])
def test_uniform_batch_is_the_general_path_bit_for_bit(K, B, kinds):
    a, _, pool = _case(K)
    xs = [pool[(p * 5 + p // 8) % len(pool)] for p in range(B)]
    uni, out = _both_ways(K, B, kinds, xs)
    g, j = out[ta.EVAL_BOTH]
    for p in sorted({0, B // 2, B - 1}):
        rg, _, _, rj = a.P.eval(xs[p])
        assert_parity(a.S, g[uni.g_off[p]:uni.g_off[p + 1]], j[uni.jac_off[p]:uni.jac_off[p + 1]], rg, rj, "K=%d problem %d" % (K, p))


def test_nan_in_one_problem_stays_in_it():
    """A NaN in the x of one problem of a uniform batch: the same bits as on the general path, the other problems untouched."""
    K, B = 40, 11
    a, _, pool = _case(K)
    xs = [pool[p % len(pool)].copy() for p in range(B)]
    base = next(v for v in a.S.var_sets if v["name"] == "base-ang")
    xs[6][base["offset"] + base["size"] // 2] = np.nan
    uni, out = _both_ways(K, B, 4, xs)
    g, j = out[ta.EVAL_BOTH]
    assert np.isnan(g[uni.g_off[6]:uni.g_off[7]]).any() and np.isnan(j[uni.jac_off[6]:uni.jac_off[7]]).any()
    for p in (5, 7):
        rg, _, _, rj = a.P.eval(xs[p])
        assert_parity(a.S, g[uni.g_off[p]:uni.g_off[p + 1]], j[uni.jac_off[p]:uni.jac_off[p + 1]], rg, rj, "neighbour %d" % p)
