"""twr_jac_gram / twr_jac_gram_mul / twr_jac_lsq_solve_gram / TWR_JAC_LM_GRAM on the device: the Gram matrix and its product against
scipy on the device's own Jacobian values, the solve against a dense direct solve on the oracle's Jacobian and against the numpy
restatement (scripts/gram_cpu.py), the masked and scaled rules, bit-reproducibility across batches, calls, streams and iteration
caps, containment of NaN and bad mu / c, the edge cases, hipGraph capture, what the handles report to hold, and the bounded LM
driver with the Gram solve against the restatement's loop.

The ragged batch is the one of tests/jac_device.py (ragged) less the structure of more than 3412 variables, which the Gram
tables refuse (TWR_ERR_UNSUPPORTED: the solve's six vectors would not fit one workgroup's LDS; checked here), its first 100
problems: all seven structures, more than one block of every kernel, rows of J of more than 256 entries.

Bounds.  N and N v: every entry within 1e-12 of the sum of the magnitudes of its terms (the bound of the products' tests).  The
solve on the oracle's Jacobian: |d - d_direct| <= 10 STEP_FIGURE |d_direct| = 2.6e-8, ten times what the restatement measures on
the same inputs (tests/test_gram_cpu.py: 2.57e-9).  Where mu is chosen here it is 1e-2 max_i sum_j |C N C|_ij >= 1e-2 lambda_max,
so cond <= 101 and |e - e_direct| <= 2 * 101 * tol |e_direct| in e = d / c (the bound of tests/jac_ref.py).  The driver: the
merit after one step within 1e-6 relative of the restatement's loop, after 8 steps within [0.5, 2] (the bounds of
tests/test_jac_lm.py, on its problems, GROUPS of tests/jac_ref.py: none of them is a seed the jitter rule of tests/test_gram_cpu.py
drops)."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .common import baseline_cases, random_case
from .jac_device import F, GramBatch, JacBatch, LmBatch, assert_replay_equals_eager, capture, dev, nan, ragged, ragged_x, torch_ctx
from .jac_ref import COND, DEVICE_INPUTS, DROPPED, GROUPS, ITERS, ROOT, STEP_FIGURE, STEPS, TOL, case_of, lm_case, same_bits

sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gram_cpu as gc  # noqa: E402

pytestmark = pytest.mark.gpu

MAX_VARS = 3412   # the limit of twr_jac_ops_reserve_gram (include/towr_amd.h)
groups = pytest.mark.parametrize("group", list(GROUPS))


@functools.lru_cache(maxsize=None)
def _ragged_gram(n=100):
    """The ragged batch the Gram tables take, linearised on the device at x_perturbed: shared by the tests, never changed."""
    cases, order = ragged()
    keep = [i for i, c in enumerate(cases) if c.S.n <= MAX_VARS]
    assert len(keep) == len(cases) - 1 and cases[3].S.n > MAX_VARS
    with pytest.raises(ta.TowrError, match="error -5.*variables"):   # the limit fires at reserve time, for the whole handle
        ta.JacOps([cases[0].S, cases[3].S], [0, 1]).reserve_gram()
    pairs = [(i, s) for i, s in enumerate(order) if s in keep][:n]
    G = GramBatch([cases[i].S for i in keep], [keep.index(s) for _, s in pairs])
    x = dev(np.concatenate([cases[s].x_perturbed(i) for i, s in pairs]))
    g, jac = G.eval(x)
    r, wa, _ = G.violation(g)
    assert len(set(G.order)) == len(keep) and max(int(np.diff(S.row_ptr).max()) for S in G.structs) > 256
    assert (G.no % 2 == 0).all()
    return G, jac, -r, wa


def _mu_of(Nc, c):
    """1e-2 of the largest absolute row sum of C N C (>= 1e-2 lambda_max: cond <= 101)."""
    H = abs(sp.diags(c) @ Nc @ sp.diags(c))
    return 1e-2 * float(H.sum(axis=1).max()) if H.nnz else 1.0


# ---------------------------------------------------------------- 1. / 2. the matrix and its product against scipy

def test_gram_against_scipy_on_a_ragged_batch():
    G, jac, b, wa = _ragged_gram()
    jac_h = jac.cpu().numpy()
    rng = np.random.default_rng(41)
    w_h = rng.uniform(0.0, 3.0, size=int(G.go[-1]))
    w_h[rng.integers(0, w_h.size, size=w_h.size // 10)] = 0.0   # non-negative, some exactly 0 (an inactive row)
    ones = dev(np.ones(int(G.go[-1])))
    N_null = G.form(jac).cpu().numpy()
    assert same_bits(N_null, G.form(jac, ones).cpu().numpy()), "d_w = NULL is not unit weights bit for bit"
    for name, N_h, wh in (("unit", N_null, np.ones(w_h.size)), ("random", G.form(jac, dev(w_h)).cpu().numpy(), w_h)):
        worst = 0.0
        for p in range(G.P):
            A = G.A(p, jac_h)
            W = sp.diags(wh[G.gs(p)])
            ref, mag = (A.T @ W @ A).toarray(), (abs(A).T @ W @ abs(A)).toarray()
            got = G.csr(p, N_h)
            assert not np.isnan(got.data).any(), (name, p, "a stored value was not written")
            dense = got.toarray()
            err = np.abs(dense - ref)
            assert (err <= 1e-12 * mag).all(), (name, p, G.order[p], float((err / np.maximum(mag, 1e-300)).max()))
            assert np.array_equal(dense.view(np.int64), dense.T.copy().view(np.int64)), (name, p, "N_ij and N_ji differ in their bits")
            worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
        print("%s weights: worst |N - ref| / sum|terms| %.2e over %d problems" % (name, worst, G.P))


def test_gram_mul_against_scipy_on_the_same_matrices():
    G, jac, b, wa = _ragged_gram()
    N = G.form(jac, wa)
    N_h = N.cpu().numpy()
    v_h = np.random.default_rng(42).normal(size=int(G.xo[-1]))
    u = G.mul(N, dev(v_h))
    worst = 0.0
    for p in range(G.P):
        Nc = G.csr(p, N_h)
        ref, mag = Nc @ v_h[G.xs(p)], abs(Nc) @ np.abs(v_h[G.xs(p)])
        err = np.abs(u[G.xs(p)] - ref)
        assert (err <= 1e-12 * mag).all(), (p, G.order[p], float((err / np.maximum(mag, 1e-300)).max()))
        empty = np.diff(G.pat[p][0]) == 0
        assert not u[G.xs(p)][empty].any() and not np.signbit(u[G.xs(p)][empty]).any(), (p, "an empty row of N is not an exact 0")
        worst = max(worst, float((err / np.maximum(mag, 1e-300)).max()))
    print("worst |N v - ref| / sum|terms| %.2e" % worst)


# ---------------------------------------------------------------- 3. the solve against a direct solve and the restatement

def test_solve_against_a_dense_solve_on_the_oracle_jacobian():
    torch, device, st = torch_ctx()
    cases = [case_of(name) for name, _ in DEVICE_INPUTS]
    G = GramBatch([c.S for c in cases], range(len(cases)))
    sys_ = [gc.first_system(c, seed) for c, (_, seed) in zip(cases, DEVICE_INPUTS)]   # (A, w, N, z, cf, b) on the oracle's J
    jac = dev(np.concatenate([q[0].data for q in sys_]))
    w = dev(np.concatenate([q[1] for q in sys_]))
    wb = dev(np.concatenate([q[1] * q[5] for q in sys_]))
    c = dev(np.concatenate([q[4] for q in sys_]))
    mu_h = [gc.mu_of(q[2], q[4]) for q in sys_]
    N = G.form(jac, w)
    z = G.tmul(jac, wb)
    d, info = G.solve(N, z, dev(mu_h), c)
    for p, (q, (name, seed)) in enumerate(zip(sys_, DEVICE_INPUTS)):
        dd = gc.dense_step(q[2], q[3], mu_h[p], q[4])
        err = np.linalg.norm(d[G.xs(p)] - dd) / np.linalg.norm(dd)
        k_np = gc.gram_cg(q[2], q[3], mu_h[p], q[4], ITERS, TOL)[0]
        print("%s seed %d: device %d iterations (numpy %d), |s|/|s0| %.2e, |d - dense| / |dense| %.3e" % (name, seed, info[p, 0], k_np, info[p, 1], err))
        assert info[p, 3] == 0 and 0 < info[p, 0] < ITERS and info[p, 1] <= TOL, info[p]
        assert err <= 10 * STEP_FIGURE, (name, err)
        masked = q[4] == 0
        assert masked.any() and not d[G.xs(p)][masked].any() and not np.signbit(d[G.xs(p)][masked]).any()


def test_iteration_counts_equal_the_restatement_on_the_ragged_batch():
    """cond <= 101, tol = 1e-10: the device stops every problem at the iteration at which the restatement stops it.  The
    restatement here is gram_cg_device, which takes the kernel's roundings in the kernel's order (multiply, then add; lane t of
    256 adds the elements t, t + 256, ...; the butterflies; the waves in order; 16 lanes per row of N), because near the end
    |s| / |s0| falls by up to a factor 3 per iteration and the count of plain numpy (gram_cg, another summation order) moves by
    one under a change of N by a single rounding: against gram_cg 14 of these 100 problems differed by one iteration, which is
    why the kernel has no fused multiply-add and the restatement follows its order.  With the same arithmetic the two agree
    in every bit: counts, |s| / |s0|, |s0| and d.  d is also held to plain numpy's, to 1e-6."""
    G, jac, b, wa = _ragged_gram()
    torch, device, st = torch_ctx()
    N = G.form(jac, wa)
    z = G.tmul(jac, wa * b)
    N_h, z_h = N.cpu().numpy(), z.cpu().numpy()
    colsq = nan(G.xo[-1])
    c = nan(G.xo[-1])
    G.ops.col_sqnorms_device(jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
    G.lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), 1e-12, stream=st)
    torch.cuda.synchronize()
    c_h = c.cpu().numpy()
    mats = [G.csr(p, N_h) for p in range(G.P)]
    mu_h = np.array([_mu_of(mats[p], c_h[G.xs(p)]) for p in range(G.P)])
    d, info = G.solve(N, z, dev(mu_h), c)
    off, other_bits, plain_off = [], [], 0
    for p in range(G.P):
        k, d_np, rel, status = gc.gram_cg_device(mats[p], z_h[G.xs(p)], mu_h[p], c_h[G.xs(p)], ITERS, TOL)
        k_plain, d_plain, _, _ = gc.gram_cg(mats[p], z_h[G.xs(p)], mu_h[p], c_h[G.xs(p)], ITERS, TOL)
        assert status == 0 and info[p, 3] == 0 and info[p, 1] <= TOL, (p, G.order[p], info[p], k, rel)
        assert np.linalg.norm(d[G.xs(p)] - d_plain) <= 1e-6 * np.linalg.norm(d_plain), p   # the same iterates up to rounding
        plain_off += int(info[p, 0] != k_plain)
        if info[p, 0] != k:
            off.append((p, G.order[p], int(info[p, 0]), k, float(info[p, 1]), float(rel)))
        if not (same_bits(d[G.xs(p)], d_np) and info[p, 1] == rel):
            other_bits.append(p)
    print("iteration counts: %d of %d problems differ from the restatement in the device's order (problem, structure, device, numpy, "
          "|s|/|s0| device, numpy): %s; %d differ in the bits of d or |s|/|s0|; %d differ from plain numpy's count"
          % (len(off), G.P, off, len(other_bits), plain_off))
    assert not off, off
    assert not other_bits, other_bits


def test_iteration_counts_equal_the_restatement_under_heavy_damping():
    """An addition to the test above, not a replacement: with mu = 10 max_i sum_j |C N C|_ij the condition number is at most
    1.1, CG contracts by (sqrt(1.1) - 1) / (sqrt(1.1) + 1) = 0.024 per iteration, so consecutive |s| / |s0| lie a factor 40
    apart and the iterate that first passes tol = 1e-10 is the same under any rounding: here the counts are a property of the
    iteration, and the device's must equal the restatement's on every problem."""
    G, jac, b, wa = _ragged_gram()
    N = G.form(jac, wa)
    z = G.tmul(jac, wa * b)
    N_h, z_h = N.cpu().numpy(), z.cpu().numpy()
    mats = [G.csr(p, N_h) for p in range(G.P)]
    mu_h = np.array([1e3 * _mu_of(mats[p], np.ones(G.xo[p + 1] - G.xo[p])) for p in range(G.P)])
    d, info = G.solve(N, z, dev(mu_h))
    counts = set()
    for p in range(G.P):
        k, d_np, rel, status = gc.gram_cg(mats[p], z_h[G.xs(p)], mu_h[p], np.ones(G.xo[p + 1] - G.xo[p]), ITERS, TOL)
        assert status == 0 and info[p, 3] == 0 and info[p, 0] == k and k < 12, (p, G.order[p], info[p], k, rel)
        assert np.linalg.norm(d[G.xs(p)] - d_np) <= 1e-12 * np.linalg.norm(d_np), p
        counts.add(k)
    print("iteration counts under heavy damping: %s" % sorted(counts))


# ---------------------------------------------------------------- 4. the masked and scaled rules

@functools.lru_cache(maxsize=None)
def _small():
    """The first 12 ragged problems as a batch of their own, with N, z, a scale with zeros in it and mu: shared, never changed."""
    G0, jac0, b0, wa0 = _ragged_gram()
    P = 12
    G = GramBatch(G0.structs, G0.order[:P])
    jac, b, wa = jac0[:int(G.jo[-1])].clone(), b0[:int(G.go[-1])].clone(), wa0[:int(G.go[-1])].clone()
    N = G.form(jac, wa)
    z = G.tmul(jac, wa * b)
    rng = np.random.default_rng(43)
    c_h = np.exp(rng.normal(size=int(G.xo[-1])))
    c_h[rng.integers(0, c_h.size, size=c_h.size // 8)] = 0.0
    N_h = N.cpu().numpy()
    mu_h = np.array([_mu_of(G.csr(p, N_h), c_h[G.xs(p)]) for p in range(P)])
    return G, jac, wa, N, z, c_h, mu_h


def test_masked_and_scaled_rules():
    G, jac, wa, N, z, c_h, mu_h = _small()
    N_h, z_h = N.cpu().numpy(), z.cpu().numpy()
    d, info = G.solve(N, z, dev(mu_h), dev(c_h))
    assert (info[:, 3] == 0).all() and (c_h == 0).sum() > 100
    assert not d[c_h == 0].any() and not np.signbit(d[c_h == 0]).any(), "a masked variable is not an exact +0"
    for p in range(G.P):   # the columns taken out by hand, a dense solve
        c = c_h[G.xs(p)]
        dd = gc.dense_step(G.csr(p, N_h), z_h[G.xs(p)], mu_h[p], c)
        free = c != 0
        err = np.linalg.norm((d[G.xs(p)] - dd)[free] / c[free]) / np.linalg.norm(dd[free] / c[free])
        assert err <= 2 * COND * TOL, (p, err)
        s0 = np.linalg.norm(np.where(free, c * z_h[G.xs(p)], 0.0))
        assert abs(info[p, 2] - s0) <= 1e-12 * s0, (p, "|s0| is not taken over the free space")
    # c = 1 gives the bits of d_scale = NULL
    mu1 = dev(np.array([_mu_of(G.csr(p, N_h), np.ones(G.xo[p + 1] - G.xo[p])) for p in range(G.P)]))
    d1, i1 = G.solve(N, z, mu1, None)
    d2, i2 = G.solve(N, z, mu1, dev(np.ones(int(G.xo[-1]))))
    assert same_bits(d1, d2) and same_bits(i1, i2) and (i1[:, 3] == 0).all()
    # bad input: status 2 and d = 0 for that problem alone
    for what, val in (("c", -1.0), ("c", np.nan), ("c", np.inf), ("mu", -1.0), ("mu", np.nan), ("mu", np.inf)):
        cb, mb = c_h.copy(), mu_h.copy()
        if what == "c":
            cb[G.xo[5] + 7] = val
        else:
            mb[5] = val
        db, ib = G.solve(N, z, dev(mb), dev(cb))
        assert ib[5, 3] == 2 and ib[5, 0] == 0 and not db[G.xs(5)].any(), (what, val, ib[5])
        assert np.isnan(ib[5, 1]) if what == "c" and not val < 0 else ib[5, 1] == 1.0, (what, val, ib[5])   # NaN where |s0| is not finite
        rest = np.ones(d.size, dtype=bool)
        rest[G.xs(5)] = False
        assert same_bits(db[rest], d[rest]) and same_bits(np.delete(ib, 5, axis=0), np.delete(info, 5, axis=0)), (what, val)


# ---------------------------------------------------------------- 5. bits

def test_bits_do_not_depend_on_the_batch_the_call_the_stream_or_the_cap():
    torch, device, st = torch_ctx()
    G, jac, wa, N, z, c_h, mu_h = _small()
    c, mu = dev(c_h), dev(mu_h)
    v = dev(np.random.default_rng(44).normal(size=int(G.xo[-1])))
    N_h, u = N.cpu().numpy(), G.mul(N, v)
    d, info = G.solve(N, z, mu, c)
    # repeated calls
    assert same_bits(G.form(jac, wa).cpu().numpy(), N_h) and same_bits(G.mul(N, v), u)
    d2, i2 = G.solve(N, z, mu, c)
    assert same_bits(d2, d) and same_bits(i2, info), "two calls differ"
    # another stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        N3 = G.form(jac, wa, stream=side.cuda_stream)
        u3 = G.mul(N3, v, stream=side.cuda_stream)
        d3, i3 = G.solve(N3, z, mu, c, stream=side.cuda_stream)
    assert same_bits(N3.cpu().numpy(), N_h) and same_bits(u3, u) and same_bits(d3, d) and same_bits(i3, info), "another stream differs"
    # a larger cap; a smaller one stops the rest at the cap and leaves the finished ones alone
    d4, i4 = G.solve(N, z, mu, c, iters=5 * ITERS)
    assert same_bits(d4, d) and same_bits(i4, info)
    assert info[:, 0].max() > info[:, 0].min()
    k = int(info[:, 0].min())
    dk, ik = G.solve(N, z, mu, c, iters=k)
    for p in range(G.P):
        if info[p, 0] <= k:
            assert same_bits(dk[G.xs(p)], d[G.xs(p)]) and same_bits(ik[p], info[p]), p
        else:
            assert ik[p, 3] == 1 and ik[p, 0] == k, ik[p]
    assert len(set(info[:, 0] <= k)) == 2
    # the same problems at other positions of another batch (reversed order, two of them twice)
    perm = list(range(G.P))[::-1] + [3, 0]
    H = GramBatch(G.structs, [G.order[p] for p in perm])
    cat = lambda t, off: torch.cat([t[int(off[p]):int(off[p + 1])] for p in perm])   # noqa: E731
    jac_h, wa_h, z_h, c_q, v_h = cat(jac, G.jo), cat(wa, G.go), cat(z, G.xo), cat(c, G.xo), cat(v, G.xo)
    NH = H.form(jac_h, wa_h)
    uH = H.mul(NH, v_h)
    dH, iH = H.solve(NH, z_h, dev(mu_h[perm]), c_q)
    NH_h = NH.cpu().numpy()
    for q, p in enumerate(perm):
        nn = len(G.pat[p][1])
        assert same_bits(NH_h[H.no[q]:H.no[q] + nn], N_h[G.no[p]:G.no[p] + nn]), (q, p, "N")
        assert same_bits(uH[H.xs(q)], u[G.xs(p)]) and same_bits(dH[H.xs(q)], d[G.xs(p)]) and same_bits(iH[q], info[p]), (q, p)


# ---------------------------------------------------------------- 6. poison and edge cases

def test_poison_stays_in_its_problem():
    G, jac, wa, N, z, c_h, mu_h = _small()
    c, mu = dev(c_h), dev(mu_h)
    N_h = N.cpu().numpy()
    d, info = G.solve(N, z, mu, c)
    bad, nn = 4, len(G.pat[4][1])
    rest_x = np.ones(d.size, dtype=bool)
    rest_x[G.xs(bad)] = False
    rest_n = np.ones(N_h.size, dtype=bool)
    rest_n[G.no[bad]:G.no[bad + 1]] = False
    for what in ("J", "w", "z", "c"):
        jp, wp, zp, cp = jac.clone(), wa.clone(), z.clone(), c.clone()
        if what == "J":
            jp[int(G.jo[bad]) + 11] = float("nan")
        elif what == "w":
            wp[int(G.go[bad]) + 2] = float("nan")
        elif what == "z":
            zp[int(G.xo[bad]) + int(np.flatnonzero(c_h[G.xs(bad)] != 0)[0])] = float("nan")
        else:
            cp[int(G.xo[bad]) + 1] = float("nan")
        Np = G.form(jp, wp)
        Np_h = Np.cpu().numpy()
        assert same_bits(Np_h[rest_n], N_h[rest_n]), (what, "N of another problem changed")
        assert np.isnan(Np_h[G.no[bad]:G.no[bad] + nn]).any() == (what in "Jw"), what
        dp, ip = G.solve(Np, zp, mu, cp)
        assert ip[bad, 3] == 2 and not dp[G.xs(bad)].any(), (what, ip[bad])   # nothing of it was usable: d = 0
        # |s| / |s0| on bad input: NaN where |s0| is not finite (z, c), 1 where the first delta is not a number (N from J, w)
        assert ip[bad, 0] == 0 and (np.isnan(ip[bad, 1]) and np.isnan(ip[bad, 2]) if what in "zc" else ip[bad, 1] == 1.0), (what, ip[bad])
        k_np, _, rel_np, st_np = gc.gram_cg(G.csr(bad, Np_h), zp.cpu().numpy()[G.xs(bad)], mu_h[bad], cp.cpu().numpy()[G.xs(bad)], ITERS, TOL)
        k_dv, _, rel_dv, st_dv = gc.gram_cg_device(G.csr(bad, Np_h), zp.cpu().numpy()[G.xs(bad)], mu_h[bad], cp.cpu().numpy()[G.xs(bad)], ITERS, TOL)
        assert (k_np, st_np) == (k_dv, st_dv) == (0, 2) and np.array_equal([rel_np, rel_dv], [ip[bad, 1]] * 2, equal_nan=True), (what, rel_np, rel_dv)
        assert same_bits(dp[rest_x], d[rest_x]) and same_bits(np.delete(ip, bad, axis=0), np.delete(info, bad, axis=0)), what
        if what in "Jw":
            up = G.mul(Np, dev(np.ones(d.size)))
            assert np.isnan(up[G.xs(bad)]).any() and not np.isnan(up[rest_x]).any(), what


def test_edge_cases():
    rng = np.random.default_rng(45)
    norows, hopper = random_case(5111).S, baseline_cases()["C1_hopper"]().S
    assert norows.m == 0 and hopper.n % 2 == 1
    G = GramBatch([hopper, norows], [0, 1, 0, 1, 1])
    assert [int(v) for v in np.diff(G.no)] == [len(G.pat[p][1]) + len(G.pat[p][1]) % 2 for p in range(G.P)] and G.no[2] == G.no[1]
    jac = dev(rng.normal(size=int(G.jo[-1])))
    w = dev(rng.uniform(0.5, 2.0, size=int(G.go[-1])))
    N = G.form(jac, w)
    N_h = N.cpu().numpy()
    z_h = rng.normal(size=int(G.xo[-1]))
    z_h[G.xs(2)] = 0.0   # z = 0: converged at the start
    z = dev(z_h)
    mu_h = np.array([_mu_of(G.csr(p, N_h), np.ones(G.xo[p + 1] - G.xo[p])) for p in range(G.P)])
    d, info = G.solve(N, z, dev(mu_h))
    u = G.mul(N, z)
    for p in (1, 3, 4):   # no rows: N = 0, so N v = 0 and (0 + mu I) d = z converges in one iteration to z / mu
        assert not u[G.xs(p)].any() and info[p, 3] == 0 and info[p, 0] == 1
        assert np.abs(d[G.xs(p)] - z_h[G.xs(p)] / mu_h[p]).max() <= 1e-15 * np.abs(z_h[G.xs(p)] / mu_h[p]).max()
    assert tuple(info[2]) == (0.0, 0.0, 0.0, 0.0) and not d[G.xs(2)].any() and not np.signbit(d[G.xs(2)]).any()
    dd = gc.dense_step(G.csr(0, N_h), z_h[G.xs(0)], mu_h[0], np.ones(hopper.n))
    assert info[0, 3] == 0 and np.linalg.norm(d[G.xs(0)] - dd) <= 2 * COND * TOL * np.linalg.norm(dd)
    # z = 0 everywhere on a structure without rows: d = 0, status 0, no iterations
    d0, i0 = G.solve(N, dev(np.zeros(int(G.xo[-1]))), dev(mu_h))
    assert not d0.any() and (i0 == 0).all()
    # iters = 0: d = 0, |s0|, status 1 where there is something to do
    dz, iz = G.solve(N, z, dev(mu_h), iters=0)
    assert not dz.any() and (iz[:, 0] == 0).all() and list(iz[:, 3]) == [1, 1, 0, 1, 1]
    assert all(abs(iz[p, 2] - np.linalg.norm(z_h[G.xs(p)])) <= 1e-14 * np.linalg.norm(z_h[G.xs(p)]) for p in range(G.P))
    # a batch of one problem: the bits of the same problem in the batch above
    one = GramBatch([hopper], [0])
    j1, w1 = jac[:int(G.jo[1])].clone(), w[:int(G.go[1])].clone()
    N1 = one.form(j1, w1)
    assert same_bits(N1.cpu().numpy()[:len(one.pat[0][1])], N_h[:len(one.pat[0][1])])
    d1, i1 = one.solve(N1, z[:hopper.n].clone(), dev(mu_h[:1]))
    assert same_bits(d1, d[G.xs(0)]) and same_bits(i1[0], info[0])
    # a handle of structures without rows only
    E = GramBatch([norows], [0, 0])
    assert E.no[-1] == 0
    NE = E.form(dev(np.zeros(1)), None)
    dE, iE = E.solve(NE, dev(np.ones(2 * norows.n)), dev(np.array([2.0, 4.0])))
    assert (iE[:, 3] == 0).all() and np.array_equal(dE, np.repeat([0.5, 0.25], norows.n))


# ---------------------------------------------------------------- 7. capture, and what the handles hold

def test_capture_eval_violation_tmul_gram_solve_as_one_graph():
    torch, device, _ = torch_ctx()
    cases, order = ragged()
    order = [s for s in order if s != 3][:24]
    B = JacBatch([c.S for c in cases], order)
    ops0 = B.ops.bytes()["resident"]
    B.ops.reserve_gram()
    ops1 = B.ops.bytes()["resident"]
    assert ops1 > ops0
    B.ops.reserve_gram()
    assert B.ops.bytes()["resident"] == ops1, "the Gram tables are made once"
    X, G_, J, NN = int(B.xo[-1]), int(B.go[-1]), int(B.jo[-1]), int(B.ops.gram_layout()[-1])
    x = dev(ragged_x(cases, order))
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device=device)   # noqa: E731
    g, jac, r, t, wa, merit, z, N, d, info = z64(G_), z64(J), z64(G_), z64(G_), z64(G_), z64(B.P), z64(X), z64(NN), z64(X), z64(4 * B.P)
    mu = dev(np.full(B.P, 50.0))
    outs = (g, jac, r, t, wa, merit, z, N, d, info)
    lsq0 = B.lsq.bytes()["resident"]

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, stream)
        B.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=stream)
        torch.mul(wa, r, out=t)
        t.neg_()
        B.ops.tmul_device(jac.data_ptr(), t.data_ptr(), z.data_ptr(), stream)
        B.ops.gram_device(jac.data_ptr(), N.data_ptr(), d_w=wa.data_ptr(), stream=stream)
        B.lsq.solve_gram_device(N.data_ptr(), z.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), 25, 1e-6, stream=stream)
        x.add_(d)

    graph = capture(step)
    x1 = ragged_x(cases, order, seed0=100)

    def reset():
        x.copy_(torch.from_numpy(x1))
        for t in outs:
            t.zero_()

    assert_replay_equals_eager(step, graph, reset, outs + (x,))
    assert info.cpu().numpy().reshape(-1, 4)[:, 0].max() > 3 and d.abs().max().item() > 0
    assert B.ops.bytes()["resident"] == ops1 and B.lsq.bytes()["resident"] == lsq0, "a call after the reserve changed what the handles hold"


# ---------------------------------------------------------------- 8. the driver with TWR_JAC_LM_GRAM

@functools.lru_cache(maxsize=None)
def _gram_run(group):
    B = LmBatch(GROUPS[group], solver="gram")
    return B, B.run()


@functools.lru_cache(maxsize=None)
def _cpu(name, seed):
    case, (lo, up) = lm_case(name)
    return gc.lm_gram(case, case.x_perturbed(seed), lo, up, steps=STEPS)


@groups
def test_driver_with_the_gram_solve_against_the_restatement(group):
    B, hist = _gram_run(group)
    assert not set(GROUPS[group]) & set(DROPPED)
    x_end, rec_end = hist[-1]
    rec1 = hist[1][1]
    for p, (name, seed) in enumerate(B.problems):
        lo, up = B.lo_h[B.xs(p)], B.up_h[B.xs(p)]
        xp = x_end[B.xs(p)]
        fixed = lo == up
        assert np.array_equal(xp[fixed], lo[fixed]), (name, seed, "a fixed variable left its value")
        assert ((xp >= lo) & (xp <= up)).all(), (name, seed, "x left its box")
        assert all(((h[0][B.xs(p)] >= lo) & (h[0][B.xs(p)] <= up)).all() for h in hist)
        if name == "norows":
            assert rec_end[p, F["state"]] == ta.JacLm.DONE and rec_end[p, F["merit"]] == 0
            continue
        cpu = _cpu(name, seed)
        m1, m8 = rec1[p, F["merit"]], rec_end[p, F["merit"]]
        print("%s seed %d: merit after one step %.9e (numpy %.9e, rel %.2e), after %d %.6e (numpy %.6e, ratio %.4f), accepted %d (numpy %d)"
              % (name, seed, m1, cpu["merit"][1], abs(m1 - cpu["merit"][1]) / cpu["merit"][1], STEPS, m8, cpu["merit"][-1], m8 / cpu["merit"][-1],
                 rec_end[p, F["accepted"]], sum(cpu["accepted"])))
        assert abs(m1 - cpu["merit"][1]) <= 1e-6 * cpu["merit"][1], (name, seed)
        assert 0.5 <= m8 / cpu["merit"][-1] <= 2.0, (name, seed)
        assert rec_end[p, F["state"]] == ta.JacLm.RUNNING and rec_end[p, F["steps"]] == STEPS


@groups
def test_driver_eight_gram_steps_as_one_graph_give_the_eager_bits(group):
    torch, device, _ = torch_ctx()
    ref, hist = _gram_run(group)
    B = LmBatch(GROUPS[group], solver="gram")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        B.start(stream=side.cuda_stream)
        B.step(1, stream=side.cuda_stream)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        B.step(STEPS, stream=torch.cuda.current_stream().cuda_stream)
    B.start()   # a fresh start: the graph then takes all eight steps
    torch.cuda.synchronize()
    graph.replay()
    x, rec = B.read()
    assert same_bits(x, hist[-1][0]) and same_bits(rec, hist[-1][1])


@groups
def test_driver_left_at_cgls_is_unchanged_and_bytes_grow_at_set_solver(group):
    a, b = LmBatch(GROUPS[group]), LmBatch(GROUPS[group], solver="cgls")
    ops0, lm0 = a.ops.bytes()["resident"], a.lm.bytes()["resident"]
    ha, hb = a.run(), b.run()
    for (xa, ra), (xb, rb) in zip(ha, hb):
        assert same_bits(xa, xb) and same_bits(ra, rb)
    assert a.ops.bytes()["resident"] == ops0 and a.lm.bytes()["resident"] == lm0, "a CGLS driver holds what it held"
    g, hist = _gram_run(group)
    n_gram = int(g.ops.gram_layout()[-1])
    assert g.lm.bytes()["resident"] == lm0 + 8 * max(2, n_gram) and g.ops.bytes()["resident"] > ops0
    # the two solvers are different iterations: close, not equal
    differs = False
    for p, (name, _) in enumerate(g.problems):
        if name != "norows":
            ma, mg = ha[-1][1][p, F["merit"]], hist[-1][1][p, F["merit"]]
            assert 0.5 <= mg / ma <= 2.0, (name, ma, mg)
            differs = differs or ma != mg
    assert differs
    with pytest.raises(ta.TowrError, match="error -1"):   # legal between create and start only
        ta._check(ta.lib().twr_jac_lm_set_solver(a.lm._h, 1))
