"""twr_jac_col_sqnorms / twr_jac_col_scale / twr_jac_lsq_solve_scaled on the device: the weighted squared column norms against
scipy on the device's own Jacobian values, bit-reproducibility across batches, calls and iteration caps, c = 1 giving the bits
of twr_jac_lsq_solve, the Marquardt-scaled step against a direct solve of its normal equations, its invariance under a change
of the variables' units, containment of NaN / Inf and bad c / mu, the edge cases, hipGraph capture, the Levenberg-Marquardt
loop with both dampings, and a full C3 batch.

The bounds of the solve tests are those of check_scaled_step, derived in tests/jac_ref.py: the bounds of the unscaled solve in the
scaled variables e = d / c, with tol = 1e-10 and mu = 1e-2 lambda_max(C J^T W J C).
The column norms: a sum of non-negative terms, at most a few thousand per column, against the same sum in another order:
1e-12 relative leaves three orders over len 2^-53.

The LM test's threshold: scripts/lm_damping_cpu.py (numpy on the CPU oracle) on exactly its 2 x 64 inputs gives a final-merit
ratio marquardt / identity of 0.111 .. 0.138 for C3 and 7.2e-5 .. 1.4e-4 for the stairs; the worst is below 0.25, so the
condition is ratio <= 0.5 for every problem."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case
from .jac_device import JacBatch, assert_replay_equals_eager, c3_batch, capture, dev, nan, ragged, ragged_x, torch_ctx
from .jac_ref import COND, ITERS, REL_FLOOR, ROOT, TOL, check_scaled_step, csr, lam_max, same_bits

pytestmark = pytest.mark.gpu


def _ragged_batch(n=None, point="x_perturbed"):
    cases, order = ragged()
    order = order[:n]
    B = JacBatch([c.S for c in cases], order)
    return cases, order, B, dev(ragged_x(cases, order, point))


def _scaled_lam_max(B, p, jac_h, w_h, c_h):
    return lam_max((B.A(p, jac_h) @ sp.diags(c_h[B.xs(p)])).tocsr(), w_h[B.gs(p)])


# ---------------------------------------------------------------- 1. column norms against scipy

@pytest.mark.parametrize("point", ["x_perturbed", "x_wild"])
def test_col_sqnorms_against_scipy_on_a_ragged_batch(point):
    cases, order, B, x = _ragged_batch(point=point)
    g, jac = B.eval(x)
    _, wa, _ = B.violation(g, merit=False)
    jac_h = jac.cpu().numpy()
    assert np.isfinite(jac_h[:B.J]).all()
    w_rand = dev(np.random.default_rng(21).uniform(0.1, 3.0, size=B.G))
    sq = [B.A(p, jac_h).multiply(B.A(p, jac_h)).T.tocsr() for p in range(B.P)]
    for name, w in (("random", w_rand), ("active", wa), ("unit", None)):
        got = B.colsq(jac, w).cpu().numpy()[:B.X]
        w_h = np.ones(B.G) if w is None else w.cpu().numpy()[:B.G]
        zero_cols = worst = 0
        for p in range(B.P):
            ref = sq[p] @ w_h[B.gs(p)]
            gp = got[B.xs(p)]
            assert (ref >= 0).all()
            err = np.abs(gp - ref)
            assert (err <= 1e-12 * ref).all(), (name, p, order[p], float((err / np.maximum(ref, 1e-300)).max()))
            assert not gp[ref == 0].any() and not np.signbit(gp[ref == 0]).any(), (name, p)
            zero_cols += int((ref == 0).sum())
            worst = max(worst, float((err[ref > 0] / ref[ref > 0]).max()) if (ref > 0).any() else 0.0)
        print("%s %s: worst relative error %.2e, %d columns with norm 0" % (point, name, worst, zero_cols))
        if name == "active":
            assert zero_cols > 0, "no column without an active entry: the exact-zero check is vacuous"


# ---------------------------------------------------------------- 2. bit-reproducibility

def test_bits_do_not_depend_on_the_batch_the_call_or_the_cap():
    torch, device, st = torch_ctx()
    c, B, _, _, jac, b, wa = c3_batch(512, merit=False)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    q1, q2 = B.colsq(jac, wa), B.colsq(jac, wa)
    assert same_bits(q1.cpu().numpy(), q2.cpu().numpy()), "two col_sqnorms calls differ"
    c1, c2 = B.scale(q1), B.scale(q1)
    assert same_bits(c1.cpu().numpy(), c2.cpu().numpy()), "two col_scale calls differ"
    q_h, c_h = q1.cpu().numpy()[:B.X], c1.cpu().numpy()[:B.X]
    assert np.isfinite(c_h).all() and (c_h > 0).all()
    lam = _scaled_lam_max(B, 0, jac_h, w_h, c_h)
    mu = dev(np.full(B.P, 1e-2 * lam))
    d1, i1 = B.solve(jac, b, wa, mu, c1, "scaled")
    d2, i2 = B.solve(jac, b, wa, mu, c1, "scaled")
    assert same_bits(d1, d2) and same_bits(i1, i2), "two calls differ"
    assert (i1[:, 3] == 0).all(), i1[:, 3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q3 = B.colsq(jac, wa, stream=side.cuda_stream)
        c3 = B.scale(q3, stream=side.cuda_stream)
        d3, i3 = B.solve(jac, b, wa, mu, c3, "scaled", stream=side.cuda_stream)
    assert same_bits(q3.cpu().numpy()[:B.X], q_h) and same_bits(c3.cpu().numpy()[:B.X], c_h), "another stream differs"
    assert same_bits(d1, d3) and same_bits(i1, i3), "another stream differs"
    one = JacBatch([c.S], [0])
    for p in (0, 201, 511):   # alone in a one-problem handle, its values copied to fresh buffers
        jp, bp, wp = jac[B.jo[p]:B.jo[p + 1]].clone(), b[B.gs(p)].clone(), wa[B.gs(p)].clone()
        qo = one.colsq(jp, wp)
        co = one.scale(qo)
        do, io = one.solve(jp, bp, wp, mu[p:p + 1].clone(), co, "scaled")
        assert same_bits(qo.cpu().numpy()[:one.X], q_h[B.xs(p)]) and same_bits(co.cpu().numpy()[:one.X], c_h[B.xs(p)]), p
        assert same_bits(do, d1[B.xs(p)]) and same_bits(io[0], i1[p]), p
    # mu from 1e-2 to 10 lambda_max: every problem converges, at different counts; a problem that has converged does not move
    # while the others go on
    P = 16
    S16 = JacBatch([c.S], [0] * P)
    mus = dev(lam * np.logspace(-2, 1, P))
    sl = lambda t, off: t[:int(off[P])]   # noqa: E731  (one structure: the first 16 problems are a batch of their own)
    args = (sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus, sl(c1, B.xo))
    d200, i200 = S16.solve(*args, "scaled")
    assert (i200[:, 3] == 0).all() and (i200[:, 0] < ITERS).all() and len(set(i200[:, 0])) > 4, i200[:, 0]
    for k in sorted(set(int(v) for v in i200[:, 0])):
        dk, ik = S16.solve(*args, "scaled", iters=k)
        for p in np.nonzero(i200[:, 0] <= k)[0]:
            assert same_bits(dk[S16.xs(p)], d200[S16.xs(p)]) and same_bits(ik[p], i200[p]), (k, p)
        assert (ik[i200[:, 0] > k, 3] == 1).all() and (ik[i200[:, 0] > k, 0] == k).all()   # the others: the cap


# ---------------------------------------------------------------- 3. c = 1 is the unscaled solve

def test_a_scale_of_ones_gives_the_bits_of_the_unscaled_solve():
    torch, device, st = torch_ctx()
    cases, order, B, x = _ragged_batch()
    jac, b, wa = B.linearise(x, merit=False)
    q = B.colsq(jac, wa).cpu().numpy()[:B.X]
    # any mu > 0 serves: 1e-2 of the largest diagonal entry of J^T W J (a lower bound of lambda_max), from the device's norms
    mu = dev([1e-2 * max(q[B.xs(p)].max(), 1e-300) for p in range(B.P)])
    ones = torch.ones(B.X, dtype=torch.float64, device=device)
    for w in (wa, None):
        for iters, tol in ((60, TOL), (7, 0.0)):
            d0, i0 = B.solve(jac, b, w, mu, None, iters=iters, tol=tol)
            d1, i1 = B.solve(jac, b, w, mu, ones, "scaled", iters=iters, tol=tol)
            assert np.isfinite(d0).all() and (i0[:, 0] > 0).all()
            assert same_bits(d0, d1), "d differs"
            assert same_bits(i0, i1), "info differs"


# ---------------------------------------------------------------- 4. the scaled step against a direct solve

def test_scaled_step_against_a_direct_solve():
    cases, order, B, x = _ragged_batch()
    jac, b, wa = B.linearise(x, merit=False)
    q = B.colsq(jac, wa)
    c = B.scale(q)
    jac_h, b_h, w_h, q_h, c_h = (t.cpu().numpy() for t in (jac, b, wa, q, c))
    assert np.isfinite(c_h[:B.X]).all() and (c_h[:B.X] > 0).all()
    first = {s: order.index(s) for s in sorted(set(order))}   # every structure once: C3, the all-sets gap, the grid, the wide one ...
    sample = sorted(set(first.values()) | {4, 57, 123, 211, 299})
    assert {0, 1, 2, 3} <= set(sample)
    mu_h = np.full(B.P, 1e-2)   # the others: any mu > 0 (they are solved, not checked)
    for p in sample:
        mu_h[p] = 1e-2 * _scaled_lam_max(B, p, jac_h, w_h, c_h)
    assert (mu_h[sample] > 0).all()
    d, info = B.solve(jac, b, wa, dev(mu_h), c, "scaled")
    assert np.isfinite(d).all() and (info[:, 3] != 2).all()
    zeros = 0
    for p in sample:
        zero = q_h[B.xs(p)] == 0
        zeros += int(zero.sum())
        check_scaled_step(B.A(p, jac_h), b_h[B.gs(p)], w_h[B.gs(p)], mu_h[p], c_h[B.xs(p)], d[B.xs(p)], info[p], zero,
                          "ragged problem %d (struct %d)" % (p, order[p]))
    assert zeros > 0


# ---------------------------------------------------------------- 5. unit invariance

def _unit_invariance(rel_floor, all_columns):
    """The same problems in other units, J' = J diag(2^j): (relative difference of the scaled steps in e over the columns
    that are at the floor in neither run, per problem; the same for the unscaled steps over all columns)."""
    cases, order, B, x = _ragged_batch(12)
    jac, b, wa = B.linearise(x, merit=False)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    rng = np.random.default_rng(77)
    j = rng.integers(-20, 21, size=B.X)
    f_h = np.ones(max(1, B.J))
    for p in range(B.P):
        f_h[B.jo[p]:B.jo[p + 1]] = np.ldexp(1.0, j[B.xs(p)])[B.structs[order[p]].col_idx]
    jac2 = jac * dev(f_h)   # exact: a power of two each
    two_j = np.ldexp(1.0, j)
    q1, q2 = B.colsq(jac, wa), B.colsq(jac2, wa)
    c1, c2 = B.scale(q1, rel_floor), B.scale(q2, rel_floor)
    q1_h, q2_h, c1_h, c2_h = (t.cpu().numpy()[:B.X] for t in (q1, q2, c1, c2))
    assert same_bits(q2_h, q1_h * two_j ** 2), "the norms of the rescaled columns are not the rescaled norms"
    mu_s = np.array([1e-2 * _scaled_lam_max(B, p, jac_h, w_h, c1_h) for p in range(B.P)])
    d1, i1 = B.solve(jac, b, wa, dev(mu_s), c1, "scaled")
    d2, i2 = B.solve(jac2, b, wa, dev(mu_s), c2, "scaled")
    assert (i1[:, 3] == 0).all() and (i2[:, 3] == 0).all(), (i1[:, 3], i2[:, 3])
    jac2_h = jac2.cpu().numpy()
    mu_1 = np.array([1e-2 * lam_max(B.A(p, jac_h), w_h[B.gs(p)]) for p in range(B.P)])
    mu_2 = np.array([1e-2 * lam_max(B.A(p, jac2_h), w_h[B.gs(p)]) for p in range(B.P)])
    u1, k1 = B.solve(jac, b, wa, dev(mu_1), None)
    u2, k2 = B.solve(jac2, b, wa, dev(mu_2), None)
    assert (k1[:, 3] == 0).all() and (k2[:, 3] == 0).all()
    scaled, unscaled, checked = [], [], 0
    for p in range(B.P):
        s = B.xs(p)
        keep = (q1_h[s] >= rel_floor * q1_h[s].max()) & (q2_h[s] >= rel_floor * q2_h[s].max())
        if all_columns:
            pos = q1_h[s] > 0
            assert np.array_equal(keep, pos) and keep.sum() > 100, (
                p, keep.sum(), pos.sum(), (q1_h[s][pos] / q1_h[s].max()).min(), (q2_h[s][pos] / q2_h[s].max()).min())
        checked += int(keep.sum())
        e1, e2 = (d1[s] / c1_h[s])[keep], (d2[s] * two_j[s] / c1_h[s])[keep]
        scaled.append(np.linalg.norm(e2 - e1) / np.linalg.norm(e1))
        unscaled.append(np.linalg.norm(u2[s] * two_j[s] - u1[s]) / np.linalg.norm(u1[s]))
    print("rel_floor %g: %d of %d columns checked; scaled steps differ by at most %.2e, unscaled by %.3f .. %.3f"
          % (rel_floor, checked, B.X, max(scaled), min(unscaled), max(unscaled)))
    return np.array(scaled), np.array(unscaled)


def test_the_scaled_step_does_not_depend_on_the_units_of_x():
    """Columns times 2^j, j in [-20, 20]: d'_k 2^j_k = d_k within the bound of the direct-solve test (in e, in norm) for every
    column at the floor in neither run, while the unscaled steps differ by more than 10 %.

    The floor: a column at the floor in one run only is damped differently in the two runs, and through J^T W J that moves the
    other columns' d as well, so the two systems are the same only when no column with a non-zero norm is at the floor in either
    run.  2^(2j) moves the squared norms by up to 1e12 either way, and they span many orders to begin with: with rel_floor = 1e-12
    most columns are at the floor in one run or the other (measured: 137 of 640 at it in neither, problem 0), which tests
    nothing, and a few columns of the all-sets gap problem lie as low as 3e-59 of the largest (measured).  So rel_floor = 1e-200
    here: the floor then holds exactly the columns of norm 0, in both runs, and EVERY other column is checked (asserted per
    problem: the columns kept are the columns with a non-zero norm)."""
    scaled, unscaled = _unit_invariance(1e-200, True)
    assert (unscaled > 0.1).all(), unscaled
    assert (scaled <= COND * 2 * TOL).all(), scaled


# ---------------------------------------------------------------- 6. containment and edge cases

def test_poison_stays_in_its_problem():
    cases, order, B, x = _ragged_batch(40)
    jac, b, wa = B.linearise(x, merit=False)
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()

    def run(jv, bv, wv, mu_h, c_over):
        q = B.colsq(jv, wv)
        c = B.scale(q)
        c_h = c.cpu().numpy()
        for p, val in c_over.items():
            c_h[B.xo[p]:B.xo[p + 1]:3] = val
        d, info = B.solve(jv, bv, wv, dev(mu_h), dev(c_h), "scaled", iters=60)
        return q.cpu().numpy()[:B.X], c.cpu().numpy()[:B.X], d, info

    q0, c0, _, _ = run(jac, b, wa, np.ones(B.P), {})
    mu_h = np.array([1e-2 * _scaled_lam_max(B, p, jac_h, w_h, c0) for p in range(B.P)])
    q0, c0, d0, i0 = run(jac, b, wa, mu_h, {})
    assert np.isfinite(q0).all() and np.isfinite(c0).all() and np.isfinite(d0).all() and np.isfinite(i0).all() and (i0[:, 0] > 0).all()
    bad = {5: ("jac", np.nan), 6: ("b", np.inf), 7: ("w", np.nan), 8: ("mu", -1.0), 9: ("mu", np.nan), 10: ("c", np.nan),
           11: ("c", 0.0), 12: ("c", -1.0), 13: ("c", np.inf), 20: ("jac", np.inf), 21: ("b", np.nan), 22: ("w", np.inf),
           23: ("mu", -np.inf), 24: ("c", -np.inf)}
    jb, bb, wb, mb, cb = jac_h.copy(), b_h.copy(), w_h.copy(), mu_h.copy(), {}
    for p, (where, val) in bad.items():
        if where == "mu":
            mb[p] = val
        elif where == "c":
            cb[p] = val
        else:
            arr, off = {"jac": (jb, B.jo), "b": (bb, B.go), "w": (wb, B.go)}[where]
            arr[off[p]:off[p + 1]:3] = val
    q1, c1, d1, i1 = run(dev(jb), dev(bb), dev(wb), mb, cb)
    for p in range(B.P):
        s = B.xs(p)
        if p not in bad or bad[p][0] in ("b", "mu", "c"):   # the norms and the scale read J and w only
            assert same_bits(q1[s], q0[s]) and same_bits(c1[s], c0[s]), p
        if p not in bad:
            assert same_bits(d1[s], d0[s]) and same_bits(i1[p], i0[p]), p
        elif bad[p][0] in ("mu", "c"):
            assert i1[p, 3] == 2 and i1[p, 0] == 0 and not d1[s].any(), (p, i1[p])
        else:
            assert i1[p, 3] == 2 or not np.isfinite(d1[s]).all(), (p, i1[p])
        if p in bad and bad[p][0] in ("jac", "w"):   # a NaN norm gives a NaN c_k for that k, and status 2
            assert not np.isfinite(q1[s]).all() and i1[p, 3] == 2, (p, i1[p])
            nan = np.isnan(q1[s])
            assert np.isnan(c1[s][nan]).all(), p


def test_edge_cases():
    torch, device, st = torch_ctx()
    # a structure without rows: norms 0, c = 1, d = 0, status 0, no iterations
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    B = JacBatch([case.S], [0, 0, 0])
    one = torch.zeros(8, dtype=torch.float64, device=device)
    q = B.colsq(one, None)
    c = B.scale(q)
    assert not q.cpu().numpy()[:B.X].any() and (c.cpu().numpy()[:B.X] == 1.0).all()
    d, info = B.solve(one, one, None, dev([0.0, 1.0, 2.0]), c, "scaled")
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 0).all() and not info[:, 1:3].any()
    # a problem with no active row: top == 0 -> c = 1, d = 0, status 0; its neighbours keep their bits
    c3, B, _, _, jac, b, wa = c3_batch(3, merit=False)
    q0 = B.colsq(jac, wa)
    cc0 = B.scale(q0)
    lam = _scaled_lam_max(B, 0, jac.cpu().numpy(), wa.cpu().numpy(), cc0.cpu().numpy())
    mu = dev(np.full(3, 1e-2 * lam))
    dref, iref = B.solve(jac, b, wa, mu, cc0, "scaled")
    assert (iref[:, 3] == 0).all()
    wz = wa.clone()
    wz[B.gs(1)] = 0.0
    q = B.colsq(jac, wz)
    cc = B.scale(q)
    q_h, c_h = q.cpu().numpy(), cc.cpu().numpy()
    assert not q_h[B.xs(1)].any() and (c_h[B.xs(1)] == 1.0).all()
    d, info = B.solve(jac, b, wz, mu, cc, "scaled")
    assert not d[B.xs(1)].any() and np.array_equal(info[1], [0, 0, 0, 0])
    for p in (0, 2):
        assert same_bits(c_h[B.xs(p)], cc0.cpu().numpy()[B.xs(p)]) and same_bits(d[B.xs(p)], dref[B.xs(p)]) and same_bits(info[p], iref[p])
    # the running maximum: max(colsq_max, colsq) in / out, and the scale of it
    rng = np.random.default_rng(4)
    m_h = q0.cpu().numpy()[:B.X] * rng.choice([0.25, 4.0], size=B.X)
    cmax = dev(m_h)
    cm = B.scale(q0, colmax=cmax).cpu().numpy()[:B.X]
    a_h = np.maximum(m_h, q0.cpu().numpy()[:B.X])
    assert same_bits(cmax.cpu().numpy(), a_h)
    for p in range(3):
        a = a_h[B.xs(p)]
        assert np.allclose(cm[B.xs(p)], 1.0 / np.sqrt(np.maximum(a, REL_FLOOR * a.max())), rtol=1e-15, atol=0), p
    # rel_floor = 1 is allowed (every c_k = 1 / sqrt(top)); outside (0, 1] it is an error
    c1 = B.scale(q0, rel_floor=1.0).cpu().numpy()
    for p in range(3):
        assert len(set(c1[B.xs(p)])) == 1
    cbuf = nan(B.X)
    for rf in (0.0, -1e-12, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.lsq.col_scale_device(q0.data_ptr(), cbuf.data_ptr(), rf, stream=st)
    # iters = 0: zeros and the scaled |s0|
    d, info = B.solve(jac, b, wa, mu, cc0, "scaled", iters=0)
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 1).all() and (info[:, 1] == 1).all()
    assert same_bits(info[:, 2], iref[:, 2])
    jac_h, w_h, b_h, c0_h = jac.cpu().numpy(), wa.cpu().numpy(), b.cpu().numpy(), cc0.cpu().numpy()
    for p in range(3):
        s0 = np.linalg.norm(c0_h[B.xs(p)] * (B.A(p, jac_h).T @ (w_h[B.gs(p)] * b_h[B.gs(p)])))
        assert abs(info[p, 2] - s0) <= 1e-9 * s0, p
    # w NULL is w = 1
    ones = torch.ones_like(b)
    qn, q1 = B.colsq(jac, None), B.colsq(jac, ones)
    assert same_bits(qn.cpu().numpy(), q1.cpu().numpy())
    cn = B.scale(qn)
    dn, inn = B.solve(jac, b, None, mu, cn, "scaled", iters=30)
    d1, i1 = B.solve(jac, b, ones, mu, cn, "scaled", iters=30)
    assert same_bits(dn, d1) and same_bits(inn, i1) and (inn[:, 0] > 0).all()
    # NULL and misaligned buffers, negative iters, a NaN tol
    out = torch.zeros(4 * 3, dtype=torch.float64, device=device)
    dd = torch.zeros(B.X, dtype=torch.float64, device=device)
    a = (jac.data_ptr(), b.data_ptr(), mu.data_ptr(), cc0.data_ptr(), dd.data_ptr(), out.data_ptr())
    for i in range(6):
        for badptr in (0, a[i] + 4):
            args = list(a)
            args[i] = badptr
            with pytest.raises(ta.TowrError, match="error -1"):
                B.lsq.solve_scaled_device(*args, 10, TOL, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_scaled_device(*a, 10, TOL, d_w=wa.data_ptr() + 4, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_scaled_device(*a, -1, TOL, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_scaled_device(*a, 10, float("nan"), stream=st)
    for args in ((0, dd.data_ptr()), (jac.data_ptr() + 4, dd.data_ptr()), (jac.data_ptr(), 0), (jac.data_ptr(), dd.data_ptr() + 4)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.ops.col_sqnorms_device(*args, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.ops.col_sqnorms_device(jac.data_ptr(), dd.data_ptr(), d_w=wa.data_ptr() + 4, stream=st)
    for args in ((0, dd.data_ptr()), (q0.data_ptr() + 4, dd.data_ptr()), (q0.data_ptr(), 0), (q0.data_ptr(), dd.data_ptr() + 4)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.lsq.col_scale_device(*args, REL_FLOOR, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.col_scale_device(q0.data_ptr(), dd.data_ptr(), REL_FLOOR, d_colsq_max=cmax.data_ptr() + 4, stream=st)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. hipGraph

def test_capture_eval_violation_norms_scale_solve_update_as_one_graph():
    torch, device, _ = torch_ctx()
    cases, order = ragged()
    order = order[:24]
    B = JacBatch([c.S for c in cases], order)
    x = dev(ragged_x(cases, order))
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device=device)   # noqa: E731
    g, jac, r, b, wa, merit, q, c, d, info = (z64(B.G), z64(B.J), z64(B.G), z64(B.G), z64(B.G), z64(B.P), z64(B.X), z64(B.X), z64(B.X),
                                              z64(4 * B.P))
    mu = dev(np.full(B.P, 1e-2))
    outs = (g, jac, r, b, wa, merit, q, c, d, info)
    before = B.lsq.bytes()["resident"]
    B.lsq.reserve_scaled()   # the one allocation, outside the capture
    assert B.lsq.bytes()["resident"] == before + 8 * 2 * (B.X + B.X % 2)

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, stream)
        B.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=stream)
        torch.neg(r, out=b)
        B.ops.col_sqnorms_device(jac.data_ptr(), q.data_ptr(), d_w=wa.data_ptr(), stream=stream)
        B.lsq.col_scale_device(q.data_ptr(), c.data_ptr(), REL_FLOOR, stream=stream)
        B.lsq.solve_scaled_device(jac.data_ptr(), b.data_ptr(), mu.data_ptr(), c.data_ptr(), d.data_ptr(), info.data_ptr(), 25, 1e-6,
                                  d_w=wa.data_ptr(), stream=stream)
        x.add_(d)

    graph = capture(step)
    x1 = ragged_x(cases, order, seed0=100)

    def reset():
        x.copy_(torch.from_numpy(x1))
        for t in outs:
            t.zero_()

    assert_replay_equals_eager(step, graph, reset, outs + (x,))
    assert info.cpu().numpy().reshape(-1, 4)[:, 0].max() > 3 and d.abs().max().item() > 0 and (c > 0).all().item()
    assert not torch.equal(x, torch.from_numpy(x1).to(device))


# ---------------------------------------------------------------- 8. the LM loop with both dampings

@pytest.mark.parametrize("name", ["C3", "C4_stairs"])
def test_lm_loop_marquardt_against_identity(name):
    """64 problems at x_perturbed(seed), 8 steps of 60 CG iterations, the loop and accept rule of scripts/jac_lsq.py: for every
    problem the final merit with mu C^-2 is at most half of the one with mu I (the CPU restatement on these inputs, module
    docstring: at most 0.138)."""
    torch, device, st = torch_ctx()
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import jac_lsq
    finally:
        sys.path.pop(0)
    case = {"C3": lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200)),
            "C4_stairs": baseline_cases()["C4_anymal_stairs_K200"]}[name]()
    n = 64
    x0 = np.concatenate([case.x_perturbed(seed) for seed in range(n)])
    Q = jac_lsq.Problem(torch, [case.S], [0] * n, x0)
    final = {}
    for damping in ("identity", "marquardt"):
        Q.x = torch.from_numpy(x0).to(device)
        mu = None
        if damping == "identity":
            g, r, wa = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G)
            Q.batch.eval_device(Q.x.data_ptr(), g.data_ptr(), Q.jac.data_ptr(), ta.EVAL_BOTH, st)
            Q.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), stream=st)
            mu = 1e-2 * Q.lambda_max(wa, 30)
        res = jac_lsq.lm_loop(torch, Q, damping, mu, 8, 60, 30)
        final[damping] = Q.merit_after.cpu().numpy()
        start = Q.merit_before.cpu().numpy()
        print("%s %s: merit %.4e -> %.4e, accepted per step %s" % (name, damping, res["merit_before"], res["merit_after"], res["accepted_per_step"]))
        assert np.isfinite(final[damping]).all() and (final[damping] < start).all()
    ratio = final["marquardt"] / final["identity"]
    print("%s: final merit marquardt / identity: min %.3e, median %.3e, worst %.3e" % (name, ratio.min(), np.median(ratio), ratio.max()))
    assert (ratio <= 0.5).all(), (ratio.max(), int(ratio.argmax()))


# ---------------------------------------------------------------- 9. a full C3 batch

def test_c3_full_batch():
    torch, device, st = torch_ctx()
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    S = c.S
    n = 8192
    B = JacBatch([S], [0] * n)
    # before the scaled solve is reserved: the formula tests/test_jac_lsq.py pins
    want = 8 * (2 * S.n * n + 3 * S.m * n + 4 * n) + 2 * 8 * S.m + 40 * n
    assert S.n % 2 == 0 and S.m % 2 == 0 and B.lsq.bytes()["resident"] == want
    gen = torch.Generator(device=device)
    gen.manual_seed(5)
    x0 = dev(c.x_guess())
    scale = dev((c.x_perturbed(0) - c.x_guess()) / np.random.default_rng(1234).normal(size=S.n))   # 0.05 * the per-variable scale
    x = (x0[None, :] + scale[None, :] * torch.randn((n, S.n), generator=gen, dtype=torch.float64, device=device)).reshape(-1).contiguous()
    jac, b, wa = B.linearise(x, merit=False)
    q = B.colsq(jac, wa)
    cc = B.scale(q)
    assert B.lsq.bytes()["resident"] == want, "the norms and the scale need no workspace"
    B.lsq.reserve_scaled()
    assert B.lsq.bytes()["resident"] == want + 8 * 2 * S.n * n   # e and c o p in the x layout
    B.lsq.reserve_scaled()
    assert B.lsq.bytes()["resident"] == want + 8 * 2 * S.n * n   # once
    q_h, c_h = q.cpu().numpy()[:B.X], cc.cpu().numpy()[:B.X]
    assert np.isfinite(q_h).all() and (q_h >= 0).all() and np.isfinite(c_h).all() and (c_h > 0).all()
    lam = lam_max((csr(S, jac[:B.jo[1]].cpu().numpy()) @ sp.diags(c_h[:S.n])).tocsr(), wa[:S.m].cpu().numpy())
    mu = dev(np.full(n, 1e-2 * lam))
    d, info = B.solve(jac, b, wa, mu, cc, "scaled", iters=20)
    assert np.isfinite(d).all() and np.isfinite(info).all()
    assert (info[:, 0] == 20).all() and (info[:, 3] == 1).all()
