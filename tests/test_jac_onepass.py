"""twr_jac_normal_mul / twr_jac_lsq_solve_onepass on the device: the one-pass product against scipy on the device's own Jacobian
values, the one-pass solve (unscaled and Marquardt-scaled) against a direct solve of its normal equations with the inputs and
the bounds of tests/jac_ref.py (check_step, check_scaled_step), its agreement with twr_jac_lsq_solve at the Levenberg-Marquardt
cap, bit-reproducibility across batches, calls, streams and iteration caps, c = 1 giving the bits of the unscaled solve, exact
invariance under powers of two, containment of NaN / Inf and bad mu / c, the edge cases, hipGraph capture, what the handles
report to hold, and a full C3 batch.

The bounds of the solve tests are those of tests/jac_ref.py::check_step (tol = 1e-10, mu = 1e-2 lambda_max, cond <= 101): true relative
normal-equation residual <= 2 tol, |d - d_direct| <= 101 2 tol |d_direct|, iterations in (0, 200).  The numpy restatement of the
one-pass iteration (scripts/onepass_cpu.py onepass) on the oracle Jacobian of the five BASELINE cases stays inside them: it
stops within 0 to 4 iterations of CGLS, its true residual equals the recurred one to three digits, and |d - d_direct| /
|d_direct| is at most 2.2e-9; the factor 2 is for the device's other summation order."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case
from .jac_device import JacBatch, assert_replay_equals_eager, c3_batch, capture, dev, nan, ragged, ragged_x, torch_ctx
from .jac_ref import COND, ITERS, TOL, check_step, csr, lam_max, row_weights, same_bits, viol

pytestmark = pytest.mark.gpu


def _ragged_batch(n=None):
    cases, order = ragged()
    order = order[:n]
    B = JacBatch([c.S for c in cases], order)
    return cases, order, B, dev(ragged_x(cases, order))


# ---------------------------------------------------------------- 1. the product against scipy

def test_normal_product_against_scipy_on_a_ragged_batch():
    cases, order, B, x = _ragged_batch()
    assert B.P == 300 and max(c.S.n for c in cases) > 6144
    _, jac = B.eval(x)
    jac_h = jac.cpu().numpy()
    X, G = int(B.xo[-1]), int(B.go[-1])
    rng = np.random.default_rng(31)
    v_h, w_h = rng.normal(size=X), rng.uniform(0.1, 3.0, size=G)
    v = dev(v_h)
    As = [B.A(p, jac_h) for p in range(B.P)]
    for name, w in (("unit", None), ("random", dev(w_h))):
        wh = np.ones(G) if w is None else w_h
        y, u = B.normal(jac, v, w)
        _, u_alone = B.normal(jac, v, w, with_y=False)
        assert same_bits(u, u_alone), "u depends on whether y is asked for"
        worst_y = worst_u = 0.0
        empty_cols = 0
        for p in range(B.P):
            A, absA = As[p], abs(As[p])
            xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
            y_ref, y_mag = A @ v_h[xs], absA @ np.abs(v_h[xs])
            u_ref, u_mag = A.T @ (wh[gs] * y_ref), absA.T @ (wh[gs] * y_mag)
            ey, eu = np.abs(y[gs] - y_ref), np.abs(u[xs] - u_ref)
            assert (ey <= 1e-12 * y_mag).all(), (name, p, order[p], "y", float((ey / np.maximum(y_mag, 1e-300)).max()))
            assert (eu <= 1e-12 * u_mag).all(), (name, p, order[p], "u", float((eu / np.maximum(u_mag, 1e-300)).max()))
            empty = np.bincount(A.indices, minlength=A.shape[1]) == 0
            assert not u[xs][empty].any() and not np.signbit(u[xs][empty]).any(), (name, p, "a column without entries is not an exact 0")
            empty_cols += int(empty.sum())
            worst_y = max(worst_y, float((ey / np.maximum(y_mag, 1e-300)).max()))
            worst_u = max(worst_u, float((eu / np.maximum(u_mag, 1e-300)).max()))
        print("%s weights: worst |y - ref| / sum|terms| %.2e, worst |u - ref| / sum|terms| %.2e, %d columns without entries"
              % (name, worst_y, worst_u, empty_cols))
        assert empty_cols > 0, "no column without entries: the exact-zero check is vacuous"


def test_rows_longer_than_a_tile_on_the_device():
    """The long-row form of the kernel (tile passes for y_r, the tiles again, a partial per entry) on the device: no structure
    the factory builds has a row of more than 2048 entries, so the handle is reserved with a tile of 48 entries, which makes
    every longer row of the first 40 ragged problems (C3's 60-entry rows, the 348-entry rows of the optimised timings, the wide
    structure whose v is gathered from memory) a block of its own, several tiles long.  Product and solve are held to the
    bounds of the tests above and below."""
    tile = 48
    cases, order, B, x = _ragged_batch(40)
    long_rows = sum(int((np.diff(B.structs[s].row_ptr) > tile).sum()) for s in order)
    longest = max(int(np.diff(B.structs[s].row_ptr).max()) for s in order)
    assert long_rows > 1000 and longest > 5 * tile and B.structs[order[3]].n > 6144
    B.ops.reserve_normal(tile_entries=tile)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.ops.reserve_normal()   # the tables exist, for another tile
    with pytest.raises(ta.TowrError, match="error -1"):
        JacBatch(B.structs, order[:2]).ops.reserve_normal(tile_entries=4096)
    jac, b, wa = B.linearise(x)
    jac_h, b_h, wa_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    X, G = int(B.xo[-1]), int(B.go[-1])
    rng = np.random.default_rng(32)
    v_h, w_h = rng.normal(size=X), rng.uniform(0.1, 3.0, size=G)
    As = [B.A(p, jac_h) for p in range(B.P)]
    for name, w in (("unit", None), ("random", dev(w_h))):
        wh = np.ones(G) if w is None else w_h
        y, u = B.normal(jac, dev(v_h), w)
        _, u_alone = B.normal(jac, dev(v_h), w, with_y=False)
        assert same_bits(u, u_alone)
        for p in range(B.P):
            A, absA = As[p], abs(As[p])
            xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
            y_ref, y_mag = A @ v_h[xs], absA @ np.abs(v_h[xs])
            u_ref, u_mag = A.T @ (wh[gs] * y_ref), absA.T @ (wh[gs] * y_mag)
            assert (np.abs(y[gs] - y_ref) <= 1e-12 * y_mag).all(), (name, p, order[p], "y")
            assert (np.abs(u[xs] - u_ref) <= 1e-12 * u_mag).all(), (name, p, order[p], "u")
            empty = np.bincount(A.indices, minlength=A.shape[1]) == 0
            assert not u[xs][empty].any() and not np.signbit(u[xs][empty]).any(), (name, p)
    mu_h = np.array([1e-2 * lam_max(As[p], wa_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    d, info = B.solve(jac, b, wa, dev(mu_h), kind="onepass")
    for p in range(B.P):
        go = slice(B.go[p], B.go[p + 1])
        check_step(As[p], b_h[go], wa_h[go], mu_h[p], d[B.xo[p]:B.xo[p + 1]], info[p], "tile %d, problem %d (struct %d)" % (tile, p, order[p]),
                   direct="dense" if As[p].shape[1] <= 1500 else "lu")


# ---------------------------------------------------------------- 2. the solve against a direct solve

def _baseline_problems(seed, weighting):
    """The inputs of tests/test_jac_lsq.py _baseline_solve: the five BASELINE cases at x_perturbed(seed) on the oracle's g and J."""
    cases = [make() for _, make in sorted(baseline_cases().items())]
    names = sorted(baseline_cases())
    B = JacBatch([c.S for c in cases], range(len(cases)))
    probs = []
    for c, name in zip(cases, names):
        out = c.P.eval(c.x_perturbed(seed))
        g, jv = out[0], out[3]
        lo, hi = c.S.bounds()
        A = csr(c.S, jv)
        r = viol(g, lo, hi)
        w0 = np.ones(c.S.m) if weighting == "unit" else row_weights(A)
        w = w0 * (r != 0)
        probs.append(dict(A=A, jv=jv, b=-r, w=w, mu=1e-2 * lam_max(A, w), name="%s seed %d W %s" % (name, seed, weighting)))
    return B, probs


@pytest.mark.parametrize("weighting", ["unit", "rown"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_onepass_solve_on_the_oracle_jacobian(seed, weighting):
    B, probs = _baseline_problems(seed, weighting)
    d, info = B.solve(dev(np.concatenate([q["jv"] for q in probs])), dev(np.concatenate([q["b"] for q in probs])),
                      dev(np.concatenate([q["w"] for q in probs])), dev([q["mu"] for q in probs]), kind="onepass")
    for p, q in enumerate(probs):   # every problem: none is left out
        true, err = check_step(q["A"], q["b"], q["w"], q["mu"], d[B.xo[p]:B.xo[p + 1]], info[p], "one-pass " + q["name"])
        print("  true residual %.2e, recurred %.2e, |d - dense| / |dense| %.2e" % (true, info[p, 1], err))


def test_onepass_solve_on_the_device_jacobian_of_a_ragged_batch():
    cases, order, B, x = _ragged_batch()
    jac, b, wa = B.linearise(x)
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    As = [B.A(p, jac_h) for p in range(B.P)]
    mu_h = np.array([1e-2 * lam_max(As[p], w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    assert (mu_h > 0).all()
    d, info = B.solve(jac, b, wa, dev(mu_h), kind="onepass")
    for p in range(B.P):
        go = slice(B.go[p], B.go[p + 1])
        check_step(As[p], b_h[go], w_h[go], mu_h[p], d[B.xo[p]:B.xo[p + 1]], info[p], "one-pass ragged problem %d (struct %d)" % (p, order[p]),
                   direct="dense" if As[p].shape[1] <= 1500 else "lu")


def test_onepass_scaled_step_against_a_direct_solve():
    """The scaled form against (J^T W J + mu C^-2) d = J^T W b, as test_scaled_step_against_a_direct_solve of
    tests/test_jac_scaled.py holds twr_jac_lsq_solve_scaled: in e = d / c, with mu = 1e-2 lambda_max(C J^T W J C)."""
    cases, order, B, x = _ragged_batch()
    jac, b, wa = B.linearise(x)
    q, c = B.col_scale(jac, wa)
    X = int(B.xo[-1])
    jac_h, b_h, w_h, q_h, c_h = (t.cpu().numpy() for t in (jac, b, wa, q, c))
    assert np.isfinite(c_h[:X]).all() and (c_h[:X] > 0).all()
    sample = range(B.P)   # every problem: none is left out
    mu_h = np.zeros(B.P)
    for p in sample:
        xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
        mu_h[p] = 1e-2 * lam_max((B.A(p, jac_h) @ sp.diags(c_h[xs])).tocsr(), w_h[gs])
    assert (mu_h > 0).all()
    d, info = B.solve(jac, b, wa, dev(mu_h), c, kind="onepass")
    assert np.isfinite(d).all() and (info[:, 3] != 2).all()
    zeros = 0
    for p in sample:
        xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
        A, bp, wp, cp, dp, mu = B.A(p, jac_h), b_h[gs], w_h[gs], c_h[xs], d[xs], mu_h[p]
        n = A.shape[1]
        rhs = A.T @ (wp * bp)
        msg = "one-pass scaled problem %d (struct %d): %d iterations, |s|/|s0| %.3e, status %d" % (p, order[p], info[p, 0], info[p, 1], info[p, 3])
        assert info[p, 3] == 0, msg
        assert 0 < info[p, 0] < ITERS, msg
        res = cp * (A.T @ (wp * (A @ dp))) + mu * dp / cp - cp * rhs
        true = np.linalg.norm(res) / np.linalg.norm(cp * rhs)
        assert true <= 2 * TOL, (msg, "true residual", true)
        AC = (A @ sp.diags(cp)).tocsr()
        Hs = (AC.T @ sp.diags(wp) @ AC + mu * sp.identity(n)).tocsc()
        ed = np.linalg.solve(Hs.toarray(), cp * rhs) if n <= 1500 else spl.splu(Hs).solve(cp * rhs)
        err = np.linalg.norm(dp / cp - ed) / np.linalg.norm(ed)
        assert err <= COND * 2 * TOL, (msg, "|e - direct| / |direct|", err)
        zero = q_h[xs] == 0
        assert not dp[zero].any(), (msg, "a column of norm 0 moved")
        zeros += int(zero.sum())
        print("%s; true residual %.2e, |e - direct| / |direct| %.2e" % (msg, true, err))
    assert zeros > 0


# ---------------------------------------------------------------- 3. agreement with CGLS at the LM cap

AGREE = {"C3_anymal_trot_K200": 5.76e-13, "C4_anymal_stairs_K200": 1.12e-13}   # scripts/onepass_cpu.py, see the docstring below


@pytest.mark.parametrize("name", sorted(AGREE))
def test_onepass_agrees_with_cgls_at_the_lm_cap(name):
    """iters = 60, tol = 1e-8, active-set weights, mu = 1e-2 lambda_max: the Levenberg-Marquardt setting of scripts/jac_lsq.py.
    64 problems at x_perturbed(0 .. 63): |d_onepass - d_cgls| / |d_cgls| per problem.

    The same difference between the two numpy restatements of the iterations on the CPU oracle's Jacobian at the same 64
    points (scripts/onepass_cpu.py; both stop after 46 - 47 iterations on C3 and 52 - 53 on the stairs, the same count at
    every point): at most 5.76e-13 on C3 (median 8.3e-14) and 1.12e-13 on the stairs (median 3.8e-14).  Allowed here: ten
    times that, for the device's other summation orders: 5.76e-12 on C3, 1.12e-12 on the stairs."""
    c = baseline_cases()[name]()
    n = 64
    B = JacBatch([c.S], [0] * n)
    x = dev(np.concatenate([c.x_perturbed(i) for i in range(n)]))
    jac, b, wa = B.linearise(x)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    mu = dev([1e-2 * lam_max(B.A(p, jac_h), w_h[B.go[p]:B.go[p + 1]]) for p in range(n)])
    d0, i0 = B.solve(jac, b, wa, mu, iters=60, tol=1e-8)
    d1, i1 = B.solve(jac, b, wa, mu, iters=60, tol=1e-8, kind="onepass")
    assert (i0[:, 3] != 2).all() and (i1[:, 3] != 2).all()
    diff = np.array([np.linalg.norm(d1[B.xo[p]:B.xo[p + 1]] - d0[B.xo[p]:B.xo[p + 1]]) / np.linalg.norm(d0[B.xo[p]:B.xo[p + 1]])
                     for p in range(n)])
    print("%s: |d_onepass - d_cgls| / |d_cgls| median %.2e, max %.2e (allowed %.2e); iterations cgls %d .. %d, one-pass %d .. %d"
          % (name, np.median(diff), diff.max(), 10 * AGREE[name], i0[:, 0].min(), i0[:, 0].max(), i1[:, 0].min(), i1[:, 0].max()))
    assert (diff <= 10 * AGREE[name]).all(), (diff.max(), int(diff.argmax()), i0[diff.argmax()], i1[diff.argmax()])


# ---------------------------------------------------------------- 4. the contract

def test_bits_do_not_depend_on_the_batch_the_call_the_stream_or_the_cap():
    torch, device, st = torch_ctx()
    c, B, x, g, jac, b, wa = c3_batch(512)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    lam = lam_max(B.A(0, jac_h), w_h[B.go[0]:B.go[1]])
    mu = dev(np.full(B.P, 1e-2 * lam))
    v = dev(np.random.default_rng(8).normal(size=int(B.xo[-1])))
    y1, u1 = B.normal(jac, v, wa)
    y2, u2 = B.normal(jac, v, wa)
    assert same_bits(y1, y2) and same_bits(u1, u2), "two products differ"
    _, cs = B.col_scale(jac, wa)
    for scale in (None, cs):
        d1, i1 = B.solve(jac, b, wa, mu, scale, kind="onepass")
        d2, i2 = B.solve(jac, b, wa, mu, scale, kind="onepass")
        assert same_bits(d1, d2) and same_bits(i1, i2), "two calls differ"
        assert (i1[:, 3] == 0).all() or scale is not None   # (mu is 1e-2 lambda_max of the unscaled matrix)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d3, i3 = B.solve(jac, b, wa, mu, scale, stream=side.cuda_stream, kind="onepass")
            y3, u3 = B.normal(jac, v, wa, stream=side.cuda_stream)
        assert same_bits(d1, d3) and same_bits(i1, i3) and same_bits(y1, y3) and same_bits(u1, u3), "another stream differs"
        one = JacBatch([c.S], [0])
        for p in (0, 201, 511):   # alone in a one-problem handle, its values copied to fresh buffers
            xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
            jp, bp, wp = jac[B.jo[p]:B.jo[p + 1]].clone(), b[gs].clone(), wa[gs].clone()
            do, io = one.solve(jp, bp, wp, mu[p:p + 1].clone(), None if scale is None else scale[xs].clone(), kind="onepass")
            assert same_bits(do, d1[xs]) and same_bits(io[0], i1[p]), p
            yo, uo = one.normal(jp, v[xs].clone(), wp)
            assert same_bits(yo, y1[gs]) and same_bits(uo, u1[xs]), p
    # mu from 1e-2 to 10 lambda_max: every problem converges, at different counts; a problem that has converged does not move
    # while the others go on
    P = 16
    S16 = JacBatch([c.S], [0] * P)
    mus = dev(lam * np.logspace(-2, 1, P))
    sl = lambda t, off: t[:int(off[P])]   # noqa: E731  (one structure: the first 16 problems are a batch of their own)
    args = (sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus)
    d200, i200 = S16.solve(*args, kind="onepass")
    assert (i200[:, 3] == 0).all() and (i200[:, 0] < ITERS).all() and len(set(i200[:, 0])) > 4, i200[:, 0]
    for k in sorted(set(int(v) for v in i200[:, 0])):
        dk, ik = S16.solve(*args, iters=k, kind="onepass")
        for p in np.nonzero(i200[:, 0] <= k)[0]:
            assert same_bits(dk[S16.xo[p]:S16.xo[p + 1]], d200[S16.xo[p]:S16.xo[p + 1]]) and same_bits(ik[p], i200[p]), (k, p)
        assert (ik[i200[:, 0] > k, 3] == 1).all() and (ik[i200[:, 0] > k, 0] == k).all()   # the others: the cap


def test_a_scale_of_ones_gives_the_bits_of_the_unscaled_onepass_solve():
    torch, device, st = torch_ctx()
    cases, order, B, x = _ragged_batch()
    jac, b, wa = B.linearise(x)
    q, _ = B.col_scale(jac, wa)
    q = q.cpu().numpy()
    mu = dev([1e-2 * max(q[B.xo[p]:B.xo[p + 1]].max(), 1e-300) for p in range(B.P)])   # any mu > 0 serves
    ones = torch.ones(int(B.xo[-1]), dtype=torch.float64, device=device)
    for w in (wa, None):
        for iters, tol in ((60, TOL), (7, 0.0)):
            d0, i0 = B.solve(jac, b, w, mu, None, iters=iters, tol=tol, kind="onepass")
            d1, i1 = B.solve(jac, b, w, mu, ones, iters=iters, tol=tol, kind="onepass")
            assert np.isfinite(d0).all() and (i0[:, 0] > 0).all()
            assert same_bits(d0, d1), "d differs"
            assert same_bits(i0, i1), "info differs"


def test_powers_of_two_on_the_columns_change_the_scaled_step_by_exactly_the_inverse_factors():
    """J' = J diag(2^j): every product, sum and quotient of the scaled iteration sees the same numbers (c' = c 2^-j exactly as
    long as no column is at the floor: rel_floor = 1e-200 leaves only the columns of norm 0 there, as in
    tests/test_jac_scaled.py), so d' 2^j = d bit for bit, and info bit for bit."""
    cases, order, B, x = _ragged_batch(12)
    jac, b, wa = B.linearise(x)
    X = int(B.xo[-1])
    j = np.random.default_rng(77).integers(-20, 21, size=X)
    f_h = np.ones(max(1, int(B.jo[-1])))
    for p in range(B.P):
        f_h[B.jo[p]:B.jo[p + 1]] = np.ldexp(1.0, j[B.xo[p]:B.xo[p + 1]])[B.structs[order[p]].col_idx]
    jac2 = jac * dev(f_h)   # exact: a power of two each
    two_j = np.ldexp(1.0, j)
    (q1, c1), (q2, c2) = B.col_scale(jac, wa, 1e-200), B.col_scale(jac2, wa, 1e-200)
    c1_h, c2_h = c1.cpu().numpy()[:X], c2.cpu().numpy()[:X]
    nz = q1.cpu().numpy()[:X] > 0
    assert same_bits(c2_h[nz] * two_j[nz], c1_h[nz]) and nz.sum() > 1000 and (~nz).sum() > 0
    mu = dev(np.full(B.P, 1e-2))   # in the scaled variables lambda_max is of the order of the active rows per column: any mu > 0
    for iters, tol in ((40, 1e-8), (9, 0.0)):
        d1, i1 = B.solve(jac, b, wa, mu, c1, iters=iters, tol=tol, kind="onepass")
        d2, i2 = B.solve(jac2, b, wa, mu, c2, iters=iters, tol=tol, kind="onepass")
        assert np.isfinite(d1).all() and (i1[:, 0] > 0).all() and (i1[:, 3] != 2).all()
        assert same_bits(i1, i2), "info differs"
        assert same_bits(d2[nz] * two_j[nz], d1[nz]), "the step in the new units is not the step times the inverse factors"
        assert not d1[~nz].any() and not d2[~nz].any()


def test_poison_stays_in_its_problem():
    cases, order, B, x = _ragged_batch(40)
    jac, b, wa = B.linearise(x)
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    X = int(B.xo[-1])
    _, c = B.col_scale(jac, wa)
    c_h = c.cpu().numpy()
    v_h = np.random.default_rng(4).normal(size=X)
    for scaled in (False, True):
        mu_h = np.array([1e-2 * lam_max((B.A(p, jac_h) @ sp.diags(c_h[B.xo[p]:B.xo[p + 1]])).tocsr() if scaled else B.A(p, jac_h),
                                         w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
        d0, i0 = B.solve(jac, b, wa, dev(mu_h), c if scaled else None, iters=60, kind="onepass")
        y0, u0 = B.normal(jac, dev(v_h), wa)
        assert np.isfinite(d0).all() and np.isfinite(i0).all() and (i0[:, 0] > 0).all() and np.isfinite(u0).all()
        bad = {5: ("jac", np.nan), 6: ("b", np.inf), 7: ("w", np.nan), 8: ("mu", -1.0), 9: ("mu", np.nan), 10: ("mu", np.inf),
               20: ("jac", np.inf), 21: ("b", np.nan), 22: ("w", np.inf), 23: ("mu", -np.inf)}
        if scaled:
            bad.update({11: ("c", np.nan), 12: ("c", 0.0), 13: ("c", -1.0), 14: ("c", np.inf), 24: ("c", -np.inf)})
        jb, bb, wb, mb, cb = jac_h.copy(), b_h.copy(), w_h.copy(), mu_h.copy(), c_h.copy()
        for p, (where, val) in bad.items():   # planted values only, on indices that hold finite numbers
            if where == "mu":
                mb[p] = val
            else:
                arr, off = {"jac": (jb, B.jo), "b": (bb, B.go), "w": (wb, B.go), "c": (cb, B.xo)}[where]
                arr[off[p]:off[p + 1]:3] = val
        d1, i1 = B.solve(dev(jb), dev(bb), dev(wb), dev(mb), dev(cb) if scaled else None, iters=60, kind="onepass")
        y1, u1 = B.normal(dev(jb), dev(v_h), dev(wb))
        for p in range(B.P):
            xs, gs = slice(B.xo[p], B.xo[p + 1]), slice(B.go[p], B.go[p + 1])
            if p not in bad:
                assert same_bits(d1[xs], d0[xs]) and same_bits(i1[p], i0[p]), (scaled, p)
            elif bad[p][0] in ("mu", "c"):
                assert i1[p, 3] == 2 and i1[p, 0] == 0 and not d1[xs].any(), (scaled, p, i1[p])
            else:
                assert i1[p, 3] == 2 or not np.isfinite(d1[xs]).all(), (scaled, p, i1[p])
            if p not in bad or bad[p][0] not in ("jac", "w"):   # the product reads J, v and w only
                assert same_bits(y1[gs], y0[gs]) and same_bits(u1[xs], u0[xs]), (scaled, p)
            else:
                assert not np.isfinite(u1[xs]).all(), (scaled, p)


def test_edge_cases():
    torch, device, st = torch_ctx()
    # a structure without rows: u = 0, no y; d = 0, status 0, no iterations
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    B = JacBatch([case.S], [0, 0, 0])
    one = torch.zeros(8, dtype=torch.float64, device=device)
    v = torch.ones(int(B.xo[-1]), dtype=torch.float64, device=device)
    _, u = B.normal(one, v, None)
    assert not u.any() and not np.signbit(u).any()
    for c in (None, v):
        d, info = B.solve(one, one, None, dev([0.0, 1.0, 2.0]), c, kind="onepass")
        assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 0).all() and not info[:, 1:3].any()
    # b = 0: the same, no 0 / 0
    c, B, x, g, jac, b, wa = c3_batch(3)
    lam = lam_max(B.A(0, jac.cpu().numpy()), wa.cpu().numpy()[B.go[0]:B.go[1]])
    mu = dev(np.full(3, 1e-2 * lam))
    bz = b.clone()
    bz[B.go[1]:B.go[2]] = 0.0
    d, info = B.solve(jac, bz, wa, mu, kind="onepass")
    assert not d[B.xo[1]:B.xo[2]].any() and np.array_equal(info[1], [0, 0, 0, 0]) and (info[[0, 2], 3] == 0).all()
    dref, iref = B.solve(jac, b, wa, mu, kind="onepass")
    assert same_bits(d[B.xo[0]:B.xo[1]], dref[B.xo[0]:B.xo[1]]) and same_bits(d[B.xo[2]:], dref[B.xo[2]:])
    # iters = 0: zeros and |s0|
    d, info = B.solve(jac, b, wa, mu, iters=0, kind="onepass")
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 1).all() and (info[:, 1] == 1).all()
    assert same_bits(info[:, 2], iref[:, 2])
    # w NULL is w = 1
    ones = torch.ones_like(b)
    dn, inn = B.solve(jac, b, None, mu, iters=30, kind="onepass")
    d1, i1 = B.solve(jac, b, ones, mu, iters=30, kind="onepass")
    assert same_bits(dn, d1) and same_bits(inn, i1) and (inn[:, 0] == 30).all()
    # tol >= 1 stops at once; tol = 0 runs to the cap
    d, info = B.solve(jac, b, wa, mu, iters=5, tol=1.0, kind="onepass")
    assert not d.any() and (info[:, 3] == 0).all() and (info[:, 0] == 0).all()
    d, info = B.solve(jac, b, wa, mu, iters=5, tol=0.0, kind="onepass")
    assert (info[:, 3] == 1).all() and (info[:, 0] == 5).all()
    # mu < 0: bad input, d = 0
    d, info = B.solve(jac, b, wa, dev([1e-2 * lam, -1.0, 1e-2 * lam]), kind="onepass")
    assert info[1, 3] == 2 and info[1, 0] == 0 and not d[B.xo[1]:B.xo[2]].any() and (info[[0, 2], 3] == 0).all()
    # NULL and misaligned buffers, negative iters, a NaN tol
    out = torch.zeros(4 * 3, dtype=torch.float64, device=device)
    dd = torch.zeros(int(B.xo[-1]), dtype=torch.float64, device=device)
    yy = torch.zeros(int(B.go[-1]), dtype=torch.float64, device=device)
    a = (jac.data_ptr(), b.data_ptr(), mu.data_ptr(), dd.data_ptr(), out.data_ptr())
    for i in range(5):
        for badptr in (0, a[i] + 4):
            args = list(a)
            args[i] = badptr
            with pytest.raises(ta.TowrError, match="error -1"):
                B.lsq.solve_onepass_device(*args, 10, TOL, stream=st)
    for kw in (dict(d_w=wa.data_ptr() + 4), dict(d_scale=dd.data_ptr() + 4)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.lsq.solve_onepass_device(*a, 10, TOL, stream=st, **kw)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_onepass_device(*a, -1, TOL, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_onepass_device(*a, 10, float("nan"), stream=st)
    n = (jac.data_ptr(), dd.data_ptr(), dd.data_ptr())   # (jac, v, u)
    for i in range(3):
        for badptr in (0, n[i] + 4):
            args = list(n)
            args[i] = badptr
            with pytest.raises(ta.TowrError, match="error -1"):
                B.ops.normal_mul_device(*args, stream=st)
    for kw in (dict(d_w=wa.data_ptr() + 4), dict(d_y=yy.data_ptr() + 4)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.ops.normal_mul_device(*n, stream=st, **kw)
    torch.cuda.synchronize()
    # a handle made for other structures than its products handle
    other = ta.JacOps([c.S], [0, 0], device=0)   # two problems, a handle asked for three
    other.struct_of_problem = np.zeros(3, dtype=np.int32)
    other.n_problems = 3
    with pytest.raises(ta.TowrError, match="error -1"):
        ta.JacLsq(other)
    hop = baseline_cases()["C1_hopper"]().S
    mixed = ta.JacOps([c.S, hop], [0, 1], device=0)   # the same count, another problem's n / m
    mixed.struct_of_problem = np.zeros(2, dtype=np.int32)
    with pytest.raises(ta.TowrError, match="error -1"):
        ta.JacLsq(mixed)


def test_bytes_grow_only_with_a_reserve_or_a_onepass_call():
    torch, device, st = torch_ctx()
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    S, n = c.S, 8
    B, ref = JacBatch([S], [0] * n), JacBatch([S], [0] * n)
    ops0, lsq0 = B.ops.bytes()["resident"], B.lsq.bytes()["resident"]
    x = dev(np.concatenate([c.x_perturbed(i) for i in range(n)]))
    jac, b, wa = B.linearise(x)
    mu = dev(np.full(n, 50.0))
    B.solve(jac, b, wa, mu, iters=3)
    v = dev(np.ones(int(B.xo[-1])))
    z = nan(B.xo[-1])
    B.ops.tmul_device(jac.data_ptr(), b.data_ptr(), z.data_ptr(), st)
    torch.cuda.synchronize()
    assert B.ops.bytes()["resident"] == ops0 and B.lsq.bytes()["resident"] == lsq0, "the existing calls changed what the handles hold"
    B.ops.reserve_normal()
    ops1 = B.ops.bytes()["resident"]
    assert ops1 > ops0 and B.lsq.bytes()["resident"] == lsq0
    B.ops.reserve_normal()
    B.normal(jac, v, wa)
    assert B.ops.bytes()["resident"] == ops1, "the one-pass tables are made once"
    B.solve(jac, b, wa, mu, iters=3, kind="onepass")
    lsq1 = B.lsq.bytes()["resident"]
    assert lsq1 == lsq0 + 8 * 2 * S.n * n and B.ops.bytes()["resident"] == ops1   # s and u in the x layout
    B.solve(jac, b, wa, mu, v, iters=3, kind="onepass")
    assert B.lsq.bytes()["resident"] == lsq1 + 8 * 2 * S.n * n   # the scaled solve's e and c o p
    # a handle that only ever makes the one-pass calls reserves by itself, and ends up holding the same
    ref.solve(jac, b, wa, mu, v, iters=3, kind="onepass")
    assert ref.ops.bytes()["resident"] == ops1 and ref.lsq.bytes()["resident"] == B.lsq.bytes()["resident"]


# ---------------------------------------------------------------- 5. hipGraph

def test_capture_eval_violation_onepass_solve_update_scores_as_one_graph():
    torch, device, _ = torch_ctx()
    cases, order = ragged()
    order = order[:24]
    B = JacBatch([c.S for c in cases], order)
    X, G, J = int(B.xo[-1]), int(B.go[-1]), int(B.jo[-1])
    x = dev(ragged_x(cases, order))
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device=device)   # noqa: E731
    g, jac, r, b, wa, merit, d, info, scores = z64(G), z64(J), z64(G), z64(G), z64(G), z64(B.P), z64(X), z64(4 * B.P), z64(16 * B.P)
    mu = dev(np.full(B.P, 50.0))
    outs = (g, jac, r, b, wa, merit, d, info, scores)
    B.ops.reserve_normal()
    B.lsq.reserve_onepass()

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, stream)
        B.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=stream)
        torch.neg(r, out=b)
        B.lsq.solve_onepass_device(jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), 25, 1e-6, d_w=wa.data_ptr(),
                                   stream=stream)
        x.add_(d)
        B.batch.eval_scores_device(x.data_ptr(), scores.data_ptr(), d_g=g.data_ptr(), stream=stream)

    graph = capture(step)
    x1 = ragged_x(cases, order, seed0=100)

    def reset():
        x.copy_(torch.from_numpy(x1))
        for t in outs:
            t.zero_()

    assert_replay_equals_eager(step, graph, reset, outs + (x,))
    assert info.cpu().numpy().reshape(-1, 4)[:, 0].max() > 3 and d.abs().max().item() > 0
    assert not torch.equal(x, torch.from_numpy(x1).to(device))


# ---------------------------------------------------------------- 6. a full C3 batch

def test_c3_full_batch():
    torch, device, st = torch_ctx()
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    S = c.S
    n = 8192
    B = JacBatch([S], [0] * n)
    gen = torch.Generator(device=device)
    gen.manual_seed(5)
    x0 = dev(c.x_guess())
    scale = dev((c.x_perturbed(0) - c.x_guess()) / np.random.default_rng(1234).normal(size=S.n))   # 0.05 * the per-variable scale
    x = (x0[None, :] + scale[None, :] * torch.randn((n, S.n), generator=gen, dtype=torch.float64, device=device)).reshape(-1).contiguous()
    jac, b, wa = B.linearise(x)
    lam = lam_max(csr(S, jac[:S.nnz].cpu().numpy()), wa[:S.m].cpu().numpy())
    mu = dev(np.full(n, 1e-2 * lam))
    d, info = B.solve(jac, b, wa, mu, iters=20, kind="onepass")
    assert np.isfinite(d).all() and np.isfinite(info).all()
    assert np.isin(info[:, 3], (0, 1)).all() and (info[:, 0] == 20).all()
    dc, _ = B.solve(jac, b, wa, mu, iters=20)
    for p in (0, 4095, 8191):   # 20 iterations of CGLS on the device: the same iterates up to rounding (the bound of tests/test_jac_lsq.py)
        xs = slice(B.xo[p], B.xo[p + 1])
        assert np.linalg.norm(d[xs] - dc[xs]) <= 20 * 101 * 4.3e-13 * np.linalg.norm(dc[xs]), p
    _, cs = B.col_scale(jac, wa)
    d, info = B.solve(jac, b, wa, dev(np.full(n, 1e-2)), cs, iters=20, kind="onepass")
    assert np.isfinite(d).all() and np.isfinite(info).all() and np.isin(info[:, 3], (0, 1)).all()
