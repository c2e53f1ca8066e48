"""twr_jac_violation / twr_jac_dot / twr_jac_lsq_solve on the device against float64 numpy / scipy on the CPU: the residual bit
for bit, the damped weighted least-squares step against a dense (or sparse LU) solve of the normal equations on the oracle's
Jacobian and on the device's own, the step's effect on the oracle's merit, bit-reproducibility across batches, calls and
iteration caps, containment of NaN / Inf and bad mu, the edge cases, hipGraph capture and a full C3 batch.

The bounds of the solve tests, with tol = 1e-10 and mu = 1e-2 lambda_max(J^T W J):
  * true relative normal-equation residual of the returned d <= 2 tol (numpy's restatement of the iteration stops with recurrence
    and true residual agreeing to three digits; the factor 2 is for the device's other summation order);
  * |d - d_direct| <= cond(H) 2 tol |d_direct| with cond(H) <= (lambda_max + mu) / mu = 101;
  * iterations under the cap of 200 (CG on cond 101 contracts by (sqrt(101) - 1) / (sqrt(101) + 1) = 0.819 per iteration:
    2 0.819^k sqrt(101) <= 1e-10 from k = 131)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case

pytestmark = pytest.mark.gpu

TOL, ITERS, COND = 1e-10, 200, 101.0


def _torch():
    import torch

    return torch, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def _csr(S, vals):
    return sp.csr_matrix((vals, S.col_idx, S.row_ptr), shape=(S.m, S.n))


def _viol(g, lo, hi):
    return g - np.clip(g, lo, hi)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _cgls(A, b, w, mu, iters, tol):
    """The iteration of twr_jac_lsq_solve restated in numpy (iterations, d, |s| / |s0|)."""
    d = np.zeros(A.shape[1])
    r = b.copy()
    s = A.T @ (w * r)
    p = s.copy()
    gam = g0 = s @ s
    k = 0
    while k < iters and not gam <= tol * tol * g0:
        q = A @ p
        alpha = gam / (q @ (w * q) + mu * (p @ p))
        d += alpha * p
        r -= alpha * q
        s = A.T @ (w * r) - mu * d
        gn = s @ s
        p = s + (gn / gam) * p
        gam = gn
        k += 1
    return k, d, np.sqrt(gam / g0) if g0 > 0 else 0.0


def _lam_max(A, w):
    """lambda_max(J^T W J) on the CPU; 0 for a problem without active rows."""
    if not np.any(w):
        return 0.0
    return float(spl.svds(sp.diags(np.sqrt(w)) @ A, k=1, return_singular_vectors=False)[0] ** 2)


def _row_weights(A):
    rown = np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
    return 1.0 / np.maximum(rown, 1e-12) ** 2


def _dev(a):
    torch, dev, _ = _torch()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _solve(lsq, jac, b, w, mu, iters=ITERS, tol=TOL, stream=None):
    """(d, info[n_problems, 4]) of one solve on device tensors (w None: unit weights); d / info start as NaN."""
    torch, dev, st = _torch()
    xo, _, _ = lsq.ops.layout()
    d = torch.full((int(xo[-1]),), float("nan"), dtype=torch.float64, device=dev)
    info = torch.full((4 * lsq.n_problems,), float("nan"), dtype=torch.float64, device=dev)
    lsq.solve_device(jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, tol,
                     d_w=0 if w is None else w.data_ptr(), stream=st if stream is None else stream)
    torch.cuda.synchronize()
    return d.cpu().numpy(), info.cpu().numpy().reshape(-1, 4)


def _s0_bound(A, w, b):
    """Rounding of |J^T (w o b)| summed in another order: 1e-12 of the terms' magnitudes per component (the tolerance of the
    products' own test), over n components."""
    return 1e-12 * np.sqrt(A.shape[1]) * np.linalg.norm(abs(A).T @ np.abs(w * b))


def _check_step(A, b, w, mu, d, info, what, direct="dense"):
    """One problem's d and info against the normal equations solved directly on the CPU."""
    n = A.shape[1]
    rhs = A.T @ (w * b)
    k_np, _, rel_np = _cgls(A, b, w, mu, ITERS, TOL)
    msg = "%s: device %d iterations, |s|/|s0| %.3e, status %d; numpy %d iterations, %.3e" % (what, info[0], info[1], info[3], k_np, rel_np)
    print(msg)
    assert info[3] == 0, msg
    assert 0 < info[0] < ITERS, msg
    Hs = (A.T @ sp.diags(w) @ A + mu * sp.identity(n)).tocsc()
    true = np.linalg.norm(Hs @ d - rhs) / np.linalg.norm(rhs)
    assert true <= 2 * TOL, (msg, "true residual", true)
    assert abs(info[2] - np.linalg.norm(rhs)) <= _s0_bound(A, w, b), (msg, "|s0|")
    dd = np.linalg.solve(Hs.toarray(), rhs) if direct == "dense" else spl.splu(Hs).solve(rhs)
    err = np.linalg.norm(d - dd) / np.linalg.norm(dd)
    assert err <= COND * 2 * TOL, (msg, "|d - direct| / |direct|", err)
    return true, err


# ---------------------------------------------------------------- batches

def _ragged():
    """About 300 problems of quadruped structures: random ones, optimised timings, a grid map, one too wide for the LDS copy of
    s; struct 0 is C3."""
    cases = [Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200)),
             Case("anymal", "gap", ta.gait_combo(4, 0, 2.4, 0.9), constraint_sets=127),
             Case("anymal", "grid_map", ta.gait_combo(4, 1, 2.0),
                  grid=(np.random.default_rng(3).uniform(-0.05, 0.3, size=(40, 30)).astype(np.float32), 0.06, (0.8, -0.2))),
             Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), duration_base_poly=0.003)]
    assert cases[3].S.n > 6144
    seed = 0
    while len(cases) < 8:
        c = random_case(seed)
        if c.S.n_ee == 4:
            cases.append(c)
        seed += 1
    order = [0, 1, 2, 3] + list(np.random.default_rng(5).integers(0, len(cases), size=296))
    return cases, order


class _Batch:
    """Batch + JacOps + JacLsq of the same arguments, and the host copies of the structures' bounds in the g layout."""

    def __init__(self, structs, order):
        self.structs, self.order = structs, list(order)
        self._batch = None
        self.ops = ta.JacOps(structs, self.order, device=0)
        self.lsq = ta.JacLsq(self.ops)
        self.xo, self.go, self.jo = self.ops.layout()
        b = [structs[s].bounds() for s in self.order]
        self.lo = np.concatenate([v[0] for v in b]) if self.go[-1] else np.zeros(0)
        self.hi = np.concatenate([v[1] for v in b]) if self.go[-1] else np.zeros(0)
        self.P = len(self.order)

    @property
    def batch(self):
        if self._batch is None:
            self._batch = ta.Batch(self.structs, self.order, device=0)
        return self._batch

    def eval(self, x, flags=None):
        torch, dev, st = _torch()
        g = torch.empty(max(1, int(self.go[-1])), dtype=torch.float64, device=dev)
        jac = torch.empty(max(1, int(self.jo[-1])), dtype=torch.float64, device=dev)
        self.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH if flags is None else flags, st)
        torch.cuda.synchronize()
        return g, jac

    def violation(self, g, w=None):
        torch, dev, st = _torch()
        G = max(1, int(self.go[-1]))
        r = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
        wa = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
        merit = torch.full((self.P,), float("nan"), dtype=torch.float64, device=dev)
        self.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w=0 if w is None else w.data_ptr(), d_w_active=wa.data_ptr(),
                                  d_merit=merit.data_ptr(), stream=st)
        torch.cuda.synchronize()
        return r, wa, merit

    def A(self, p, jac_h):
        return _csr(self.structs[self.order[p]], jac_h[self.jo[p]:self.jo[p + 1]])


# ---------------------------------------------------------------- 1. violation and dot

@pytest.mark.parametrize("point", ["x_perturbed", "x_wild"])
def test_violation_and_dot_on_a_ragged_batch(point):
    torch, dev, st = _torch()
    cases, order = _ragged()
    B = _Batch([c.S for c in cases], order)
    x = _dev(np.concatenate([getattr(cases[s], point)(i) for i, s in enumerate(order)]))
    g, _ = B.eval(x, ta.EVAL_VALUES)
    G = int(B.go[-1])
    rng = np.random.default_rng(21)
    w_h = rng.uniform(0.1, 3.0, size=G)
    g_h = g.cpu().numpy()[:G].copy()
    g_h[[5, int(B.go[7]) + 3, G - 1]] = np.nan   # a NaN g_i gives a NaN r_i, as numpy's clip does
    g_h[int(B.go[9]) + 1] = np.inf
    g = _dev(g_h)
    with np.errstate(invalid="ignore"):
        ref = _viol(g_h, B.lo, B.hi)
    assert np.isnan(ref[5]) and (ref != 0).sum() > G // 100
    for w in (None, _dev(w_h)):
        wh = np.ones(G) if w is None else w_h
        r, wa, merit = B.violation(g, w)
        r, wa, merit = r.cpu().numpy()[:G], wa.cpu().numpy()[:G], merit.cpu().numpy()
        fin = ~np.isnan(ref)
        assert np.array_equal(np.isnan(r), ~fin) and np.array_equal(_bits(r[fin]), _bits(ref[fin])), "r is not g - clip(g) bit for bit"
        assert np.array_equal(_bits(wa), _bits(wh * (ref != 0))), "w_active is not w [r != 0] bit for bit"
        for p in range(B.P):
            t = 0.5 * wh[B.go[p]:B.go[p + 1]] * ref[B.go[p]:B.go[p + 1]] ** 2
            if not np.isfinite(t).all():   # the planted NaN / Inf: the same non-number
                assert np.array_equal(merit[p], t.sum(), equal_nan=True), p
            else:
                assert abs(merit[p] - t.sum()) <= 1e-12 * np.abs(t).sum(), (p, merit[p], t.sum())
    # r alone: the optional outputs left out
    r2 = torch.full((G,), float("nan"), dtype=torch.float64, device=dev)
    B.lsq.violation_device(g.data_ptr(), r2.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert _same_bits(r2.cpu().numpy()[fin], ref[fin])
    # |r| is the per-row quantity twr_batch_score reduces: the inf-norm of a clean problem's r is the largest of its scores
    scores = torch.zeros(16 * B.P, dtype=torch.float64, device=dev)
    B.batch.score_device(g.data_ptr(), scores.data_ptr(), st)
    torch.cuda.synchronize()
    sc = scores.cpu().numpy().reshape(B.P, 8, 2)
    for p in (1, 2, 3, 50, 150):   # (problems whose g holds no planted NaN / Inf)
        assert np.abs(ref[B.go[p]:B.go[p + 1]]).max() == sc[p, :, 0].max(), p
    # dot over both layouts
    for space, off in ((B.lsq.X, B.xo), (B.lsq.G, B.go)):
        a_h, b_h = rng.normal(size=int(off[-1])), rng.normal(size=int(off[-1]))
        out = torch.full((B.P,), float("nan"), dtype=torch.float64, device=dev)
        a, b = _dev(a_h), _dev(b_h)
        B.lsq.dot_device(space, a.data_ptr(), b.data_ptr(), out.data_ptr(), st)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        for p in range(B.P):
            t = a_h[off[p]:off[p + 1]] * b_h[off[p]:off[p + 1]]
            assert abs(out[p] - t.sum()) <= 1e-12 * np.abs(t).sum(), (space, p)


# ---------------------------------------------------------------- 2. + 4. the oracle's Jacobian

@functools.lru_cache(maxsize=None)
def _baseline_solve(seed, weighting):
    """The five BASELINE cases in one handle at x_perturbed(seed): oracle g and J, b = -viol, active-set weights."""
    cases = [make() for _, make in sorted(baseline_cases().items())]
    names = sorted(baseline_cases())
    B = _Batch([c.S for c in cases], range(len(cases)))
    probs = []
    for c in cases:
        x = c.x_perturbed(seed)
        out = c.P.eval(x)
        g, jv = out[0], out[3]
        lo, hi = c.S.bounds()
        A = _csr(c.S, jv)
        r = _viol(g, lo, hi)
        w0 = np.ones(c.S.m) if weighting == "unit" else _row_weights(A)
        w = w0 * (r != 0)
        probs.append(dict(case=c, x=x, A=A, jv=jv, r=r, b=-r, w0=w0, w=w, mu=1e-2 * _lam_max(A, w), lo=lo, hi=hi))
    d, info = _solve(B.lsq, _dev(np.concatenate([q["jv"] for q in probs])), _dev(np.concatenate([q["b"] for q in probs])),
                     _dev(np.concatenate([q["w"] for q in probs])), _dev([q["mu"] for q in probs]))
    for p, q in enumerate(probs):
        q["d"], q["info"], q["name"] = d[B.xo[p]:B.xo[p + 1]], info[p], "%s seed %d W %s" % (names[p], seed, weighting)
    return probs


@pytest.mark.parametrize("weighting", ["unit", "rown"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solve_on_the_oracle_jacobian(seed, weighting):
    for q in _baseline_solve(seed, weighting):   # every problem: none is left out
        true, err = _check_step(q["A"], q["b"], q["w"], q["mu"], q["d"], q["info"], q["name"])
        print("  true residual %.2e, |d - dense| / |dense| %.2e" % (true, err))


@pytest.mark.parametrize("weighting", ["unit", "rown"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_step_reduces_the_oracle_merit(seed, weighting):
    for q in _baseline_solve(seed, weighting):
        g2 = q["case"].P.eval(q["x"] + q["d"])[0]
        r2 = _viol(g2, q["lo"], q["hi"])
        before, after = 0.5 * q["r"] @ (q["w0"] * q["r"]), 0.5 * r2 @ (q["w0"] * r2)
        print("%s: merit %.4e -> %.4e, ratio %.3f" % (q["name"], before, after, after / before))
        assert after < before, q["name"]


# ---------------------------------------------------------------- 3. the device's own Jacobian

def test_solve_on_the_device_jacobian_of_a_ragged_batch():
    torch, dev, st = _torch()
    cases, order = _ragged()
    B = _Batch([c.S for c in cases], order)
    x = _dev(np.concatenate([cases[s].x_perturbed(i) for i, s in enumerate(order)]))
    g, jac = B.eval(x)
    r, wa, _ = B.violation(g)
    b = -r
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    As = [B.A(p, jac_h) for p in range(B.P)]
    mu_h = np.array([1e-2 * _lam_max(As[p], w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    assert (mu_h > 0).all()
    d, info = _solve(B.lsq, jac, b, wa, _dev(mu_h))
    for p in range(B.P):
        go = slice(B.go[p], B.go[p + 1])
        _check_step(As[p], b_h[go], w_h[go], mu_h[p], d[B.xo[p]:B.xo[p + 1]], info[p], "ragged problem %d (struct %d)" % (p, order[p]),
                    direct="dense" if As[p].shape[1] <= 1500 else "lu")


# ---------------------------------------------------------------- 5. bit-reproducibility

def _c3_batch(n, seed0=0):
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    B = _Batch([c.S], [0] * n)
    x = _dev(np.concatenate([c.x_perturbed(seed0 + i) for i in range(n)]))
    g, jac = B.eval(x)
    r, wa, _ = B.violation(g)
    return c, B, x, g, jac, -r, wa


def test_bits_do_not_depend_on_the_batch_the_call_or_the_cap():
    torch, dev, st = _torch()
    c, B, x, g, jac, b, wa = _c3_batch(512)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    lam = _lam_max(B.A(0, jac_h), w_h[B.go[0]:B.go[1]])
    mu = _dev(np.full(B.P, 1e-2 * lam))
    d1, i1 = _solve(B.lsq, jac, b, wa, mu)
    d2, i2 = _solve(B.lsq, jac, b, wa, mu)
    assert _same_bits(d1, d2) and _same_bits(i1, i2), "two calls differ"
    assert (i1[:, 3] == 0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d3, i3 = _solve(B.lsq, jac, b, wa, mu, stream=side.cuda_stream)
    assert _same_bits(d1, d3) and _same_bits(i1, i3), "another stream differs"
    one = _Batch([c.S], [0])
    for p in (0, 201, 511):   # alone in a one-problem handle, its values copied to fresh buffers
        do, io = _solve(one.lsq, jac[B.jo[p]:B.jo[p + 1]].clone(), b[B.go[p]:B.go[p + 1]].clone(), wa[B.go[p]:B.go[p + 1]].clone(),
                        mu[p:p + 1].clone())
        assert _same_bits(do, d1[B.xo[p]:B.xo[p + 1]]) and _same_bits(io[0], i1[p]), p
    # mu from 1e-2 to 10 lambda_max: cond <= 101, every problem converges, at different counts; a problem that has converged
    # does not move while the others go on
    P = 16
    S16 = _Batch([c.S], [0] * P)
    mus = _dev(lam * np.logspace(-2, 1, P))
    sl = lambda t, off: t[:int(off[P])]   # noqa: E731  (one structure: the first 16 problems are a batch of their own)
    d200, i200 = _solve(S16.lsq, sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus)
    assert (i200[:, 3] == 0).all() and (i200[:, 0] < ITERS).all() and len(set(i200[:, 0])) > 4, i200[:, 0]
    for k in sorted(set(int(v) for v in i200[:, 0])):
        dk, ik = _solve(S16.lsq, sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus, iters=k)
        for p in np.nonzero(i200[:, 0] <= k)[0]:
            assert _same_bits(dk[S16.xo[p]:S16.xo[p + 1]], d200[S16.xo[p]:S16.xo[p + 1]]) and _same_bits(ik[p], i200[p]), (k, p)
        assert (ik[i200[:, 0] > k, 3] == 1).all() and (ik[i200[:, 0] > k, 0] == k).all()   # the others: the cap


# ---------------------------------------------------------------- 6. containment and edge cases

def test_poison_stays_in_its_problem():
    torch, dev, st = _torch()
    cases, order = _ragged()
    order = order[:40]
    B = _Batch([c.S for c in cases], order)
    x = _dev(np.concatenate([cases[s].x_perturbed(i) for i, s in enumerate(order)]))
    g, jac = B.eval(x)
    r, wa, _ = B.violation(g)
    b = -r
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    mu_h = np.array([1e-2 * _lam_max(B.A(p, jac_h), w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    d0, i0 = _solve(B.lsq, jac, b, wa, _dev(mu_h), iters=60)
    assert np.isfinite(d0).all() and np.isfinite(i0).all()
    bad = {5: ("jac", np.nan), 6: ("b", np.inf), 7: ("w", np.nan), 8: ("mu", -1.0), 9: ("mu", np.nan), 10: ("mu", np.inf),
           20: ("jac", np.inf), 21: ("b", np.nan), 22: ("w", np.inf), 23: ("mu", -np.inf)}
    jb, bb, wb, mb = jac_h.copy(), b_h.copy(), w_h.copy(), mu_h.copy()
    for p, (where, val) in bad.items():
        if where == "mu":
            mb[p] = val
        else:
            arr, off = {"jac": (jb, B.jo), "b": (bb, B.go), "w": (wb, B.go)}[where]
            arr[off[p]:off[p + 1]:3] = val
    d1, i1 = _solve(B.lsq, _dev(jb), _dev(bb), _dev(wb), _dev(mb), iters=60)
    for p in range(B.P):
        dp = d1[B.xo[p]:B.xo[p + 1]]
        if p not in bad:
            assert _same_bits(dp, d0[B.xo[p]:B.xo[p + 1]]) and _same_bits(i1[p], i0[p]), p
        elif bad[p][0] == "mu":
            assert i1[p, 3] == 2 and i1[p, 0] == 0 and not dp.any(), (p, i1[p])
        else:
            assert i1[p, 3] == 2 or not np.isfinite(dp).all(), (p, i1[p])


def test_edge_cases():
    torch, dev, st = _torch()
    # a structure without rows: d = 0, status 0, no iterations
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    B = _Batch([case.S], [0, 0, 0])
    one = torch.zeros(8, dtype=torch.float64, device=dev)
    d, info = _solve(B.lsq, one, one, None, _dev([0.0, 1.0, 2.0]))
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 0).all() and not info[:, 1:3].any()
    # b = 0: the same, no 0 / 0
    c, B, x, g, jac, b, wa = _c3_batch(3)
    lam = _lam_max(B.A(0, jac.cpu().numpy()), wa.cpu().numpy()[B.go[0]:B.go[1]])
    mu = _dev(np.full(3, 1e-2 * lam))
    bz = b.clone()
    bz[B.go[1]:B.go[2]] = 0.0
    d, info = _solve(B.lsq, jac, bz, wa, mu)
    assert not d[B.xo[1]:B.xo[2]].any() and np.array_equal(info[1], [0, 0, 0, 0]) and (info[[0, 2], 3] == 0).all()
    dref, iref = _solve(B.lsq, jac, b, wa, mu)
    assert _same_bits(d[B.xo[0]:B.xo[1]], dref[B.xo[0]:B.xo[1]]) and _same_bits(d[B.xo[2]:], dref[B.xo[2]:])
    # iters = 0: zeros and |s0|
    d, info = _solve(B.lsq, jac, b, wa, mu, iters=0)
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 1).all() and (info[:, 1] == 1).all()
    assert _same_bits(info[:, 2], iref[:, 2])
    jac_h, w_h, b_h = jac.cpu().numpy(), wa.cpu().numpy(), b.cpu().numpy()
    for p in range(3):
        A, go = B.A(p, jac_h), slice(B.go[p], B.go[p + 1])
        assert abs(info[p, 2] - np.linalg.norm(A.T @ (w_h[go] * b_h[go]))) <= _s0_bound(A, w_h[go], b_h[go]), p
    # w NULL is w = 1
    ones = torch.ones_like(b)
    dn, inn = _solve(B.lsq, jac, b, None, mu, iters=30)
    d1, i1 = _solve(B.lsq, jac, b, ones, mu, iters=30)
    assert _same_bits(dn, d1) and _same_bits(inn, i1) and (inn[:, 0] == 30).all()
    # tol >= 1 stops at once; tol = 0 runs to the cap
    d, info = _solve(B.lsq, jac, b, wa, mu, iters=5, tol=1.0)
    assert not d.any() and (info[:, 3] == 0).all() and (info[:, 0] == 0).all()
    d, info = _solve(B.lsq, jac, b, wa, mu, iters=5, tol=0.0)
    assert (info[:, 3] == 1).all() and (info[:, 0] == 5).all()
    # NULL and misaligned buffers, a bad space, negative iters, another batch's structures
    out = torch.zeros(4 * 3, dtype=torch.float64, device=dev)
    dd = torch.zeros(int(B.xo[-1]), dtype=torch.float64, device=dev)
    a = (jac.data_ptr(), b.data_ptr(), mu.data_ptr(), dd.data_ptr(), out.data_ptr())
    for i in range(5):
        for badptr in (0, a[i] + 4):
            args = list(a)
            args[i] = badptr
            with pytest.raises(ta.TowrError, match="error -1"):
                B.lsq.solve_device(*args, 10, TOL, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_device(*a, 10, TOL, d_w=wa.data_ptr() + 4, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_device(*a, -1, TOL, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.solve_device(*a, 10, float("nan"), stream=st)
    for args in ((0, dd.data_ptr()), (g.data_ptr() + 4, dd.data_ptr()), (g.data_ptr(), 0)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.lsq.violation_device(*args, stream=st)
    with pytest.raises(ta.TowrError, match="error -1"):
        B.lsq.violation_device(g.data_ptr(), dd.data_ptr(), d_merit=out.data_ptr() + 4, stream=st)
    for args in ((2, dd.data_ptr(), dd.data_ptr(), out.data_ptr()), (0, 0, dd.data_ptr(), out.data_ptr()),
                 (0, dd.data_ptr(), dd.data_ptr() + 4, out.data_ptr()), (1, b.data_ptr(), b.data_ptr(), 0)):
        with pytest.raises(ta.TowrError, match="error -1"):
            B.lsq.dot_device(*args, stream=st)
    torch.cuda.synchronize()
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


# ---------------------------------------------------------------- 7. hipGraph

def test_capture_eval_violation_solve_update_scores_as_one_graph():
    torch, dev, _ = _torch()
    cases, order = _ragged()
    order = order[:24]
    B = _Batch([c.S for c in cases], order)
    X, G, J = int(B.xo[-1]), int(B.go[-1]), int(B.jo[-1])
    x0 = np.concatenate([cases[s].x_perturbed(i) for i, s in enumerate(order)])
    x = _dev(x0)
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device=dev)   # noqa: E731
    g, jac, r, b, wa, merit, d, info, scores = z64(G), z64(J), z64(G), z64(G), z64(G), z64(B.P), z64(X), z64(4 * B.P), z64(16 * B.P)
    mu = _dev(np.full(B.P, 50.0))
    outs = (g, jac, r, b, wa, merit, d, info, scores)

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, stream)
        B.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=stream)
        torch.neg(r, out=b)
        B.lsq.solve_device(jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), 25, 1e-6, d_w=wa.data_ptr(),
                           stream=stream)
        x.add_(d)
        B.batch.eval_scores_device(x.data_ptr(), scores.data_ptr(), d_g=g.data_ptr(), stream=stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # warm-up outside the capture (module load)
        step(side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # captures on a non-default stream of its own
        step(torch.cuda.current_stream().cuda_stream)
    x1 = np.concatenate([cases[s].x_perturbed(100 + i) for i, s in enumerate(order)])
    x.copy_(torch.from_numpy(x1))
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in outs] + [x.clone()]
    x.copy_(torch.from_numpy(x1))
    for t in outs:
        t.zero_()
    step(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a, e in zip(got, list(outs) + [x]):
        assert _same_bits(a.cpu().numpy(), e.cpu().numpy())
    assert info.cpu().numpy().reshape(-1, 4)[:, 0].max() > 3 and d.abs().max().item() > 0
    assert not torch.equal(x, torch.from_numpy(x1).to(dev))


# ---------------------------------------------------------------- 8. a full C3 batch

def test_c3_full_batch():
    torch, dev, st = _torch()
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    S = c.S
    n = 8192
    B = _Batch([S], [0] * n)
    # workspace (p, z: x layout; q, r, t: g layout; 4 scalars per problem) + the one bound table + a 40-byte record per problem
    want = 8 * (2 * S.n * n + 3 * S.m * n + 4 * n) + 2 * 8 * S.m + 40 * n
    assert S.n % 2 == 0 and S.m % 2 == 0 and B.lsq.bytes()["resident"] == want
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    x0 = _dev(c.x_guess())
    scale = _dev((c.x_perturbed(0) - c.x_guess()) / np.random.default_rng(1234).normal(size=S.n))   # 0.05 * the per-variable scale
    x = (x0[None, :] + scale[None, :] * torch.randn((n, S.n), generator=gen, dtype=torch.float64, device=dev)).reshape(-1).contiguous()
    g, jac = B.eval(x)
    r, wa, merit = B.violation(g)
    b = -r
    sample = (0, 4095, 8191)
    jac_h = {p: jac[B.jo[p]:B.jo[p + 1]].cpu().numpy() for p in sample}
    lam = _lam_max(_csr(S, jac_h[0]), wa[:S.m].cpu().numpy())
    mu = _dev(np.full(n, 1e-2 * lam))
    d, info = _solve(B.lsq, jac, b, wa, mu, iters=20)
    assert np.isfinite(d).all() and np.isfinite(info).all() and np.isfinite(merit.cpu().numpy()).all()
    assert (info[:, 0] == 20).all() and (info[:, 3] == 1).all()
    for p in sample:
        A = _csr(S, jac_h[p])
        bp, wp = b[B.go[p]:B.go[p + 1]].cpu().numpy(), wa[B.go[p]:B.go[p + 1]].cpu().numpy()
        dp = d[B.xo[p]:B.xo[p + 1]]
        rhs = A.T @ (wp * bp)
        true = np.linalg.norm(A.T @ (wp * (bp - A @ dp)) - 1e-2 * lam * dp) / np.linalg.norm(rhs)
        # the recurrence residual the device reports against the true one: they drift apart by rounding only.  The CPU
        # restatement agrees with its true residual to three digits at 1e-10 after 60 to 108 iterations: a drift below 1e-13 in
        # units of |s0|; ten times that, and 1e-9 relative for the other order of the norm's sum
        assert abs(info[p, 1] - true) <= 1e-12 + 1e-9 * true, (p, info[p], true)
        # 20 iterations of the numpy restatement: the same iterates up to rounding.  A dot product of m = 3866 terms carries
        # 3866 * 1.1e-16 = 4.3e-13; an error in alpha / beta is amplified by at most cond(H) = 101 over the 20 iterations
        k, dn, rel = _cgls(A, bp, wp, 1e-2 * lam, 20, 0.0)
        assert k == 20 and np.linalg.norm(dp - dn) <= 20 * 101 * 4.3e-13 * np.linalg.norm(dn), (p, np.linalg.norm(dp - dn) / np.linalg.norm(dn))
