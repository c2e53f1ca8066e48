"""twr_jac_violation / twr_jac_dot / twr_jac_lsq_solve on the device against float64 numpy / scipy on the CPU: the residual bit
for bit, the damped weighted least-squares step against a dense (or sparse LU) solve of the normal equations on the oracle's
Jacobian and on the device's own, the step's effect on the oracle's merit, bit-reproducibility across batches, calls and
iteration caps, containment of NaN / Inf and bad mu, the edge cases, hipGraph capture and a full C3 batch.

The bounds of the solve tests (tol = 1e-10, mu = 1e-2 lambda_max(J^T W J): true residual <= 2 tol, |d - d_direct| <= 101 2 tol
|d_direct|, iterations in (0, 200)) are derived in tests/jac_ref.py, which holds check_step and the numpy restatement cgls."""
import functools

import numpy as np
import pytest

import towr_amd as ta

from .common import Case, baseline_cases, k_params, random_case
from .jac_device import JacBatch, assert_replay_equals_eager, c3_batch, capture, dev, ragged, ragged_x, torch_ctx
from .jac_ref import ITERS, TOL, bits, cgls, check_step, csr, lam_max, row_weights, s0_bound, same_bits, viol

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1. violation and dot

@pytest.mark.parametrize("point", ["x_perturbed", "x_wild"])
def test_violation_and_dot_on_a_ragged_batch(point):
    torch, device, st = torch_ctx()
    cases, order = ragged()
    B = JacBatch([c.S for c in cases], order)
    x = dev(ragged_x(cases, order, point))
    g, _ = B.eval(x, ta.EVAL_VALUES)
    G = int(B.go[-1])
    rng = np.random.default_rng(21)
    w_h = rng.uniform(0.1, 3.0, size=G)
    g_h = g.cpu().numpy()[:G].copy()
    g_h[[5, int(B.go[7]) + 3, G - 1]] = np.nan   # a NaN g_i gives a NaN r_i, as numpy's clip does
    g_h[int(B.go[9]) + 1] = np.inf
    g = dev(g_h)
    with np.errstate(invalid="ignore"):
        ref = viol(g_h, B.lo, B.hi)
    assert np.isnan(ref[5]) and (ref != 0).sum() > G // 100
    for w in (None, dev(w_h)):
        wh = np.ones(G) if w is None else w_h
        r, wa, merit = B.violation(g, w)
        r, wa, merit = r.cpu().numpy()[:G], wa.cpu().numpy()[:G], merit.cpu().numpy()
        fin = ~np.isnan(ref)
        assert np.array_equal(np.isnan(r), ~fin) and np.array_equal(bits(r[fin]), bits(ref[fin])), "r is not g - clip(g) bit for bit"
        assert np.array_equal(bits(wa), bits(wh * (ref != 0))), "w_active is not w [r != 0] bit for bit"
        for p in range(B.P):
            t = 0.5 * wh[B.go[p]:B.go[p + 1]] * ref[B.go[p]:B.go[p + 1]] ** 2
            if not np.isfinite(t).all():   # the planted NaN / Inf: the same non-number
                assert np.array_equal(merit[p], t.sum(), equal_nan=True), p
            else:
                assert abs(merit[p] - t.sum()) <= 1e-12 * np.abs(t).sum(), (p, merit[p], t.sum())
    # r alone: the optional outputs left out
    r2 = torch.full((G,), float("nan"), dtype=torch.float64, device=device)
    B.lsq.violation_device(g.data_ptr(), r2.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert same_bits(r2.cpu().numpy()[fin], ref[fin])
    # |r| is the per-row quantity twr_batch_score reduces: the inf-norm of a clean problem's r is the largest of its scores
    scores = torch.zeros(16 * B.P, dtype=torch.float64, device=device)
    B.batch.score_device(g.data_ptr(), scores.data_ptr(), st)
    torch.cuda.synchronize()
    sc = scores.cpu().numpy().reshape(B.P, 8, 2)
    for p in (1, 2, 3, 50, 150):   # (problems whose g holds no planted NaN / Inf)
        assert np.abs(ref[B.go[p]:B.go[p + 1]]).max() == sc[p, :, 0].max(), p
    # dot over both layouts
    for space, off in ((B.lsq.X, B.xo), (B.lsq.G, B.go)):
        a_h, b_h = rng.normal(size=int(off[-1])), rng.normal(size=int(off[-1]))
        out = torch.full((B.P,), float("nan"), dtype=torch.float64, device=device)
        a, b = dev(a_h), dev(b_h)
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
    B = JacBatch([c.S for c in cases], range(len(cases)))
    probs = []
    for c in cases:
        x = c.x_perturbed(seed)
        out = c.P.eval(x)
        g, jv = out[0], out[3]
        lo, hi = c.S.bounds()
        A = csr(c.S, jv)
        r = viol(g, lo, hi)
        w0 = np.ones(c.S.m) if weighting == "unit" else row_weights(A)
        w = w0 * (r != 0)
        probs.append(dict(case=c, x=x, A=A, jv=jv, r=r, b=-r, w0=w0, w=w, mu=1e-2 * lam_max(A, w), lo=lo, hi=hi))
    d, info = B.solve(dev(np.concatenate([q["jv"] for q in probs])), dev(np.concatenate([q["b"] for q in probs])),
                      dev(np.concatenate([q["w"] for q in probs])), dev([q["mu"] for q in probs]))
    for p, q in enumerate(probs):
        q["d"], q["info"], q["name"] = d[B.xo[p]:B.xo[p + 1]], info[p], "%s seed %d W %s" % (names[p], seed, weighting)
    return probs


@pytest.mark.parametrize("weighting", ["unit", "rown"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_solve_on_the_oracle_jacobian(seed, weighting):
    for q in _baseline_solve(seed, weighting):   # every problem: none is left out
        true, err = check_step(q["A"], q["b"], q["w"], q["mu"], q["d"], q["info"], q["name"])
        print("  true residual %.2e, |d - dense| / |dense| %.2e" % (true, err))


@pytest.mark.parametrize("weighting", ["unit", "rown"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_step_reduces_the_oracle_merit(seed, weighting):
    for q in _baseline_solve(seed, weighting):
        g2 = q["case"].P.eval(q["x"] + q["d"])[0]
        r2 = viol(g2, q["lo"], q["hi"])
        before, after = 0.5 * q["r"] @ (q["w0"] * q["r"]), 0.5 * r2 @ (q["w0"] * r2)
        print("%s: merit %.4e -> %.4e, ratio %.3f" % (q["name"], before, after, after / before))
        assert after < before, q["name"]


# ---------------------------------------------------------------- 3. the device's own Jacobian

def test_solve_on_the_device_jacobian_of_a_ragged_batch():
    torch, device, st = torch_ctx()
    cases, order = ragged()
    B = JacBatch([c.S for c in cases], order)
    x = dev(ragged_x(cases, order))
    jac, b, wa = B.linearise(x)
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    As = [B.A(p, jac_h) for p in range(B.P)]
    mu_h = np.array([1e-2 * lam_max(As[p], w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    assert (mu_h > 0).all()
    d, info = B.solve(jac, b, wa, dev(mu_h))
    for p in range(B.P):
        go = slice(B.go[p], B.go[p + 1])
        check_step(As[p], b_h[go], w_h[go], mu_h[p], d[B.xo[p]:B.xo[p + 1]], info[p], "ragged problem %d (struct %d)" % (p, order[p]),
                   direct="dense" if As[p].shape[1] <= 1500 else "lu")


# ---------------------------------------------------------------- 5. bit-reproducibility

def test_bits_do_not_depend_on_the_batch_the_call_or_the_cap():
    torch, device, st = torch_ctx()
    c, B, x, g, jac, b, wa = c3_batch(512)
    jac_h, w_h = jac.cpu().numpy(), wa.cpu().numpy()
    lam = lam_max(B.A(0, jac_h), w_h[B.go[0]:B.go[1]])
    mu = dev(np.full(B.P, 1e-2 * lam))
    d1, i1 = B.solve(jac, b, wa, mu)
    d2, i2 = B.solve(jac, b, wa, mu)
    assert same_bits(d1, d2) and same_bits(i1, i2), "two calls differ"
    assert (i1[:, 3] == 0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        d3, i3 = B.solve(jac, b, wa, mu, stream=side.cuda_stream)
    assert same_bits(d1, d3) and same_bits(i1, i3), "another stream differs"
    one = JacBatch([c.S], [0])
    for p in (0, 201, 511):   # alone in a one-problem handle, its values copied to fresh buffers
        do, io = one.solve(jac[B.jo[p]:B.jo[p + 1]].clone(), b[B.go[p]:B.go[p + 1]].clone(), wa[B.go[p]:B.go[p + 1]].clone(),
                              mu[p:p + 1].clone())
        assert same_bits(do, d1[B.xo[p]:B.xo[p + 1]]) and same_bits(io[0], i1[p]), p
    # mu from 1e-2 to 10 lambda_max: cond <= 101, every problem converges, at different counts; a problem that has converged
    # does not move while the others go on
    P = 16
    S16 = JacBatch([c.S], [0] * P)
    mus = dev(lam * np.logspace(-2, 1, P))
    sl = lambda t, off: t[:int(off[P])]   # noqa: E731  (one structure: the first 16 problems are a batch of their own)
    d200, i200 = S16.solve(sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus)
    assert (i200[:, 3] == 0).all() and (i200[:, 0] < ITERS).all() and len(set(i200[:, 0])) > 4, i200[:, 0]
    for k in sorted(set(int(v) for v in i200[:, 0])):
        dk, ik = S16.solve(sl(jac, B.jo), sl(b, B.go), sl(wa, B.go), mus, iters=k)
        for p in np.nonzero(i200[:, 0] <= k)[0]:
            assert same_bits(dk[S16.xo[p]:S16.xo[p + 1]], d200[S16.xo[p]:S16.xo[p + 1]]) and same_bits(ik[p], i200[p]), (k, p)
        assert (ik[i200[:, 0] > k, 3] == 1).all() and (ik[i200[:, 0] > k, 0] == k).all()   # the others: the cap


# ---------------------------------------------------------------- 6. containment and edge cases

def test_poison_stays_in_its_problem():
    torch, device, st = torch_ctx()
    cases, order = ragged()
    order = order[:40]
    B = JacBatch([c.S for c in cases], order)
    x = dev(ragged_x(cases, order))
    jac, b, wa = B.linearise(x)
    jac_h, b_h, w_h = jac.cpu().numpy(), b.cpu().numpy(), wa.cpu().numpy()
    mu_h = np.array([1e-2 * lam_max(B.A(p, jac_h), w_h[B.go[p]:B.go[p + 1]]) for p in range(B.P)])
    d0, i0 = B.solve(jac, b, wa, dev(mu_h), iters=60)
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
    d1, i1 = B.solve(dev(jb), dev(bb), dev(wb), dev(mb), iters=60)
    for p in range(B.P):
        dp = d1[B.xo[p]:B.xo[p + 1]]
        if p not in bad:
            assert same_bits(dp, d0[B.xo[p]:B.xo[p + 1]]) and same_bits(i1[p], i0[p]), p
        elif bad[p][0] == "mu":
            assert i1[p, 3] == 2 and i1[p, 0] == 0 and not dp.any(), (p, i1[p])
        else:
            assert i1[p, 3] == 2 or not np.isfinite(dp).all(), (p, i1[p])


def test_edge_cases():
    torch, device, st = torch_ctx()
    # a structure without rows: d = 0, status 0, no iterations
    case = random_case(5111)
    assert case.S.m == 0 and case.S.nnz == 0
    B = JacBatch([case.S], [0, 0, 0])
    one = torch.zeros(8, dtype=torch.float64, device=device)
    d, info = B.solve(one, one, None, dev([0.0, 1.0, 2.0]))
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 0).all() and not info[:, 1:3].any()
    # b = 0: the same, no 0 / 0
    c, B, x, g, jac, b, wa = c3_batch(3)
    lam = lam_max(B.A(0, jac.cpu().numpy()), wa.cpu().numpy()[B.go[0]:B.go[1]])
    mu = dev(np.full(3, 1e-2 * lam))
    bz = b.clone()
    bz[B.go[1]:B.go[2]] = 0.0
    d, info = B.solve(jac, bz, wa, mu)
    assert not d[B.xo[1]:B.xo[2]].any() and np.array_equal(info[1], [0, 0, 0, 0]) and (info[[0, 2], 3] == 0).all()
    dref, iref = B.solve(jac, b, wa, mu)
    assert same_bits(d[B.xo[0]:B.xo[1]], dref[B.xo[0]:B.xo[1]]) and same_bits(d[B.xo[2]:], dref[B.xo[2]:])
    # iters = 0: zeros and |s0|
    d, info = B.solve(jac, b, wa, mu, iters=0)
    assert not d.any() and (info[:, 0] == 0).all() and (info[:, 3] == 1).all() and (info[:, 1] == 1).all()
    assert same_bits(info[:, 2], iref[:, 2])
    jac_h, w_h, b_h = jac.cpu().numpy(), wa.cpu().numpy(), b.cpu().numpy()
    for p in range(3):
        A, go = B.A(p, jac_h), slice(B.go[p], B.go[p + 1])
        assert abs(info[p, 2] - np.linalg.norm(A.T @ (w_h[go] * b_h[go]))) <= s0_bound(A, w_h[go], b_h[go]), p
    # w NULL is w = 1
    ones = torch.ones_like(b)
    dn, inn = B.solve(jac, b, None, mu, iters=30)
    d1, i1 = B.solve(jac, b, ones, mu, iters=30)
    assert same_bits(dn, d1) and same_bits(inn, i1) and (inn[:, 0] == 30).all()
    # tol >= 1 stops at once; tol = 0 runs to the cap
    d, info = B.solve(jac, b, wa, mu, iters=5, tol=1.0)
    assert not d.any() and (info[:, 3] == 0).all() and (info[:, 0] == 0).all()
    d, info = B.solve(jac, b, wa, mu, iters=5, tol=0.0)
    assert (info[:, 3] == 1).all() and (info[:, 0] == 5).all()
    # NULL and misaligned buffers, a bad space, negative iters, another batch's structures
    out = torch.zeros(4 * 3, dtype=torch.float64, device=device)
    dd = torch.zeros(int(B.xo[-1]), dtype=torch.float64, device=device)
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
    torch, device, _ = torch_ctx()
    cases, order = ragged()
    order = order[:24]
    B = JacBatch([c.S for c in cases], order)
    X, G, J = B.X, B.G, B.J
    x = dev(ragged_x(cases, order))
    z64 = lambda n: torch.zeros(n, dtype=torch.float64, device=device)   # noqa: E731
    g, jac, r, b, wa, merit, d, info, scores = z64(G), z64(J), z64(G), z64(G), z64(G), z64(B.P), z64(X), z64(4 * B.P), z64(16 * B.P)
    mu = dev(np.full(B.P, 50.0))
    outs = (g, jac, r, b, wa, merit, d, info, scores)

    def step(stream):   # a single chain: no parallel branches
        B.batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, stream)
        B.lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=stream)
        torch.neg(r, out=b)
        B.lsq.solve_device(jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), 25, 1e-6, d_w=wa.data_ptr(),
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


# ---------------------------------------------------------------- 8. a full C3 batch

def test_c3_full_batch():
    torch, device, st = torch_ctx()
    c = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))
    S = c.S
    n = 8192
    B = JacBatch([S], [0] * n)
    # workspace (p, z: x layout; q, r, t: g layout; 4 scalars per problem) + the one bound table + a 40-byte record per problem
    want = 8 * (2 * S.n * n + 3 * S.m * n + 4 * n) + 2 * 8 * S.m + 40 * n
    assert S.n % 2 == 0 and S.m % 2 == 0 and B.lsq.bytes()["resident"] == want
    gen = torch.Generator(device=device)
    gen.manual_seed(5)
    x0 = dev(c.x_guess())
    scale = dev((c.x_perturbed(0) - c.x_guess()) / np.random.default_rng(1234).normal(size=S.n))   # 0.05 * the per-variable scale
    x = (x0[None, :] + scale[None, :] * torch.randn((n, S.n), generator=gen, dtype=torch.float64, device=device)).reshape(-1).contiguous()
    g, jac = B.eval(x)
    r, wa, merit = B.violation(g)
    b = -r
    sample = (0, 4095, 8191)
    jac_h = {p: jac[B.jo[p]:B.jo[p + 1]].cpu().numpy() for p in sample}
    lam = lam_max(csr(S, jac_h[0]), wa[:S.m].cpu().numpy())
    mu = dev(np.full(n, 1e-2 * lam))
    d, info = B.solve(jac, b, wa, mu, iters=20)
    assert np.isfinite(d).all() and np.isfinite(info).all() and np.isfinite(merit.cpu().numpy()).all()
    assert (info[:, 0] == 20).all() and (info[:, 3] == 1).all()
    for p in sample:
        A = csr(S, jac_h[p])
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
        k, dn, rel = cgls(A, bp, wp, 1e-2 * lam, 20, 0.0)
        assert k == 20 and np.linalg.norm(dp - dn) <= 20 * 101 * 4.3e-13 * np.linalg.norm(dn), (p, np.linalg.norm(dp - dn) / np.linalg.norm(dn))
