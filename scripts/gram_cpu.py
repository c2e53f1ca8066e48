"""The Gram-matrix solve (twr_jac_gram, twr_jac_lsq_solve_gram) and the bounded LM driver with it (TWR_JAC_LM_GRAM) restated in
numpy on the CPU oracle's Jacobian.  No GPU: it is the reference the device tests of tests/test_jac_gram.py compare with, and
what tests/test_gram_cpu.py checks on its own.

  gram(A, w):     N = A^T diag(w) A (scipy CSR, the full symmetric matrix)
  gram_cg(...):   (C N C + mu I) e = c o z, d = c o e by CG from e = 0 with a recurred gradient; an exact 0 in c takes its
                  variable out; the stopping rule gamma <= tol^2 gamma0 of twr_jac_lsq_solve_scaled
  lm_gram(...):   the loop of scripts/lm_box_cpu.py::lm_box with that solve in place of CGLS (everything else imported from there)
Prints one line per problem (CGLS loop and Gram loop side by side), then one JSON line.
Usage:  python scripts/gram_cpu.py --seeds 3 --jobs 12
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lm_box_cpu import CG_TOL, MU_DOWN, MU_MAX, MU_MIN, MU_UP, TAU, blocked, case_bounds, cases, lambda_max, lm_box  # noqa: E402
from lm_damping_cpu import col_scale  # noqa: E402

CASES = ("anymal", "C2_biped_K100", "hopper_all", "C1_hopper", "biped_all")   # the inputs of DESIGN 6.L's Gram addendum, seeds 0-2


def gram(A, w):
    """N = A^T diag(w) A as CSR with sorted columns."""
    N = (A.T @ sp.diags(w) @ A).tocsr()
    N.sort_indices()
    return N


def gram_cg(N, z, mu, c, iters, tol):
    """(iterations, d, |s| / |s0|, status) of twr_jac_lsq_solve_gram: status 0 converged, 1 iteration cap, 2 bad input."""
    n = N.shape[0]
    free = c != 0
    s = np.where(free, c * z, 0.0)
    e = np.zeros(n)
    gam = g0 = s @ s
    bad_c = bool(((c < 0) | ~np.isfinite(c)).any())
    if not mu >= 0 or not np.isfinite(mu) or not np.isfinite(g0) or bad_c:
        return 0, e, (1.0 if g0 > 0 else 0.0) if np.isfinite(g0) else float("nan"), 2   # sqrt(gamma0 / gamma0), as the device writes it
    p = s.copy()
    k, status = 0, 0 if gam <= tol * tol * g0 else 1
    while status == 1 and k < iters:
        u = np.where(free, c * (N @ (c * p)), 0.0)
        delta = p @ u + mu * (p @ p)
        if not delta > 0 or not np.isfinite(delta):
            status = 2
            break
        alpha = gam / delta
        e += alpha * p
        s = s - alpha * (u + mu * p)
        gn = s @ s
        k += 1
        if not np.isfinite(gn):
            gam, status = gn, 2
            break
        if gn <= tol * tol * g0:
            gam, status = gn, 0
            break
        p = s + (gn / gam) * p
        gam = gn
    return k, np.where(free, c * e, 0.0), np.sqrt(gam / g0) if g0 > 0 else 0.0, status


ROW_LANES, THREADS, WAVE = 16, 256, 64   # kGramRowLanes, kGramThreads and the wave of jac/gram.h


def _butterfly(a, width):
    """The xor butterfly over the last axis (`width` lanes): every lane ends with the same sum; lane 0's is returned."""
    lanes = np.arange(width)
    s = width // 2
    while s >= 1:
        a = a + a[..., lanes ^ s]
        s //= 2
    return a[..., 0]


def _block_sum(terms):
    """lsq_sum of jac/lsq.h over the per-element terms of a vector: lane t adds the terms t, t + 256, ... in index order, a
    butterfly over each wave of 64 lanes, then the four waves' sums in wave order."""
    n = terms.size
    rounds = max(1, -(-n // THREADS))
    padded = np.zeros(rounds * THREADS)
    padded[:n] = terms
    acc = np.zeros(THREADS)
    for row in padded.reshape(rounds, THREADS):   # (adding the +0.0 of the padding changes nothing)
        acc = acc + row
    waves = _butterfly(acc.reshape(THREADS // WAVE, WAVE), WAVE)
    total = waves[0]
    for w in waves[1:]:
        total = total + w
    return total


class _RowProduct:
    """gram_row_dot of jac/gram.h for every row of N at once: lane l of a row's 16 adds the products l, l + 16, ... in column
    order (multiply, then add), then a butterfly over the 16 lanes."""

    def __init__(self, N):
        self.N = N
        n = N.shape[0]
        lens = np.diff(N.indptr)
        j = np.arange(N.nnz) - np.repeat(N.indptr[:-1], lens)   # position within the row
        self.row, self.lane, self.step = np.repeat(np.arange(n), lens), j % ROW_LANES, j // ROW_LANES
        self.steps = int(self.step.max()) + 1 if N.nnz else 0
        self.n = n

    def __call__(self, v):
        prod = np.zeros((self.steps, self.n, ROW_LANES))
        prod[self.step, self.row, self.lane] = self.N.data * v[self.N.indices]
        acc = np.zeros((self.n, ROW_LANES))
        for t in range(self.steps):
            acc = acc + prod[t]
        return _butterfly(acc, ROW_LANES)


def gram_cg_device(N, z, mu, c, iters, tol):
    """gram_cg in the arithmetic of gram_cg_kernel: the same multiplications and additions in the same order (no fused
    multiply-add anywhere), so the iterates, the stopping decisions and d are the device's bit for bit.  Returns what gram_cg
    returns."""
    n = N.shape[0]
    free = c != 0
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.where(free, c * z, 0.0)
        e = np.zeros(n)
        g0 = _block_sum(s * s)
        gam = g0
        tol2 = tol * tol
        bad_c = bool((~(c >= 0) | ~np.isfinite(c)).any())
        if not mu >= 0 or not np.isfinite(mu) or not np.isfinite(g0) or bad_c:
            return 0, e, float(np.sqrt(gam / g0)) if g0 != 0 else 0.0, 2
        p = s.copy()
        cp = np.where(free, c * p, 0.0)
        rows = _RowProduct(N)
        k, status = 0, 0 if g0 <= tol2 * g0 else 1
        while status == 1 and k < iters:
            u = np.where(free, c * rows(cp), 0.0)
            delta = _block_sum(p * u) + mu * _block_sum(p * p)
            if not delta > 0 or not np.isfinite(delta):
                status = 2
                break
            alpha = gam / delta
            e = e + alpha * p
            s = s - alpha * (mu * p + u)
            gn = _block_sum(s * s)
            k += 1
            beta = 0.0
            if not np.isfinite(gn):
                status = 2
            elif gn <= tol2 * g0:
                status = 0
            else:
                beta = gn / gam
            gam = gn
            if status != 1:
                break
            p = s + beta * p
            cp = np.where(free, c * p, 0.0)
        d = np.where(free, c * e, 0.0) if k > 0 else np.zeros(n)
        return k, d, float(np.sqrt(gam / g0)) if g0 != 0 else 0.0, status


def lm_gram(case, x0, lo, up, steps=8, cg_iters=60, power_iters=30, jitter=0.0, jitter_seed=0, keep=False):
    """lm_box_cpu.lm_box (bounded) with the Gram solve.  Returns the same dict; with keep, `lin` holds (N, z, cf, mu) per step."""
    S, P = case.S, case.P
    glo, ghi = S.bounds()
    rng = np.random.default_rng(jitter_seed)

    def at(x, jac):
        out = P.eval(x)
        r = out[0] - np.clip(out[0], glo, ghi)
        A = sp.csr_matrix((out[3], S.col_idx, S.row_ptr), shape=(S.m, S.n)) if jac else None
        return r, A

    def linearise(x, colmax):
        r, A = at(x, True)
        w = (r != 0).astype(np.float64)
        colmax, c = col_scale(colmax, np.asarray(A.multiply(A).T @ w).ravel())
        z = A.T @ (w * -r)
        cf = np.where(blocked(x, lo, up, z), 0.0, c)
        return r, A, w, z, cf, colmax

    x = np.clip(x0, lo, up)
    colmax = np.zeros(S.n)
    r, A, w, z, cf, colmax = linearise(x, colmax)
    merit = 0.5 * (r @ r)
    mu = TAU * lambda_max((A @ sp.diags(cf)).tocsr(), w, power_iters) if power_iters else TAU
    mu = min(max(mu, MU_MIN), MU_MAX)
    res = dict(merit=[merit], accepted=[], nfree=[], mu=[mu], cg=[], lin=[], done=False)
    for _ in range(steps):
        r, A, w, z, cf, colmax = linearise(x, colmax)
        if 0.5 * (r @ r) <= 0.0:
            res["done"] = True
            break
        N = gram(A, w)
        k, d, _, _ = gram_cg(N, z, mu, cf, cg_iters, CG_TOL)
        if keep:
            res["lin"].append((N, z, cf, mu))
        if jitter:
            d = d * (1.0 + jitter * rng.normal(size=S.n))
        xt = np.clip(x + d, lo, up)
        r2, _ = at(xt, False)
        mt = 0.5 * (r2 @ r2)
        ok = bool(mt < merit)
        if ok:
            x, merit = xt, mt
        mu = min(max(mu * (MU_DOWN if ok else MU_UP), MU_MIN), MU_MAX)
        res["accepted"].append(int(ok))
        res["nfree"].append(int((cf != 0).sum()))
        res["cg"].append(k)
        res["merit"].append(merit)
        res["mu"].append(mu)
    res["x"] = x
    return res


def dense_step(N, z, mu, c):
    """The same system solved directly on the free variables: d."""
    free = np.flatnonzero(c != 0)
    cf = c[free]
    H = (sp.diags(cf) @ N[free][:, free] @ sp.diags(cf)).toarray() + mu * np.eye(free.size)
    d = np.zeros(N.shape[0])
    d[free] = cf * np.linalg.solve(H, cf * z[free])
    return d


def first_system(case, seed):
    """What the first step of lm_gram solves at the projection of x_perturbed(seed): (A, w, N, z, cf, b), z = A^T (w o b)."""
    S = case.S
    lo, up = case_bounds(case)
    glo, ghi = S.bounds()
    x = np.clip(case.x_perturbed(seed), lo, up)
    out = case.P.eval(x)
    r = out[0] - np.clip(out[0], glo, ghi)
    A = sp.csr_matrix((out[3], S.col_idx, S.row_ptr), shape=(S.m, S.n))
    w = (r != 0).astype(np.float64)
    _, c = col_scale(np.zeros(S.n), np.asarray(A.multiply(A).T @ w).ravel())
    z = A.T @ (w * -r)
    return A, w, gram(A, w), z, np.where(blocked(x, lo, up, z), 0.0, c), -r


def mu_of(N, c, tau=TAU):
    """tau lambda_max(C N C), lambda_max from a dense symmetric eigensolve: cond(C N C + mu I) <= 1 + 1 / tau."""
    H = (sp.diags(c) @ N @ sp.diags(c)).toarray()
    return tau * float(np.linalg.eigvalsh(0.5 * (H + H.T))[-1])


_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = cases()[name]()
    return _cases[name]


def one(job):
    name, seed, a = job
    case = get_case(name)
    lo, up = case_bounds(case)
    x0 = case.x_perturbed(seed)
    B = lm_box(case, x0, lo, up, a["steps"], a["cg_iters"], a["power_iters"])
    G = lm_gram(case, x0, lo, up, a["steps"], a["cg_iters"], a["power_iters"])
    factor = 1.0   # the Gram loop's own sensitivity: its final merit under a relative jitter of every step
    for draw in range(a["jitter_draws"]):
        m = lm_gram(case, x0, lo, up, a["steps"], a["cg_iters"], a["power_iters"], jitter=a["jitter"], jitter_seed=draw)["merit"][-1]
        if m > 0 and G["merit"][-1] > 0:
            factor = max(factor, m / G["merit"][-1], G["merit"][-1] / m)
    return dict(case=name, seed=seed, n=case.S.n, m=case.S.m, merit_before=B["merit"][0], cgls_merit=B["merit"][-1],
                cgls_accepted=B["accepted"], gram_merit=G["merit"][-1], gram_accepted=G["accepted"], cgls_cg=B["cg"], gram_cg=G["cg"],
                gram_merit_1=G["merit"][1] if len(G["merit"]) > 1 else G["merit"][0], jitter_factor=factor)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--cg-iters", type=int, default=60)
    ap.add_argument("--power-iters", type=int, default=30)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--jitter", type=float, default=2e-8)
    ap.add_argument("--jitter-draws", type=int, default=0, help="16: the sensitivity runs of DESIGN 6.L")
    a = ap.parse_args()
    opts = dict(steps=a.steps, cg_iters=a.cg_iters, power_iters=a.power_iters, jitter=a.jitter, jitter_draws=a.jitter_draws)
    jobs = [(name, seed, opts) for name in a.cases.split(",") for seed in range(a.seeds)]
    out = []
    with ProcessPoolExecutor(max_workers=a.jobs) as pool:
        for r in pool.map(one, jobs, chunksize=1):
            print("%-14s seed %2d n %4d m %4d: merit %.3e -> CGLS %.3e (%d accepted) | Gram %.3e (%d accepted), ratio %.4f, jitter factor %.3f"
                  % (r["case"], r["seed"], r["n"], r["m"], r["merit_before"], r["cgls_merit"], sum(r["cgls_accepted"]), r["gram_merit"],
                     sum(r["gram_accepted"]), r["gram_merit"] / r["cgls_merit"] if r["cgls_merit"] else float("nan"), r["jitter_factor"]), flush=True)
            out.append(r)
    print(json.dumps({"gram_cpu": out, **opts}), flush=True)


if __name__ == "__main__":
    main()
