"""The Levenberg-Marquardt loop of scripts/jac_lsq.py restated in numpy on the CPU oracle's Jacobian, with both dampings:
mu I (twr_jac_lsq_solve) and Marquardt's mu C^-2, C = diag(1 / weighted column norm) with Moré's running maximum and a
relative floor of 1e-12 (twr_jac_col_sqnorms -> twr_jac_col_scale -> twr_jac_lsq_solve_scaled).  No GPU: it is the reference
for the ratio tests/test_jac_scaled.py::test_lm_loop_marquardt_against_identity asserts on the device, on exactly that test's
inputs: --problems N of C3 (ANYmal trot, flat, K = 200) and of C4 stairs K = 200 at x_perturbed(seed), seed = 0 .. N - 1.

Per step: g, J at x; r = viol(g), w = [r != 0], merit = 1/2 sum r^2; CGLS of at most --cg-iters iterations, tol 1e-8, on
(J^T W J + mu D) d = -J^T W r; accept when the merit at x + d is lower (mu / 3), else mu * 10.  mu starts at 1e-2 lambda_max of
the matrix the variant iterates on (J^T W J, or C J^T W J C), lambda_max by --power-iters power iterations.
Prints one line per problem and one JSON line: the final merits and the worst (largest) ratio marquardt / identity per case.
Usage:  python scripts/lm_damping_cpu.py --problems 64 --jobs 16
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

REL_FLOOR = 1e-12


def cases():
    import towr_amd as ta
    from tests.common import Case, baseline_cases, k_params

    return {"C3": lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200)),
            "C4_stairs": baseline_cases()["C4_anymal_stairs_K200"]}


def cgls(A, b, w, mu, iters, tol):
    """twr_jac_lsq_solve's iteration (tests/jac_ref.py::cgls)."""
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
    return k, d


def lambda_max(A, w, iters):
    v = np.random.default_rng(3).normal(size=A.shape[1])
    lam = 0.0
    for _ in range(iters):
        z = A.T @ (w * (A @ v))
        lam = (v @ z) / max(v @ v, 1e-300)
        v = z / max(np.linalg.norm(z), 1e-300)
    return lam


def col_scale(colsq_max, colsq):
    """twr_jac_col_scale with the running maximum: (colsq_max, c)."""
    a = np.maximum(colsq_max, colsq)
    top = a.max() if a.size else 0.0
    if top == 0.0:
        return a, np.ones_like(a)
    return a, 1.0 / np.sqrt(np.maximum(a, REL_FLOOR * top))


def lm(case, x0, damping, steps, cg_iters, power_iters):
    S, P = case.S, case.P
    lo, hi = S.bounds()

    def at(x, jac):
        out = P.eval(x)
        r = out[0] - np.clip(out[0], lo, hi)
        A = sp.csr_matrix((out[3], S.col_idx, S.row_ptr), shape=(S.m, S.n)) if jac else None
        return r, A

    x = x0.copy()
    colmax = np.zeros(S.n)
    mu = None
    merit0 = None
    accepted = []
    for _ in range(steps):
        r, A = at(x, True)
        w = (r != 0).astype(np.float64)
        merit = 0.5 * (r @ r)
        if merit0 is None:
            merit0 = merit
        if damping == "marquardt":
            colmax, c = col_scale(colmax, np.asarray(A.multiply(A).T @ w).ravel())
            A = (A @ sp.diags(c)).tocsr()
        else:
            c = 1.0
        if mu is None:
            mu = 1e-2 * lambda_max(A, w, power_iters)
        _, e = cgls(A, -r, w, mu, cg_iters, 1e-8)
        xt = x + c * e
        r2, _ = at(xt, False)
        ok = 0.5 * (r2 @ r2) < merit
        if ok:
            x = xt
        mu = mu / 3.0 if ok else mu * 10.0
        accepted.append(int(ok))
    r, _ = at(x, False)
    return merit0, 0.5 * (r @ r), accepted


_cases = {}


def one(job):
    name, seed, a = job
    if name not in _cases:
        _cases[name] = cases()[name]()
    case = _cases[name]
    x0 = case.x_perturbed(seed)
    m0, mi, ai = lm(case, x0, "identity", a["steps"], a["cg_iters"], a["power_iters"])
    _, mm, am = lm(case, x0, "marquardt", a["steps"], a["cg_iters"], a["power_iters"])
    return name, seed, m0, mi, mm, sum(ai), sum(am)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--cg-iters", type=int, default=60)
    ap.add_argument("--power-iters", type=int, default=30)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--cases", default="C3,C4_stairs")
    a = ap.parse_args()
    opts = dict(steps=a.steps, cg_iters=a.cg_iters, power_iters=a.power_iters)
    jobs = [(name, seed, opts) for name in a.cases.split(",") for seed in range(a.problems)]
    res = {}
    with ProcessPoolExecutor(max_workers=a.jobs) as pool:
        for name, seed, m0, mi, mm, ai, am in pool.map(one, jobs, chunksize=1):
            print("%-10s seed %3d: merit %.4e -> identity %.4e (%d accepted), marquardt %.4e (%d accepted), ratio %.3e"
                  % (name, seed, m0, mi, ai, mm, am, mm / mi), flush=True)
            res.setdefault(name, []).append((m0, mi, mm))
    out = {}
    for name, v in res.items():
        v = np.array(v)
        ratio = v[:, 2] / v[:, 1]
        out[name] = {"problems": len(v), "merit_before_sum": float(v[:, 0].sum()), "identity_after_sum": float(v[:, 1].sum()),
                     "marquardt_after_sum": float(v[:, 2].sum()), "ratio_min": float(ratio.min()),
                     "ratio_median": float(np.median(ratio)), "ratio_worst": float(ratio.max())}
    print(json.dumps({"lm_damping_cpu": out, **opts}), flush=True)


if __name__ == "__main__":
    main()
