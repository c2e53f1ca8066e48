"""The two iterations of the device's least-squares solves restated in numpy on the CPU oracle's Jacobian: CGLS
(twr_jac_lsq_solve: s = J^T(w o r) - mu d from the residual) and the one-pass iteration (twr_jac_lsq_solve_onepass: s recurred,
s -= alpha (J^T(w o (J p)) + mu p)).  Prints, per case, how far the two d are apart at the Levenberg-Marquardt setting
(60 iterations, tol = 1e-8, active-set weights, mu = 1e-2 lambda_max) over 64 points x_perturbed(0 .. 63): the figures the
agreement test of tests/test_jac_onepass.py takes its bound from.  No device.
Usage: python scripts/onepass_cpu.py [--points 64]
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.common import baseline_cases  # noqa: E402


def cgls(A, b, w, mu, iters, tol):
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


def onepass(A, b, w, mu, iters, tol):
    d = np.zeros(A.shape[1])
    s = A.T @ (w * b)
    p = s.copy()
    gam = g0 = s @ s
    k = 0
    while k < iters and not gam <= tol * tol * g0:
        q = A @ p
        u = A.T @ (w * q)
        alpha = gam / (q @ (w * q) + mu * (p @ p))
        d += alpha * p
        s = s - alpha * (u + mu * p)
        gn = s @ s
        p = s + (gn / gam) * p
        gam = gn
        k += 1
    return k, d, np.sqrt(gam / g0) if g0 > 0 else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--tol", type=float, default=1e-8)
    a = ap.parse_args()
    out = {}
    for name in ("C3_anymal_trot_K200", "C4_anymal_stairs_K200"):
        c = baseline_cases()[name]()
        lo, hi = c.S.bounds()
        diff, its = [], []
        for i in range(a.points):
            ev = c.P.eval(c.x_perturbed(i))
            g, jv = ev[0], ev[3]
            A = sp.csr_matrix((jv, c.S.col_idx, c.S.row_ptr), shape=(c.S.m, c.S.n))
            r = g - np.clip(g, lo, hi)
            w = (r != 0).astype(np.float64)
            mu = 1e-2 * float(spl.svds(sp.diags(np.sqrt(w)) @ A, k=1, return_singular_vectors=False)[0] ** 2)
            k1, d1, _ = cgls(A, -r, w, mu, a.iters, a.tol)
            k2, d2, _ = onepass(A, -r, w, mu, a.iters, a.tol)
            diff.append(float(np.linalg.norm(d2 - d1) / np.linalg.norm(d1)))
            its.append((k1, k2))
        out[name] = {"points": a.points, "rel_diff_max": max(diff), "rel_diff_median": float(np.median(diff)),
                     "iterations_cgls_min_max": [min(k for k, _ in its), max(k for k, _ in its)],
                     "iterations_onepass_min_max": [min(k for _, k in its), max(k for _, k in its)]}
    print(json.dumps({"onepass_cpu": out}), flush=True)


if __name__ == "__main__":
    main()
