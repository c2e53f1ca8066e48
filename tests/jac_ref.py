"""The host-only reference of the Jacobian solver tests (tests/test_jac_*.py on the device, tests/test_lm_box_cpu.py and
tests/test_gram_cpu.py on the CPU): float64 numpy / scipy restatements, the bounds the solves are held to, and the problem tables
the CPU and the device tests share.  Nothing here needs a GPU, torch or the product's shared library.

The bounds of the solve tests (check_step), with tol = 1e-10 and mu = 1e-2 lambda_max(J^T W J):
  * true relative normal-equation residual of the returned d <= 2 tol (numpy's restatement of the iteration, cgls, stops with
    recurrence and true residual agreeing to three digits; the factor 2 is for the device's other summation order);
  * |d - d_direct| <= cond(H) 2 tol |d_direct| with cond(H) <= (lambda_max + mu) / mu = 101;
  * iterations under the cap of 200 (CG on cond 101 contracts by (sqrt(101) - 1) / (sqrt(101) + 1) = 0.819 per iteration:
    2 0.819^k sqrt(101) <= 1e-10 from k = 131).
The Marquardt-scaled solve (check_scaled_step) is held to the same bounds in the scaled variables e = d / c, with
mu = 1e-2 lambda_max(C J^T W J C):
  * true relative residual |C (H d - J^T W b)| / |C J^T W b| <= 2 tol, H = J^T W J + mu C^-2;
  * |e - e_direct| <= cond 2 tol |e_direct| with cond <= (lambda_max + mu) / mu = 101;
  * iterations under the cap of 200 (converged from k = 131, as above).
The masked solve is that iteration on fewer columns and takes the same bounds on the free columns."""
import functools
import os
import sys

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

from .common import baseline_cases, random_case
from .probe import bits

TOL, ITERS, COND, REL_FLOOR = 1e-10, 200, 101.0, 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def csr(S, vals):
    return sp.csr_matrix((vals, S.col_idx, S.row_ptr), shape=(S.m, S.n))


def viol(g, lo, hi):
    return g - np.clip(g, lo, hi)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def lam_max(A, w):
    """lambda_max(A^T W A) on the CPU; 0 for a problem without active rows."""
    if not np.any(w):
        return 0.0
    return float(spl.svds(sp.diags(np.sqrt(w)) @ A, k=1, return_singular_vectors=False)[0] ** 2)


def row_weights(A):
    rown = np.sqrt(np.asarray(A.multiply(A).sum(axis=1)).ravel())
    return 1.0 / np.maximum(rown, 1e-12) ** 2


def s0_bound(A, w, b):
    """Rounding of |J^T (w o b)| summed in another order: 1e-12 of the terms' magnitudes per component (the tolerance of the
    products' own test), over n components."""
    return 1e-12 * np.sqrt(A.shape[1]) * np.linalg.norm(abs(A).T @ np.abs(w * b))


def cgls(A, b, w, mu, iters, tol):
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


def check_step(A, b, w, mu, d, info, what, direct="dense"):
    """One problem's d and info against the normal equations solved directly on the CPU."""
    n = A.shape[1]
    rhs = A.T @ (w * b)
    k_np, _, rel_np = cgls(A, b, w, mu, ITERS, TOL)
    msg = "%s: device %d iterations, |s|/|s0| %.3e, status %d; numpy %d iterations, %.3e" % (what, info[0], info[1], info[3], k_np, rel_np)
    print(msg)
    assert info[3] == 0, msg
    assert 0 < info[0] < ITERS, msg
    Hs = (A.T @ sp.diags(w) @ A + mu * sp.identity(n)).tocsc()
    true = np.linalg.norm(Hs @ d - rhs) / np.linalg.norm(rhs)
    assert true <= 2 * TOL, (msg, "true residual", true)
    assert abs(info[2] - np.linalg.norm(rhs)) <= s0_bound(A, w, b), (msg, "|s0|")
    dd = np.linalg.solve(Hs.toarray(), rhs) if direct == "dense" else spl.splu(Hs).solve(rhs)
    err = np.linalg.norm(d - dd) / np.linalg.norm(dd)
    assert err <= COND * 2 * TOL, (msg, "|d - direct| / |direct|", err)
    return true, err


def check_scaled_step(A, b, w, mu, c, d, info, zero, what):
    """One problem's scaled (or, on its free columns, masked) d and info against a direct solve in e = d / c on the CPU."""
    n = A.shape[1]
    rhs = A.T @ (w * b)
    msg = "%s: %d iterations, |s|/|s0| %.3e, status %d" % (what, info[0], info[1], info[3])
    assert info[3] == 0, msg
    assert 0 < info[0] < ITERS, msg
    res = c * (A.T @ (w * (A @ d))) + mu * d / c - c * rhs
    true = np.linalg.norm(res) / np.linalg.norm(c * rhs)
    assert true <= 2 * TOL, (msg, "true residual", true)
    AC = (A @ sp.diags(c)).tocsr()
    Hs = (AC.T @ sp.diags(w) @ AC + mu * sp.identity(n)).tocsc()
    ed = np.linalg.solve(Hs.toarray(), c * rhs) if n <= 1500 else spl.splu(Hs).solve(c * rhs)
    err = np.linalg.norm(d / c - ed) / np.linalg.norm(ed)
    assert err <= COND * 2 * TOL, (msg, "|e - direct| / |direct|", err)
    assert not d[zero].any(), (msg, "a column of norm 0 moved")
    print("%s; true residual %.2e, |e - direct| / |direct| %.2e, %d columns of norm 0" % (msg, true, err, zero.sum()))


# ---------------------------------------------------------------- the problems of the bounded LM driver (CPU and device)

GROUPS = {"hopper": (("C1_hopper", 0), ("hopper_all", 0), ("C1_hopper", 1), ("hopper_all", 1), ("C1_hopper", 2), ("hopper_all", 2)),
          "biped": (("biped_all", 1), ("norows", 0), ("biped_all", 2), ("biped_all", 3)),
          "anymal": (("anymal", 0), ("anymal", 2))}
REJECTS_FIRST = ("biped_all", 1)   # rejects its first step on the CPU (tests/test_lm_box_cpu.py)
STEPS = 8


def _lm_box_cpu():
    """scripts/lm_box_cpu.py, imported on first use."""
    scripts = os.path.join(ROOT, "scripts")
    if scripts not in sys.path:
        sys.path.insert(0, scripts)
    import lm_box_cpu

    return lm_box_cpu


@functools.lru_cache(maxsize=None)
def lm_case(name):
    """(case, (lo, up)) of a problem of scripts/lm_box_cpu.py::cases, or of the structure without rows."""
    lb = _lm_box_cpu()
    case = random_case(5111) if name == "norows" else lb.cases()[name]()
    return case, lb.case_bounds(case)


# ---------------------------------------------------------------- the Gram solve: what tests/test_gram_cpu.py measures

DEVICE_INPUTS = [(name, 0) for name in list(baseline_cases()) + ["hopper_all", "biped_all"]]
# |d - d_direct| / |d_direct| of the restatement: the largest over INPUTS and DEVICE_INPUTS as measured by test_step_* of
# tests/test_gram_cpu.py; the device test's bound is ten times this (tests/test_jac_gram.py), the project's convention
STEP_FIGURE = 2.6e-9
# the Gram loop's jitter factors (tests/test_gram_cpu.py), seed by seed, and the seeds the rule drops
JITTER_MEASURED = {("anymal", 0): 1.033, ("anymal", 1): 104.7, ("anymal", 2): 1.0001, ("C2_biped_K100", 0): 1.0005,
                   ("C2_biped_K100", 1): 1.0, ("C2_biped_K100", 2): 1.0, ("hopper_all", 0): 1.0, ("hopper_all", 1): 1.0,
                   ("hopper_all", 2): 1.0, ("C1_hopper", 0): 1.0, ("C1_hopper", 1): 1.0002, ("C1_hopper", 2): 1.0044,
                   ("biped_all", 0): 1.565, ("biped_all", 1): 1.0002, ("biped_all", 2): 1.0011}
DROPPED = tuple(k for k, f in JITTER_MEASURED.items() if f > 1.4)


@functools.lru_cache(maxsize=None)
def case_of(name):
    return baseline_cases()[name]() if name in baseline_cases() else _lm_box_cpu().cases()[name]()
