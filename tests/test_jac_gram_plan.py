"""Host side of the Gram matrix (twr_jac_gram, twr_jac_gram_mul, twr_jac_lsq_solve_gram, twr_jac_lm_set_solver): the plan of
twr::PlanJacGram checked by tests/jac_gram_plan_driver.cc (g++ against the host planner, tests/host_build.py, under AddressSanitizer +
UndefinedBehaviorSanitizer) -- the pattern against the structural P^T P taken naively, symmetry and ascending columns, every
term of every stored entry against the rows of J, gram_off, shared tables, the work lists' coverage and the limits -- the
argument checks of the new entry points, which need no device, and Structure.gram_pattern() against scipy."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .common import Case, baseline_cases, hopper_schedule, random_case
from .host_build import plan_driver


def test_gram_plans():
    exe = plan_driver("jac_gram_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr


def test_entry_points_check_their_arguments_without_a_device():
    L = ta.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    odd = p + 4
    nnz = C.c_int64(0)
    assert (ta.JacLm.SOLVERS["cgls"], ta.JacLm.SOLVERS["gram"]) == (0, 1)
    # NULL handles and arguments: refused before any device is touched (fake non-NULL handles are never dereferenced first)
    assert L.twr_structure_gram_pattern(None, None, None, C.byref(nnz)) == -1
    assert L.twr_jac_ops_reserve_gram(None) == -1
    assert L.twr_jac_ops_gram_layout(None, C.cast(p, C.POINTER(C.c_int64))) == -1
    assert L.twr_jac_ops_gram_layout(p, None) == -1
    assert b"null" in L.twr_last_error()
    for k in range(4):   # ops, d_jac, d_w (may be NULL), d_gram
        args = [p, p, p, p, None]
        if k != 2:
            args[k] = None
            assert L.twr_jac_gram(*args) == -1, k
        if k > 0:
            args[k] = odd
            assert L.twr_jac_gram(*args) == -1, k
    for k in range(4):   # ops, d_gram, d_v, d_u
        args = [p, p, p, p, None]
        args[k] = None
        assert L.twr_jac_gram_mul(*args) == -1, k
        if k > 0:
            args[k] = odd
            assert L.twr_jac_gram_mul(*args) == -1, k
    base = [p, p, p, p, None, 10, 1e-8, p, p, None]   # lsq, d_gram, d_z, d_mu, d_scale, iters, tol, d_d, d_info, stream
    for k in (0, 1, 2, 3, 7, 8):
        args = list(base)
        args[k] = None
        assert L.twr_jac_lsq_solve_gram(*args) == -1, k
    for k in (1, 2, 3, 4, 7, 8):
        args = list(base)
        args[k] = odd
        assert L.twr_jac_lsq_solve_gram(*args) == -1, k
        assert b"aligned" in L.twr_last_error()
    args = list(base)
    args[5] = -1
    assert L.twr_jac_lsq_solve_gram(*args) == -1
    args = list(base)
    args[6] = float("nan")
    assert L.twr_jac_lsq_solve_gram(*args) == -1
    args[6] = -1e-8
    assert L.twr_jac_lsq_solve_gram(*args) == -1
    assert L.twr_jac_lm_set_solver(None, 1) == -1
    assert L.twr_jac_lm_set_solver(p, 2) == -1 and L.twr_jac_lm_set_solver(p, -1) == -1
    with pytest.raises(TypeError):
        ta.JacLm(None, None, solver="direct")


def _pattern_cases():
    yield "C1_hopper", baseline_cases()["C1_hopper"]()
    yield "biped_all", Case("biped", "flat", ta.gait_combo(2, 0, 2.0), constraint_sets=ta.SETS_ALL)
    yield "hopper_all", Case("monoped", "flat", hopper_schedule(), constraint_sets=ta.SETS_ALL)
    yield "anymal", Case("anymal", "flat", ta.gait_combo(4, 1, 2.0))
    for seed in (0, 1, 2, 3, 4, 5111):   # 5111: a structure without rows
        yield "random_case(%d)" % seed, random_case(seed)


def test_gram_pattern_against_scipy():
    no_rows = 0
    for name, case in _pattern_cases():
        S = case.S
        rp, ci = S.gram_pattern()
        P = sp.csr_matrix((np.ones(S.nnz), S.col_idx, S.row_ptr), shape=(S.m, S.n))   # structural: explicit zeros would count
        N = (P.T @ P).tocsr()
        N.sort_indices()
        assert rp.dtype == np.int32 and ci.dtype == np.int32 and rp.shape == (S.n + 1,), name
        assert np.array_equal(rp, N.indptr) and np.array_equal(ci, N.indices), name
        assert (np.diff(rp) == 0).sum() == (np.bincount(S.col_idx, minlength=S.n) == 0).sum(), name   # empty columns of J
        nnz = C.c_int64(-1)
        assert ta.lib().twr_structure_gram_pattern(S._h, None, None, C.byref(nnz)) == 0 and nnz.value == N.nnz, name
        assert ta.lib().twr_structure_gram_pattern(S._h, None, None, None) == 0, name
        no_rows += S.m == 0
        print("%-18s n %4d m %4d nnz J %6d nnz N %6d longest row of J %3d, of N %3d"
              % (name, S.n, S.m, S.nnz, N.nnz, int(np.diff(S.row_ptr).max(initial=0)), int(np.diff(rp).max(initial=0))))
    assert no_rows == 1
