"""Host side of the bounded LM driver (twr_jac_lm_*, twr_jac_free_set, twr_jac_lsq_solve_masked): the workspace plan of
twr::PlanJacLm checked by tests/jac_lm_plan_driver.cc (g++ against the host planner, tests/host_build.py, under AddressSanitizer +
UndefinedBehaviorSanitizer) -- segments disjoint, on 16-byte boundaries and inside the reported size, on ragged batches, odd n and
a structure without rows -- and the argument checks of the new entry points, which need no device."""
import ctypes as C
import subprocess

import numpy as np

import towr_amd as ta

from tests.host_build import plan_driver


def test_lm_plans():
    exe = plan_driver("jac_lm_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr


def test_entry_points_check_their_arguments_without_a_device():
    L = ta.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    odd = p + 4
    h = C.c_void_p()
    params = ta.JacLmParams()
    assert L.twr_jac_lm_params_default(None) == -1
    assert L.twr_jac_lm_params_default(C.byref(params)) == 0
    assert (params.cg_iters, params.power_iters, params.cg_tol, params.mu_up, params.rel_floor, params.tau, params.merit_done) == \
        (60, 30, 1e-8, 10.0, 1e-12, 1e-2, 0.0) and params.mu_down == 1.0 / 3.0 and 0 < params.mu_min < params.mu_max < np.inf
    assert ta.JacLm.REC == 8 == len(ta.JacLm.FIELDS)
    # NULL handles and arguments: refused before any device is touched (fake non-NULL handles are never dereferenced first)
    assert L.twr_jac_lm_create(None, None, C.byref(params), C.byref(h)) == -1
    assert L.twr_jac_lm_create(p, None, C.byref(params), C.byref(h)) == -1
    assert L.twr_jac_lm_create(None, p, C.byref(params), C.byref(h)) == -1
    assert L.twr_jac_lm_create(p, p, None, C.byref(h)) == -1
    assert L.twr_jac_lm_create(p, p, C.byref(params), None) == -1
    assert h.value is None and b"argument" in L.twr_last_error()
    assert L.twr_jac_lm_bytes(None, None) == -1
    assert L.twr_jac_lm_start(None, p, p, p, p, p, None) == -1
    assert L.twr_jac_lm_step(None, None) == -1
    assert L.twr_jac_lm_state(None, p, None) == -1
    L.twr_jac_lm_destroy(None)   # a no-op
    assert L.twr_jac_free_set(None, p, p, p, p, None, p, p, None) == -1
    assert L.twr_jac_lsq_solve_masked(None, p, p, None, p, p, 10, 1e-8, p, p, None) == -1
    for k in range(1, 8):   # every required buffer of the two calls, NULL in turn (the handle is not read before these checks)
        args = [p, p, p, p, p, None, p, p, None]
        if k == 5:
            continue   # d_scale_in may be NULL
        args[k] = None
        assert L.twr_jac_free_set(*args) == -1, k
        args[k] = odd
        assert L.twr_jac_free_set(*args) == -1, k
    for k in (1, 2, 4, 5, 8, 9):
        args = [p, p, p, None, p, p, 10, 1e-8, p, p, None]
        args[k] = None
        assert L.twr_jac_lsq_solve_masked(*args) == -1, k
    assert L.twr_jac_lsq_solve_masked(p, p, p, None, p, p, -1, 1e-8, p, p, None) == -1
    assert L.twr_jac_lsq_solve_masked(p, p, p, None, p, p, 10, float("nan"), p, p, None) == -1
    assert L.twr_jac_lsq_solve_masked(p, p, p, None, p, odd, 10, 1e-8, p, p, None) == -1
