"""Host side of the Marquardt-scaled least-squares step (twr_jac_col_sqnorms / twr_jac_col_scale / twr_jac_lsq_solve_scaled): the
second workspace twr::PlanJacLsq plans for it, checked by tests/jac_scaled_plan_driver.cc (g++ against
the host planner, tests/host_build.py, under AddressSanitizer + UndefinedBehaviorSanitizer) -- segments on 16-byte boundaries, disjoint,
inside the second allocation, the same when planned twice, the first workspace unchanged -- and the argument checks of the new
entry points, which need no device."""
import subprocess

import numpy as np

import towr_amd as ta

from tests.host_build import plan_driver


def test_scaled_plans():
    exe = plan_driver("jac_scaled_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr


def test_new_entry_points_check_their_arguments_without_a_device():
    L = ta.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert L.twr_jac_col_sqnorms(None, p, None, p, None) == -1 and b"argument" in L.twr_last_error()
    assert L.twr_jac_lsq_reserve_scaled(None) == -1
    assert L.twr_jac_col_scale(None, p, None, 1e-12, p, None) == -1
    assert L.twr_jac_lsq_solve_scaled(None, p, p, None, p, p, 10, 1e-8, p, p, None) == -1
    assert callable(ta.JacOps.col_sqnorms_device)
    assert all(callable(getattr(ta.JacLsq, name)) for name in ("col_scale_device", "reserve_scaled", "solve_scaled_device"))
