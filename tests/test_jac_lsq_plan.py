"""Host side of the least-squares step (twr_jac_lsq_*): the plan of twr::PlanJacLsq checked by tests/jac_lsq_plan_driver.cc (g++
against the host planner, tests/host_build.py, under AddressSanitizer + UndefinedBehaviorSanitizer) on the shapes test_jac_plan.py uses --
workspace segments disjoint and inside the allocation, every problem's record pointing at its own offsets, bound tables equal
to the structures' per-row bounds (what twr_structure_bounds hands out) and shared exactly when byte-identical -- and the
argument checks of the entry points, which need no device."""
import ctypes as C
import subprocess

import numpy as np

import towr_amd as ta

from .common import baseline_cases
from .host_build import plan_driver


def test_lsq_plans():
    exe = plan_driver("jac_lsq_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr


def test_entry_points_check_their_arguments_without_a_device():
    L = ta.lib()
    h = C.c_void_p()
    S = baseline_cases()["C1_hopper"]().S
    hs = (C.c_void_p * 1)(S._h)
    sop = (C.c_int32 * 1)(0)
    assert L.twr_jac_lsq_create(None, hs, 1, sop, 1, C.byref(h)) == ta.lib().twr_jac_lsq_create(None, None, 0, None, 0, None) == -1
    assert h.value is None and b"argument" in L.twr_last_error()
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert L.twr_jac_lsq_bytes(None, None) == -1
    assert L.twr_jac_dot(None, 0, p, p, p, None) == -1
    assert L.twr_jac_violation(None, p, None, p, None, None, None) == -1
    assert L.twr_jac_lsq_solve(None, p, p, None, p, 10, 1e-8, p, p, None) == -1
    L.twr_jac_lsq_destroy(None)   # a no-op
