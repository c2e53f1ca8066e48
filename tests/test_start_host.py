"""The start of a planning request on the host: twr_structure_start_host -- the structure's start table (one record per
variable: where its value and its bounds come from) run on the CPU by the decode the device kernel shares -- against the
existing twr_structure_initial_guess / twr_structure_variable_bounds, bit for bit, and against the oracle; the table's
properties, the work list of twr_batch_start and a sanitizer run of all of it in a stand-alone program
(tests/start_plan_driver.cc)."""
import subprocess

import numpy as np
import pytest

import towr_amd as ta
from tests import start_cases as sc
from tests.common import Case, RTOL, FLOOR, hopper_schedule
from tests.host_build import plan_driver

ROBOTS = {"monoped": 1, "biped": 2, "anymal": 4, "go1": 4}
TERRAINS = ("flat", "stairs", "gap", "slope", "csv", "grid_map")


def check_structure(S, P, terrain, grid, what):
    n = 0
    for yaw in sc.YAWS:
        for goal in sc.goals(terrain, grid):
            rq = sc.request(S, goal, yaw, seed=n)
            ref = sc.host_start(S, rq)
            got = S.start_host(rq)
            for name, g, r in zip(("x0", "x_l", "x_u"), got, ref):
                assert sc.same_bits(g, r), "%s: %s differs from the host function at %s (yaw %r, goal %r)" % (
                    what, name, np.nonzero(sc.bits(g) != sc.bits(r))[0][:8], yaw, goal)
            if P is not None and n % 3 == 0:   # the oracle, to the bar of tests/common.py (scale: the largest entry of the variable set)
                ee = rq[24:24 + 3 * S.n_ee]
                ox = P.initial_guess(rq[0:3], rq[6:9], rq[12:15], rq[18:21], ee)
                olo, oup = P.variable_bounds(rq[0:12], rq[12:24], ee)
                scale = np.zeros(S.n)
                for vs in S.var_sets:
                    seg = slice(vs["offset"], vs["offset"] + vs["size"])
                    scale[seg] = np.abs(ox[seg]).max() if vs["size"] else 0.0
                for name, g, r in zip(("x0", "x_l", "x_u"), got, (ox, olo, oup)):
                    bad = ~(np.abs(g - r) <= RTOL * np.abs(r) + FLOOR * scale)
                    assert not bad.any(), "%s: %s off the oracle at %s (yaw %r, goal %r)" % (what, name, np.nonzero(bad)[0][:8], yaw, goal)
            n += 1
    return n


@pytest.mark.parametrize("terrain", TERRAINS)
@pytest.mark.parametrize("robot", list(ROBOTS))
def test_start_host_matches_host_functions_bit_for_bit(robot, terrain):
    """every gait combo of the sanitizer tier (0 .. 4), fixed and optimised timings; yaw 0, 0.3, -2.0, pi/2; goals on and off the
    terrain's breakpoints; non-zero start velocities.  Compared as uint64, so -0.0 and 1e20 count."""
    grid = sc.terrain_grid(terrain)
    n_ee = ROBOTS[robot]
    for combo in range(5):
        for sets in (27, sc.TIMINGS):
            case = Case(robot, terrain, ta.gait_combo(n_ee, combo, 1.4 + 0.2 * combo), grid=grid, constraint_sets=sets,
                        dt_dynamic=0.2, dt_rom=0.2)
            check_structure(case.S, case.P, terrain, grid, "%s %s combo %d sets %d" % (robot, terrain, combo, sets))


def test_start_host_hopper_and_partial_outputs():
    """towr's hopper schedule; and each output alone (the C function takes NULL for the others)"""
    import ctypes as C
    case = Case("monoped", "stairs", hopper_schedule(), constraint_sets=sc.TIMINGS)
    S = case.S
    check_structure(S, case.P, "stairs", None, "hopper")
    rq = sc.request(S, (1.0, 0.0), 0.3)
    ref = sc.host_start(S, rq)
    for k in range(3):
        out = np.full(S.n, -7.0)
        ptrs = [None, None, None]
        ptrs[k] = out.ctypes.data
        assert ta.lib().twr_structure_start_host(S._h, rq.ctypes.data_as(C.POINTER(C.c_double)), *ptrs) == 0
        assert sc.same_bits(out, ref[k])
    assert ta.lib().twr_structure_start_host(None, rq.ctypes.data_as(C.POINTER(C.c_double)), None, None, None) != 0
    assert ta.lib().twr_structure_start_host(S._h, None, None, None, None) != 0


def test_start_request_layout():
    rec = ta.start_request(np.arange(12), 100 + np.arange(12), [[1, 2, 3], [4, 5, 6]])
    assert rec.shape == (ta.START_REC,) and ta.START_REC == 36
    assert np.array_equal(rec[:12], np.arange(12)) and np.array_equal(rec[12:24], 100 + np.arange(12))
    assert np.array_equal(rec[24:], [1, 2, 3, 4, 5, 6, 0, 0, 0, 0, 0, 0])
    with pytest.raises(ta.TowrError):
        ta.start_request(np.zeros(11), np.zeros(12), np.zeros(3))


def test_start_table_planner_and_sanitizer():
    """tests/start_plan_driver.cc, a program with its own main compiled here with g++ -fsanitize=address,undefined from the host
    sources (tests/host_build.py): the table's properties (one record per variable, a shared variable names the later node,
    values that are no variables are no bound targets), StartHost against InitialGuess / VariableBounds, and the work list of
    six batch shapes covered exactly once inside every problem."""
    exe = plan_driver("start_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr
