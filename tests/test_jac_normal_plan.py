"""Host side of the one-pass normal product (twr_jac_normal_mul): the plan of twr::PlanJacNormal checked by
tests/jac_normal_plan_driver.cc (g++ against the host planner, tests/host_build.py, under AddressSanitizer + UndefinedBehaviorSanitizer)
over the six batches of the product plans' test and a batch with rows longer than one tile: every entry in exactly one block
and one partial, blocks of whole rows within the limits (a longer row alone), every partial folded once, by its column, in
block order, every table inside the tables, identical plans when planning twice and alone.  The driver's emulation of the
plan's summation order on a random matrix is held against scipy here, PlanJacOps's output against its fingerprints from
before the one-pass plan existed, and the argument checks of the entry points, which need no device."""
import os
import subprocess
import tempfile

import numpy as np
import scipy.sparse as sp

import towr_amd as ta

from tests.host_build import plan_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# FNV-1a over everything twr::PlanJacOps returns (ops_fingerprint of the driver: offsets, table bytes, the three work lists as
# bytes -- their records have no padding --, slab and counters), taken from the commit before twr::PlanJacNormal existed.
# PlanJacOps is meant to stay as it is; after an INTENDED change to it, take them again by the same recipe, from a checkout of
# the commit that has the change:
#   cd towr_amd/csrc && g++ -O1 -std=c++17 -DOPS_ONLY -o ops_only ../../tests/jac_normal_plan_driver.cc structure.cc presets.cc jac_plan.cc
#   ./ops_only
# or, in the tests' own build, tests.host_build.plan_driver("jac_normal_plan_driver", defines=("OPS_ONLY",))
# (-DOPS_ONLY leaves out everything that needs PlanJacNormal, so the driver builds against sources that lack it) and copy the
# "opsplan <case> <fingerprint>" lines here.
OPS_FINGERPRINTS = {
    "C3x16": "af3262ce29b9c99e",
    "twins": "28b684b44e304db1",
    "every": "68efcf684296470f",
    "ragged": "d55fc266ef874cc1",
    "grid": "5816a3fd96933b35",
    "wide": "0ad1dc1a6ea3ccb7",
    "longrow": "bae639324fbf9b55",
}


def _records(path):
    """The (A, v, w, y, u) the driver wrote: one per distinct structure of the case."""
    raw = open(path, "rb").read()
    at = 0

    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=at)
        at += a.nbytes
        return a

    while at < len(raw):
        n, m, nnz = (int(v) for v in take(np.int64, 3))
        row_ptr, col = take(np.int32, m + 1), take(np.int32, nnz)
        a, v, w, y, u = take(np.float64, nnz), take(np.float64, n), take(np.float64, m), take(np.float64, m), take(np.float64, n)
        yield sp.csr_matrix((a, col, row_ptr), shape=(m, n)), v, w, y, u


def test_normal_product_plans():
    with tempfile.TemporaryDirectory() as tmp:
        exe = plan_driver("jac_normal_plan_driver")
        out = os.path.join(tmp, "out")
        os.mkdir(out)
        r = subprocess.run([exe, out], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "ERROR: AddressSanitizer" not in r.stderr
        print(r.stdout)
        got = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("opsplan "))
        assert got == OPS_FINGERPRINTS, "PlanJacOps no longer returns what it returned before the one-pass plan"
        cases = sorted(f[:-4] for f in os.listdir(out))
        assert cases == sorted(["C3x16", "twins", "every", "ragged", "grid", "wide", "longrow"])
        longest = 0
        for name in cases:
            count = 0
            for A, v, w, y, u in _records(os.path.join(out, name + ".bin")):
                absA = abs(A)
                y_ref, y_mag = A @ v, absA @ np.abs(v)
                u_ref, u_mag = A.T @ (w * y_ref), absA.T @ (w * y_mag)
                assert (np.abs(y - y_ref) <= 1e-12 * y_mag).all(), (name, count, np.abs(y - y_ref).max())
                assert (np.abs(u - u_ref) <= 1e-12 * u_mag).all(), (name, count, np.abs(u - u_ref).max())
                empty = np.diff(A.tocsc().indptr) == 0
                assert not u[empty].any() and not np.signbit(u[empty]).any()   # an exact 0 for a column without entries
                longest = max(longest, int(np.diff(A.indptr).max()) if A.shape[0] else 0)
                count += 1
            assert count >= 1, name
        assert longest > 2048   # a row longer than one tile was there


def test_entry_points_check_their_arguments_without_a_device():
    L = ta.lib()
    buf = np.zeros(8)
    p = buf.ctypes.data
    assert L.twr_jac_ops_reserve_normal(None) == -1
    assert L.twr_jac_normal_mul(None, p, None, p, None, p, None) == -1
    assert L.twr_jac_lsq_reserve_onepass(None, 0) == -1
    assert L.twr_jac_lsq_solve_onepass(None, p, p, None, p, None, 10, 1e-8, p, p, None) == -1
    assert b"null" in L.twr_last_error()
