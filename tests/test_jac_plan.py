"""Host side of the Jacobian products (twr_jac_mul / twr_jac_tmul): the CSC view twr_structure_transpose against scipy, and
the product plans of twr::PlanJacOps checked by tests/jac_plan_driver.cc (g++ against the host planner, tests/host_build.py, under AddressSanitizer +
UndefinedBehaviorSanitizer): every entry covered once per product, every row and column written once, the order of every
sum a function of the structure alone, identical plans when planning twice, one table for byte-identical patterns, and the
layout of PlanBatch."""
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import towr_amd as ta

from .common import Case, baseline_cases, random_case
from .host_build import plan_driver


def _assert_transpose(S, what=""):
    col_ptr, row_idx, csr_pos = S.transpose()
    vals = np.arange(1, S.nnz + 1, dtype=np.float64)   # every entry tagged with its CSR position + 1
    ref = sp.csr_matrix((vals, S.col_idx, S.row_ptr), shape=(S.m, S.n)).tocsc()
    ref.sort_indices()
    assert np.array_equal(col_ptr, ref.indptr), what
    assert np.array_equal(row_idx, ref.indices), what
    assert np.array_equal(vals[csr_pos], ref.data), what
    for c in range(S.n):   # rows ascend within a column
        assert np.all(np.diff(row_idx[col_ptr[c]:col_ptr[c + 1]]) > 0), (what, c)


@pytest.mark.parametrize("name", sorted(baseline_cases()))
def test_transpose_baseline(name):
    _assert_transpose(baseline_cases()[name]().S, name)


@pytest.mark.parametrize("seed", range(40))
def test_transpose_random(seed):
    _assert_transpose(random_case(seed).S, "seed %d" % seed)


def test_transpose_timings_every_set_grid_map_and_no_rows():
    m = ta.model_preset("anymal", "gap")
    S = ta.Structure(m, ta.gait_combo(4, 0, 2.4, 0.9), ta.params_default(constraint_sets=ta.SETS_EVERY, base_z_init=0.42))
    assert any(v["name"].startswith("ee-schedule") for v in S.var_sets)
    _assert_transpose(S, "every set, optimised timings")
    rng = np.random.default_rng(3)
    gm = ta.GridMap(rng.uniform(-0.05, 0.3, size=(40, 30)).astype(np.float32), 0.06, (0.8, -0.2))
    G = ta.Structure(ta.model_preset("anymal", "grid_map"), ta.gait_combo(4, 1, 2.0), grid=gm)
    _assert_transpose(G, "grid map")
    case = random_case(5111)   # no rows at all
    assert case.S.m == 0 and case.S.nnz == 0
    col_ptr, row_idx, csr_pos = case.S.transpose()
    assert np.array_equal(col_ptr, np.zeros(case.S.n + 1)) and row_idx.size == 0 and csr_pos.size == 0


def test_transpose_of_c3_sizes():
    S = Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), dt_dynamic=2.0 / 198.5, dt_rom=2.0 / 198.5).S
    assert (S.n, S.m, S.nnz) == (640, 3866, 102896)
    col_ptr, _, _ = S.transpose()
    assert np.diff(S.row_ptr).max() == 60 and np.diff(col_ptr).max() == 315


def test_product_plans():
    exe = plan_driver("jac_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr
