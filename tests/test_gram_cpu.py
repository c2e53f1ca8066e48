"""scripts/gram_cpu.py on its own, on the CPU: the numpy restatement of twr_jac_gram / twr_jac_lsq_solve_gram against a dense direct
solve of the same system, and the bounded LM loop with that solve against the CGLS loop of scripts/lm_box_cpu.py.

Inputs: anymal, C2_biped_K100, hopper_all, C1_hopper, biped_all (scripts/lm_box_cpu.py::cases) at x_perturbed(seed), seeds 0-2:
15 problems; the step test also takes the seven problems tests/test_jac_gram.py solves on the device (the five BASELINE cases,
hopper_all and biped_all at seed 0).

Step accuracy.  The system is the first step's of the Gram loop, (C_f N C_f + mu I) e = c_f o z, d = c_f o e, with
mu = 1e-2 lambda_max(C_f N C_f) from a dense eigensolve, so cond <= 101; tol = 1e-10, cap 3000.  CG stops when its recurred
gradient is below tol |s0|; with |e - e*| <= |residual| / mu and |e*| >= |s0| / (lambda_max + mu) that is
|e - e*| <= 101 tol |e*|, and the bound asserted is 2 * 101 * tol in e = d / c over the free variables (the 2 for the drift of the
recurred gradient, the bound of tests/jac_ref.py).  Measured: at most 1.85e-9 in e; in d (what the device test compares,
STEP_FIGURE) at most 2.57e-9 over both input sets (C4 stairs; 1.85e-9 over the 15), in 37 to 95 iterations.

LM loop.  Final merit after 8 steps within [0.5, 2] of the CGLS loop's.  Measured: 0.9718 .. 1.0044 on the 15 inputs, equal accept
sequences on all of them.  Under a 2e-8 relative jitter of every step (16 draws, python scripts/gram_cpu.py --seeds 3
--jitter-draws 16) the Gram loop's own final merit moves by the factors of JITTER_MEASURED (tests/jac_ref.py, with the
other figures the device tests share); a seed above 1.4 is dropped
from the loop comparison by the rule of DESIGN 6.L (DROPPED: ANYmal seed 1 and biped SETS_ALL seed 0, the two seeds the CGLS loop
flips on as well), and no input is dropped for another reason."""
import os
import sys

import numpy as np
import pytest

from .jac_ref import COND, DEVICE_INPUTS, DROPPED, JITTER_MEASURED, ROOT, STEP_FIGURE, TOL, case_of

sys.path.insert(0, os.path.join(ROOT, "scripts"))

import gram_cpu as gc  # noqa: E402
import lm_box_cpu as lb  # noqa: E402

CAP = 3000
INPUTS = [(name, seed) for name in gc.CASES for seed in range(3)]


def step_errors(name, seed):
    """(relative error in e over the free variables, in d, iterations, status) of the restatement against the dense solve."""
    _, _, N, z, cf, _ = gc.first_system(case_of(name), seed)
    mu = gc.mu_of(N, cf)
    k, d, rel, status = gc.gram_cg(N, z, mu, cf, CAP, TOL)
    dd = gc.dense_step(N, z, mu, cf)
    free = cf != 0
    assert not d[~free].any() and not np.signbit(d[~free]).any()
    err_e = np.linalg.norm((d - dd)[free] / cf[free]) / np.linalg.norm(dd[free] / cf[free])
    return err_e, np.linalg.norm(d - dd) / np.linalg.norm(dd), k, status, rel


@pytest.mark.parametrize("name,seed", INPUTS + [i for i in DEVICE_INPUTS if i not in INPUTS])
def test_step_against_a_dense_solve(name, seed):
    err_e, err_d, k, status, rel = step_errors(name, seed)
    print("%s seed %d: %d iterations, |s|/|s0| %.2e, status %d, |e - direct| / |direct| %.3e, |d - direct| / |direct| %.3e"
          % (name, seed, k, rel, status, err_e, err_d))
    assert status == 0 and 0 < k < CAP and rel <= TOL
    assert err_e <= 2 * COND * TOL, err_e
    assert err_d <= STEP_FIGURE, (err_d, "the recorded figure no longer covers this input")


@pytest.mark.parametrize("name,seed", [i for i in INPUTS if i not in DROPPED])
def test_lm_loop_against_cgls(name, seed):
    case = case_of(name)
    lo, up = lb.case_bounds(case)
    x0 = case.x_perturbed(seed)
    B = lb.lm_box(case, x0, lo, up, steps=8)
    G = gc.lm_gram(case, x0, lo, up, steps=8)
    ratio = G["merit"][-1] / B["merit"][-1]
    print("%s seed %d: CGLS %.6e (%s), Gram %.6e (%s), ratio %.4f" % (name, seed, B["merit"][-1], B["accepted"], G["merit"][-1], G["accepted"], ratio))
    assert 0.5 <= ratio <= 2.0, ratio
    fixed = lo == up
    assert np.array_equal(G["x"][fixed], lo[fixed]) and ((G["x"] >= lo) & (G["x"] <= up)).all()
    assert all(b <= a for a, b in zip(G["merit"], G["merit"][1:]))   # the recorded merit never rises


def test_the_jitter_table_is_the_committed_run():
    """JITTER_MEASURED (which decides the seeds that are dropped) is profiles/gram_cpu_jitter.json, the output of
    scripts/gram_cpu.py --seeds 3 --jitter-draws 16: the two cannot drift apart."""
    import json

    with open(os.path.join(ROOT, "profiles", "gram_cpu_jitter.json")) as f:
        run = json.load(f)
    assert (run["jitter"], run["jitter_draws"], run["steps"], run["cg_iters"]) == (2e-8, 16, 8, 60)
    got = {(r["case"], r["seed"]): r["jitter_factor"] for r in run["gram_cpu"]}
    assert set(got) == set(JITTER_MEASURED) == set(INPUTS)
    for key, f in got.items():
        assert abs(f - JITTER_MEASURED[key]) <= 5e-4 * f, (key, f, JITTER_MEASURED[key])
    assert set(DROPPED) == {k for k, f in got.items() if f > 1.4} == {("anymal", 1), ("biped_all", 0)}


@pytest.mark.parametrize("name", ["C1_hopper", "biped_all"])
def test_the_restatement_in_the_device_order_is_the_same_iteration(name):
    """gram_cg_device (the kernel's roundings in the kernel's order) against gram_cg (plain numpy): the same iterates to
    rounding, and the same answers to the rules."""
    _, _, N, z, cf, _ = gc.first_system(case_of(name), 0)
    mu = gc.mu_of(N, cf)
    k, d, rel, status = gc.gram_cg(N, z, mu, cf, 200, TOL)
    kd, dd, reld, statusd = gc.gram_cg_device(N, z, mu, cf, 200, TOL)
    assert status == statusd == 0 and abs(k - kd) <= 2 and reld <= TOL
    assert np.linalg.norm(d - dd) <= 1e-6 * np.linalg.norm(d)
    assert not dd[cf == 0].any() and not np.signbit(dd[cf == 0]).any()
    k3, d3, _, s3 = gc.gram_cg_device(N, z, mu, cf, 3, TOL)
    assert (k3, s3) == (3, 1) and np.linalg.norm(d3 - gc.gram_cg(N, z, mu, cf, 3, TOL)[1]) <= 1e-12 * np.linalg.norm(d3)
    assert gc.gram_cg_device(N, z, mu, cf, 0, TOL)[::3] == (0, 1) and not gc.gram_cg_device(N, z, mu, cf, 0, TOL)[1].any()
    assert gc.gram_cg_device(N, 0 * z, mu, cf, 50, TOL)[::3] == (0, 0)
    for bad in (-1.0, np.nan, np.inf):
        c = cf.copy()
        c[5] = bad
        assert gc.gram_cg_device(N, z, bad, cf, 50, TOL)[3] == 2 and gc.gram_cg_device(N, z, mu, c, 50, TOL)[3] == 2
    kk, d2, _, _ = gc.gram_cg_device(N, z, mu, cf, 2000, TOL)
    assert kk == kd and np.array_equal(d2, dd)


def test_gram_cg_rules():
    """The rules the device call states, on the restatement: masked variables, c = 1, bad input, z = 0, iters = 0, a larger cap."""
    _, _, N, z, cf, _ = gc.first_system(case_of("C1_hopper"), 0)
    mu = gc.mu_of(N, cf)
    k, d, rel, status = gc.gram_cg(N, z, mu, cf, 200, TOL)
    k2, d2, _, _ = gc.gram_cg(N, z, mu, cf, 2000, TOL)
    assert status == 0 and k2 == k and np.array_equal(d, d2)
    assert gc.gram_cg(N, z, mu, cf, 0, TOL)[3] == 1 and not gc.gram_cg(N, z, mu, cf, 0, TOL)[1].any()
    assert gc.gram_cg(N, z, mu, cf, 3, TOL)[0] == 3 and gc.gram_cg(N, z, mu, cf, 3, TOL)[3] == 1
    assert gc.gram_cg(N, 0 * z, mu, cf, 50, TOL)[::3] == (0, 0)
    for bad_mu in (-1.0, np.nan, np.inf):
        assert gc.gram_cg(N, z, bad_mu, cf, 50, TOL)[3] == 2
    for bad_c in (-1.0, np.nan, np.inf):
        c = cf.copy()
        c[5] = bad_c
        kb, db, _, sb = gc.gram_cg(N, z, mu, c, 50, TOL)
        assert sb == 2 and kb == 0 and not db.any()
    # the masked system is the free one: the same d from the matrix with the masked rows and columns taken out
    free = np.flatnonzero(cf != 0)
    assert free.size < cf.size
    kf, df, _, sf = gc.gram_cg(N[free][:, free].tocsr(), z[free], mu, cf[free], 200, TOL)
    assert sf == 0 and np.abs(df - d[free]).max() <= 1e-12 * np.abs(d).max()
