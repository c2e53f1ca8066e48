"""scripts/lm_box_cpu.py, the numpy restatement of the bound-constrained LM driver on the CPU oracle (no GPU): on the hopper (C1),
the hopper and the biped with every constraint set of TWR_SETS_ALL (optimised timings: every phase duration boxed), seeds 0 .. 3,
  * the fixed variables (lo == up) keep the bits of their bound, every x stays inside its box, the recorded merit never rises;
  * the masked CGLS step agrees with a dense direct solve on the free columns, under the bounds of
    tests/jac_ref.py::check_scaled_step (tol 1e-10, mu = 1e-2 lambda_max: true residual <= 2 tol, |e - direct| <= 101 * 2
    tol |direct|, converged under 200 iterations): it is that iteration on fewer columns; masked variables get an exact +0;
  * the free loop on the same inputs moves every fixed variable off its value, and with optimised timings leaves durations
    outside their box: what the driver is for."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from .jac_ref import ITERS, ROOT, TOL, check_scaled_step, lam_max, lm_case

sys.path.insert(0, os.path.join(ROOT, "scripts"))

import lm_box_cpu as lb  # noqa: E402
from lm_damping_cpu import cgls  # noqa: E402

CASES = ("C1_hopper", "hopper_all", "biped_all")
SEEDS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def _run(name, seed, bounded):
    case, (lo, up) = lm_case(name)
    return lb.lm_box(case, case.x_perturbed(seed), lo, up, bounded=bounded, keep=True)


def test_start_vector_is_the_drivers():
    """lm_v0 of jac/lm.h in plain integers."""
    def ref(k):
        h = (k * 2654435761 + 0x9e3779b9) & 0xffffffff
        h ^= h >> 15
        h = (h * 0x85ebca6b) & 0xffffffff
        h ^= h >> 13
        return 0.5 + (h >> 8) / 16777216.0

    v = lb.v0(3000)
    assert ((v >= 0.5) & (v < 1.5)).all() and len(set(v)) > 2900
    assert all(v[k] == ref(k) for k in (0, 1, 2, 511, 512, 2999))


@pytest.mark.parametrize("name", CASES)
def test_bounds_are_what_the_issue_counts(name):
    case, (lo, up) = lm_case(name)
    fixed = lo == up
    assert fixed.sum() == 23 + 3 * case.S.n_ee
    assert (lo <= up).all()
    boxed = ~fixed & ((lo > -1e19) | (up < 1e19))
    if name == "C1_hopper":
        assert not boxed.any()
    else:   # optimised timings: every duration in [0.2, 1.0]
        assert boxed.any() and set(lo[boxed]) == {0.2} and set(up[boxed]) == {1.0}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", CASES)
def test_bounded_loop_honours_the_box(name, seed):
    case, (lo, up) = lm_case(name)
    R = _run(name, seed, True)
    x, fixed = R["x"], lo == up
    assert np.array_equal(x[fixed].view(np.int64), lo[fixed].view(np.int64)), "a fixed variable lost the bits of its bound"
    assert ((x >= lo) & (x <= up)).all()
    m = np.array(R["merit"])
    assert len(m) == 9 and np.isfinite(m).all() and (np.diff(m) <= 0).all(), m
    assert m[-1] < m[0], m
    acc = np.array(R["accepted"])
    assert np.array_equal(np.diff(m) < 0, acc == 1)
    mu = np.array(R["mu"])
    assert np.allclose(mu[1:] / mu[:-1], np.where(acc == 1, 1.0 / 3.0, 10.0), rtol=1e-14)
    nfree = np.array(R["nfree"])
    assert (nfree <= case.S.n - fixed.sum()).all() and (nfree > 0).all()
    print("%s seed %d: merit %.3e -> %.3e, accepted %s, free %s" % (name, seed, m[0], m[-1], R["accepted"], R["nfree"]))


@pytest.mark.parametrize("name", CASES[1:])
def test_the_active_set_is_exercised(name):
    """With optimised timings some run blocks a duration on its bound: the free count falls below n - fixed, and moves."""
    case, (lo, up) = lm_case(name)
    most = case.S.n - int((lo == up).sum())
    counts = set(v for seed in SEEDS for v in _run(name, seed, True)["nfree"])
    assert min(counts) < most and len(counts) > 1, counts


def test_the_biped_with_all_sets_rejects_its_first_step_at_seed_1():
    assert _run("biped_all", 1, True)["accepted"][0] == 0   # what the device test of rejected steps relies on


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", CASES)
def test_masked_step_against_a_dense_direct_solve(name, seed):
    case, (lo, up) = lm_case(name)
    L = _run(name, seed, True)["lin"][0]
    free = L.cf != 0
    assert np.array_equal(L.cf[free], L.c[free]) and (~free).sum() >= (lo == up).sum()
    ACf = (L.A @ sp.diags(L.cf)).tocsr()
    mu = 1e-2 * lam_max(ACf, L.w)
    k, e = cgls(ACf, L.b, L.w, mu, ITERS, TOL)
    d = L.cf * e
    assert not d[~free].any() and not np.signbit(d[~free]).any()
    Af = L.A[:, np.nonzero(free)[0]].tocsr()
    cfree = L.c[free]
    s0 = cfree * (Af.T @ (L.w * L.b))
    s = cfree * (Af.T @ (L.w * (L.b - Af @ d[free]))) - mu * d[free] / cfree
    info = [k, np.linalg.norm(s) / np.linalg.norm(s0), np.linalg.norm(s0), 0 if k < ITERS else 1]
    zero = np.asarray(Af.multiply(Af).T @ L.w).ravel() == 0
    check_scaled_step(Af, L.b, L.w, mu, cfree, d[free], info, zero, "%s seed %d, %d free of %d" % (name, seed, free.sum(), case.S.n))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", CASES)
def test_free_loop_leaves_every_fixed_variable_off_its_value(name, seed):
    case, (lo, up) = lm_case(name)
    x = _run(name, seed, False)["x"]
    fixed = lo == up
    off = np.abs(x[fixed] - lo[fixed])
    assert (off > 0).all(), (off.min(), off.max())
    boxed = ~fixed & (up < 1e19)
    outside = int((boxed & ((x < lo) | (x > up))).sum())
    print("%s seed %d: free loop moved all %d fixed variables by up to %.2f, %d durations outside their box"
          % (name, seed, fixed.sum(), off.max(), outside))
