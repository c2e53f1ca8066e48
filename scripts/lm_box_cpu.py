"""The bound-constrained Levenberg-Marquardt driver (twr_jac_lm_*) restated in numpy on the CPU oracle's Jacobian, next to the
free loop of scripts/lm_damping_cpu.py (Marquardt damping) on the same inputs.  No GPU: it is the reference the device tests of
tests/test_jac_lm.py compare with, and what tests/test_lm_box_cpu.py checks on its own.

Bounds: twr_structure_variable_bounds for the start and goal of Case.x_guess (the start state, the final base state and the
initial footholds fixed with lo == up; with optimised timings every phase duration boxed in [0.2, 1.0]).

Per step (projected active-set LM): g, J at x; r = viol(g), w = [r != 0]; c from the weighted column norms with the running
maximum and a relative floor of 1e-12; z = J^T(w o b), b = -r; variable k is blocked when (x_k <= lo_k and z_k <= 0) or
(x_k >= up_k and z_k >= 0) and gets c_k = 0; CGLS of at most --cg-iters iterations, tol 1e-8, on J C_f in e = d / c;
x_t = clip(x + d, lo, up); accept when the merit at x_t is below the recorded one (mu / 3), else mu * 10, mu clamped to
[1e-16, 1e16].  mu starts at 1e-2 lambda_max(C_f J^T W J C_f), lambda_max by --power-iters power iterations from the driver's
fixed start vector.  A recorded merit <= 0 at a linearisation ends the problem.
Prints one line per problem: the bounded loop (merit, accepted steps, free counts, variables on a bound at the end, the largest
distance of a fixed variable from its value: 0) and the free loop (merit, the fixed variables it moved and by how much, the
variables it left outside their box); then one JSON line.
Usage:  python scripts/lm_box_cpu.py --seeds 3 --jobs 12
"""
import argparse
import json
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lm_damping_cpu import cgls, col_scale  # noqa: E402

MU_DOWN, MU_UP, MU_MIN, MU_MAX, TAU, CG_TOL = 1.0 / 3.0, 10.0, 1e-16, 1e16, 1e-2, 1e-8


def cases():
    import towr_amd as ta
    from tests.common import Case, baseline_cases, hopper_schedule, k_params

    return {"C1_hopper": baseline_cases()["C1_hopper"],
            "C2_biped_K100": baseline_cases()["C2_biped_K100"],
            "hopper_all": lambda: Case("monoped", "flat", hopper_schedule(), constraint_sets=ta.SETS_ALL),
            "biped_all": lambda: Case("biped", "flat", ta.gait_combo(2, 0, 2.0), constraint_sets=ta.SETS_ALL),
            "anymal": lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0)),
            "C3": lambda: Case("anymal", "flat", ta.gait_combo(4, 1, 2.0), **k_params(2.0, 200))}


def case_bounds(case, goal_x=1.0):
    """(lo, up) of twr_structure_variable_bounds for the start and the goal Case.x_guess(goal_x) interpolates between."""
    lin0, ee = case.nominal_start()
    init = lin0 + [0.0] * 9
    final = [goal_x, 0.0, lin0[2]] + [0.0] * 9
    return case.S.variable_bounds(init, final, ee)


def v0(n):
    """The start vector of the driver's power iteration (lm_v0, jac/lm.h): a fixed pattern in [0.5, 1.5)."""
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x9e3779b9)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    h ^= h >> np.uint64(13)
    return 0.5 + (h >> np.uint64(8)).astype(np.float64) / 16777216.0


def lambda_max(A, w, iters):
    """lambda of the last of `iters` power iterations on A^T W A from v0 (the driver's start: lm_normalise_kernel)."""
    v = v0(A.shape[1])
    lam = 1.0
    for _ in range(iters):
        u = A.T @ (w * (A @ v))
        lam = (v @ u) / max(v @ v, 1e-300)
        v = u / max(np.linalg.norm(u), 1e-300)
    return lam


def blocked(x, lo, up, z):
    return ((x <= lo) & (z <= 0)) | ((x >= up) & (z >= 0))


class Linearisation:
    """What a step of the bounded loop solves, for tests that check the solve on its own."""

    def __init__(self, A, b, w, c, cf, mu):
        self.A, self.b, self.w, self.c, self.cf, self.mu = A, b, w, c, cf, mu


def lm_box(case, x0, lo, up, steps=8, cg_iters=60, power_iters=30, bounded=True, jitter=0.0, jitter_seed=0, keep=False):
    """The loop from x0.  bounded False: the free loop (no projection, no mask: scripts/lm_damping_cpu.py's marquardt loop).
    jitter: every step d multiplied by (1 + jitter N(0, 1)) per component (the sensitivity runs).
    Returns a dict: x, merit (steps + 1 recorded merits), accepted, nfree, mu (steps + 1), and with keep the Linearisation of
    every step."""
    S, P = case.S, case.P
    glo, ghi = S.bounds()
    rng = np.random.default_rng(jitter_seed)

    def at(x, jac):
        out = P.eval(x)
        r = out[0] - np.clip(out[0], glo, ghi)
        A = sp.csr_matrix((out[3], S.col_idx, S.row_ptr), shape=(S.m, S.n)) if jac else None
        return r, A

    def linearise(x, colmax):
        r, A = at(x, True)
        w = (r != 0).astype(np.float64)
        colmax, c = col_scale(colmax, np.asarray(A.multiply(A).T @ w).ravel())
        z = A.T @ (w * -r)
        cf = np.where(blocked(x, lo, up, z), 0.0, c) if bounded else c
        return r, A, w, c, cf, colmax

    x = np.clip(x0, lo, up) if bounded else x0.copy()
    colmax = np.zeros(S.n)
    r, A, w, c, cf, colmax = linearise(x, colmax)
    merit = 0.5 * (r @ r)
    mu = TAU * lambda_max((A @ sp.diags(cf)).tocsr(), w, power_iters) if power_iters else TAU
    mu = min(max(mu, MU_MIN), MU_MAX)
    res = dict(merit=[merit], accepted=[], nfree=[], mu=[mu], cg=[], lin=[], done=False)
    for _ in range(steps):
        r, A, w, c, cf, colmax = linearise(x, colmax)
        if 0.5 * (r @ r) <= 0.0:
            res["done"] = True
            break
        k, e = cgls((A @ sp.diags(cf)).tocsr(), -r, w, mu, cg_iters, CG_TOL)
        d = cf * e
        if keep:
            res["lin"].append(Linearisation(A, -r, w, c, cf, mu))
        if jitter:
            d = d * (1.0 + jitter * rng.normal(size=S.n))
        xt = np.clip(x + d, lo, up) if bounded else x + d
        r2, _ = at(xt, False)
        mt = 0.5 * (r2 @ r2)
        ok = bool(mt < merit)
        if ok:
            x, merit = xt, mt
        mu = min(max(mu * (MU_DOWN if ok else MU_UP), MU_MIN), MU_MAX)
        res["accepted"].append(int(ok))
        res["nfree"].append(int((cf != 0).sum()))
        res["cg"].append(k)
        res["merit"].append(merit)
        res["mu"].append(mu)
    res["x"] = x
    return res


_cases = {}


def one(job):
    name, seed, a = job
    if name not in _cases:
        _cases[name] = cases()[name]()
    case = _cases[name]
    lo, up = case_bounds(case)
    x0 = case.x_perturbed(seed)
    fixed = lo == up
    B = lm_box(case, x0, lo, up, a["steps"], a["cg_iters"], a["power_iters"])
    F = lm_box(case, x0, lo, up, a["steps"], a["cg_iters"], a["power_iters"], bounded=False)
    xb, xf = B["x"], F["x"]
    boxed = ~fixed & ((lo > -1e19) | (up < 1e19))
    return dict(case=name, seed=seed, n=case.S.n, m=case.S.m, fixed=int(fixed.sum()), merit_before=B["merit"][0],
                bounded_merit=B["merit"][-1], bounded_accepted=B["accepted"], bounded_nfree=B["nfree"],
                bounded_fixed_off=float(np.abs(xb[fixed] - lo[fixed]).max()), bounded_inside=bool(((xb >= lo) & (xb <= up)).all()),
                bounded_on_bound=int((boxed & ((xb == lo) | (xb == up))).sum()),
                free_merit=F["merit"][-1], free_accepted=F["accepted"], free_fixed_moved=int((xf[fixed] != lo[fixed]).sum()),
                free_fixed_off_min=float(np.abs(xf[fixed] - lo[fixed]).min()), free_fixed_off_max=float(np.abs(xf[fixed] - lo[fixed]).max()),
                free_outside_box=int((boxed & ((xf < lo) | (xf > up))).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--cg-iters", type=int, default=60)
    ap.add_argument("--power-iters", type=int, default=30)
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--cases", default="C1_hopper,C2_biped_K100,biped_all,hopper_all")
    a = ap.parse_args()
    opts = dict(steps=a.steps, cg_iters=a.cg_iters, power_iters=a.power_iters)
    jobs = [(name, seed, opts) for name in a.cases.split(",") for seed in range(a.seeds)]
    out = []
    with ProcessPoolExecutor(max_workers=a.jobs) as pool:
        for r in pool.map(one, jobs, chunksize=1):
            print("%-14s seed %2d n %4d m %4d: merit %.3e -> bounded %.3e (%d accepted, free %d..%d, %d on a bound, fixed off by %.1e, "
                  "inside %s) | free loop %.3e (%d accepted): %d of %d fixed moved by %.2f..%.2f, %d outside their box"
                  % (r["case"], r["seed"], r["n"], r["m"], r["merit_before"], r["bounded_merit"], sum(r["bounded_accepted"]),
                     min(r["bounded_nfree"], default=0), max(r["bounded_nfree"], default=0), r["bounded_on_bound"], r["bounded_fixed_off"],
                     r["bounded_inside"], r["free_merit"], sum(r["free_accepted"]), r["free_fixed_moved"], r["fixed"],
                     r["free_fixed_off_min"], r["free_fixed_off_max"], r["free_outside_box"]), flush=True)
            out.append(r)
    print(json.dumps({"lm_box_cpu": out, **opts}), flush=True)


if __name__ == "__main__":
    main()
