"""Time twr_jac_lsq_solve on the device and run a small Levenberg-Marquardt loop on top of it; prints one JSON line.

Workloads: C3 (ANYmal trot, K = 200, 8192 problems of one structure) and the 1024-candidate C5 Stairs sweep, built as
scripts/jac_products.py builds them; buffers as torch hands them out, HIP events, median of --rounds.
  * cgls: milliseconds per CGLS iteration (a --cg-iters solve with tol = 0, so that no problem stops, divided by --cg-iters)
    against one twr_jac_mul + one twr_jac_tmul timed in the same process on the same buffers, and the ratio of the two.  By
    bytes an iteration is 2 * 8 (n + m + nnz) in the two products plus about 8 (8 n + 6 m) in the vector kernels.
  * lm: --lm-steps steps of eval -> violation -> solve -> x + d -> eval(values) -> violation, the accept / reject per problem in
    torch on the device (mu / 3 on accept, * 10 on reject; no synchronise inside a step): the batch's merit 1/2 sum viol^2 and
    its summed inf-norm scores before and after, and the device time per step split into evaluation and solve.
mu starts at 1e-2 lambda_max(J^T W J) per problem, lambda_max from --power-iters power iterations with the two products and
twr_jac_dot, all on the device.
--damping identity (default: the output above, unchanged) | marquardt | both.  marquardt damps with mu C^-2, C = diag(1 / weighted
column norm): per LM step twr_jac_col_sqnorms (active-set weights) -> twr_jac_col_scale (running maximum, rel_floor 1e-12) ->
twr_jac_lsq_solve_scaled, mu starting at 1e-2 lambda_max(C J^T W J C) (the same power iteration, c applied in torch).  It adds
  * scaled: ms of twr_jac_col_sqnorms against twr_jac_tmul on the same buffers, of twr_jac_col_scale, and per iteration of the
    scaled solve against the unscaled one;
  * lm_marquardt: the lm block for the scaled damping, from the same x0.
--solver cgls (default: the output above, unchanged) | onepass | both.  onepass is twr_jac_lsq_solve_onepass: J read once per
iteration by twr_jac_normal_mul, the gradient recurred.  It adds
  * onepass: ms of twr_jac_normal_mul against twr_jac_mul + twr_jac_tmul on the same buffers, and per iteration of the one-pass
    solve by the protocol of cgls (same process, same buffers, (a --cg-iters solve - a 0-iteration solve) / --cg-iters at
    tol = 0); with both, its ratio to the CGLS iteration of this process, next to the ratio by bytes: an iteration moves
    8 (n + m + nnz) + 8 (n + m) in the product (plus its tables and partials) and about 8 (7 n + 5 m) in the vector kernel,
    against 2 * 8 (n + m + nnz) + 8 (8 n + 6 m);
  * lm_onepass (lm_marquardt_onepass): the lm blocks with the one-pass solve, from the same x0.  With onepass alone the CGLS
    blocks are left out.
Usage (each GPU step under its own time limit):
  timeout -k 10 600 python scripts/jac_lsq.py --workload c3 && timeout -k 10 600 python scripts/jac_lsq.py --workload c5
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import towr_amd as ta  # noqa: E402
from jac_products import c3, c5  # noqa: E402


class Problem:
    def __init__(self, torch, structs, order, x_h):
        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        self.batch = ta.Batch(structs, order, device=0)
        self.ops = ta.JacOps(structs, order, device=0)
        self.lsq = ta.JacLsq(self.ops)
        self.xo, self.go, self.jo = self.ops.layout()
        self.P = len(order)
        self.X, self.G, self.J = int(self.xo[-1]), int(self.go[-1]), int(self.jo[-1])
        self.x = torch.from_numpy(x_h).to(self.dev)
        self.of_x = torch.repeat_interleave(torch.arange(self.P, device=self.dev), torch.from_numpy(np.diff(self.xo)).to(self.dev))
        self.jac = self.vec(self.J)

    def vec(self, n):
        return self.torch.zeros(n, dtype=self.torch.float64, device=self.dev)

    def lambda_max(self, wa, iters, c=None):
        """Per-problem power iteration on J^T W J (c given: on C J^T W J C): v <- J^T (w o (J v)) / |v|,
        lambda = v^T J^T W J v / v^T v."""
        torch = self.torch
        v = torch.from_numpy(np.random.default_rng(3).normal(size=self.X)).to(self.dev)
        y, z, vv, vz = self.vec(self.G), self.vec(self.X), self.vec(self.P), self.vec(self.P)
        for _ in range(iters):
            cv = v if c is None else c * v
            self.ops.mul_device(self.jac.data_ptr(), cv.data_ptr(), y.data_ptr(), self.st)
            y.mul_(wa)
            self.ops.tmul_device(self.jac.data_ptr(), y.data_ptr(), z.data_ptr(), self.st)
            if c is not None:
                z.mul_(c)
            self.lsq.dot_device(self.lsq.X, v.data_ptr(), v.data_ptr(), vv.data_ptr(), self.st)
            self.lsq.dot_device(self.lsq.X, v.data_ptr(), z.data_ptr(), vz.data_ptr(), self.st)
            v = z / torch.sqrt(self.lsq_dot(z, z))[self.of_x].clamp_min(1e-300)
        return vz / vv.clamp_min(1e-300)

    def lsq_dot(self, a, b):
        out = self.vec(self.P)
        self.lsq.dot_device(self.lsq.X, a.data_ptr(), b.data_ptr(), out.data_ptr(), self.st)
        return out


def timed(torch, f, steps, rounds):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(rounds):
        e0.record()
        for _ in range(steps):
            f()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


REL_FLOOR = 1e-12


def lm_loop(torch, Q, damping, mu, lm_steps, lm_cg_iters, power_iters=30, solver="cgls"):
    """The LM loop from Q.x (left at the last accepted point).  damping "identity": mu I with the given mu; "marquardt": mu C^-2,
    mu = 1e-2 lambda_max(C J^T W J C) at the start when None.  solver "onepass": twr_jac_lsq_solve_onepass for the step."""
    st, lsq, ops, batch = Q.st, Q.lsq, Q.ops, Q.batch
    g, r, b, wa, merit, d, info = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.P), Q.vec(Q.X), Q.vec(4 * Q.P)
    g2, r2, merit2, scores = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.P), Q.vec(16 * Q.P)
    scaled = damping == "marquardt"
    if scaled:
        colsq, colmax, c = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X)
        lsq.reserve_scaled()
    if solver == "onepass":
        lsq.reserve_onepass(scaled)

    def linearise():
        batch.eval_device(Q.x.data_ptr(), g.data_ptr(), Q.jac.data_ptr(), ta.EVAL_BOTH, st)
        lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=st)
        torch.neg(r, out=b)
        if scaled:
            ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
            lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, d_colsq_max=colmax.data_ptr(), stream=st)

    def score_sum():
        batch.eval_scores_device(Q.x.data_ptr(), scores.data_ptr(), d_g=g2.data_ptr(), stream=st)
        return float(scores.view(Q.P, 8, 2)[:, :, 0].sum())

    linearise()
    if mu is None:
        mu = 1e-2 * Q.lambda_max(wa, power_iters, c if scaled else None)
    else:
        mu = mu.clone()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(lm_steps)]
    res = {"steps": lm_steps, "cg_iters": lm_cg_iters, "merit_before": float(merit.sum()), "scores_before": score_sum()}
    merit_before = merit.clone()
    accepted = Q.vec(lm_steps)
    for k in range(lm_steps):   # nothing in here waits for the device
        ev[k][0].record()
        linearise()
        ev[k][1].record()
        if solver == "onepass":
            lsq.solve_onepass_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), lm_cg_iters, 1e-8,
                                     d_w=wa.data_ptr(), d_scale=c.data_ptr() if scaled else 0, stream=st)
        elif scaled:
            lsq.solve_scaled_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), c.data_ptr(), d.data_ptr(), info.data_ptr(),
                                    lm_cg_iters, 1e-8, d_w=wa.data_ptr(), stream=st)
        else:
            lsq.solve_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), lm_cg_iters, 1e-8,
                             d_w=wa.data_ptr(), stream=st)
        ev[k][2].record()
        xt = Q.x + d
        batch.eval_device(xt.data_ptr(), g2.data_ptr(), 0, ta.EVAL_VALUES, st)
        lsq.violation_device(g2.data_ptr(), r2.data_ptr(), d_merit=merit2.data_ptr(), stream=st)
        ok = merit2 < merit
        Q.x = torch.where(ok[Q.of_x], xt, Q.x)
        mu = torch.where(ok, mu / 3.0, mu * 10.0)
        accepted[k] = ok.sum()
        ev[k][3].record()
    torch.cuda.synchronize()
    batch.eval_device(Q.x.data_ptr(), g.data_ptr(), 0, ta.EVAL_VALUES, st)
    lsq.violation_device(g.data_ptr(), r.data_ptr(), d_merit=merit.data_ptr(), stream=st)
    torch.cuda.synchronize()
    ms_eval = [e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3]) for e in ev]
    ms_solve = [e[1].elapsed_time(e[2]) for e in ev]
    res.update(merit_after=float(merit.sum()), scores_after=score_sum(), accepted_per_step=[int(v) for v in accepted.cpu()],
               ms_eval_per_step=float(np.median(ms_eval)), ms_solve_per_step=float(np.median(ms_solve)),
               viol_inf_after_min_median_max=[float(v) for v in np.quantile(
                   scores.view(Q.P, 8, 2)[:, :, 0].max(dim=1).values.cpu().numpy(), [0, 0.5, 1])])
    Q.merit_before, Q.merit_after = merit_before, merit.clone()   # per problem, for callers that compare dampings
    return res


def measure_scaled(torch, Q, b, wa, mu, a):
    """twr_jac_col_sqnorms against twr_jac_tmul, and the scaled CGLS iteration against the unscaled one, on the same buffers
    (J, b, wa of the starting point)."""
    st, lsq, ops = Q.st, Q.lsq, Q.ops
    colsq, c, z, d, info = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(4 * Q.P)
    lsq.reserve_scaled()
    ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
    lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, stream=st)
    calls = {"tmul": lambda: ops.tmul_device(Q.jac.data_ptr(), wa.data_ptr(), z.data_ptr(), st),
             "col_sqnorms": lambda: ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st),
             "col_scale": lambda: lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, stream=st)}
    for iters in (a.cg_iters, 0):
        calls["solve%d" % iters] = lambda iters=iters: lsq.solve_device(
            Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_w=wa.data_ptr(), stream=st)
        calls["scaled%d" % iters] = lambda iters=iters: lsq.solve_scaled_device(
            Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), c.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_w=wa.data_ptr(),
            stream=st)
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    t = {k: timed(torch, f, a.steps if k in ("tmul", "col_sqnorms", "col_scale") else 2, a.rounds) for k, f in calls.items()}
    n = a.cg_iters
    per = {k: (t["%s%d" % (k, n)][0] - t["%s0" % k][0]) / n for k in ("solve", "scaled")}
    nb = 2 * 8 * (Q.X + Q.G + Q.J) + 8 * (8 * Q.X + 6 * Q.G)
    cs = colsq.view(-1)
    return {"ms_tmul": t["tmul"], "ms_col_sqnorms": t["col_sqnorms"], "col_sqnorms_to_tmul": t["col_sqnorms"][0] / t["tmul"][0],
            "ms_col_scale": t["col_scale"], "cg_iters": n, "ms_solve": t["solve%d" % n], "ms_solve_scaled": t["scaled%d" % n],
            "ms_per_iteration_without_start": per["solve"], "ms_per_scaled_iteration_without_start": per["scaled"],
            "scaled_to_unscaled": per["scaled"] / per["solve"], "ratio_by_bytes": 1.0 + 8 * 4 * Q.X / nb,
            "jac_lsq_bytes_with_scaled": lsq.bytes()["resident"],
            "zero_columns": int((cs == 0).sum()), "col_norm_min_positive_max": [
                float(cs[cs > 0].min().sqrt()) if bool((cs > 0).any()) else 0.0, float(cs.max().sqrt())]}


def measure_onepass(torch, Q, b, wa, mu, a, cgls_per_iter):
    """twr_jac_normal_mul against the two products, and the one-pass iteration by the protocol of the cgls block, on the same
    buffers (J, b, wa of the starting point).  cgls_per_iter: the CGLS iteration of this process (None: not measured)."""
    st, lsq, ops = Q.st, Q.lsq, Q.ops
    y, z, u, d, info = Q.vec(Q.G), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(4 * Q.P)
    v = torch.from_numpy(np.random.default_rng(9).normal(size=Q.X)).to(Q.dev)
    ops_bytes_before = ops.bytes()["resident"]
    if a.normal_tile:
        ops.reserve_normal(a.normal_tile)
    lsq.reserve_onepass()

    def solve(iters, tol):
        lsq.solve_onepass_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, tol,
                                 d_w=wa.data_ptr(), stream=st)

    calls = {"mul": lambda: ops.mul_device(Q.jac.data_ptr(), v.data_ptr(), y.data_ptr(), st),
             "tmul": lambda: ops.tmul_device(Q.jac.data_ptr(), y.data_ptr(), z.data_ptr(), st),
             "normal": lambda: ops.normal_mul_device(Q.jac.data_ptr(), v.data_ptr(), u.data_ptr(), d_w=wa.data_ptr(), d_y=y.data_ptr(),
                                                     stream=st),
             "solve": lambda: solve(a.cg_iters, 0.0), "solve0": lambda: solve(0, 0.0)}
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    t = {k: timed(torch, f, a.steps if k in ("mul", "tmul", "normal") else 2, a.rounds) for k, f in calls.items()}
    per_iter = (t["solve"][0] - t["solve0"][0]) / a.cg_iters
    nb = 8 * (Q.X + Q.G + Q.J)
    by_onepass, by_cgls = nb + 8 * (Q.X + Q.G) + 8 * (7 * Q.X + 5 * Q.G), 2 * nb + 8 * (8 * Q.X + 6 * Q.G)
    res = {"cg_iters": a.cg_iters, "tile": a.normal_tile or 2048, "ms_solve": t["solve"], "ms_start": t["solve0"],
           "ms_per_iteration_without_start": per_iter, "ms_normal": t["normal"], "ms_mul": t["mul"], "ms_tmul": t["tmul"],
           "normal_to_products": t["normal"][0] / (t["mul"][0] + t["tmul"][0]),
           "bytes_onepass_iteration": by_onepass, "bytes_cgls_iteration": by_cgls, "ratio_by_bytes": by_onepass / by_cgls,
           "jac_ops_bytes_before": ops_bytes_before, "jac_ops_bytes_with_normal": ops.bytes()["resident"],
           "jac_lsq_bytes_with_onepass": lsq.bytes()["resident"]}
    if cgls_per_iter is not None:
        res["ms_per_cgls_iteration_without_start"] = cgls_per_iter
        res["onepass_to_cgls"] = per_iter / cgls_per_iter
    solve(a.cg_iters, 1e-10)
    torch.cuda.synchronize()
    it = info.view(-1, 4)
    res["at_tol_1e-10"] = {"iterations_min_max": [float(it[:, 0].min()), float(it[:, 0].max())],
                           "status_counts": [int((it[:, 3] == s).sum()) for s in (0, 1, 2)]}
    return res


def measure(torch, name, structs, order, x_h, a):
    Q = Problem(torch, structs, order, x_h)
    st, lsq, ops, batch = Q.st, Q.lsq, Q.ops, Q.batch
    g, r, wa, d, info = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.X), Q.vec(4 * Q.P)
    batch.eval_device(Q.x.data_ptr(), g.data_ptr(), Q.jac.data_ptr(), ta.EVAL_BOTH, st)
    lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), stream=st)
    b = -r
    lam = Q.lambda_max(wa, a.power_iters)
    mu = 1e-2 * lam
    cgls, onepass = a.solver != "onepass", a.solver != "cgls"   # which solvers are measured: nothing is run for the other
    torch.cuda.synchronize()
    out = {"workload": name, "problems": Q.P, "jac_lsq_bytes": lsq.bytes()["resident"], "jac_ops_bytes": ops.bytes()["resident"],
           "lambda_max": [float(lam.min()), float(lam.max())]}

    # ---- one CGLS iteration against the two products
    per_iter = None
    if cgls:
        y, z = Q.vec(Q.G), Q.vec(Q.X)

        def solve(iters, tol):
            lsq.solve_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, tol, d_w=wa.data_ptr(), stream=st)

        calls = {"mul": lambda: ops.mul_device(Q.jac.data_ptr(), d.data_ptr(), y.data_ptr(), st),
                 "tmul": lambda: ops.tmul_device(Q.jac.data_ptr(), r.data_ptr(), z.data_ptr(), st),
                 "solve": lambda: solve(a.cg_iters, 0.0), "solve0": lambda: solve(0, 0.0)}
        for f in calls.values():
            f()
            f()
        torch.cuda.synchronize()
        t = {k: timed(torch, f, a.steps if k in ("mul", "tmul") else 2, a.rounds) for k, f in calls.items()}
        per_iter = (t["solve"][0] - t["solve0"][0]) / a.cg_iters
        products = t["mul"][0] + t["tmul"][0]
        nb = 8 * (Q.X + Q.G + Q.J)
        out["cgls"] = {"cg_iters": a.cg_iters, "ms_solve": t["solve"], "ms_start": t["solve0"], "ms_per_iteration": t["solve"][0] / a.cg_iters,
                       "ms_per_iteration_without_start": per_iter, "ms_mul": t["mul"], "ms_tmul": t["tmul"],
                       "ms_products": products, "ratio_to_products": t["solve"][0] / a.cg_iters / products,
                       "ratio_without_start": per_iter / products,
                       "bytes_products": 2 * nb, "bytes_vectors": 8 * (8 * Q.X + 6 * Q.G),
                       "ratio_by_bytes": 1.0 + 8 * (8 * Q.X + 6 * Q.G) / (2 * nb)}
        solve(a.cg_iters, 1e-10)
        torch.cuda.synchronize()
        it = info.view(-1, 4)
        out["cgls"]["at_tol_1e-10"] = {"iterations_min_max": [float(it[:, 0].min()), float(it[:, 0].max())],
                                       "status_counts": [int((it[:, 3] == s).sum()) for s in (0, 1, 2)]}

    # ---- Levenberg-Marquardt
    x0 = Q.x.clone()
    if cgls and a.damping != "identity":
        out["scaled"] = measure_scaled(torch, Q, b, wa, mu, a)   # J, b, wa still those of x0
    if onepass:
        out["onepass"] = measure_onepass(torch, Q, b, wa, mu, a, per_iter)
    for damping, key in (("identity", "lm"), ("marquardt", "lm_marquardt")):
        if a.damping not in (damping, "both"):
            continue
        for solver, suffix in (("cgls", ""), ("onepass", "_onepass")):
            if (cgls, onepass)[solver == "onepass"]:
                Q.x = x0.clone()   # every loop from the same point (a loop leaves Q.x at its last accepted one)
                out[key + suffix] = lm_loop(torch, Q, damping, mu if damping == "identity" else None, a.lm_steps, a.lm_cg_iters,
                                            a.power_iters, solver=solver)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cg-iters", type=int, default=50)
    ap.add_argument("--power-iters", type=int, default=30)
    ap.add_argument("--lm-steps", type=int, default=8)
    ap.add_argument("--lm-cg-iters", type=int, default=60)
    ap.add_argument("--workload", choices=("c3", "c5", "both"), default="both")
    ap.add_argument("--c3-problems", type=int, default=8192)
    ap.add_argument("--damping", choices=("identity", "marquardt", "both"), default="identity")
    ap.add_argument("--solver", choices=("cgls", "onepass", "both"), default="cgls")
    ap.add_argument("--normal-tile", type=int, default=0, help="LDS tile of the one-pass product in entries (0: the default, 2048)")
    a = ap.parse_args()
    import torch

    res = []
    if a.workload in ("c3", "both"):
        res.append(measure(torch, "C3", *c3(a.c3_problems), a))
        torch.cuda.empty_cache()
    if a.workload in ("c5", "both"):
        res.append(measure(torch, "C5 stairs sweep", *c5(), a))
    print(json.dumps({"jac_lsq": res}), flush=True)


if __name__ == "__main__":
    main()
