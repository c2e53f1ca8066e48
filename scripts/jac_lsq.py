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
--bounds (default off: the output above, unchanged): towr's variable bounds (twr_structure_variable_bounds for the start and goal
of the guess: 23 base values and 3 per foot fixed, every phase duration boxed with optimised timings).  It adds
  * to every lm block: fixed_off_max, the largest distance of a fixed variable from its value at the end, and outside_box;
  * masked: ms per iteration of twr_jac_lsq_solve_masked against twr_jac_lsq_solve_scaled by the protocol of cgls, on the same
    buffers (the scale of the starting point with its free set's zeros);
  * lm_box: the Marquardt loop as projected active-set LM, in torch on top of twr_jac_free_set and twr_jac_lsq_solve_masked
    (free counts per step as well);
  * with --driver device, lm_box_device: the same loop by twr_jac_lm_start / twr_jac_lm_step, nothing in torch: merits, accepted
    per step, free counts, states, and ms per step eager and as a replayed hipGraph of one step, next to the torch loop's.
--solver gram (next to cgls, which is timed in the same process on the same buffers): the Gram matrix N = J^T W J formed once
(twr_jac_gram) and the solve on it in one launch (twr_jac_lsq_solve_gram).  It adds
  * gram: ms of twr_jac_gram against twr_jac_tmul, of twr_jac_gram_mul, per iteration of the Gram solve against the masked CGLS
    iteration by the protocol of cgls ((a --lm-cg-iters solve - a 0-iteration solve) / --lm-cg-iters at tol = 0), the whole
    --lm-cg-iters solve with formation against twr_jac_lsq_solve_masked, the ratio by bytes (8 nnz N + 2 nnz N of column indices
    against 2 * 8 (n + m + nnz) + 8 (8 n + 6 m)) and what the handles hold; the scale is the starting point's, with its free
    set's zeros under --bounds.
--lm-solver gram | both (with --bounds --driver device): lm_box_device_gram, the driver's loop with TWR_JAC_LM_GRAM, next to
lm_box_device.
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


def variable_bounds(torch, Q, structs, order):
    """(lo, up) on the device: twr_structure_variable_bounds of every problem for the start and goal of bench.perturbed_inputs."""
    per = {}
    for s in set(order):
        S, m = structs[s], structs[s].model
        z = -m.nominal_stance[0][2]
        ee = [[m.nominal_stance[e][0], m.nominal_stance[e][1], 0.0] for e in range(m.n_ee)]
        per[s] = S.variable_bounds([0, 0, z] + [0] * 9, [1.0, 0, z] + [0] * 9, ee)
    lo, up = (np.concatenate([per[s][k] for s in order]) for k in (0, 1))
    return torch.from_numpy(lo).to(Q.dev), torch.from_numpy(up).to(Q.dev)


def box_report(Q, bounds):
    lo, up = bounds
    fixed = lo == up
    return {"fixed_variables": int(fixed.sum()), "fixed_off_max": float((Q.x - lo)[fixed].abs().max()),
            "outside_box": int(((Q.x < lo) | (Q.x > up))[~fixed].sum())}


def lm_loop(torch, Q, damping, mu, lm_steps, lm_cg_iters, power_iters=30, solver="cgls", bounds=None, box=False):
    """The LM loop from Q.x (left at the last accepted point).  damping "identity": mu I with the given mu; "marquardt": mu C^-2,
    mu = 1e-2 lambda_max(C J^T W J C) at the start when None.  solver "onepass": twr_jac_lsq_solve_onepass for the step.
    bounds (lo, up): reported on; with box (marquardt, cgls) honoured: projected active-set LM, the restatement of twr_jac_lm_step
    in torch."""
    st, lsq, ops, batch = Q.st, Q.lsq, Q.ops, Q.batch
    g, r, b, wa, merit, d, info = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.P), Q.vec(Q.X), Q.vec(4 * Q.P)
    g2, r2, merit2, scores = Q.vec(Q.G), Q.vec(Q.G), Q.vec(Q.P), Q.vec(16 * Q.P)
    scaled = damping == "marquardt"
    if scaled:
        colsq, colmax, c = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X)
        lsq.reserve_scaled()
    if solver == "onepass":
        lsq.reserve_onepass(scaled)
    if box:
        assert scaled and solver == "cgls" and bounds is not None
        lo, up = bounds
        Q.x = torch.minimum(torch.maximum(Q.x, lo), up)
        z, cf, nfree = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.P)
        free_counts = torch.zeros(lm_steps, 3, dtype=torch.float64, device=Q.dev)

    def linearise():
        batch.eval_device(Q.x.data_ptr(), g.data_ptr(), Q.jac.data_ptr(), ta.EVAL_BOTH, st)
        lsq.violation_device(g.data_ptr(), r.data_ptr(), d_w_active=wa.data_ptr(), d_merit=merit.data_ptr(), stream=st)
        torch.neg(r, out=b)
        if scaled:
            ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
            lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, d_colsq_max=colmax.data_ptr(), stream=st)
        if box:
            t = wa * b
            ops.tmul_device(Q.jac.data_ptr(), t.data_ptr(), z.data_ptr(), st)
            lsq.free_set_device(Q.x.data_ptr(), lo.data_ptr(), up.data_ptr(), z.data_ptr(), cf.data_ptr(), nfree.data_ptr(),
                                d_scale_in=c.data_ptr(), stream=st)

    def score_sum():
        batch.eval_scores_device(Q.x.data_ptr(), scores.data_ptr(), d_g=g2.data_ptr(), stream=st)
        return float(scores.view(Q.P, 8, 2)[:, :, 0].sum())

    linearise()
    if mu is None:
        mu = 1e-2 * Q.lambda_max(wa, power_iters, (cf if box else c) if scaled else None)
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
        elif box:
            lsq.solve_masked_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), cf.data_ptr(), d.data_ptr(), info.data_ptr(),
                                    lm_cg_iters, 1e-8, d_w=wa.data_ptr(), stream=st)
            free_counts[k] = torch.stack([nfree.min(), nfree.median(), nfree.max()])
        elif scaled:
            lsq.solve_scaled_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), c.data_ptr(), d.data_ptr(), info.data_ptr(),
                                    lm_cg_iters, 1e-8, d_w=wa.data_ptr(), stream=st)
        else:
            lsq.solve_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), lm_cg_iters, 1e-8,
                             d_w=wa.data_ptr(), stream=st)
        ev[k][2].record()
        xt = Q.x + d
        if box:
            xt = torch.minimum(torch.maximum(xt, lo), up)
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
    if bounds is not None:
        res.update(box_report(Q, bounds), ms_step=float(np.median([e[0].elapsed_time(e[3]) for e in ev])))
    if box:
        res["free_min_median_max_per_step"] = free_counts.cpu().numpy().tolist()
    return res


def lm_device(torch, Q, bounds, a, solver="cgls"):
    """The bounded loop by the driver (twr_jac_lm_*): eager steps, then from the same start a captured graph of one step replayed."""
    lo, up = bounds
    st = Q.st
    lm = ta.JacLm(Q.batch, Q.lsq, solver=solver, cg_iters=a.lm_cg_iters, power_iters=a.power_iters)
    g, rec = Q.vec(Q.G), Q.vec(ta.JacLm.REC * Q.P)
    x0 = Q.x.clone()
    F = {k: i for i, k in enumerate(ta.JacLm.FIELDS)}

    def state():
        lm.state_device(rec.data_ptr(), st)
        torch.cuda.synchronize()
        return rec.view(Q.P, -1).clone()

    def start():
        Q.x.copy_(x0)
        lm.start_device(Q.x.data_ptr(), lo.data_ptr(), up.data_ptr(), g.data_ptr(), Q.jac.data_ptr(), st)

    def timed_steps(step):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.lm_steps + 1)]
        acc = []
        ev[0].record()
        for k in range(a.lm_steps):
            step()
            ev[k + 1].record()
            lm.state_device(rec.data_ptr(), st)   # stream-ordered copy of the records: no synchronise
            acc.append(rec.view(Q.P, -1)[:, F["accepted"]].sum().clone())
        torch.cuda.synchronize()
        acc = [float(v) for v in acc]
        return [ev[k].elapsed_time(ev[k + 1]) for k in range(a.lm_steps)], [int(b - c) for b, c in zip(acc, [0.0] + acc[:-1])]

    start()
    s0 = state()
    ms_eager, accepted = timed_steps(lambda: lm.step_device(st))
    s1 = state()
    x_eager = Q.x.clone()
    res = {"steps": a.lm_steps, "cg_iters": a.lm_cg_iters, "solver": solver, "jac_lm_bytes": lm.bytes()["resident"],
           "merit_before": float(s0[:, F["merit"]].sum()), "merit_after": float(s1[:, F["merit"]].sum()),
           "accepted_per_step": accepted, "states_running_done_bad": [int((s1[:, F["state"]] == v).sum()) for v in (0, 1, 2)],
           "free_min_median_max": [float(v) for v in (s1[:, F["free"]].min(), s1[:, F["free"]].median(), s1[:, F["free"]].max())],
           "mu0_min_max": [float(s0[:, F["mu"]].min()), float(s0[:, F["mu"]].max())],
           "ms_step_eager": float(np.median(ms_eager)), **box_report(Q, bounds)}
    start()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lm.step_device(torch.cuda.current_stream().cuda_stream)
    ms_graph, _ = timed_steps(graph.replay)
    res.update(ms_step_graph=float(np.median(ms_graph)), graph_bits_equal_eager=bool(torch.equal(Q.x, x_eager)))
    Q.merit_before, Q.merit_after = s0[:, F["merit"]].clone(), s1[:, F["merit"]].clone()
    return res


def measure_masked(torch, Q, b, wa, mu, a, bounds):
    """The masked CGLS iteration against the scaled one: same process, same buffers, the protocol of the cgls block."""
    st, lsq, ops = Q.st, Q.lsq, Q.ops
    lo, up = bounds
    colsq, c, cf, z, d, info, nfree = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(4 * Q.P), Q.vec(Q.P)
    lsq.reserve_scaled()
    xp = torch.minimum(torch.maximum(Q.x, lo), up)
    t = wa * b
    ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
    lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, stream=st)
    ops.tmul_device(Q.jac.data_ptr(), t.data_ptr(), z.data_ptr(), st)
    calls = {"free_set": lambda: lsq.free_set_device(xp.data_ptr(), lo.data_ptr(), up.data_ptr(), z.data_ptr(), cf.data_ptr(),
                                                     nfree.data_ptr(), d_scale_in=c.data_ptr(), stream=st)}
    for iters in (a.cg_iters, 0):
        calls["scaled%d" % iters] = lambda iters=iters: lsq.solve_scaled_device(
            Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), c.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_w=wa.data_ptr(),
            stream=st)
        calls["masked%d" % iters] = lambda iters=iters: lsq.solve_masked_device(
            Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), cf.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_w=wa.data_ptr(),
            stream=st)
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    t = {k: timed(torch, f, a.steps if k == "free_set" else 2, a.rounds) for k, f in calls.items()}
    n = a.cg_iters
    per = {k: (t["%s%d" % (k, n)][0] - t["%s0" % k][0]) / n for k in ("scaled", "masked")}
    return {"cg_iters": n, "ms_free_set": t["free_set"], "ms_solve_scaled": t["scaled%d" % n], "ms_solve_masked": t["masked%d" % n],
            "ms_per_scaled_iteration_without_start": per["scaled"], "ms_per_masked_iteration_without_start": per["masked"],
            "masked_to_scaled": per["masked"] / per["scaled"], "ratio_by_bytes": 1.0,
            "free_min_max": [float(nfree.min()), float(nfree.max())]}


def measure_gram(torch, Q, b, wa, mu, a, bounds):
    """twr_jac_gram, twr_jac_gram_mul and the Gram solve against twr_jac_tmul and the masked CGLS solve: same process, same
    buffers (J, b, wa of the starting point), the protocol of the cgls block."""
    st, lsq, ops = Q.st, Q.lsq, Q.ops
    colsq, c, cf, z, u, d, info, nfree = Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(Q.X), Q.vec(4 * Q.P), Q.vec(Q.P)
    lsq.reserve_scaled()
    ops_before = ops.bytes()
    ops.reserve_gram()
    gram_off = ops.gram_layout()
    N = Q.vec(max(2, int(gram_off[-1])))
    t = wa * b
    ops.col_sqnorms_device(Q.jac.data_ptr(), colsq.data_ptr(), d_w=wa.data_ptr(), stream=st)
    lsq.col_scale_device(colsq.data_ptr(), c.data_ptr(), REL_FLOOR, stream=st)
    ops.tmul_device(Q.jac.data_ptr(), t.data_ptr(), z.data_ptr(), st)
    if bounds is not None:
        lo, up = bounds
        xp = torch.minimum(torch.maximum(Q.x, lo), up)
        lsq.free_set_device(xp.data_ptr(), lo.data_ptr(), up.data_ptr(), z.data_ptr(), cf.data_ptr(), nfree.data_ptr(),
                            d_scale_in=c.data_ptr(), stream=st)
    else:
        cf.copy_(c)
    # mu for the system the two solves see, C_f J^T W J C_f (the caller's mu is 1e-2 lambda_max of the unscaled matrix, under which
    # the scaled system is mu I to rounding and a recurred gradient reaches exactly 0 within a few iterations)
    mu = 1e-2 * Q.lambda_max(wa, a.power_iters, cf)
    n = a.lm_cg_iters
    calls = {"tmul": lambda: ops.tmul_device(Q.jac.data_ptr(), t.data_ptr(), z.data_ptr(), st),
             "gram": lambda: ops.gram_device(Q.jac.data_ptr(), N.data_ptr(), d_w=wa.data_ptr(), stream=st),
             "gram_mul": lambda: ops.gram_mul_device(N.data_ptr(), z.data_ptr(), u.data_ptr(), stream=st)}
    for iters in (n, 0):
        calls["masked%d" % iters] = lambda iters=iters: lsq.solve_masked_device(
            Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), cf.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_w=wa.data_ptr(),
            stream=st)
        calls["solve_gram%d" % iters] = lambda iters=iters: lsq.solve_gram_device(
            N.data_ptr(), z.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), iters, 0.0, d_scale=cf.data_ptr(), stream=st)
    for f in calls.values():
        f()
        f()
    torch.cuda.synchronize()
    tm = {k: timed(torch, f, a.steps if k in ("tmul", "gram", "gram_mul") else 2, a.rounds) for k, f in calls.items()}
    per = {k: (tm["%s%d" % (k, n)][0] - tm["%s0" % k][0]) / n for k in ("masked", "solve_gram")}
    nnz_n = int(np.diff(gram_off).sum())
    by_gram, by_cgls = 10 * nnz_n, 2 * 8 * (Q.X + Q.G + Q.J) + 8 * (8 * Q.X + 6 * Q.G)
    res = {"cg_iters": n, "ms_tmul": tm["tmul"], "ms_gram": tm["gram"], "gram_to_tmul": tm["gram"][0] / tm["tmul"][0],
           "ms_gram_mul": tm["gram_mul"], "ms_solve_masked": tm["masked%d" % n], "ms_solve_gram": tm["solve_gram%d" % n],
           "ms_solve_gram_start": tm["solve_gram0"], "ms_per_masked_iteration_without_start": per["masked"],
           "ms_per_gram_iteration_without_start": per["solve_gram"], "gram_to_cgls_iteration": per["solve_gram"] / per["masked"],
           "bytes_gram_iteration": by_gram, "bytes_cgls_iteration": by_cgls, "ratio_by_bytes": by_gram / by_cgls,
           "ms_gram_plus_solve": tm["gram"][0] + tm["solve_gram%d" % n][0],
           "gram_plus_solve_to_masked": (tm["gram"][0] + tm["solve_gram%d" % n][0]) / tm["masked%d" % n][0],
           "nnz_jac": Q.J, "nnz_gram_padded": nnz_n, "gram_value_bytes": 8 * int(gram_off[-1]),
           "jac_ops_bytes_before": ops_before["resident"], "jac_ops_bytes_with_gram": ops.bytes()["resident"],
           "distinct_patterns": ops_before["distinct_patterns"],
           "mu_scaled_min_max": [float(mu.min()), float(mu.max())]}
    calls["solve_gram%d" % n]()   # the timed solve again: every problem must have run to the cap, or the times above are not iterations
    torch.cuda.synchronize()
    res["gram_iterations_at_tol_0_min_max"] = [float(info.view(-1, 4)[:, 0].min()), float(info.view(-1, 4)[:, 0].max())]
    for name in ("gram", "masked"):   # what --lm-cg-iters iterations reach at the driver's tol
        if name == "gram":
            lsq.solve_gram_device(N.data_ptr(), z.data_ptr(), mu.data_ptr(), d.data_ptr(), info.data_ptr(), n, 1e-8, d_scale=cf.data_ptr(), stream=st)
        else:
            lsq.solve_masked_device(Q.jac.data_ptr(), b.data_ptr(), mu.data_ptr(), cf.data_ptr(), d.data_ptr(), info.data_ptr(), n, 1e-8,
                                    d_w=wa.data_ptr(), stream=st)
        torch.cuda.synchronize()
        it = info.view(-1, 4)
        res["%s_at_tol_1e-8" % name] = {"iterations_min_max": [float(it[:, 0].min()), float(it[:, 0].max())],
                                        "rel_min_max": [float(it[:, 1].min()), float(it[:, 1].max())],
                                        "status_counts": [int((it[:, 3] == s).sum()) for s in (0, 1, 2)]}
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
    cgls, onepass = a.solver != "onepass", a.solver in ("onepass", "both")   # which solvers are measured: nothing is run for the other
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
    bounds = variable_bounds(torch, Q, structs, order) if a.bounds else None
    if a.bounds:
        out["masked"] = measure_masked(torch, Q, b, wa, mu, a, bounds)
    if cgls and a.damping != "identity":
        out["scaled"] = measure_scaled(torch, Q, b, wa, mu, a)   # J, b, wa still those of x0
    if onepass:
        out["onepass"] = measure_onepass(torch, Q, b, wa, mu, a, per_iter)
    if a.solver == "gram":
        out["gram"] = measure_gram(torch, Q, b, wa, mu, a, bounds)
    for damping, key in (("identity", "lm"), ("marquardt", "lm_marquardt")):
        if a.damping not in (damping, "both"):
            continue
        for solver, suffix in (("cgls", ""), ("onepass", "_onepass")):
            if (cgls, onepass)[solver == "onepass"]:
                Q.x = x0.clone()   # every loop from the same point (a loop leaves Q.x at its last accepted one)
                out[key + suffix] = lm_loop(torch, Q, damping, mu if damping == "identity" else None, a.lm_steps, a.lm_cg_iters,
                                            a.power_iters, solver=solver, bounds=bounds)
    if a.bounds:
        Q.x = x0.clone()
        out["lm_box"] = lm_loop(torch, Q, "marquardt", None, a.lm_steps, a.lm_cg_iters, a.power_iters, bounds=bounds, box=True)
        if a.driver == "device":
            if a.lm_solver in ("cgls", "both"):
                Q.x = x0.clone()
                out["lm_box_device"] = lm_device(torch, Q, bounds, a)
            if a.lm_solver in ("gram", "both"):
                Q.x = x0.clone()
                out["lm_box_device_gram"] = lm_device(torch, Q, bounds, a, solver="gram")
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
    ap.add_argument("--solver", choices=("cgls", "onepass", "both", "gram"), default="cgls")
    ap.add_argument("--lm-solver", choices=("cgls", "gram", "both"), default="cgls", help="with --driver device: the driver's linear solve")
    ap.add_argument("--bounds", action="store_true", help="honour towr's variable bounds: the masked solve and the bounded LM loop")
    ap.add_argument("--driver", choices=("torch", "device"), default="torch", help="with --bounds: also run the loop by twr_jac_lm_*")
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
