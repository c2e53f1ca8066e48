"""A/B of the planner step: scores and this shard's decision from x, the three-launch way and without g.

  A: eval_device(EVAL_VALUES) into g, then score_best_device (values kernel writes g, score_kernel reads it, best_kernel)
  B: eval_score_best_device (the values kernel's scoring instantiation, the fold, best_kernel; no g)

Alternating A/B rounds in one process, for the 1024-candidate C5 Stairs sweep (towr_amd.sweep, as bench.py builds it)
and for a batch of 8192 C3 problems.  Per step: device-only time (HIP events around `--steps` back-to-back steps) and the
time of a step that brings its 16-byte decision to the host (copy + synchronisation, as bench.py's planner leg).
Usage: python scripts/planner_scores_ab.py [--rounds 6] [--steps 200] [--workload c5|c3|both]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import towr_amd as ta  # noqa: E402
from bench import perturbed_inputs  # noqa: E402


def c5_batch():
    from towr_amd import sweep

    m5 = ta.model_preset("anymal", "stairs")
    cands = sweep.enumerate_candidates(1024)
    mine = sweep.candidate_structures(m5, cands, threads=min(16, os.cpu_count() or 1))
    batch = ta.Batch(mine, list(range(len(mine))), device=0)
    x = np.concatenate([perturbed_inputs(s, m5, 1, first_seed=i)[0] for i, s in enumerate(mine)])
    return batch, x


def c3_batch(n):
    model = ta.model_preset("anymal", "flat")
    S = ta.Structure(model, ta.gait_combo(4, 1, 2.0))
    batch = ta.Batch([S], [0] * n, device=0)
    x = np.concatenate(list(perturbed_inputs(S, model, n, first_seed=0)))
    return batch, x


def measure(torch, name, batch, x_host, rounds, steps):
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    n = batch.n_problems
    x = torch.from_numpy(x_host).to(dev)
    g = torch.empty(int(batch.g_off[-1]), dtype=torch.float64, device=dev)
    sa = torch.empty((n, 16), dtype=torch.float64, device=dev)
    sb = torch.empty((n, 16), dtype=torch.float64, device=dev)
    ba = torch.zeros(2, dtype=torch.float64, device=dev)
    bb = torch.zeros(2, dtype=torch.float64, device=dev)
    best_h = torch.zeros(2, dtype=torch.float64).pin_memory()
    assert batch.scores_without_g, name

    def step_a():
        batch.eval_device(x.data_ptr(), g.data_ptr(), 0, ta.EVAL_VALUES, stream)
        batch.score_best_device(g.data_ptr(), sa.data_ptr(), ba.data_ptr(), stream=stream)

    def step_b():
        batch.eval_score_best_device(x.data_ptr(), sb.data_ptr(), bb.data_ptr(), stream=stream)

    for _ in range(20):
        step_a()
        step_b()
    torch.cuda.synchronize()
    assert torch.equal(ba, bb), (ba.cpu(), bb.cpu())
    ia, ib = sa[:, 0::2], sb[:, 0::2]
    assert torch.equal(ia, ib), "inf-norms differ"
    res = {"A": {"device_us": [], "host_us": []}, "B": {"device_us": [], "host_us": []}}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for r in range(rounds):
        for key, step in (("A", step_a), ("B", step_b)) if r % 2 == 0 else (("B", step_b), ("A", step_a)):
            best = ba if key == "A" else bb
            e0.record()
            for _ in range(steps):
                step()
            e1.record()
            torch.cuda.synchronize()
            res[key]["device_us"].append(e0.elapsed_time(e1) * 1e3 / steps)
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
                best_h.copy_(best, non_blocking=True)
                torch.cuda.current_stream().synchronize()
            res[key]["host_us"].append((time.perf_counter() - t0) * 1e6 / steps)
    out = {"workload": name, "problems": n, "g_bytes": 8 * int(batch.g_off[-1]), "rounds": rounds, "steps": steps}
    for key in ("A", "B"):
        for m in ("device_us", "host_us"):
            v = res[key][m]
            out[f"{key}_{m}"] = {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    out["A"] = "eval(VALUES) + score_best: values kernel -> g -> score_kernel -> best_kernel"
    out["B"] = "eval_score_best: eval_scores_kernel -> score_fold_kernel -> best_kernel (no g)"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--workload", choices=("c5", "c3", "both"), default="both")
    ap.add_argument("--c3-problems", type=int, default=8192)
    a = ap.parse_args()
    import torch

    if a.workload in ("c5", "both"):
        print(json.dumps(measure(torch, "C5 stairs sweep", *c5_batch(), a.rounds, a.steps)), flush=True)
    if a.workload in ("c3", "both"):
        print(json.dumps(measure(torch, "C3", *c3_batch(a.c3_problems), a.rounds, a.steps)), flush=True)


if __name__ == "__main__":
    main()
