"""Time twr_jac_mul / twr_jac_tmul on the device and print one JSON line.

Workloads: C3 (ANYmal trot, K = 200, 8192 problems of one structure) and the 1024-candidate C5 Stairs sweep (towr_amd.sweep, as
bench.py builds it).  The Jacobian values come from one twr_batch_eval(JACOBIAN) on buffers as torch hands them out (no
placement search); v and w are seeded normals.  Per product: milliseconds per call (HIP events around --steps back-to-back
calls, median of --rounds), the bytes counted -- Jacobian values + the vector read + the vector written (8 (n + m + nnz) per
problem) + per distinct pattern its 16-bit columns and row_ptr (both products) and fold_ptr (J^T w); the block maps, fold
slots and slab of J^T w are not counted -- and their fraction of 8 TB/s.
Usage: python scripts/jac_products.py [--steps 50] [--rounds 5] [--workload c3|c5|both]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import towr_amd as ta  # noqa: E402
from bench import perturbed_inputs  # noqa: E402

PEAK = 8e12


def c3(n):
    model = ta.model_preset("anymal", "flat")
    dt = 2.0 / (200 - 1.5)   # K = 200 time nodes, as bench.py
    S = ta.Structure(model, ta.gait_combo(4, 1, 2.0), ta.params_default(dt_dynamic=dt, dt_rom=dt))
    assert (S.n, S.m, S.nnz) == (640, 3866, 102896)
    return [S], [0] * n, np.concatenate(list(perturbed_inputs(S, model, n, first_seed=0)))


def c5():
    from towr_amd import sweep

    m5 = ta.model_preset("anymal", "stairs")
    mine = sweep.candidate_structures(m5, sweep.enumerate_candidates(1024), threads=min(16, os.cpu_count() or 1))
    x = np.concatenate([perturbed_inputs(s, m5, 1, first_seed=i)[0] for i, s in enumerate(mine)])
    return mine, list(range(len(mine))), x


def table_bytes(structs, order):
    """Bytes of the distinct index tables counted for each product (see the module docstring)."""
    seen, mul, tmul = {}, 0, 0
    for s in order:
        S = structs[s]
        key = (S.n, S.row_ptr.tobytes(), S.col_idx.tobytes())
        if key not in seen:
            seen[key] = True
            mul += 2 * S.nnz + 4 * (S.m + 1)
            tmul += 2 * S.nnz + 4 * (S.m + 1) + 4 * (S.n + 1)
    return mul, tmul, len(seen)


def measure(torch, name, structs, order, x_h, steps, rounds):
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    batch = ta.Batch(structs, order, device=0)
    ops = ta.JacOps(structs, order, device=0)
    xo, go, jo = ops.layout()
    x = torch.from_numpy(x_h).to(dev)
    jac = torch.empty(int(jo[-1]), dtype=torch.float64, device=dev)
    batch.eval_device(x.data_ptr(), 0, jac.data_ptr(), ta.EVAL_JACOBIAN, st)
    rng = np.random.default_rng(1)
    v = torch.from_numpy(rng.normal(size=int(xo[-1]))).to(dev)
    w = torch.from_numpy(rng.normal(size=int(go[-1]))).to(dev)
    y = torch.empty(int(go[-1]), dtype=torch.float64, device=dev)
    z = torch.empty(int(xo[-1]), dtype=torch.float64, device=dev)
    del batch
    calls = {"mul": lambda: ops.mul_device(jac.data_ptr(), v.data_ptr(), y.data_ptr(), st),
             "tmul": lambda: ops.tmul_device(jac.data_ptr(), w.data_ptr(), z.data_ptr(), st)}
    for f in calls.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for r in range(rounds):
        for k, f in calls.items():
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / steps)
    alg = 8 * int(xo[-1] + go[-1] + jo[-1])
    t_mul, t_tmul, distinct = table_bytes(structs, order)
    b = ops.bytes()
    out = {"workload": name, "problems": len(order), "algorithmic_bytes": alg, "jac_ops_bytes": b}
    for k, tb in (("mul", t_mul), ("tmul", t_tmul)):
        med = float(np.median(ms[k]))
        out[k] = {"ms": med, "ms_min": float(np.min(ms[k])), "ms_max": float(np.max(ms[k])), "table_bytes": tb,
                  "bytes": alg + tb, "fraction_of_8TBs": (alg + tb) / (med * 1e-3) / PEAK,
                  "fraction_algorithmic": alg / (med * 1e-3) / PEAK}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workload", choices=("c3", "c5", "both"), default="both")
    ap.add_argument("--c3-problems", type=int, default=8192)
    a = ap.parse_args()
    import torch

    res = []
    if a.workload in ("c3", "both"):
        res.append(measure(torch, "C3", *c3(a.c3_problems), a.steps, a.rounds))
        torch.cuda.empty_cache()
    if a.workload in ("c5", "both"):
        res.append(measure(torch, "C5 stairs sweep", *c5(), a.steps, a.rounds))
    print(json.dumps({"jac_products": res}), flush=True)


if __name__ == "__main__":
    main()
