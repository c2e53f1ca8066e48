"""A new map per plan request, two ways, in one process: what a caller had to do before twr_batch_grid_map_sync existed --
destroy the structures and the batch and build them again on a handle of the new map -- against the in-place update of the live
batch (GridMap.update + Batch.sync_grid_map, and Batch.update_grid_map_device from a layer already on the device).

Workload: the 64-candidate `Grid` sweep of tests/test_gpu_parity.py::test_grid_map_sweep_through_create_many (ANYmal, a 60 x 44
map at 5 cm).  Each figure is the median of --rounds rounds (default five) of host wall-clock time from the new layer in host
(device) memory to the end of a final stream synchronise, after one round that is not counted; every round brings another map,
with a moved centre and a rolled buffer.  One evaluation before and after checks that the update took.  One JSON line.

    timeout -k 10 300 python scripts/grid_map_update_cost.py
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import towr_amd as ta  # noqa: E402
from towr_amd import sweep  # noqa: E402

SIZE, RES = (60, 44), 0.05


def new_map(k):
    rng = np.random.default_rng(21 + k)
    elev = (0.04 * np.arange(SIZE[0])[:, None] * RES + rng.uniform(0.0, 0.05, size=SIZE)).astype(np.float32)
    start = ((7 * k) % SIZE[0], (5 * k) % SIZE[1])
    return np.asfortranarray(np.roll(elev, start, axis=(0, 1))), start, (1.2 + 0.01 * k, 0.005 * k)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of twr_structure_create_many")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    model = ta.model_preset("anymal", "grid_map")
    cands = sweep.enumerate_candidates(a.candidates)

    def build(buf, start, pos):
        gm = ta.GridMap(np.roll(buf, (-start[0], -start[1]), axis=(0, 1)), RES, pos)
        structs = sweep.candidate_structures(model, cands, threads=a.threads, grid=gm)
        return gm, structs, ta.Batch(structs, list(range(len(structs))), device=0)

    def timed(fn):
        t = []
        for k in range(a.rounds + 1):
            args = new_map(k + 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            keep = fn(*args)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
            del keep
        return statistics.median(t[1:]) * 1e3

    # (1) what it replaces: everything is destroyed and built again
    held = [build(*new_map(0))]

    def rebuild(buf, start, pos):
        held.clear()   # the structures, the batch and the handle go first, as in a caller that holds one sweep
        held.append(build(buf, start, pos))

    rebuild_ms = timed(rebuild)
    gm, structs, batch = held[0]

    # one evaluation around an update: the same x, other constraint values
    lin0 = [0.0, 0.0, -model.nominal_stance[0][2]]
    ee = [[model.nominal_stance[e][0], model.nominal_stance[e][1], 0.0] for e in range(4)]
    x = torch.from_numpy(np.concatenate([S.initial_guess(lin0, [0, 0, 0], [1.5, 0, lin0[2]], [0, 0, 0], ee) for S in structs])).to(dev)
    g = torch.zeros(int(batch.g_off[-1]), dtype=torch.float64, device=dev)
    jac = torch.zeros(int(batch.jac_off[-1]), dtype=torch.float64, device=dev)
    batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, st)
    torch.cuda.synchronize()
    g_before = g.clone()

    # (2) the in-place update from a host layer, (3) from a device layer
    def host_update(buf, start, pos):
        gm.update(buf, pos, start)
        batch.sync_grid_map(gm, st)

    sync_ms = timed(host_update)
    layers = {}

    def device_update(buf, start, pos):
        batch.update_grid_map_device(gm, layers[start], start, pos, st)

    for k in range(a.rounds + 1):   # the layers are on the device already: that is the case this call is for
        buf, start, _ = new_map(k + 1)
        layers[start] = torch.from_numpy(np.ascontiguousarray(buf.T)).to(dev).t()
    device_ms = timed(device_update)
    host_update(*new_map(99))   # (the timed rounds end on the map the last rebuild began with)
    batch.eval_device(x.data_ptr(), g.data_ptr(), jac.data_ptr(), ta.EVAL_BOTH, st)
    torch.cuda.synchronize()
    assert not torch.equal(g, g_before), "the update did not reach the evaluation"
    print(json.dumps(dict(workload="grid_map sweep", candidates=len(structs), map_cells=list(SIZE), rounds=a.rounds, threads=a.threads,
                          table_bytes=batch.table_bytes()["resident"], rebuild_ms=round(rebuild_ms, 3), sync_ms=round(sync_ms, 4),
                          update_device_ms=round(device_ms, 4), rebuild_over_sync=round(rebuild_ms / sync_ms, 1),
                          rebuild_over_update_device=round(rebuild_ms / device_ms, 1))))


if __name__ == "__main__":
    main()
