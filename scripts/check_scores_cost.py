"""Cost of the trajectory checks of a sweep, in one process: Batch.checks_device (sample records -> check records) and
Batch.check_scores_device (check records -> eight doubles per candidate), with Batch.joints_device beside them for scale, each
against a torch copy of as many bytes as the call moves -- a new capability has no earlier time, the copy rate is the yardstick.

Workloads: the 1024-candidate Go1 Stairs sweep and the 64-candidate Go1 `Grid` sweep (a 60 x 44 map at 5 cm), dt = 0.01.
Each time is the median of --rounds rounds (default 20) between two events on one stream, after three rounds that are not
counted; the bytes are what a call reads and writes in global memory apart from the tables (records and scores), the copy
reads half of them and writes half.  One JSON line per workload.  The checks kernel has two forms (direct, the default: every
lane reads its own record; staged: make DIAG=-DTWR_CHECKS_STAGED, a work item's records go through LDS); they are measured by
running this script once on each build (TWR_AMD_LIB selects the library, --form labels the JSON lines).
A time is one launch between two events, so on the small sweep (0.02 - 0.03 ms) launch and event overhead are a visible part of
it, and a copy of a few megabytes runs out of the last-level cache: read the small sweep's ratios as orders of magnitude.

    timeout -k 10 300 python scripts/check_scores_cost.py
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import towr_amd as ta  # noqa: E402
from towr_amd import sweep  # noqa: E402

SIZE, RES = (60, 44), 0.05


def grid_map():
    rng = np.random.default_rng(21)
    elev = (0.04 * np.arange(SIZE[0])[:, None] * RES + rng.uniform(0.0, 0.05, size=SIZE)).astype(np.float32)
    return ta.GridMap(elev, RES, (1.2, 0.0))


def measure(name, model, structs, dt, rounds, form):
    import torch

    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    kin = ta.leg_kinematics_preset("go1")
    batch = ta.Batch(structs, list(range(len(structs))), device=0)
    n = len(structs)
    lin0 = [0.0, 0.0, -model.nominal_stance[0][2]]
    ee = [[model.nominal_stance[e][0], model.nominal_stance[e][1], 0.0] for e in range(4)]
    x = torch.from_numpy(np.concatenate([S.initial_guess(lin0, [0, 0, 0], [1.0, 0, lin0[2]], [0, 0, 0], ee) for S in structs])).to(dev)
    counts = [S.sample_count(dt) for S in structs]
    trec, jrec, crec = 20 + 13 * 4, ta.joint_rec(4), ta.check_rec(4)
    tstride, jstride, cstride = max(counts) * trec, max(counts) * jrec, max(counts) * crec
    traj = torch.empty(n * tstride, dtype=torch.float64, device=dev)
    joints = torch.empty(n * jstride, dtype=torch.float64, device=dev)
    checks = torch.empty(n * cstride, dtype=torch.float64, device=dev)
    scores = torch.zeros((n, ta.CHECK_SCORE_REC), dtype=torch.float64, device=dev)
    batch.sample_device(x.data_ptr(), dt, traj.data_ptr(), tstride, st)
    samples = int(sum(counts))
    calls = {
        "checks": (lambda: batch.checks_device(model, traj.data_ptr(), tstride, dt, checks.data_ptr(), cstride, st), 8 * samples * (trec + crec)),
        "check_scores": (lambda: batch.check_scores_device(checks.data_ptr(), cstride, dt, scores.data_ptr(), st),
                         8 * samples * crec + 8 * ta.CHECK_SCORE_REC * n),
        "joints": (lambda: batch.joints_device(kin, traj.data_ptr(), tstride, dt, joints.data_ptr(), jstride, st), 8 * samples * (trec + jrec)),
    }

    def timed(fn):
        ms = []
        for k in range(rounds + 3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms[3:])

    out = dict(workload=name, form=form, candidates=n, dt=dt, samples=samples, rounds=rounds)
    for what, (fn, nbytes) in calls.items():
        src = torch.empty(nbytes // 16, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        ms, copy_ms = timed(fn), timed(lambda: dst.copy_(src))
        out[what] = dict(ms=round(ms, 4), bytes=nbytes, gb_s=round(nbytes / ms / 1e6, 1), copy_ms=round(copy_ms, 4),
                         copy_gb_s=round(nbytes / copy_ms / 1e6, 1), of_copy_rate=round(copy_ms / ms, 3))
    torch.cuda.synchronize()
    s = scores.cpu().numpy()
    out.update(max_linear_residual=float(np.nanmax(s[:, 1])), min_swing_clearance_m=float(np.nanmin(s[:, 3])),
               candidates_with_a_foot_under_ground=int((s[:, 3] < 0).sum()), max_rom_m=float(np.nanmax(s[:, 7])))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16, help="host threads of twr_structure_create_many")
    ap.add_argument("--form", default="direct", help="label of the JSON lines: the form of the checks kernel in the library that is loaded")
    a = ap.parse_args()
    model = ta.model_preset("go1", "stairs")
    measure("go1 stairs sweep", model, sweep.candidate_structures(model, sweep.enumerate_candidates(1024), threads=a.threads), 0.01, a.rounds, a.form)
    model = ta.model_preset("go1", "grid_map")
    measure("go1 grid_map sweep", model, sweep.candidate_structures(model, sweep.enumerate_candidates(64), threads=a.threads, grid=grid_map()),
            0.01, a.rounds, a.form)


if __name__ == "__main__":
    main()
