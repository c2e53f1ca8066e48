"""bench.py --dump-outputs: what the timed path computed in its last step, written so that two builds can be compared output for
output -- at most 64 MB, the same problems on every run, and on the GPU the values the oracle computes for bench.py's inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def test_dump_is_a_fixed_sample_of_whole_problems_within_64_mb(tmp_path):
    import torch

    rng = np.random.default_rng(5)
    g_off, jac_off = _offsets(rng.integers(1000, 5000, 300)), _offsets(rng.integers(20000, 60000, 300))   # ~110 MB of values
    g = torch.arange(int(g_off[-1]), dtype=torch.float64)
    jac = -torch.arange(int(jac_off[-1]), dtype=torch.float64)
    picked = bench.dump_outputs(str(tmp_path / "a"), g, jac, g_off, jac_off)
    assert 0 < len(picked) < 300 and np.all(np.diff(picked) > 0)
    assert np.array_equal(picked, bench.dump_problems(g_off, jac_off))      # seeded: the same problems every time
    files = [tmp_path / "a" / "g.npy", tmp_path / "a" / "jac.npy"]
    assert sum(os.path.getsize(f) for f in files) <= 64 * 10**6
    dg, dj = np.load(files[0]), np.load(files[1])
    assert dg.dtype == np.float64 and dj.dtype == np.float64
    assert np.array_equal(dg, np.concatenate([np.arange(g_off[p], g_off[p + 1]) for p in picked]))
    assert np.array_equal(dj, -np.concatenate([np.arange(jac_off[p], jac_off[p + 1]) for p in picked]))
    # a batch that fits: every problem, the buffers as they are
    g_off, jac_off = g_off[:11], jac_off[:11]
    assert np.array_equal(bench.dump_outputs(str(tmp_path / "b"), g, jac, g_off, jac_off), np.arange(10))
    assert np.array_equal(np.load(tmp_path / "b" / "jac.npy"), jac[:int(jac_off[-1])].numpy())


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_computed(tmp_path):
    """A C3 run of 128 problems (more than the dump holds): the line reports the steps asked for, and the dumped values of the
    sampled problems are the oracle's at the inputs bench.py builds."""
    import towr_amd as ta
    from oracle import binding as ob
    from tests.common import assert_parity

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "128",
           "--placement-tries", "1", "--device-warmup-s", "0", "--no-cpu-baseline", "--no-scale-c5", "--no-values-c3",
           "--no-timings-c3", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0

    model = ta.model_preset("anymal", "flat")
    sched, params, S = bench.build_case(ta, model)
    x = bench.perturbed_inputs(S, model, 128, first_seed=0)
    g_off, jac_off = np.arange(129) * S.m, np.arange(129) * S.nnz
    picked = bench.dump_problems(g_off, jac_off)
    assert 0 < len(picked) < 128
    dg = np.load(tmp_path / "g.npy").reshape(len(picked), S.m)
    dj = np.load(tmp_path / "jac.npy").reshape(len(picked), S.nnz)
    P = ob.OracleProblem("anymal", "flat", sched.durations(), sched.contact(), dt_dynamic=params.dt_dynamic, dt_rom=params.dt_rom,
                         duration_base_poly=params.duration_base_poly, polys_per_swing=params.polys_per_swing,
                         polys_per_stance_force=params.polys_per_stance_force, constraint_sets=params.constraint_sets)
    for i, p in enumerate(picked):
        og, _, _, ov = P.eval(x[p])
        assert_parity(S, dg[i], dj[i], og, ov, "problem %d" % p, x=x[p])
