"""The committed rocprofv3 summaries must belong to the kernels in this tree: profiles/traffic.json carries a hash of
the kernel sources and build flags (bench.kernel_source_hash), bench.py drops roofline.traffic when it differs -- this
test makes a stale profile a red CPU tier instead of a silent null.  The kernel bodies live in towr_amd/csrc/kernels/*.h,
which that hash does not read: a second field (scripts/kernel_header_hash.py) covers them, and only this test checks it."""
import json
import os
import sys

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from kernel_header_hash import kernel_header_hash  # noqa: E402


def test_traffic_profile_matches_kernel_sources():
    with open(os.path.join(ROOT, "profiles", "traffic.json")) as f:
        t = json.load(f)
    assert t["kernel_source_sha256"] == bench.kernel_source_hash(), \
        "kernel sources changed after profiles/ was taken: re-run scripts/profile_r05.sh (GPU box) and scripts/profile_summary.py gpurun_out/prof_r05 r05"
    assert t["kernel_header_sha256"] == kernel_header_hash(), \
        "kernel headers changed after profiles/ was taken: re-run scripts/profile_r05.sh (GPU box) and scripts/profile_summary.py on its output"
    assert bench.traffic_from_profile("C3", "twr::rom_kernel", t["problems_per_gpu"]) > 0
    assert bench.traffic_from_profile("C3+timings", "twr::dyn_phase_kernel", 2048) > 0
    assert sum(t["sweep_1024"]["hbm_bytes_per_launch"].values()) > 0
