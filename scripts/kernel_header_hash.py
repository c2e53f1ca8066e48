"""Identity of the kernel bodies a profile was taken on: bench.kernel_source_hash covers kernels.hip, rom_tu.hip,
device_tables.h and the Makefile; the kernels themselves live in towr_amd/csrc/kernels/*.h and, the utility kernels, in
towr_amd/csrc/util_tu.hip, which this hash covers
(profiles/traffic.json "kernel_header_sha256", written by profile_summary.py, asserted by tests/test_profiles_fresh.py)."""
import glob
import hashlib
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_header_hash():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "towr_amd", "csrc")
    for path in sorted(glob.glob(os.path.join(csrc, "kernels", "*.h"))) + [os.path.join(csrc, "util_tu.hip")]:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


if __name__ == "__main__":
    print(kernel_header_hash())
