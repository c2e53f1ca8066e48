"""The instantiation matrix of the evaluation kernels (tests/eval_matrix.py), checked on the host: tests/eval_matrix_driver.cc,
built with g++ against the product's planner (tests/host_build.py) under AddressSanitizer + UndefinedBehaviorSanitizer.  The driver
enumerates the complete set of instantiations from the key lists of eval_plan.h, builds every row of the matrix, plans every
flag set with and without per-kernel events plus the two scoring requests, and asserts that every row reaches what it
claims and that the claims plus the exclusion list (at most 8 rule-quoted entries) are exactly the complete set."""
import os
import subprocess
import tempfile

from tests import eval_matrix
from tests.host_build import plan_driver


def test_matrix_covers_every_instantiation():
    with tempfile.TemporaryDirectory() as tmp:
        exe = plan_driver("eval_matrix_driver")

        def run(name, text):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
            return subprocess.run([exe, os.path.join(tmp, name)], capture_output=True, text=True, timeout=600)

        r = run("matrix.txt", eval_matrix.MATRIX)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "87 of 87 instantiations reached, 0 excluded, 0 failures" in r.stdout and "runtime error" not in r.stderr
        # a row removed leaves its instantiations without cover, and the driver says which
        r = run("without.txt", "\n".join(l for l in eval_matrix.MATRIX.splitlines() if not l.startswith("row p40p6_p40 ")))
        assert r.returncode == 1 and "no row reaches rom_phase_kernel<0,GJ>" in r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_both_readers_parse_the_same_rows():
    structs, rows, exclusions = eval_matrix.parse()
    assert len(rows) == sum(l.startswith("row ") for l in eval_matrix.MATRIX.splitlines())
    assert len({r["name"] for r in rows}) == len(rows) and len(exclusions) <= 8
    for r in rows:
        assert set(r["structs"]) <= set(structs) and all(0 <= s < len(r["structs"]) for s in r["order"]), r["name"]
        limit = {"cheap": 8, "wide": 8}.get(r["kind"])
        assert limit is None or len(r["order"]) <= limit, r["name"]
        if r["kind"] == "cheap":
            assert all(int(structs[s].get("K", 40)) <= 200 and structs[s].get("terrain", "flat") in ("flat", "stairs", "gap") for s in r["structs"])
        if r["kind"] == "nt":
            assert r["nt"] and 4 * len(r["structs"]) > len(r["order"]), r["name"]
