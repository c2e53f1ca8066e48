"""The uniform dyn plan, checked on the host: tests/dyn_uniform_plan_driver.cc, built with g++ against the product's planner
(tests/host_build.py) under AddressSanitizer + UndefinedBehaviorSanitizer.  ANYmal at K = 200 / 52 / 40 (16 / 5 / 4 slices per problem,
the trimmed grid at 5) in batches of 1, 5, 8, 400 and 1603 problems: the schedule dyn_uniform_kernel runs evaluates every
slice of every problem exactly once, every wave sees one slice kind, a problem's slices share XCD and iteration, the grid
rule and its fallback hold, planning twice gives identical bytes, and the lists and plans of every batch -- two equal
structures alternating, ragged, optimised timings, and the uniform batches' own lists and fused / values-only plans --
are the parent commit's (hashes recorded from it)."""
import subprocess

from tests.host_build import plan_driver


def test_dyn_uniform_plan():
    exe = plan_driver("dyn_uniform_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr
