"""The scoring plan of twr_batch_eval_scores, checked on the host: tests/score_plan_driver.cc, built with g++ against the
product's planner (tests/host_build.py) under AddressSanitizer + UndefinedBehaviorSanitizer, covers every row of every problem with
the fold's partial records exactly once, the slots of the slab, identical plans when planning twice, the scoring launches
of the fused path and of each fallback, and the unchanged plans of the existing evaluation flags."""
import subprocess

from tests.host_build import plan_driver


def test_score_plan():
    exe = plan_driver("score_plan_driver")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr
