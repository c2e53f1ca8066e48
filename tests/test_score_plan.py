"""The scoring plan of twr_batch_eval_scores, checked on the host: tests/score_plan_driver.cc, built with g++ against the
product's planner (towr_amd/csrc/structure.cc) under UndefinedBehaviorSanitizer, covers every row of every problem with
the fold's partial records exactly once, the slots of the slab, identical plans when planning twice, the scoring launches
of the fused path and of each fallback, and the unchanged plans of the existing evaluation flags."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_plan():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "score_plan_driver")
        subprocess.check_call(["g++", "-O1", "-g", "-D_GLIBCXX_ASSERTIONS", "-fsanitize=undefined", "-fno-sanitize-recover=undefined",
                               "-std=c++17", "-Wall", "-Wno-sign-compare", "-o", exe,
                               os.path.join(ROOT, "tests", "score_plan_driver.cc"),
                               os.path.join(ROOT, "towr_amd", "csrc", "structure.cc")])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr
