"""Builds the stand-alone host plan drivers (tests/*_driver.cc) for the CPU tests: the product's host planner
(towr_amd/csrc: structure, presets and the batch, evaluation and solver plans -- no HIP in them) is compiled ONCE per
process under AddressSanitizer + UndefinedBehaviorSanitizer, every driver is compiled with the same flags and linked against
those objects.  The objects live in a temporary directory of this process, removed at exit: two pytest processes never
write the same file.  The drivers are programs with a main of their own; nothing here is loaded into Python."""
import atexit
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "towr_amd", "csrc")
HOST_SOURCES = ["structure.cc", "presets.cc", "batch_plan.cc", "eval_plan.cc", "jac_plan.cc"]
FLAGS = ["-O1", "-g", "-D_GLIBCXX_ASSERTIONS", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
         "-std=c++17", "-Wall", "-Wno-sign-compare"]

_dir = None
_objects = None


def _run(cmd):
    print("host_build:", " ".join(cmd), file=sys.stderr)   # (one line per compiler invocation: the tests' log shows how many)
    subprocess.check_call(cmd)


def _planner_objects():
    global _dir, _objects
    if _objects is None:
        _dir = tempfile.mkdtemp(prefix="twr_host_build_")
        atexit.register(shutil.rmtree, _dir, ignore_errors=True)
        objects = [os.path.join(_dir, src[:-3] + ".o") for src in HOST_SOURCES]
        jobs = [subprocess.Popen(["g++"] + FLAGS + ["-c", "-o", obj, os.path.join(CSRC, src)]) for src, obj in zip(HOST_SOURCES, objects)]
        for job in jobs:   # (side by side: five compiler invocations, once)
            print("host_build:", " ".join(job.args), file=sys.stderr)
            job.wait()
        for job in jobs:
            if job.returncode != 0:
                raise subprocess.CalledProcessError(job.returncode, job.args)
        _objects = objects
    return _objects


def plan_driver(name, defines=()):
    """The path of tests/<name>.cc built against the host planner (with -D<define> for every define)."""
    objects = _planner_objects()
    exe = os.path.join(_dir, "_".join([name, *defines]))
    if not os.path.exists(exe):
        _run(["g++"] + FLAGS + ["-D" + d for d in defines] + ["-o", exe, os.path.join(ROOT, "tests", name + ".cc")] + objects)
    return exe
