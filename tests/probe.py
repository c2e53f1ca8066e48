"""Builds and runs the stand-alone device probes (tests/<name>.hip on tests/probe_host.h) for tests/test_*_probe.py, and holds
the few helpers those files share.  A probe is a program with a main of its own; every run is a fresh child process
`<exe> <mode> IN OUT` on a file of raw doubles, and nothing here is loaded into Python.

A probe's exit status (probe_host.h): 0 done, 2 usage / file error, 3 no HIP device, 4 a HIP call failed.

The failure rule of this runner:
 1. The outcome of Probe.run is remembered per (probe, mode), success or failure (a mode always gets the same data).  A second
    request for a mode that failed raises the recorded failure; it starts no child.
 2. Exit 2 is a refused file or a usage error: it comes from the host-side parser or the file layer, never from a device, and
    stops nothing else.  Every other end but 0 -- exit 3, exit 4, death by a signal (a negative status, 134, 139), the time limit,
    or a status the probes do not define -- stops the session: every later child of any probe in this process, run or refusal
    check, fails at once with a message that names the probe, the mode and the status that stopped it, and starts nothing.
    Nothing more is started on a device after a fault until its cause is known.
 3. A failed build is remembered too: the same broken source is not compiled once per test."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
GOLDEN = os.path.join(ROOT, "tests", "golden")
RUN_LIMIT = 120     # seconds for a run on a device; a refusal is decided on the host and gets half

_stop = None        # why no further child is started in this process (rule 2), or None


def product_cxxflags():
    """CXXFLAGS of towr_amd/csrc/Makefile, the flags kernels.o is compiled with"""
    text = open(os.path.join(ROOT, "towr_amd", "csrc", "Makefile")).read()
    m = re.search(r"^CXXFLAGS \?= (.*)$", text, re.M)
    assert m, "CXXFLAGS ?= ... not found in towr_amd/csrc/Makefile"
    return m.group(1).split()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def load_fixture(name):
    """tests/golden/<name>.npz as a dict of read-only arrays"""
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = {k: d[k] for k in d.files}
    for v in out.values():
        v.flags.writeable = False
    return out


class Probe:
    """tests/<name>.hip compiled for gfx950 with `flags` (default: the product's CXXFLAGS plus -Wextra)"""

    def __init__(self, name, flags=None):
        self.name, self.flags = name, flags
        self.started = 0        # children started, runs and refusal checks
        self._dir = self._built = None
        self._runs = {}         # mode -> (raw doubles, None) or (None, the failure's message)

    def build(self):
        """the executable's path; compiled at most once, without a warning"""
        if self._built is None:
            self._dir = tempfile.mkdtemp(prefix="twr_%s_" % self.name)
            atexit.register(shutil.rmtree, self._dir, ignore_errors=True)
            exe = os.path.join(self._dir, self.name)
            flags = product_cxxflags() + ["-Wextra"] if self.flags is None else list(self.flags)
            cmd = [HIPCC, "--offload-arch=gfx950"] + flags + ["-I", os.path.join(ROOT, "towr_amd", "csrc"),
                                                               os.path.join(ROOT, "tests", self.name + ".hip"), "-o", exe]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0 or "warning" in r.stdout + r.stderr:
                self._built = (None, "%s: hipcc exit %d\n%s%s" % (self.name, r.returncode, r.stdout, r.stderr))
            else:
                self._built = (exe, None)
        exe, failure = self._built
        if failure:
            raise AssertionError(failure)
        return exe

    def _child(self, mode_args, data, stem, limit):
        """(exit status, stderr, stdout + stderr, OUT) of a fresh child `exe mode_args... IN OUT` on a file IN of `data` (of
        `exe` alone where mode_args is empty), under rule 2"""
        global _stop
        what = " ".join([self.name] + list(mode_args))
        if _stop:
            raise AssertionError("%s: not started: %s" % (what, _stop))
        cmd, fout = [self.build()] + list(mode_args), os.path.join(self._dir, stem + ".out")
        if mode_args:
            fin = os.path.join(self._dir, stem + ".in")
            np.ascontiguousarray(data, dtype=np.float64).tofile(fin)
            cmd += [fin, fout]
        self.started += 1
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            _stop = "%s ran into its time limit of %d s; nothing more is started in this session" % (what, limit)
            raise AssertionError(_stop)
        if r.returncode not in (0, 2):
            _stop = "%s ended with exit %d; nothing more is started in this session" % (what, r.returncode)
        return r.returncode, r.stderr, r.stdout + r.stderr, fout

    def run(self, mode, data):
        """the raw doubles (read-only) the probe writes for `mode` on the doubles `data`, under rule 1"""
        if mode not in self._runs:
            status, _, output, fout = self._child([mode], data, mode, RUN_LIMIT)    # (raises, unrecorded, once the session is stopped)
            if status == 0:
                out = np.fromfile(fout, dtype=np.float64)
                out.flags.writeable = False
                self._runs[mode] = (out, None)
            else:
                self._runs[mode] = (None, "%s %s: exit %d\n%s" % (self.name, mode, status, output))
        out, failure = self._runs[mode]
        if failure:
            raise AssertionError(failure)
        return out

    def refuses(self, mode_args, data, text):
        """(CPU tier) the probe, started with `mode_args` on a file of `data` (with no argument at all where mode_args is
        empty), exits 2 with `text` in its stderr: refused on the host before anything reaches a device"""
        status, err, output, _ = self._child(mode_args, data, "refused", RUN_LIMIT // 2)
        assert status == 2 and text in err, "%s %s: exit %d, no %r in\n%s" % (self.name, " ".join(mode_args), status, text, output)
