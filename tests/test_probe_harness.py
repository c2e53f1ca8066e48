"""The failure rule of tests/probe.py (its module docstring), on the CPU tier: no test here touches a device.

The refusals are real: trig_probe is compiled once for this file and refuses its input on the host (exit 2).  The ends that
stop a session -- a signal, exit 4, the time limit -- are fabricated: subprocess.run is replaced inside tests.probe, no child
is started and no fault is provoked.  The stop state is set and restored through monkeypatch, so nothing is left behind for
the tests that follow.

That tests/probe_host.h compiles without a warning under both flag sets in use (the product's CXXFLAGS plus -Wextra, and
trig_probe's plain -O3 -std=c++17 -Wall -Wextra) is covered by the four test_probe_compiles_without_warning tests, which build
all four probes; it is not compiled a fifth time here."""
import subprocess

import pytest

from . import probe
from .probe import Probe

TRIG = Probe("trig_probe", flags=["-O3", "-std=c++17", "-Wall", "-Wextra"])


def _fresh_trig():
    """a Probe that remembers nothing yet, on the executable built once for this file"""
    p = Probe("trig_probe", flags=TRIG.flags)
    p._built, p._dir = (TRIG.build(), None), TRIG._dir
    return p


def test_a_refused_run_is_remembered_and_stops_nothing_else(monkeypatch):
    monkeypatch.setattr(probe, "_stop", None)
    p = _fresh_trig()
    with pytest.raises(AssertionError, match="trig_probe sincos: exit 2") as first:
        p.run("sincos", [])
    assert "do not make whole inputs" in str(first.value) and p.started == 1
    with pytest.raises(AssertionError, match="trig_probe sincos: exit 2") as second:
        p.run("sincos", [])
    assert str(second.value) == str(first.value) and p.started == 1, "the recorded failure, without a second child"
    with pytest.raises(AssertionError, match="trig_probe rot: exit 2"):      # two doubles are no whole triple
        p.run("rot", [0.1, 0.2])
    assert p.started == 2 and probe._stop is None, "exit 2 stops no other run"
    p.refuses(["rotquad"], [0.1, 0.2], "do not make whole inputs")
    assert p.started == 3


def _ends_with(status):
    def run(cmd, **kw):
        run.calls += 1
        if status is None:
            raise subprocess.TimeoutExpired(cmd, kw["timeout"])
        return subprocess.CompletedProcess(cmd, status, "", "fabricated\n")
    run.calls = 0
    return run


@pytest.mark.parametrize("status, words", [(-11, "exit -11"), (4, "exit 4"), (3, "exit 3"), (134, "exit 134"), (None, "time limit")])
def test_a_device_failure_stops_every_later_run(monkeypatch, status, words):
    p, other = _fresh_trig(), Probe("ik_probe")                  # (built before subprocess.run is replaced)
    monkeypatch.setattr(probe, "_stop", None)
    fake = _ends_with(status)
    monkeypatch.setattr(probe.subprocess, "run", fake)
    with pytest.raises(AssertionError, match=words):
        p.run("sincos", [0.5])
    assert fake.calls == 1 and "trig_probe sincos" in probe._stop and words in probe._stop
    for again in (lambda: p.run("sincos", [0.5]), lambda: p.run("rot", [0.1, 0.2, 0.3]), lambda: other.run("leg", [0.0]),
                  lambda: other.refuses([], None, "usage")):
        with pytest.raises(AssertionError, match=words) as e:
            again()
        assert "trig_probe sincos" in str(e.value)
    assert fake.calls == 1 and p.started == 1 and other.started == 0 and other._built is None, "nothing was compiled or started"


def test_a_failed_build_is_remembered(monkeypatch):
    calls = []
    monkeypatch.setattr(probe.subprocess, "run", lambda cmd, **kw: calls.append(cmd) or subprocess.CompletedProcess(cmd, 1, "", "error: fabricated\n"))
    p = Probe("trig_probe")
    for _ in range(2):
        with pytest.raises(AssertionError, match="hipcc exit 1"):
            p.build()
    assert len(calls) == 1
