"""TEST INFRASTRUCTURE ONLY -- builds oracle/_ref/ik_ref from the reference's two Go1 inverse-kinematics sources, compiled where
they lie against the stand-ins under tests/ik_ref/shim, and records tests/golden/refik_go1.npz: the feet of tests/ik_points.py
and what GetJointAngles (both bends) and GetAllJointAngles return for them, as doubles.  Data only.

    python -m tests.ik_ref.record          # re-records the fixture (where the reference sources are)
"""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from tests import ik_points as ip

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def _reference_dir():
    """where oracle/ref_dump/build.sh looks for the reference's towr/ tree: TOWR_REFERENCE_DIR, else that recipe's default"""
    env = os.environ.get("TOWR_REFERENCE_DIR")
    if env:
        return env
    m = re.search(r"^REF=\$\{TOWR_REFERENCE_DIR:-([^}]*)\}", open(os.path.join(ROOT, "oracle", "ref_dump", "build.sh")).read(), re.M)
    return m.group(1) if m else ""


REF = _reference_dir()
EXE = os.path.join(ROOT, "oracle", "_ref", "ik_ref")
FIXTURE = os.path.join(ROOT, "tests", "golden", "refik_go1.npz")
SOURCES = ("src/go1/go1leg_inverse_kinematics.cc", "src/go1/inverse_kinematics_go1.cc")


def available():
    """True where the reference's sources are"""
    return all(os.path.exists(os.path.join(REF, s)) for s in SOURCES)


def build():
    """oracle/_ref/ik_ref: g++ -O2 -ffp-contract=off on the recorder's main and the reference's two files"""
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = [shutil.which("g++") or "g++", "-O2", "-ffp-contract=off", "-std=c++17", "-I", os.path.join(HERE, "shim"),
           "-I", os.path.join(REF, "include"), os.path.join(HERE, "main.cc")] + [os.path.join(REF, s) for s in SOURCES] + ["-o", EXE]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


def compute():
    """the arrays of the fixture, from a run of the reference's code"""
    feet, bends, _ = ip.leg_points()
    body = ip.body_points()
    exe = build()
    with tempfile.TemporaryDirectory(prefix="twr_ik_ref_") as d:
        fin, fout = os.path.join(d, "in"), os.path.join(d, "out")
        np.concatenate([[float(len(feet))], np.column_stack([feet, bends]).ravel(), [float(len(body))], body.ravel()]).tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out = np.fromfile(fout, dtype=np.float64)
    assert out.size == 8 + 3 * len(feet) + 12 * len(body)
    return dict(constants=out[:8], leg_feet=np.array(feet), leg_bend=np.array(bends), leg_q=out[8:8 + 3 * len(feet)].reshape(-1, 3),
                body_feet=np.array(body), body_q=out[8 + 3 * len(feet):].reshape(-1, 4, 3))


def main():
    if not available():
        raise SystemExit("the reference sources are not at %s" % REF)
    np.savez_compressed(FIXTURE, **compute())
    print("%s: %d bytes" % (FIXTURE, os.path.getsize(FIXTURE)))


if __name__ == "__main__":
    main()
