"""Shared by the stamp_*.py scripts (the product source has no diagnostic hooks): patches a COPY of one kernel source by
exact text, compiles the unit that holds or includes it (kernels.hip) from a copy of the sources and links a diagnostic library
from that object and the product's other objects (run `make -C towr_amd/csrc` first)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SRC = os.path.join(ROOT, "towr_amd", "csrc")
OTHER_OBJ = ["rom_tu.o", "util_tu.o", "jac_tu.o", "structure.o", "presets.o", "batch_plan.o", "eval_plan.o", "jac_plan.o", "capi.o", "capi_jac.o"]
UNIT_END = "\n}  // namespace twr\n"


def build(source, patches, accessor, lib):
    """source: the file that holds the patched text, relative to towr_amd/csrc (kernels/dyn.h, kernels/dyn_phase.h); patches: (old, new) pairs, every `old`
    must occur; accessor: code appended to the unit inside namespace twr; lib: name of the library under towr_amd/."""
    tmp = os.path.join(ROOT, "towr_amd", "_stamp_csrc")   # a sibling of csrc: relative includes resolve as in the product
    obj = os.path.join(SRC, "_kernels_stamps.o")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    shutil.rmtree(tmp, ignore_errors=True)
    try:
        os.makedirs(tmp)
        for f in os.listdir(SRC):
            if f.endswith(".h") or f == "kernels.hip":
                shutil.copy(os.path.join(SRC, f), tmp)
        shutil.copytree(os.path.join(SRC, "kernels"), os.path.join(tmp, "kernels"))
        path = os.path.join(tmp, source)
        s = open(path).read()
        for old, new in patches:
            assert old in s, old[:70]
            s = s.replace(old, new, 1)
        open(path, "w").write(s)
        unit = open(os.path.join(tmp, "kernels.hip")).read()
        assert unit.endswith(UNIT_END), "end of kernels.hip"
        open(os.path.join(tmp, "kernels.hip"), "w").write(unit[:-len(UNIT_END)] + "\n" + accessor + UNIT_END)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "-o", obj, "kernels.hip"], cwd=tmp)
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "--hip-link", "-fPIC", "-shared", "-o", os.path.join(ROOT, "towr_amd", lib),
                               os.path.basename(obj)] + OTHER_OBJ, cwd=SRC)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
        if os.path.exists(obj):
            os.remove(obj)
