#!/usr/bin/env python3
"""Diagnostic build of the library with s_memtime stamps around the phases of dyn_kernel's loop (the product source has no
diagnostic hooks): patches a COPY of kernels/dyn.h, compiles kernels.hip with it and links towr_amd/libtowr_amd_dynstamps.so.  Run
scripts/diag/dyn_stamps.py with TWR_AMD_LIB pointing at that library for the per-phase split.
Every stamp waits for the wave's LDS / scalar queue (s_memtime returns through lgkmcnt): the split is what matters, and a
phase that follows LDS traffic is charged for draining it."""
from stamp_build import build

P = []


def rep(old, new):
    P.append((old, new))


rep("// XC = 64-entry chunks of the staging map the slices of the batch use",
    "__device__ unsigned long long g_dyn_stamps[1024 * 8];\n"
    "#define STAMP(k) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); acc[k] += t_ - t_last; t_last = t_; }\n"
    "// XC = 64-entry chunks of the staging map the slices of the batch use")
rep("  for (; i <= last; i += stride) {\n    const DynWork w3 = work[min(i + 3 * stride, last)];",
    "  unsigned long long acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t_last = __builtin_amdgcn_s_memtime();\n"
    "  const int i_first = i;\n"
    "  for (; i <= last; i += stride) {\n    const DynWork w3 = work[min(i + 3 * stride, last)];")
rep("    dyn2_front(fr0, xs, lane, S);                                                            // F\n",
    "    dyn2_front(fr0, xs, lane, S);\n    STAMP(0)\n")
rep("    dyn2_load_front(w1, sel1, lane, fr1);                                                    //    front records of slice i+1\n",
    "    dyn2_load_front(w1, sel1, lane, fr1);\n    STAMP(1)\n")
rep("    __builtin_amdgcn_s_setprio(0);\n    dyn2_back(", "    __builtin_amdgcn_s_setprio(0);\n    STAMP(2)\n    dyn2_back(")
rep("    stage_x(xr);                                                                             // S\n", "    STAMP(3)\n    stage_x(xr);\n")
rep("    mapr = load_map(w3);\n    wp = w0;", "    mapr = load_map(w3);\n    STAMP(4)\n    wp = w0;")
rep("    w2 = w3;\n  }\n  dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wp.nvals, wp.cnt, lane);   // last slice of this workgroup",
    "    w2 = w3;\n    acc[7] += 1;\n  }\n"
    "  if (lane == 0 && i_first < 1024 && WANT_G && WANT_J)\n    for (int q = 0; q < 8; ++q) g_dyn_stamps[i_first * 8 + q] = acc[q];\n"
    "  dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wp.nvals, wp.cnt, lane);   // last slice of this workgroup")
build("kernels/dyn.h", P,
      "extern \"C\" int twr_debug_dyn_stamps(unsigned long long* out, int n) {\n"
      "  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dyn_stamps), sizeof(unsigned long long) * (size_t)n);\n}\n",
      "libtowr_amd_dynstamps.so")
print("towr_amd/libtowr_amd_dynstamps.so built; run: TWR_AMD_LIB=$PWD/towr_amd/libtowr_amd_dynstamps.so python3 scripts/diag/dyn_stamps.py")
