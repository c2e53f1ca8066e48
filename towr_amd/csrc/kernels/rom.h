#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../eval_plan.h"
#include "common.h"
#include "copy_out.h"
#include "rom_item.h"

namespace twr {
// rom_kernel is compiled in its own translation unit (rom_tu.hip) with a different instruction scheduling
// strategy: it is store bound and gains 4-5 % from clause-oriented scheduling, the VALU-bound kernels lose.
// (64 lanes x ~84 values -> 39 KiB, four workgroups per CU; kRomStage, the image: device_tables.h)
constexpr int kRomLds = kRomStage + 2 + 64 + 192;   // doubles: image, per-lane trash slots, g
// NIT = store instructions of the copy-out (eval_plan.cc PlanEval picks it).
// (The hand-scheduled form of dyn_phase_kernel -- asm loads into AGPRs, one counted wait behind the copy-out -- was built
// for this loop too and is SLOWER here, 0.98 vs 0.90 ms on one box: the compiler's clause-oriented schedule of the 28
// loads with scalar bases and immediate offsets beats 28 separate asm loads with per-lane 64-bit addresses.)
template <int NIT, bool WANT_G, bool WANT_J, bool NT>
TWR_DEV void rom_body(const RomWork* __restrict__ work, int n_work, const double* __restrict__ x, double* __restrict__ g,
                      double* __restrict__ jac, double* stage, int lane, int i, int stride) {
  static_assert(NIT * 128 <= kRomStage + 2 + 127, "copy-out longer than the image");
  const int trash = kRomStage + 2 + lane;
  double* gst = stage + (WANT_J ? kRomStage + 2 + 64 : 0);   // (values only: the wave's LDS is the 192 constraint values alone)
  if (i >= n_work) return;
  // Every prefetch is issued unconditionally, with the slice index clamped to this workgroup's last slice (a repeated load
  // of the last slice's records / x is harmless): no prefetched value goes through a phi or a conditional copy, which is
  // what makes the compiler wait for a load right where it is issued (round 4: a `r2 = r1; if (has2) r2 = load` form of
  // this loop waited with vmcnt(0) behind the record loads in every iteration -- +8 % with L2-resident tables, +17 % in a sweep).
  const int last = i + (n_work - 1 - i) / stride * stride;
  RomWork w0 = work[i], w1 = work[min(i + stride, last)], w2 = work[min(i + 2 * stride, last)];
  RomNode n0 = rom_load_node(w0, lane), n1 = rom_load_node(w1, lane), n2 = rom_load_node(w2, lane);
  RomSeg s0 = rom_load_seg(w0, n0), s1 = rom_load_seg(w1, n1);
  RomX X;
  rom_load_x(w0, n0, s0, x, X);
  for (; i <= last; i += stride) {
    const RomWork w3 = work[min(i + 3 * stride, last)];
    double* dst = jac + w0.j_off;
    const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
    if (lane < w0.cnt) rom_item(w0, rom_rec_of(w0, n0, s0, lane), X, gst, stage, par, 0, trash, lane, WANT_G, WANT_J);   // C
    const RomNode n3 = rom_load_node(w3, lane);         // A: node records three slices ahead, segment records two ahead
    const RomSeg s2 = rom_load_seg(w2, n2);             //    (records first: the wait for x retires them too)
    rom_load_x(w1, n1, s1, x, X);
    if (WANT_J) copy_out_fixed<NIT, 13, NT>(dst, stage, w0.nvals, par, lane);   // B
    if (WANT_G) {                                       //   3 constraint values per time node, contiguous in g: clamped
      double* go = g + w0.g_off;                        //   lanes instead of predicates (see copy_out_fixed)
      const int last_g = 3 * w0.cnt - 1;
#pragma unroll
      for (int t = 0; t < 3; ++t) go[min(lane + 64 * t, last_g)] = gst[min(lane + 64 * t, last_g)];
    }
    w0 = w1; n0 = n1; s0 = s1;
    w1 = w2; n1 = n2; s1 = s2;
    w2 = w3; n2 = n3;
  }
}

using RomFn = void (*)(const RomWork*, int, const double*, double*, double*);
RomFn rom_kernel_fn(const LaunchStep& p);   // rom_kernel's lookup, compiled in the rom unit
}  // namespace twr
