#pragma once
#include <stddef.h>

#include "../device_tables.h"
#include "dyn.h"
#include "node.h"
#include "rom.h"

namespace twr {
// Small and mid-size batches: the three kernels above as ONE launch, so that their pipeline fills and drains overlap
// instead of adding up (three dependent launches cost ~14 us of a 19-us step at 32 candidates).  Workgroups of two waves
// and 40 KB: blocks [0, g_rom) take the rom role (wave 0 only; the image is 39 KB), the next g_dyn blocks the dyn role
// (both waves, one 20-KB half each), the rest the node role (two families per block) -- the residency per CU of each
// role is that of its own kernel, and blocks are dispatched in this order, so a later role starts as the earlier drains.
template <int ROM_NIT, bool WANT_G, bool WANT_J, int XC, bool NT>
__global__ __launch_bounds__(128, 2) void eval_fused_kernel(const RomWork* __restrict__ rom, int n_rom, int g_rom,
                                                            const DynWork* __restrict__ dyn, int n_dyn, int g_dyn,
                                                            const NodeWork* __restrict__ node, const double* __restrict__ x,
                                                            double* __restrict__ g, double* __restrict__ jac,
                                                            double* __restrict__ dump) {
  constexpr int kFusedLds = 2 * kDynLds >= kRomLds ? 2 * kDynLds : kRomLds;   // (the second case: experiment builds with small dyn images)
  static_assert(kDynLds >= kStageForce, "LDS of the fused kernel");
  __shared__ __attribute__((aligned(16))) double stage[kFusedLds];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  int b = blockIdx.x;
  if (b < g_rom) {
    if (wave == 0) rom_body<ROM_NIT, WANT_G, WANT_J, NT>(rom, n_rom, x, g, jac, stage, lane, b, g_rom);
    return;
  }
  b -= g_rom;
  if (b < g_dyn) {
    // Which slices a block's two waves take: the work list is ordered so that position j wants XCD j % 8 (all slices of one
    // problem on one XCD, capi.cc), and blocks are dealt round-robin over the XCDs -- so block 8 q + r takes positions
    // 16 q + r and 16 q + 8 + r: every position a block ever visits is r modulo 8.  (With positions 2 b, 2 b + 1 the
    // slices of a problem ran on two XCDs, and its x and tables were fetched by both.)  Needs g_dyn to be a multiple
    // of 8 (the launcher rounds it down); tiny grids keep the plain mapping.
    const int first = (g_dyn & 7) == 0 ? ((b >> 3) << 4) + (wave << 3) + (b & 7) : 2 * b + wave;
    dyn_body<WANT_G, WANT_J, XC, NT>(dyn, n_dyn, x, g, jac, dump, stage + wave * kDynLds, lane, first, 2 * g_dyn);
    return;
  }
  b -= g_dyn;
  const int family = 2 * (b & 1) + wave;
  node_body(node[b >> 1], x, g, jac, (WANT_G ? 1 : 0) | (WANT_J ? 2 : 0), stage + wave * kDynLds, family, lane);
}
}  // namespace twr
