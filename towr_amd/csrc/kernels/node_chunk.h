#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "copy_out.h"
#include "node.h"
#include "terrain.h"

namespace twr {
// ---------------------------------------------------------------- node-based sets of large batches: persistent chunks
// node_kernel is one chain of dependent loads per wave (work item -> header -> records -> x) and lives on occupancy alone
// (PMC: waiting 0.80-0.85 of the wave cycles).  For batches of more than a few thousand problems the same rows are evaluated
// by PERSISTENT waves instead: one wave = one family, walking that family's chunk list (FamWork) with a stride, the
// records of the chunk two items ahead and its x values one item ahead already in flight while the current chunk is
// computed and streamed out.  Every prefetch is unconditional with a clamped index (no phi on in-flight values, see
// rom_body).  Same arithmetic as node_body, statement by statement, so the same bits.
template <int FAM>
struct FamIn {
  int32_t a[6];        // the lane's record: TerrainRow | ForceNode | (unused) | SwingNode
  double c[6];         // family 2: the junction's six coefficients
  double v[8];         // x values: 3 | 5 | 6 | 8
};
template <int FAM>
TWR_DEV void fam_load_rec(const FamWork& w, int lane, FamIn<FAM>& in) {
  const int i = min(lane, w.cnt - 1);
  if (FAM == 0 || FAM == 1) {
    const int2 r = gptr<int2>(w.table)[i];
    in.a[0] = r.x; in.a[1] = r.y;
  } else if (FAM == 2) {
    const int rem = (w.i0 + i) % w.aux0;
    const TWR_GLOBAL double* a = reinterpret_cast<const TWR_GLOBAL double*>(w.table) + 6 * (rem / 3);
#pragma unroll
    for (int q = 0; q < 6; ++q) in.c[q] = a[q];
  } else {
    const TWR_GLOBAL int32_t* r = reinterpret_cast<const TWR_GLOBAL int32_t*>(w.table) + 6 * i;
#pragma unroll
    for (int q = 0; q < 5; ++q) in.a[q] = r[q];
  }
}
template <int FAM>
TWR_DEV void fam_load_x(const FamWork& w, int lane, const double* __restrict__ x, FamIn<FAM>& in) {
  const double* xp = x + w.x_off;
  if (FAM == 0) {        // TerrainRow {idx, stride}
    in.v[0] = xp[in.a[0]]; in.v[1] = xp[in.a[0] + in.a[1]]; in.v[2] = xp[in.a[0] + 2 * in.a[1]];
  } else if (FAM == 1) { // ForceNode {fidx, hidx}
    in.v[0] = xp[in.a[0]]; in.v[1] = xp[in.a[0] + 2]; in.v[2] = xp[in.a[0] + 4];
    in.v[3] = xp[in.a[1]]; in.v[4] = xp[in.a[1] + 1];
  } else if (FAM == 2) {
    const int r = w.i0 + min(lane, w.cnt - 1);
    const int which = r >= w.aux0, rem = r - which * w.aux0;
    const int j = rem / 3, d = rem - 3 * j;
    const double* xb = xp + (which ? w.aux1 : 0) + 6 * j + d;
#pragma unroll
    for (int q = 0; q < 6; ++q) in.v[q] = xb[3 * q];
  } else {               // SwingNode {cur, prev_x, prev_y, next_x, next_y}
    in.v[0] = xp[in.a[1]]; in.v[1] = xp[in.a[3]]; in.v[2] = xp[in.a[0]]; in.v[3] = xp[in.a[0] + 1];
    in.v[4] = xp[in.a[2]]; in.v[5] = xp[in.a[4]]; in.v[6] = xp[in.a[0] + 2]; in.v[7] = xp[in.a[0] + 3];
  }
}
// Items per chunk, Jacobian values and constraint values per item, store instructions of the copy-out (128 doubles each:
// the largest chunk + parity shift), g store instructions (64 values each)
template <int FAM>
struct FamShape {
  static constexpr int kItems = FAM == 1 ? 32 : 64;
  static constexpr int kPer = FAM == 0 ? 3 : (FAM == 1 ? 25 : (FAM == 2 ? 6 : 12));
  static constexpr int kRows = FAM == 0 ? 1 : (FAM == 1 ? 5 : (FAM == 2 ? 1 : 4));
  static constexpr int kNit = (kItems * kPer + 1 + 2 + 127) / 128;
  static constexpr int kGit = (kItems * kRows + 63) / 64;
};
// The chunk's values go to the LDS image (Jacobian) and to `gst` (constraint values); fam_store then streams both out with a
// COMPILE-TIME number of store instructions and no store inside a divergent branch -- like rom_body / dyn_body, and for the
// same reason: with the run-time copy-out loop and the lanes' own g stores of the first form of this kernel the compiler
// could not count the stores behind the prefetched loads, and every chunk began with s_waitcnt vmcnt(0), i.e. with the
// drain of the previous chunk's stores (A/B on one box with the work items three chunks ahead as well: 0.078 -> 0.069-0.074 ms per
// 8192 problems with towr's default list).
template <int FAM, bool WANT_G, bool WANT_J>
TWR_DEV void fam_compute(const FamWork& w, const FamIn<FAM>& in, double* stage, double* gst, int par, int lane) {
  const DevStruct* S = reinterpret_cast<const DevStruct*>(w.blob);
  if (lane < w.cnt) {
    if (FAM == 0) {
      const Terr t = terrain_eval(S, S->terrain_id, S->flat_height, in.v[0], in.v[1]);
      if (WANT_G) gst[lane] = in.v[2] - t.h;
      if (WANT_J) {
        stage[par + 3 * lane + 0] = -t.hx;
        stage[par + 3 * lane + 1] = -t.hy;
        stage[par + 3 * lane + 2] = 1.0;
      }
    } else if (FAM == 1) {
      const double f[3] = {in.v[0], in.v[1], in.v[2]};
      force_core(S, f, in.v[3], in.v[4], gst + 5 * lane, stage + par + 25 * lane, WANT_G, WANT_J);
    } else if (FAM == 2) {
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        v += in.c[q] * in.v[q];
        if (WANT_J) stage[par + 6 * lane + q] = in.c[q];
      }
      if (WANT_G) gst[lane] = v;
    } else {
      const double it = w.inv_t_swing;
#pragma unroll
      for (int dim = 0; dim < 2; ++dim) {
        const double prev = in.v[4 * dim], next = in.v[4 * dim + 1], pos = in.v[4 * dim + 2], vel = in.v[4 * dim + 3];
        const double distance = next - prev;
        if (WANT_G) {
          gst[4 * lane + 2 * dim] = pos - (prev + 0.5 * distance);
          gst[4 * lane + 2 * dim + 1] = vel - distance * it;
        }
        if (WANT_J) {
          double* st = stage + par + 12 * lane + 6 * dim;
          st[0] = -0.5; st[1] = 1.0; st[2] = -0.5;
          st[3] = it;   st[4] = 1.0; st[5] = -it;
        }
      }
    }
  }
}
template <int FAM, bool WANT_G, bool WANT_J>
TWR_DEV void fam_store(const FamWork& w, double* __restrict__ g, double* __restrict__ jac, const double* stage, const double* gst,
                       int par, int lane) {
  typedef FamShape<FAM> Sh;
  // (non-temporal: A/B on one box, towr's default list, 8192 problems of one structure: 0.067 -> 0.063 ms)
  if (WANT_J) copy_out_fixed<Sh::kNit, Sh::kNit, true>(jac + w.j_off, stage, Sh::kPer * w.cnt, par, lane);   // single wave: LDS accesses are ordered
  if (WANT_G) {   // clamped lanes instead of predicates (see copy_out_fixed)
    double* gp = g + w.g_off;
    const int last_g = Sh::kRows * w.cnt - 1;
#pragma unroll
    for (int t = 0; t < Sh::kGit; ++t) gp[min(lane + 64 * t, last_g)] = gst[min(lane + 64 * t, last_g)];
  }
}
// A use of every loaded value of the prologue that the compiler can see: it then waits for the prologue's loads IN the prologue
// and the loop is entered with none in flight.  (Otherwise the one wait in front of a chunk's math has to serve both ways
// into the loop header -- from the prologue, where the x loads of the first chunk are the youngest loads, and from the
// latch, where a counted number of stores is behind them -- and becomes s_waitcnt vmcnt(0): the store drain again.)
template <int FAM>
TWR_DEV void fam_pin(FamIn<FAM>& in, bool with_x) {
  constexpr int kA = FAM == 2 ? 0 : (FAM == 3 ? 5 : 2), kC = FAM == 2 ? 6 : 0, kV = FAM == 0 ? 3 : (FAM == 1 ? 5 : (FAM == 2 ? 6 : 8));
#pragma unroll
  for (int q = 0; q < kA; ++q) asm volatile("" : "+v"(in.a[q]));
#pragma unroll
  for (int q = 0; q < kC; ++q) asm volatile("" : "+v"(in.c[q]));
  if (with_x) {
#pragma unroll
    for (int q = 0; q < kV; ++q) asm volatile("" : "+v"(in.v[q]));
  }
}
template <int FAM, bool WANT_G, bool WANT_J>
TWR_DEV void fam_body(const FamWork* __restrict__ work, int n_work, const double* __restrict__ x, double* __restrict__ g,
                      double* __restrict__ jac, double* stage, double* gst, int lane, int i, int stride) {
  if (i >= n_work) return;
  const int last = i + (n_work - 1 - i) / stride * stride;
  FamWork w0 = work[i], w1 = work[min(i + stride, last)], w2 = work[min(i + 2 * stride, last)];
  FamIn<FAM> in0, in1;
  fam_load_rec<FAM>(w0, lane, in0);
  fam_load_rec<FAM>(w1, lane, in1);
  fam_load_x<FAM>(w0, lane, x, in0);
  fam_pin<FAM>(in0, true);
  fam_pin<FAM>(in1, false);
  for (; i <= last; i += stride) {
    const FamWork w3 = work[min(i + 3 * stride, last)];   // work item three chunks ahead (the list is a cold stream: a scalar
                                                          // load that is used in the iteration it is issued in costs its HBM latency)
    FamIn<FAM> in2;
    fam_load_rec<FAM>(w2, lane, in2);          // records two chunks ahead
    fam_load_x<FAM>(w1, lane, x, in1);         // x one chunk ahead (its records arrived an iteration ago)
    const int par = (int)((reinterpret_cast<uintptr_t>(jac + w0.j_off) >> 3) & 1);
    fam_compute<FAM, WANT_G, WANT_J>(w0, in0, stage, gst, par, lane);
    fam_store<FAM, WANT_G, WANT_J>(w0, g, jac, stage, gst, par, lane);
    w0 = w1; in0 = in1;
    w1 = w2; in1 = in2;
    w2 = w3;
  }
}
// blocks [0, g0) walk the terrain chunks, the next g1 the force chunks, then splineacc, then swing (any count may be 0)
constexpr int kStageChunk = kForceChunk * 25 + 2;                // >= 64 x 12 + 2 (swing), 64 x 6 + 2, 64 x 3 + 2
constexpr int kStageChunkG = 64 * 4;                             // constraint values of a chunk: <= 64 x 4 (swing), 32 x 5 (force)
static_assert(kStageChunk >= kStageSwing && kStageChunk >= kStageAcc && kStageChunk >= kStageTerrain, "chunk image");
static_assert(FamShape<1>::kItems == kForceChunk && FamShape<0>::kNit * 128 <= kStageChunk + 127 && FamShape<1>::kNit * 128 <= kStageChunk + 127 &&
              FamShape<2>::kNit * 128 <= kStageChunk + 127 && FamShape<3>::kNit * 128 <= kStageChunk + 127, "chunk copy-out inside the image");
template <bool WANT_G, bool WANT_J>
__global__ __launch_bounds__(64, 4) void node_chunk_kernel(const FamWork* __restrict__ f0, int n0, int g0, const FamWork* __restrict__ f1,
                                                        int n1, int g1, const FamWork* __restrict__ f2, int n2, int g2,
                                                        const FamWork* __restrict__ f3, int n3, int g3, const double* __restrict__ x,
                                                        double* __restrict__ g, double* __restrict__ jac) {
  __shared__ __attribute__((aligned(16))) double stage[kStageChunk + kStageChunkG];
  double* gst = stage + kStageChunk;
  const int lane = threadIdx.x;
  int b = blockIdx.x;
  if (b < g0) return fam_body<0, WANT_G, WANT_J>(f0, n0, x, g, jac, stage, gst, lane, b, g0);
  b -= g0;
  if (b < g1) return fam_body<1, WANT_G, WANT_J>(f1, n1, x, g, jac, stage, gst, lane, b, g1);
  b -= g1;
  if (b < g2) return fam_body<2, WANT_G, WANT_J>(f2, n2, x, g, jac, stage, gst, lane, b, g2);
  b -= g2;
  fam_body<3, WANT_G, WANT_J>(f3, n3, x, g, jac, stage, gst, lane, b, g3);
}
}  // namespace twr
