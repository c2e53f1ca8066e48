#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "copy_out.h"
#include "spline_math.h"
#include "terrain.h"

namespace twr {
// all terrain-ee-motion_e (terrain_constraint.cc:57-108), force-ee-force_e, splineacc-base-* and
// swing-ee-motion_e sets of one problem.  One workgroup of four waves per problem, one wave per family
// (each with its own LDS image, no barriers), 64 spline nodes / rows at a time.
// Candidate scoring without g (eval_scores_kernel): where the values-only kernel stores a constraint value, the scoring
// instantiation turns it into the row's bound violation max(lower - g, g - upper, 0) -- bounds from the structure's score
// record at kScoreOff (the row's 16-bit meta word, its (lower, upper) pair in the 2-KB head), exactly as score_kernel --
// and adds it to the lane's running (max, sum) of the row's family F (the TWR_SET_* bit; every call site knows its family).
// flush() reduces the lanes over a fixed xor tree and writes the wave's partial record: kScorePartial doubles laid out as a
// score row, 2 F = max, 2 F + 1 = sum.
enum ScoreFamily { kFamTerrain = 0, kFamDyn = 1, kFamAcc = 2, kFamRom = 3, kFamForce = 4, kFamSwing = 5, kFamTotal = 6, kFamBaseMotion = 7 };
struct ScoreAcc {
  const uint16_t* meta;
  const double* pairs;
  double m[8], s[8];
  TWR_DEV explicit ScoreAcc(uint64_t blob)
      : meta(reinterpret_cast<const uint16_t*>(blob + kScoreOff + kScoreHeadBytes)),
        pairs(reinterpret_cast<const double*>(blob + kScoreOff + sizeof(ScoreTables))) {
#pragma unroll
    for (int f = 0; f < 8; ++f) m[f] = s[f] = 0.0;
  }
  template <int F>
  TWR_DEV void put(int row, double val) {   // row: the problem's row index
    const int q = (int)(meta[row] & 0xFFFu);
    const double lo = pairs[2 * q], up = pairs[2 * q + 1];
    double viol = fmax(fmax(lo - val, val - up), 0.0);
    if (val != val) viol = val;
    m[F] = nan_max(m[F], viol);
    s[F] += viol;
  }
  // the n values of rows row0 .. row0 + n - 1, staged in LDS at gs[0 .. n) (n <= 64 NIT)
  template <int F, int NIT>
  TWR_DEV void rows(const double* gs, int row0, int n, int lane) {
#pragma unroll
    for (int t = 0; t < NIT; ++t)
      if (lane + 64 * t < n) put<F>(row0 + lane + 64 * t, gs[lane + 64 * t]);
  }
  template <int FA, int FB>   // the families the wave has met (FB = FA: one)
  TWR_DEV void flush(double* __restrict__ rec, int lane) {
    double r[4] = {m[FA], s[FA], m[FB], s[FB]};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1)
#pragma unroll
      for (int k = 0; k < (FA == FB ? 2 : 4); ++k) {
        const double v = __shfl_xor(r[k], o);
        r[k] = (k & 1) ? r[k] + v : nan_max(r[k], v);
      }
    if (lane < kScorePartial) {
      const int f = lane >> 1;
      const double v = f == FA ? r[lane & 1] : f == FB ? r[2 + (lane & 1)] : 0.0;
      rec[lane] = v;
    }
  }
};
constexpr int kStageTerrain = 64 * 3 + 2, kStageForce = 64 * 25 + 2, kStageAcc = 64 * 6 + 2, kStageSwing = 64 * 12 + 2;
constexpr int kNodeStageOff[4] = {0, kStageTerrain, kStageTerrain + kStageForce, kStageTerrain + kStageForce + kStageAcc};
// one family (wave-uniform 0..3) of one problem; `stage`: the family's LDS image (kStage<Family> doubles)
// (SCORE: the values go to sc instead of g -- eval_scores_kernel, flags = values only)
template <bool SCORE = false>
TWR_DEV void node_body(const NodeWork& w, const double* __restrict__ x, double* __restrict__ g, double* __restrict__ jac,
                       int flags, double* stage, int family, int lane, ScoreAcc* sc = nullptr) {
  const char* blob = reinterpret_cast<const char*>(w.blob);
  const DevStruct* S = reinterpret_cast<const DevStruct*>(blob);
  const double* xp = x + w.x_off;
  double* gp = g + w.g_off;
  double* jp = jac + w.j_off;
  const bool want_g = flags & 1, want_j = flags & 2;
  if (family == 0) {
    // The first 64 rows sit at a fixed offset behind the header (device_tables.h, node head): their load does not wait for a
    // header field.  One chunk body, called for the head records and -- structures with more than 64 rows -- for the rest.
    auto chunk = [&](const TerrainRow tr, int r0, int nr) {
      const int cnt = min(64, nr - r0);
      double* dst = jp + S->nnz_terrain + 3 * r0;
      const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
      if (lane < cnt) {
        const double px = xp[tr.idx], py = xp[tr.idx + tr.stride], pz = xp[tr.idx + 2 * tr.stride];
        const Terr t = terrain_eval(S, S->terrain_id, S->flat_height, px, py);
        if constexpr (SCORE) sc->put<kFamTerrain>(S->row_terrain + r0 + lane, pz - t.h);
        else if (want_g) gp[S->row_terrain + r0 + lane] = pz - t.h;
        if (want_j) {
          stage[par + 3 * lane + 0] = -t.hx;
          stage[par + 3 * lane + 1] = -t.hy;
          stage[par + 3 * lane + 2] = 1.0;
        }
      }
      if (want_j) copy_out(dst, stage, 3 * cnt, par, lane);  // single wave: LDS accesses are ordered
    };
    const TerrainRow tr0 = tbl<TerrainRow>(blob, kNodeHeadTerrainOff)[lane];
    const int nr = S->n_terrain_rows;
    if (nr > 0) chunk(tr0, 0, nr);
    if (nr > 64) {
      const TerrainRow* rows = tbl<TerrainRow>(blob, S->o_terrain_rows);
      for (int r0 = 64; r0 < nr; r0 += 64) chunk(rows[min(r0 + lane, nr - 1)], r0, nr);
    }
  } else if (family == 1) {
    auto chunk = [&](const ForceNode fn, int i0, int nn) {
      const int cnt = min(64, nn - i0);
      double* dst = jp + S->nnz_force + 25 * i0;
      const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
      if constexpr (SCORE) {
        if (lane < cnt) {
          double g5[5];
          force_item(S, fn, xp, g5, nullptr, true, false);
#pragma unroll
          for (int r = 0; r < 5; ++r) sc->put<kFamForce>(S->row_force + 5 * (i0 + lane) + r, g5[r]);
        }
      } else if (lane < cnt) {
        force_item(S, fn, xp, gp + S->row_force + 5 * (i0 + lane), stage + par + 25 * lane, want_g, want_j);
      }
      if (want_j) copy_out(dst, stage, 25 * cnt, par, lane);
    };
    const ForceNode fn0 = tbl<ForceNode>(blob, kNodeHeadForceOff)[lane];   // (fixed offset, see the terrain family)
    const int nn = S->n_force_nodes;
    if (nn > 0) chunk(fn0, 0, nn);
    if (nn > 64) {
      const ForceNode* nodes = tbl<ForceNode>(blob, S->o_force_nodes);
      for (int i0 = 64; i0 < nn; i0 += 64) chunk(nodes[min(i0 + lane, nn - 1)], i0, nn);
    }
  } else if (family == 2) {
    // splineacc-base-lin | splineacc-base-ang (spline_acc_constraint.cc:49-81): lane = row (set, junction j,
    // dim d); its six variables are {p,v}_d of base nodes j, j+1, j+2 and the six Jacobian values depend on
    // the polynomial durations only (AccJunction), so g = sum c_i x_i.
    const AccJunction* acc = tbl<AccJunction>(blob, S->o_acc);
    const int per_set = 3 * S->n_junctions, nr = 2 * per_set;
    for (int r0 = 0; r0 < nr; r0 += 64) {
      const int cnt = min(64, nr - r0);
      double* dst = jp + S->nnz_acc + 6 * r0;
      const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
      if (lane < cnt) {
        const int r = r0 + lane;
        const int which = r >= per_set, rem = r - which * per_set;
        const int j = rem / 3, d = rem - 3 * j;
        const AccJunction a = acc[j];
        const double* xb = xp + (which ? S->off_base_ang : 0) + 6 * j + d;
        double v = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          v += a.c[i] * xb[3 * i];
          if (want_j) stage[par + 6 * lane + i] = a.c[i];
        }
        if constexpr (SCORE) sc->put<kFamAcc>(S->row_acc + r, v);
        else if (want_g) gp[S->row_acc + r] = v;
      }
      if (want_j) copy_out(dst, stage, 6 * cnt, par, lane);
    }
    // baseMotion (base_motion_constraint.cc:60-90): lane = time node; rows AX..AZ = base-ang position,
    // LX..LZ = base-lin position, every row holds the four position weights of its dimension
    const BaseNode* bm = tbl<BaseNode>(blob, S->o_bm);
    const int nb = S->n_bm_nodes;
    for (int k0 = 0; k0 < nb; k0 += 16) {  // 16 nodes x 24 values fit the family's 384-value image
      const int cnt = min(16, nb - k0);
      double* dst = jp + S->nnz_bm + 24 * k0;
      const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
      if (lane < cnt) {
        const BaseNode n = bm[k0 + lane];
        double wP[4];
        hermite_pos(n.t, n.iT, wP);
        const double* xa = xp + S->off_base_ang + n.q6;
        const double* xl = xp + n.q6;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          if constexpr (SCORE) {
            sc->put<kFamBaseMotion>(S->row_bm + 6 * (k0 + lane) + d, wP[0] * xa[d] + wP[1] * xa[3 + d] + wP[2] * xa[6 + d] + wP[3] * xa[9 + d]);
            sc->put<kFamBaseMotion>(S->row_bm + 6 * (k0 + lane) + 3 + d, wP[0] * xl[d] + wP[1] * xl[3 + d] + wP[2] * xl[6 + d] + wP[3] * xl[9 + d]);
          } else if (want_g) {
            double* g6 = gp + S->row_bm + 6 * (k0 + lane);
            g6[d] = wP[0] * xa[d] + wP[1] * xa[3 + d] + wP[2] * xa[6 + d] + wP[3] * xa[9 + d];
            g6[3 + d] = wP[0] * xl[d] + wP[1] * xl[3 + d] + wP[2] * xl[6 + d] + wP[3] * xl[9 + d];
          }
          if (want_j) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              stage[par + 24 * lane + 4 * d + j] = wP[j];
              stage[par + 24 * lane + 12 + 4 * d + j] = wP[j];
            }
          }
        }
      }
      if (want_j) copy_out(dst, stage, 24 * cnt, par, lane);
    }
  } else {
    // swing-ee-motion_e (swing_constraint.cc:58-121): lane = swing node, rows {x pos, x vel, y pos, y vel},
    // columns {previous node, this node, next node}
    const SwingNode* sw = tbl<SwingNode>(blob, S->o_swing_nodes);
    const int nn = S->n_swing_nodes;
    const double it = S->inv_t_swing;
    for (int i0 = 0; i0 < nn; i0 += 64) {
      const int cnt = min(64, nn - i0);
      double* dst = jp + S->nnz_swing + 12 * i0;
      const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
      if (lane < cnt) {
        const SwingNode sn = sw[i0 + lane];
        const int pi[2] = {sn.prev_x, sn.prev_y}, ni[2] = {sn.next_x, sn.next_y};
#pragma unroll
        for (int dim = 0; dim < 2; ++dim) {
          const double prev = xp[pi[dim]], next = xp[ni[dim]];
          const double pos = xp[sn.cur + 2 * dim], vel = xp[sn.cur + 2 * dim + 1];
          const double distance = next - prev;
          if constexpr (SCORE) {
            sc->put<kFamSwing>(S->row_swing + 4 * (i0 + lane) + 2 * dim, pos - (prev + 0.5 * distance));
            sc->put<kFamSwing>(S->row_swing + 4 * (i0 + lane) + 2 * dim + 1, vel - distance * it);
          } else if (want_g) {
            double* g4 = gp + S->row_swing + 4 * (i0 + lane);
            g4[2 * dim] = pos - (prev + 0.5 * distance);
            g4[2 * dim + 1] = vel - distance * it;
          }
          if (want_j) {
            double* st = stage + par + 12 * lane + 6 * dim;
            st[0] = -0.5; st[1] = 1.0; st[2] = -0.5;
            st[3] = it;   st[4] = 1.0; st[5] = -it;
          }
        }
      }
      if (want_j) copy_out(dst, stage, 12 * cnt, par, lane);
    }
    // totalduration-<e> (total_duration_constraint.cc:50-72): sum of the optimised phase durations
    if (S->timings) {
      const PhaseTables* PT = tbl<PhaseTables>(blob, S->o_phase);
      if (lane < S->n_ee) {
        int voff = 0;
        for (int e = 0; e < lane; ++e) voff += PT->n_phases[e] - 1;
        const int ns = PT->n_phases[lane] - 1;
        double sum = 0.0;
        for (int i = 0; i < ns; ++i) {
          sum += xp[PT->off_sched[lane] + i];
          if (want_j) jp[PT->nnz_total + voff + i] = 1.0;
        }
        if constexpr (SCORE) sc->put<kFamTotal>(PT->row_total + lane, sum);
        else if (want_g) gp[PT->row_total + lane] = sum;
      }
    }
  }
}

__global__ __launch_bounds__(256, 4) void node_kernel(const NodeWork* __restrict__ work, const double* __restrict__ x,
                                                   double* __restrict__ g, double* __restrict__ jac, int flags) {
  __shared__ __attribute__((aligned(16))) double stage_all[kStageTerrain + kStageForce + kStageAcc + kStageSwing];
  const int family = threadIdx.x >> 6;  // wave-uniform
  // (one call site per CONSTANT family: each wave's code holds its own family's body only)
  const NodeWork w = work[blockIdx.x];
  const int lane = threadIdx.x & 63;
  if (family == 0) node_body(w, x, g, jac, flags, stage_all + kNodeStageOff[0], 0, lane);
  else if (family == 1) node_body(w, x, g, jac, flags, stage_all + kNodeStageOff[1], 1, lane);
  else if (family == 2) node_body(w, x, g, jac, flags, stage_all + kNodeStageOff[2], 2, lane);
  else node_body(w, x, g, jac, flags, stage_all + kNodeStageOff[3], 3, lane);
}

// Batches whose problems carry terrain-* and force-* sets only (the hot-path sets): workgroups of those two families.
// The kernel is one chain of dependent loads per wave (work item -> header -> rows -> x) and lives on occupancy; with
// four-wave workgroups two waves of each would find no work, i.e. 8 busy waves per CU instead of 16
// (A/B on one box, 8192 C3 problems: 0.054 -> see DESIGN 6.0).
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(4))) void node_kernel2(const NodeWork* __restrict__ work, const double* __restrict__ x,
                                                    double* __restrict__ g, double* __restrict__ jac, int flags) {
  __shared__ __attribute__((aligned(16))) double stage_all[kStageTerrain + kStageForce];
  const int family = threadIdx.x >> 6;  // wave-uniform
  // (two call sites with a CONSTANT family: the bodies of the other families are not compiled into this kernel, and the
  // register allocation is that of terrain / force alone)
  if (family == 0) node_body(work[blockIdx.x], x, g, jac, flags, stage_all + kNodeStageOff[0], 0, threadIdx.x & 63);
  else node_body(work[blockIdx.x], x, g, jac, flags, stage_all + kNodeStageOff[1], 1, threadIdx.x & 63);
}
}  // namespace twr
