#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "dyn.h"
#include "node.h"
#include "spline_math.h"

namespace twr {
// ---------------------------------------------------------------- values only: one lane per time node
// TWR_EVAL_VALUES -- Ipopt's eval_g (every line-search trial point), a planner's scoring step -- for problems with fixed
// timings.  The values-only instantiations of the Jacobian bodies were bound by vector-instruction issue, not by memory
// (72 % / 55 % of the issue slots at 0.12 of the HBM roof).  The Jacobian kernels' cuts -- "rangeofmotion-e":
// one slice per end-effector, lane = time node; "dynamic": a quad of lanes per time node -- evaluate the base splines and the
// rotation (three sin / cos pairs) of a time node once per END-EFFECTOR resp. per LANE OF THE QUAD; without an image to
// assemble one lane can take a time node for ALL end-effectors (device_tables.h FlatNode / FlatPoly / FlatWork).
// What made the first form of this slower for "dynamic" (0.205 vs 0.142 ms per 8192 C3 problems) was the ~120 per-lane global
// gathers of x behind eight 40-byte polynomial records; here the wave copies the problem's x and the item's windows of
// polynomial records into LDS (coalesced, one round trip behind the work item) and a candidate is ONE LDS read at a byte
// offset the host prepared (zero pair for candidates that are not variables, p0's variable for p1 of a stance polynomial):
// no selects, no global gathers.
// LDS of a wave (dynamic size, the launcher knows the largest problem of the batch): [ polynomial windows: 2 kMaxEE x
// kFlatWindow records | zero pair | x ]
typedef uint32_t twr_u4 __attribute__((ext_vector_type(4)));
typedef uint32_t twr_u2 __attribute__((ext_vector_type(2)));
struct FlatIn {            // what a lane fetches for an item: its time node and one polynomial record of the windows, as whole
  twr_u4 na, nb;           // dwords (no sub-dword struct fields across the loop back-edge): FlatNode = na | nb | nc
  twr_u2 nc;
  twr_u4 pa, pb, pc;       // FlatPoly
};
struct FlatNodeR {         // FlatNode unpacked (registers)
  double t, tb, iTb;
  int q6;
  uint32_t qm, qf;         // four bytes each
};
TWR_DEV FlatNodeR flat_node(const FlatIn& in) {
  static_assert(offsetof(FlatNode, q6) == 24 && offsetof(FlatNode, qm) == 28 && offsetof(FlatNode, qf) == 32, "FlatNode dwords");
  FlatNodeR n;
  n.t = __hiloint2double((int)in.na.y, (int)in.na.x);
  n.tb = __hiloint2double((int)in.na.w, (int)in.na.z);
  n.iTb = __hiloint2double((int)in.nb.y, (int)in.nb.x);
  n.q6 = (int)in.nb.z;
  n.qm = in.nb.w;
  n.qf = in.nc.x;
  return n;
}
// The work record of an item: wave-uniform, read with scalar loads (one round trip: everything an item needs that is the
// same for all its lanes is IN the record, nothing behind a pointer of it); a field is addressed by its dword.
struct FlatRec {
  const TWR_CONST uint32_t* p;
  TWR_DEV uint32_t u32(int k) const { return p[k]; }
  TWR_DEV int i32(int k) const { return (int)p[k]; }
  TWR_DEV uint64_t u64(int k) const { return ((uint64_t)p[k + 1] << 32) | p[k]; }
  TWR_DEV double f64(int k) const { return __hiloint2double((int)p[k + 1], (int)p[k]); }
};
TWR_DEV void flat_load(const FlatRec& w, int lane, FlatIn& in) {
  {
    const TWR_GLOBAL twr_u2* nd = reinterpret_cast<const TWR_GLOBAL twr_u2*>(gptr<FlatNode>(w.u64(kFwNodes)) + min(lane, w.i32(kFwCnt) - 1));   // (clamped:
    const twr_u2 a = nd[0], b = nd[1], c = nd[2], d = nd[3];   // every lane loads, the tail lanes store nothing; 8-byte aligned records)
    in.na = twr_u4{a.x, a.y, b.x, b.y};
    in.nb = twr_u4{c.x, c.y, d.x, d.y};
    in.nc = nd[4];
  }
}
TWR_DEV void flat_load_polys(const FlatRec& w, int lane, FlatIn& in) {
  // lane 8 s + j: record j of spline s's window (clamped to the window: no predicates)
  const int s = lane >> 3, j = lane & 7;
  const uint64_t st = lane < 32 ? w.u64(kFwStart) : w.u64(kFwStart + 2);
  const int first = (int)((st >> (16 * (s & 3))) & 0xFFFFu), cnt = (int)((w.u64(kFwCount) >> (8 * s)) & 0xFFu);
  const TWR_GLOBAL twr_u4* rec = reinterpret_cast<const TWR_GLOBAL twr_u4*>(gptr<FlatPoly>(w.u64(kFwPolys)) + first + min(j, max(cnt, 1) - 1));
  in.pa = rec[0];
  in.pb = rec[1];
  in.pc = rec[2];
}
TWR_DEV void flat_stage_polys(const FlatIn& in, char* lds, int lane) {
  twr_u4* dst = reinterpret_cast<twr_u4*>(lds + lane * (int)sizeof(FlatPoly));
  dst[0] = in.pa;
  dst[1] = in.pb;
  dst[2] = in.pc;
}
// x of a problem by the 256 threads of a group, NX doubles per thread (the launcher picks the smallest instantiation that
// covers the largest problem)
template <int NX>
TWR_DEV void flat_load_x(const double* __restrict__ xp, int n_x, int tid, double xr[NX]) {
#pragma unroll
  for (int j = 0; j < NX; ++j) xr[j] = xp[min(64 * kFlatGroup * j + tid, n_x - 1)];
}
template <int NX>
TWR_DEV void flat_stage_x(const double xr[NX], int n_x, double* xs, int tid) {
  if (tid < 2) xs[tid] = 0.0;
#pragma unroll
  for (int j = 0; j < NX; ++j) xs[2 + min(64 * kFlatGroup * j + tid, n_x - 1)] = xr[j];   // (clamped like the loads: the threads past
}                                                                                        // the end write the last variable once more)
// A polynomial's record in registers: from the wave's window in LDS, or -- items of a coarse grid, whose time nodes hardly
// share polynomials (FlatWork::gather) -- fetched by the lane itself from the structure's table.
struct FlatPolyR {
  double t0, iT;
  uint32_t o[6];
};
template <bool GATHER>
TWR_DEV FlatPolyR flat_poly(const FlatRec& w, const char* __restrict__ lds, int spline, int local) {
  FlatPolyR r;
  if (GATHER) {
    const int first = (int)((w.u64(kFwStart + 2 * (spline >> 2)) >> (16 * (spline & 3))) & 0xFFFFu);   // (uniform)
    const TWR_GLOBAL twr_u4* rec = reinterpret_cast<const TWR_GLOBAL twr_u4*>(gptr<FlatPoly>(w.u64(kFwPolys)) + first + local);
    const twr_u4 a = rec[0], b = rec[1];
    const twr_u2 c = reinterpret_cast<const TWR_GLOBAL twr_u2*>(rec)[4];
    r.t0 = __hiloint2double((int)a.y, (int)a.x);
    r.iT = __hiloint2double((int)a.w, (int)a.z);
    r.o[0] = b.x; r.o[1] = b.y; r.o[2] = b.z; r.o[3] = b.w; r.o[4] = c.x; r.o[5] = c.y;
  } else {
    const char* rec = lds + (spline * kFlatWindow + local) * (int)sizeof(FlatPoly);
    const double2 ti = *reinterpret_cast<const double2*>(rec);
    const uint4 oa = reinterpret_cast<const uint4*>(rec)[1];
    const uint2 ob = reinterpret_cast<const uint2*>(rec)[4];
    r.t0 = ti.x; r.iT = ti.y;
    r.o[0] = oa.x; r.o[1] = oa.y; r.o[2] = oa.z; r.o[3] = oa.w; r.o[4] = ob.x; r.o[5] = ob.y;
  }
  return r;
}
// Spline::GetPoint (spline.cc:80-93) of an ee spline in Hermite basis form, position only
TWR_DEV void flat_point(const char* __restrict__ xs, const FlatPolyR& r, double t, double p[3]) {
  double w[4], X[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) X[c] = lds_f64(xs, (c & 1) ? r.o[c >> 1] >> 16 : r.o[c >> 1] & 0xFFFFu);
  hermite_pos(t - r.t0, r.iT, w);
#pragma unroll
  for (int d = 0; d < 3; ++d) p[d] = w[0] * X[d] + w[1] * X[3 + d] + w[2] * X[6 + d] + w[3] * X[9 + d];
}
// Same formula as rom_item (RangeOfMotionConstraint::UpdateConstraintAtInstance, range_of_motion_constraint.cc:58-69).
// `lds`: the wave's polynomial windows; `xs`: the group's copy of x (zero pair first); `gs`: 192 doubles of the wave's own
template <bool GATHER, bool SCORE = false>
TWR_DEV void flat_rom_math(const FlatRec& w, const FlatNodeR& n, double* __restrict__ g, const char* lds, const char* xs, double* gs, int lane,
                           ScoreAcc* sc = nullptr) {
  const double* xv = reinterpret_cast<const double*>(xs) + 2;
  double* gp = g + (int64_t)w.u64(kFwG);
  const int n_ee = w.i32(kFwNee);
  // base splines: the twelve node values of the active polynomial are contiguous in x (nodes q, q + 1: p then v)
  double wP[4], c[3], e[3];
  hermite_pos(n.tb, n.iTb, wP);
  {
    const double* xl = xv + w.i32(kFwOffLin) + n.q6;
    const double* xa = xv + w.i32(kFwOffAng) + n.q6;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[d] = wP[0] * xl[d] + wP[1] * xl[3 + d] + wP[2] * xl[6 + d] + wP[3] * xl[9 + d];
      e[d] = wP[0] * xa[d] + wP[1] * xa[3 + d] + wP[2] * xa[6 + d] + wP[3] * xa[9 + d];
    }
  }
  Rot ro;
  rotation(e, ro);
#pragma unroll
  for (int ee = 0; ee < kMaxEE; ++ee)
    if (ee < n_ee) {   // g = b_R_w (p_ee - c)
      double p[3], v[3], gv[3];
      flat_point(xs, flat_poly<GATHER>(w, lds, 2 * ee, (n.qm >> (8 * ee)) & 0xFFu), n.t, p);
#pragma unroll
      for (int d = 0; d < 3; ++d) v[d] = p[d] - c[d];
      matTvec(ro.R, v, gv);
      // the 3 cnt values of this end-effector's rows are contiguous in g: through LDS, then whole lines (a lane storing its own
      // three values writes 16 + 8 of every 24 bytes per instruction)
      gs[3 * lane] = gv[0];
      gs[3 * lane + 1] = gv[1];
      gs[3 * lane + 2] = gv[2];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      if constexpr (SCORE) {
        sc->rows<kFamRom, 3>(gs, w.i32(kFwRowRom + ee) + 3 * w.i32(kFwK0), 3 * w.i32(kFwCnt), lane);
      } else {
        double* go = gp + w.i32(kFwRowRom + ee) + 3 * w.i32(kFwK0);
        const int last_g = 3 * w.i32(kFwCnt) - 1;
#pragma unroll
        for (int t = 0; t < 3; ++t) go[min(lane + 64 * t, last_g)] = gs[min(lane + 64 * t, last_g)];
      }
    }
}
// DynamicConstraint::UpdateConstraintAtInstance (dynamic_constraint.cc:59-77) with SingleRigidBodyDynamics::GetDynamicViolation
// (single_rigid_body_dynamics.cc:76-101) and the EulerConverter quantities (euler_converter.cc:58-83,133-166,207-221) of one time
// node on ONE lane -- the statements of dyn2_front / dyn2_back without the quad.
template <bool GATHER, bool SCORE = false>
TWR_DEV void flat_dyn_math(const FlatRec& w, const FlatNodeR& n, double* __restrict__ g, const char* lds, const char* xs, double* gs_rom, int lane,
                           ScoreAcc* sc = nullptr) {
  const double* xv = reinterpret_cast<const double*>(xs) + 2;
  const int n_ee = w.i32(kFwNee);
  const double* bl = xv + w.i32(kFwOffLin) + n.q6;   // base splines: the twelve node values of the active polynomial
  const double* ba = xv + w.i32(kFwOffAng) + n.q6;
  // base position and rotation first: with coinciding grids (FlatWork::with_rom) the lane evaluates "rangeofmotion-e" of its
  // time node along the way -- g = b_R_w (p_e - c), range_of_motion_constraint.cc:58-69 -- from the same base point, rotation and
  // end-effector positions
  const bool with_rom = w.i32(kFwWithRom) != 0;
  double* gp = g + (int64_t)w.u64(kFwG);
  const int last_rom = 3 * w.i32(kFwCnt) - 1;
  Rot ro;
  // force and torque sums over the end-effectors (single_rigid_body_dynamics.cc:81-88)
  double F[3] = {0.0, 0.0, 0.0}, tau[3] = {0.0, 0.0, 0.0};
  {
    double wP[4], c[3], e[3];
    hermite_pos(n.tb, n.iTb, wP);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[d] = wP[0] * bl[d] + wP[1] * bl[3 + d] + wP[2] * bl[6 + d] + wP[3] * bl[9 + d];
      e[d] = wP[0] * ba[d] + wP[1] * ba[3 + d] + wP[2] * ba[6 + d] + wP[3] * ba[9 + d];
    }
    rotation(e, ro);
#pragma unroll
    for (int ee = 0; ee < kMaxEE; ++ee)
      if (ee < n_ee) {
        double p[3], f[3], rv[3], t3[3];
        flat_point(xs, flat_poly<GATHER>(w, lds, 2 * ee, (n.qm >> (8 * ee)) & 0xFFu), n.t, p);
        flat_point(xs, flat_poly<GATHER>(w, lds, 2 * ee + 1, (n.qf >> (8 * ee)) & 0xFFu), n.t, f);
#pragma unroll
        for (int d = 0; d < 3; ++d) rv[d] = c[d] - p[d];
        cross3(f, rv, t3);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          F[d] += f[d];
          tau[d] += t3[d];
        }
        if (with_rom) {
          double v[3], gv[3];
#pragma unroll
          for (int d = 0; d < 3; ++d) v[d] = p[d] - c[d];
          matTvec(ro.R, v, gv);
          gs_rom[3 * lane] = gv[0];
          gs_rom[3 * lane + 1] = gv[1];
          gs_rom[3 * lane + 2] = gv[2];
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          if constexpr (SCORE) {
            sc->rows<kFamRom, 3>(gs_rom, w.i32(kFwRowRom + ee) + 3 * w.i32(kFwK0), last_rom + 1, lane);
          } else {
            double* go = gp + w.i32(kFwRowRom + ee) + 3 * w.i32(kFwK0);
#pragma unroll
            for (int t = 0; t < 3; ++t) go[min(lane + 64 * t, last_rom)] = gs_rom[min(lane + 64 * t, last_rom)];
          }
        }
      }
  }
  double cdd[3], ed[3], edd[3];
  {
    double wP[4], wV[4], wA[4];
    hermite_all(n.tb, n.iTb, wP, wV, wA);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      cdd[d] = wA[0] * bl[d] + wA[1] * bl[3 + d] + wA[2] * bl[6 + d] + wA[3] * bl[9 + d];
      ed[d] = wV[0] * ba[d] + wV[1] * ba[3 + d] + wV[2] * ba[6 + d] + wV[3] * ba[9 + d];
      edd[d] = wA[0] * ba[d] + wA[1] * ba[3 + d] + wA[2] * ba[6 + d] + wA[3] * ba[9 + d];
    }
  }
  const double sy = ro.sy, cy = ro.cy, sz = ro.sz, cz = ro.cz;
  const double xd = ed[0], yd = ed[1], zd = ed[2];
  const double Mx[3] = {cy * cz, cy * sz, -sy}, My[3] = {-sz, cz, 0.0};
  const double Mdx[3] = {-cz * sy * yd - cy * sz * zd, cy * cz * zd - sy * sz * yd, -cy * yd};
  const double Mdy[3] = {-cz * zd, -sz * zd, 0.0};
  double om[3], omd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    om[i] = Mx[i] * xd + My[i] * yd;
    omd[i] = Mdx[i] * xd + Mdy[i] * yd + Mx[i] * edd[0] + My[i] * edd[1];
  }
  om[2] += zd;
  omd[2] += edd[2];
  double Iw6[6];  // I_w = R I_b R^T (single_rigid_body_dynamics.cc:91), symmetric: (00,01,02,11,12,22)
  {
    const double (&R)[3][3] = ro.R;
    double Ib[6], Tm[3][3];
#pragma unroll
    for (int i = 0; i < 6; ++i) Ib[i] = w.f64(kFwIb + 2 * i);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Tm[i][0] = R[i][0] * Ib[0] + R[i][1] * Ib[1] + R[i][2] * Ib[2];
      Tm[i][1] = R[i][0] * Ib[1] + R[i][1] * Ib[3] + R[i][2] * Ib[4];
      Tm[i][2] = R[i][0] * Ib[2] + R[i][1] * Ib[4] + R[i][2] * Ib[5];
    }
    Iw6[0] = Tm[0][0] * R[0][0] + Tm[0][1] * R[0][1] + Tm[0][2] * R[0][2];
    Iw6[1] = Tm[0][0] * R[1][0] + Tm[0][1] * R[1][1] + Tm[0][2] * R[1][2];
    Iw6[2] = Tm[0][0] * R[2][0] + Tm[0][1] * R[2][1] + Tm[0][2] * R[2][2];
    Iw6[3] = Tm[1][0] * R[1][0] + Tm[1][1] * R[1][1] + Tm[1][2] * R[1][2];
    Iw6[4] = Tm[1][0] * R[2][0] + Tm[1][1] * R[2][1] + Tm[1][2] * R[2][2];
    Iw6[5] = Tm[2][0] * R[2][0] + Tm[2][1] * R[2][1] + Tm[2][2] * R[2][2];
  }
  double Iw_wd[3], Iw_w[3], wxIw[3];
  symmul(Iw6, omd, Iw_wd);
  symmul(Iw6, om, Iw_w);
  cross3(om, Iw_w, wxIw);
  const double m = w.f64(kFwMass);
  // the 6 cnt values of the item are contiguous in g: through LDS (the polynomial windows are no longer needed), then whole lines
  double* gs = reinterpret_cast<double*>(const_cast<char*>(lds)) + 6 * lane;
  static_assert(kFlatPolyLds >= 64 * 6 * 8, "constraint values of a dynamic item in the window region");
#pragma unroll
  for (int i = 0; i < 3; ++i) gs[i] = Iw_wd[i] + wxIw[i] - tau[i];
  gs[3] = m * cdd[0] - F[0];
  gs[4] = m * cdd[1] - F[1];
  gs[5] = m * cdd[2] - F[2] + m * w.f64(kFwGravity);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if constexpr (SCORE) {
    sc->rows<kFamDyn, 6>(reinterpret_cast<const double*>(lds), w.i32(kFwRowDyn) + 6 * w.i32(kFwK0), 6 * w.i32(kFwCnt), lane);
  } else {
    const double* gl = reinterpret_cast<const double*>(lds);
    double* go = gp + w.i32(kFwRowDyn) + 6 * w.i32(kFwK0);
    const int last_g = 6 * w.i32(kFwCnt) - 1;
#pragma unroll
    for (int t = 0; t < 6; ++t) go[min(lane + 64 * t, last_g)] = gl[min(lane + 64 * t, last_g)];
  }
}
// One launch per values-only evaluation.  Workgroups of four waves: the first n_groups take a GROUP each -- four consecutive work
// records, items of ONE problem (twr_batch_create pads a problem's list to whole groups with empty items, cnt = 0) --, so that
// the problem's x is fetched and copied to LDS once per group by all 256 threads and every wave evaluates its own item on it
// (K = 200 with coinciding grids: one group per problem); the remaining workgroups take the node families of one problem each,
// one family per wave.  Per item: fetch (the lane's time node, the thread's share of x, one polynomial record of the windows
// -- one round trip behind the work record), copy to LDS, evaluate.
// LDS (dynamic, the launcher knows the largest problem of the batch): [ zero pair | x ] [ per wave: polynomial windows | 192
// constraint values ].
// (A persistent form of this -- waves looping over strided items, the fetches of item i + 1 in flight during the math of item
// i, the work record read by one vector load and v_readlane so that no scalar load sat in the loop -- was built, is parity-
// green and is NOT faster: 0.084-0.092 / 0.067-0.072 ms against 0.068-0.073 / 0.066 ms per 8192 C3 problems as single-wave
// workgroups, at three waves per SIMD instead of four because of the prefetch registers)
static_assert(kFlatWaveLds >= kDynValuesLds * 8, "node_body stages its constraint values in a wave's region");
template <int NX>
__global__ __launch_bounds__(64 * kFlatGroup, 4) void eval_values_kernel(const FlatWork* __restrict__ flat, int n_groups, int x_bytes, const NodeWork* __restrict__ node,
                                                                         int node_families, const double* __restrict__ x, double* __restrict__ g) {
  extern __shared__ __attribute__((aligned(16))) double flat_stage[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* xs = reinterpret_cast<char*>(flat_stage);
  char* mine = xs + x_bytes + wave * kFlatWaveLds;
  int b = blockIdx.x;
  if (b >= n_groups) {
    if (wave < node_families)   // (values only: the node image is not touched)
      node_body(node[b - n_groups], x, g, nullptr, 1, reinterpret_cast<double*>(mine), wave, lane);
    return;
  }
  FlatRec w;
  w.p = cptr<uint32_t>(reinterpret_cast<uint64_t>(flat + (kFlatGroup * b + wave)));
  const int cnt = w.i32(kFwCnt);
  FlatIn in;
  double xr[NX];
  const bool gather = w.i32(kFwGather) != 0;   // (uniform) a coarse grid: every lane fetches its own polynomial records
  if (cnt > 0) flat_load(w, lane, in);
  if (cnt > 0 && !gather) flat_load_polys(w, lane, in);
  flat_load_x<NX>(x + (int64_t)w.u64(kFwX), w.i32(kFwNx), tid, xr);   // (the empty items of a group carry the problem's x as well)
  flat_stage_x<NX>(xr, w.i32(kFwNx), reinterpret_cast<double*>(xs), tid);
  if (cnt > 0 && !gather) flat_stage_polys(in, mine, lane);
  __syncthreads();
  if (cnt <= 0) return;
  double* gs = reinterpret_cast<double*>(mine + kFlatPolyLds);
  const bool dynamic = w.i32(kFwDynamic) != 0;
  if (gather) {
    if (dynamic) flat_dyn_math<true>(w, flat_node(in), g, mine, xs, gs, lane);
    else flat_rom_math<true>(w, flat_node(in), g, mine, xs, gs, lane);
  } else {
    if (dynamic) flat_dyn_math<false>(w, flat_node(in), g, mine, xs, gs, lane);
    else flat_rom_math<false>(w, flat_node(in), g, mine, xs, gs, lane);
  }
}

// twr_batch_eval_scores: the same launch in its scoring instantiation.  Every value is reduced where eval_values_kernel stores
// it (ScoreAcc: same device functions, same arithmetic, the values go to the wave's running violations instead of g), and
// every wave with work writes ONE partial record, wave w of workgroup b at slab + kScorePartial (4 b + w).  The node-based
// sets are always taken by the launch's own node waves (one workgroup per problem, node_families waves), at every batch size:
// node_chunk_kernel writes g.  score_fold_kernel then folds each problem's records in the order batch_plan.cc planned.
// group_blob[b]: the blob of group b's problem (FlatWork carries no blob; the score record sits at its kScoreOff).
template <int NX>
__global__ __launch_bounds__(64 * kFlatGroup, 4) void eval_scores_kernel(const FlatWork* __restrict__ flat, const uint64_t* __restrict__ group_blob,
                                                                         int n_groups, int x_bytes, const NodeWork* __restrict__ node,
                                                                         int node_families, const double* __restrict__ x, double* __restrict__ slab) {
  extern __shared__ __attribute__((aligned(16))) double flat_stage[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* xs = reinterpret_cast<char*>(flat_stage);
  char* mine = xs + x_bytes + wave * kFlatWaveLds;
  int b = blockIdx.x;
  double* rec = slab + kScorePartial * ((int64_t)kFlatGroup * b + wave);
  if (b >= n_groups) {
    if (wave < node_families) {   // (one call site per CONSTANT family, as node_kernel: the record names its families)
      const NodeWork w = node[b - n_groups];
      ScoreAcc sc(w.blob);
      double* st = reinterpret_cast<double*>(mine);
      if (wave == 0) {
        node_body<true>(w, x, nullptr, nullptr, 1, st, 0, lane, &sc);
        sc.flush<kFamTerrain, kFamTerrain>(rec, lane);
      } else if (wave == 1) {
        node_body<true>(w, x, nullptr, nullptr, 1, st, 1, lane, &sc);
        sc.flush<kFamForce, kFamForce>(rec, lane);
      } else if (wave == 2) {
        node_body<true>(w, x, nullptr, nullptr, 1, st, 2, lane, &sc);
        sc.flush<kFamAcc, kFamBaseMotion>(rec, lane);
      } else {
        node_body<true>(w, x, nullptr, nullptr, 1, st, 3, lane, &sc);
        sc.flush<kFamSwing, kFamTotal>(rec, lane);
      }
    }
    return;
  }
  FlatRec w;
  w.p = cptr<uint32_t>(reinterpret_cast<uint64_t>(flat + (kFlatGroup * b + wave)));
  const int cnt = w.i32(kFwCnt);
  ScoreAcc sc(group_blob[b]);
  FlatIn in;
  double xr[NX];
  const bool gather = w.i32(kFwGather) != 0;
  if (cnt > 0) flat_load(w, lane, in);
  if (cnt > 0 && !gather) flat_load_polys(w, lane, in);
  flat_load_x<NX>(x + (int64_t)w.u64(kFwX), w.i32(kFwNx), tid, xr);
  flat_stage_x<NX>(xr, w.i32(kFwNx), reinterpret_cast<double*>(xs), tid);
  if (cnt > 0 && !gather) flat_stage_polys(in, mine, lane);
  __syncthreads();
  if (cnt <= 0) return;   // (an empty item has no partial record: batch_plan.cc leaves it out of the fold)
  double* gs = reinterpret_cast<double*>(mine + kFlatPolyLds);
  if (w.i32(kFwDynamic) != 0) {
    if (gather) flat_dyn_math<true, true>(w, flat_node(in), nullptr, mine, xs, gs, lane, &sc);
    else flat_dyn_math<false, true>(w, flat_node(in), nullptr, mine, xs, gs, lane, &sc);
    sc.flush<kFamDyn, kFamRom>(rec, lane);
  } else {
    if (gather) flat_rom_math<true, true>(w, flat_node(in), nullptr, mine, xs, gs, lane, &sc);
    else flat_rom_math<false, true>(w, flat_node(in), nullptr, mine, xs, gs, lane, &sc);
    sc.flush<kFamRom, kFamRom>(rec, lane);
  }
}
// The fold: kFoldThreads threads per problem, thread j of problem p folds column j of its partial records
// slot[first[p] .. first[p + 1]) in that order (max for even columns, sum for odd ones) into scores[16 p + j].  A family
// the structure does not build has no rows, so no record names it: it scores 0, as in score_kernel (ScoreTables::
// slot_of_family < 0).  A problem without records (no rows) scores zeros.
__global__ __launch_bounds__(256) void score_fold_kernel(const int32_t* __restrict__ first, const int32_t* __restrict__ slot,
                                                         const double* __restrict__ slab, int n_problems, double* __restrict__ scores) {
  const int t = blockIdx.x * 256 + threadIdx.x, p = t / kFoldThreads, j = t % kFoldThreads;
  if (p >= n_problems) return;
  const int k0 = first[p], k1 = first[p + 1];
  double acc = 0.0;
  for (int k = k0; k < k1; ++k) {
    const double o = slab[kScorePartial * (int64_t)slot[k] + j];
    acc = (j & 1) ? acc + o : nan_max(acc, o);
  }
  scores[kScorePartial * (int64_t)p + j] = acc;
}
}  // namespace twr
