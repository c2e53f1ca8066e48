#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "copy_out.h"
#include "spline_math.h"

namespace twr {
// ---------------------------------------------------------------- dynamic (SRBD) quad
// DynamicConstraint::{UpdateModel, UpdateConstraintAtInstance, UpdateJacobianAtInstance}
// (dynamic_constraint.cc:59-137) with SingleRigidBodyDynamics::{GetDynamicViolation,
// GetJacobianWrt{BaseLin,BaseAng,Force,EEPos}} (single_rigid_body_dynamics.cc:76-192) and the
// EulerConverter derivatives (euler_converter.cc:85-131,168-198,223-304) for one time node,
// computed by the four lanes of a quad:
//   role = lane & 3 evaluates end-effector `role` (splines, [f]x J_p and {[r]x J_f ; -J_f} blocks),
//   role 0..2 additionally produce Euler dimension `role` of the base-ang block, role 3 the
//   base-lin block and the six constraint values.
// The base-ang block is evaluated in factored form: with u = (p0,v0,p1,v1) of Euler dim d,
//   d g_ang / d u_j = A_d wP[j] + B_d wV[j] + C_d wA[j],
//   A_d = d g_ang/d e_d, B_d = d g_ang/d edot_d, C_d = d g_ang/d eddot_d  (3-vectors).
// Two kernels share this mapping: dyn_kernel (fixed timings: dyn2_front / dyn2_back, every index resolved on the
// host) and dyn_phase_kernel (optimised timings: pdyn_math / pdyn_puts behind the phase_locate_kernel pre-pass).
// dynamic kernel loop.  On gfx9 a wave's loads and stores retire through ONE in-order counter, so x
// loads issued right after a slice's stores are only seen once those stores have drained (measured: a
// quarter of this kernel).  The slice is therefore copied out one phase late:
//   front(i+1): x loads of slice i+1 (behind the stores of slice i-1, long gone) -> compact state
//   copy-out(i): image of slice i -> HBM
//   back(i+1):  Jacobian blocks of slice i+1 -> image        (single call site of each half)
// ---------------------------------------------------------------- dynamic, fixed timings (dyn_kernel)
// DynamicConstraint + SingleRigidBodyDynamics + EulerConverter for one time node on a quad of lanes (as above); every
// index is an LDS byte offset prepared on the host (device_tables.h DynNodeL / DynSel / DynPolyL / DynTile): the slice's part of x
// sits in LDS ("xs"), values that are not optimisation variables read its zero slot, and a Jacobian value is stored at
// node base + a 16-bit offset from the record.
constexpr int kDynX0 = kDynG0 + 96;        // xs: zero pair, then <= kDynXsCap staged doubles of x
// (the image: 16 time nodes per wave, ~170 values each at 4 ee)
constexpr int kDynLds = kDynX0 + 2 + kDynXsCap;   // 2560 doubles = 20480 B: eight workgroups per CU (the VGPR limit too)
static_assert(kDynLds * 8 <= 20480, "dyn_kernel: eight workgroups of 20 KB per CU");
#ifndef TWR_DYN_COPY_BATCH
#define TWR_DYN_COPY_BATCH 8
#endif
#ifndef TWR_DYN_WAVES
#define TWR_DYN_WAVES 2   // waves per SIMD dyn_kernel is compiled for (experiments: 3 with -DTWR_DYN_IMAGE=1362 -DTWR_DYN_XS=126)
#endif

constexpr int kDynCopyBatch = TWR_DYN_COPY_BATCH;   // LDS reads in flight before the first store of the copy-out
struct Dyn2Front {   // (the base-spline weights are recomputed in the back half: 48 registers less across the copy-out)
  double cdd[3], ed[3], edd[3];
  double wm[4], wf[4], f[3], rv[3], F[3], tau[3];
  double sx, cx, sy, cy, sz, cz;
};

// staged candidate c of a spline: xs[idx[c]], idx = twelve bytes in three dwords
TWR_DEV void gather12s(const char* __restrict__ xs, const uint32_t w[3], double v[12]) {
#pragma unroll
  for (int c = 0; c < 12; ++c) v[c] = lds_f64(xs, ((w[c >> 2] >> (8 * (c & 3))) & 0xFFu) << 3);
}
// What a lane needs of its records for the FRONT half of a slice (prefetched during the previous slice's back half) and
// for the tile stores of the BACK half (the codes, loaded while the previous slice is copied out).  Whole dwords: no
// sub-dword struct fields cross the loop back-edge (see the compiler note in DESIGN 6.0).
struct DynFrontRec {
  DynNode nd;
  double t0m, iTm, t0f, iTf;
  uint32_t relm[3], presm[3], relf[3], presf[3];
  uint32_t flagsm, flagsf;
  uint32_t tl[5];      // DynTile as five dwords: base_m[0..1] | base_m[2], base_f[0] | base_f[1..2] | base_f[3..4] | base_f[5], s_m, s_f
};
struct DynCodes {
  uint32_t m[6];       // DynPolyL::code of the ee-motion polynomial: [c][2]
  uint32_t f[9];       // of the ee-force polynomial: [c][3]
};
TWR_DEV uint32_t dyn2_load_sel(const DynWork& w, int lane) {
  const int kk = min(lane >> 2, w.cnt - 1);
  return gptr<uint32_t>(w.sel)[kk * 4 + (lane & 3)];
}
// The records of roles >= n_ee (DynSel::dm / df = 255): every value reads the zero slot, finite weights, codes 0.  Constants of
// the code object, the same for every structure.
__device__ const DynPolyT g_dyn_dummy_t = {0.0, 1.0};
__device__ const DynPolyL g_dyn_dummy_l = {{0}, {0}, 2u | 4u, {0}};
TWR_DEV const TWR_GLOBAL char* dyn2_poly_t_addr(const DynWork& w, uint32_t d) {   // d = DynSel::dm or df
  const uint64_t rec = w.poly_t + (uint64_t)d * sizeof(DynPolyT);
  return reinterpret_cast<const TWR_GLOBAL char*>(d == (uint32_t)kDynPolyDummy ? reinterpret_cast<uint64_t>(&g_dyn_dummy_t) : rec);
}
TWR_DEV const TWR_GLOBAL char* dyn2_poly_l_addr(const DynWork& w, uint32_t d) {
  const uint64_t rec = w.poly_l + (uint64_t)d * sizeof(DynPolyL);
  return reinterpret_cast<const TWR_GLOBAL char*>(d == (uint32_t)kDynPolyDummy ? reinterpret_cast<uint64_t>(&g_dyn_dummy_l) : rec);
}
TWR_DEV void dyn2_load_front(const DynWork& w, uint32_t sel, int lane, DynFrontRec& r) {
  const int kk = min(lane >> 2, w.cnt - 1);
  const DynNodeT nt = gptr<DynNodeT>(w.nodes_t)[kk];
  const uint4 nl = gptr<uint4>(w.nodes_l)[kk];
  static_assert(sizeof(DynNodeL) == sizeof(uint4), "DynNodeL as four dwords");
  r.nd.t = nt.t; r.nd.tb = nt.tb; r.nd.iTb = nt.iTb;
  r.nd.sb_lin = (uint16_t)nl.x; r.nd.sb_ang = (uint16_t)(nl.x >> 16);
  r.nd.nb = (uint16_t)nl.y;     r.nd.rs1 = (uint16_t)(nl.y >> 16);
  r.nd.rs2 = (uint16_t)nl.z;    r.nd.rl[0] = (uint16_t)(nl.z >> 16);
  r.nd.rl[1] = (uint16_t)nl.w;  r.nd.rl[2] = (uint16_t)(nl.w >> 16);
  const uint32_t im = (sel >> 16) & 0xFFu, jf = sel >> 24;
  const TWR_GLOBAL double* dm = reinterpret_cast<const TWR_GLOBAL double*>(dyn2_poly_t_addr(w, im));
  const TWR_GLOBAL double* df = reinterpret_cast<const TWR_GLOBAL double*>(dyn2_poly_t_addr(w, jf));
  const TWR_GLOBAL uint32_t* um = reinterpret_cast<const TWR_GLOBAL uint32_t*>(dyn2_poly_l_addr(w, im));
  const TWR_GLOBAL uint32_t* uf = reinterpret_cast<const TWR_GLOBAL uint32_t*>(dyn2_poly_l_addr(w, jf));
  const TWR_GLOBAL uint32_t* tl = reinterpret_cast<const TWR_GLOBAL uint32_t*>(w.tile + (uint64_t)(sel & 0xFFFFu) * sizeof(DynTile));
  static_assert(offsetof(DynPolyL, rel) == 0 && offsetof(DynPolyL, pres) == 12 && offsetof(DynPolyL, flags) == 24 && offsetof(DynPolyL, code) == 28,
                "DynPolyL dwords");
  r.t0m = dm[0]; r.iTm = dm[1];
  r.t0f = df[0]; r.iTf = df[1];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.relm[i] = um[i]; r.presm[i] = um[3 + i];
    r.relf[i] = uf[i]; r.presf[i] = uf[3 + i];
  }
  r.flagsm = um[6];
  r.flagsf = uf[6];
#pragma unroll
  for (int i = 0; i < 5; ++i) r.tl[i] = tl[i];
}
TWR_DEV void dyn2_load_codes(const DynWork& w, uint32_t sel, DynCodes& c) {
  const TWR_GLOBAL uint32_t* um = reinterpret_cast<const TWR_GLOBAL uint32_t*>(dyn2_poly_l_addr(w, (sel >> 16) & 0xFFu));
  const TWR_GLOBAL uint32_t* uf = reinterpret_cast<const TWR_GLOBAL uint32_t*>(dyn2_poly_l_addr(w, sel >> 24));
#pragma unroll
  for (int i = 0; i < 6; ++i) c.m[i] = um[7 + i];
#pragma unroll
  for (int i = 0; i < 9; ++i) c.f[i] = uf[7 + i];
}
TWR_DEV void dyn2_front(const DynFrontRec& r, const char* __restrict__ xs, int lane, Dyn2Front& S) {
  const DynNode& nd = r.nd;
  const int role = lane & 3;
  double wP[4], wV[4], wA[4];
  hermite_all(nd.tb, nd.iTb, wP, wV, wA);
  double c[3], e[3];
  {  // base spline points (Spline::GetPoint in basis form): the active polynomial's [p0 v0 p1 v1] x 3
    double bl[12], ba[12];
    const double2* pl = reinterpret_cast<const double2*>(__builtin_assume_aligned(xs + nd.sb_lin, 16));
    const double2* pa = reinterpret_cast<const double2*>(__builtin_assume_aligned(xs + nd.sb_ang, 16));
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double2 a = pl[i], b = pa[i];
      bl[2 * i] = a.x; bl[2 * i + 1] = a.y;
      ba[2 * i] = b.x; ba[2 * i + 1] = b.y;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      c[d] = wP[0] * bl[d] + wP[1] * bl[3 + d] + wP[2] * bl[6 + d] + wP[3] * bl[9 + d];
      S.cdd[d] = wA[0] * bl[d] + wA[1] * bl[3 + d] + wA[2] * bl[6 + d] + wA[3] * bl[9 + d];
      e[d] = wP[0] * ba[d] + wP[1] * ba[3 + d] + wP[2] * ba[6 + d] + wP[3] * ba[9 + d];
      S.ed[d] = wV[0] * ba[d] + wV[1] * ba[3 + d] + wV[2] * ba[6 + d] + wV[3] * ba[9 + d];
      S.edd[d] = wA[0] * ba[d] + wA[1] * ba[3 + d] + wA[2] * ba[6 + d] + wA[3] * ba[9 + d];
    }
  }
  // staging indices of the twelve candidates of a spline, four at a time: (S4 + rel4) & pres4 -- a candidate that is not a
  // variable reads index 0, the zero slot (no selects in the spline evaluation)
  const uint32_t sm4 = ((r.tl[4] >> 16) & 0xFFu) * 0x01010101u, sf4 = (r.tl[4] >> 24) * 0x01010101u;
  // this lane's end-effector: weights and spline points
  {
    double vm[12], p[3];
    const uint32_t im[3] = {(sm4 + r.relm[0]) & r.presm[0], (sm4 + r.relm[1]) & r.presm[1], (sm4 + r.relm[2]) & r.presm[2]};
    gather12s(xs, im, vm);
    hermite_pos(nd.t - r.t0m, r.iTm, S.wm);
    S.wm[0] += (r.flagsm & 1) ? S.wm[2] : 0.0;   // stance polynomial: p1 is the same variable as p0
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      p[d] = S.wm[0] * vm[d] + S.wm[1] * vm[3 + d] + S.wm[2] * vm[6 + d] + S.wm[3] * vm[9 + d];
      S.rv[d] = c[d] - p[d];
    }
  }
  {
    double vf[12];
    const uint32_t jf[3] = {(sf4 + r.relf[0]) & r.presf[0], (sf4 + r.relf[1]) & r.presf[1], (sf4 + r.relf[2]) & r.presf[2]};
    gather12s(xs, jf, vf);
    hermite_pos(nd.t - r.t0f, r.iTf, S.wf);
#pragma unroll
    for (int d = 0; d < 3; ++d) S.f[d] = S.wf[0] * vf[d] + S.wf[1] * vf[3 + d] + S.wf[2] * vf[6 + d] + S.wf[3] * vf[9 + d];
  }
  // force and torque sums over the end-effectors (single_rigid_body_dynamics.cc:81-88); dummy roles carry f = 0
  double t3[3];
  cross3(S.f, S.rv, t3);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    S.F[d] = quad_sum(S.f[d]);
    S.tau[d] = quad_sum(t3[d]);
  }
  // rotation: lanes 0..2 of the quad evaluate one sincos each and broadcast it
  double my_s, my_c;
  sincos_fast(sel3(role, e[0], e[1], e[2]), &my_s, &my_c);
  S.sx = quad_perm<0x00>(my_s); S.cx = quad_perm<0x00>(my_c);
  S.sy = quad_perm<0x55>(my_s); S.cy = quad_perm<0x55>(my_c);
  S.sz = quad_perm<0xAA>(my_s); S.cz = quad_perm<0xAA>(my_c);
}

// Back half: Jacobian blocks and constraint values into the LDS image.  `img` is the byte address of the image
// (parity shift included), node base and row offsets come from DynNodeL, tile offsets from DynTile + DynPolyL::code.
TWR_DEV void dyn2_back(const DynWork& w, const DynFrontRec& rec, const DynCodes& cd, const Dyn2Front& S, double* __restrict__ gst,
                       char* __restrict__ img, int lane, bool want_g, bool want_j) {
  const DynNode& nd = rec.nd;
  const int kk = lane >> 2, role = lane & 3;
  if (kk >= w.cnt) return;
  const double (&cdd)[3] = S.cdd, (&ed)[3] = S.ed, (&edd)[3] = S.edd;
  const double (&wm)[4] = S.wm, (&wf)[4] = S.wf, (&f)[3] = S.f, (&rv)[3] = S.rv, (&F)[3] = S.F, (&tau)[3] = S.tau;
  const double sx = S.sx, cx = S.cx, sy = S.sy, cy = S.cy, sz = S.sz, cz = S.cz;
  char* nb = img + nd.nb;   // first value of this time node
  // --- ee-motion block [f]x J_p (:181-192) and ee-force block {[r]x J_f ; -J_f} (:167-179) of this lane's
  // end-effector, BEFORE the base blocks.  A value goes to  node base + tile start in its row (DynTile) + 8 * rank
  // (DynPolyL::code, one byte per value); see DynPolyL for where the values of candidates that are not variables end up.
  if (want_j) {
    char* rowm[3] = {nb + (rec.tl[0] & 0xFFFFu), nb + (rec.tl[0] >> 16), nb + (rec.tl[1] & 0xFFFFu)};
    char* rowf[6] = {nb + (rec.tl[1] >> 16), nb + (rec.tl[2] & 0xFFFFu), nb + (rec.tl[2] >> 16),
                     nb + (rec.tl[3] & 0xFFFFu), nb + (rec.tl[3] >> 16), nb + (rec.tl[4] & 0xFFFFu)};
    // a force node that is constant stores the values of the polynomial's other node once more (same slots, same values)
    const bool c0 = rec.flagsf & 2, c1 = rec.flagsf & 4;
    const double wfp[4] = {c0 ? wf[2] : wf[0], c0 ? wf[3] : wf[1], c1 ? wf[0] : wf[2], c1 ? wf[1] : wf[3]};
#define TWR_CODE_M(c, k) ((cd.m[(2 * (c) + (k)) >> 2] >> (8 * ((2 * (c) + (k)) & 3))) & 0xFFu)
#define TWR_CODE_F(c, k) ((cd.f[(3 * (c) + (k)) >> 2] >> (8 * ((3 * (c) + (k)) & 3))) & 0xFFu)
#define TWR_EE_TILE_M(J, D, R1, R2)                                              \
  {                                                                              \
    lds_put(rowm[R1], TWR_CODE_M((J) * 3 + D, 0), crs<R1, D>(f) * wm[J]);        \
    lds_put(rowm[R2], TWR_CODE_M((J) * 3 + D, 1), crs<R2, D>(f) * wm[J]);        \
  }
#define TWR_EE_TILE_F(J, D, R1, R2)                                              \
  {                                                                              \
    lds_put(rowf[R1], TWR_CODE_F((J) * 3 + D, 0), crs<R1, D>(rv) * wfp[J]);      \
    lds_put(rowf[R2], TWR_CODE_F((J) * 3 + D, 1), crs<R2, D>(rv) * wfp[J]);      \
    lds_put(rowf[3 + D], TWR_CODE_F((J) * 3 + D, 2), -wfp[J]);                   \
  }
#define TWR_EE_TILES(J)      \
  TWR_EE_TILE_M(J, 0, 1, 2)  \
  TWR_EE_TILE_M(J, 1, 2, 0)  \
  TWR_EE_TILE_M(J, 2, 0, 1)  \
  TWR_EE_TILE_F(J, 0, 1, 2)  \
  TWR_EE_TILE_F(J, 1, 2, 0)  \
  TWR_EE_TILE_F(J, 2, 0, 1)
    TWR_EE_TILES(3)   // (ee-motion: p0 LAST -- it overwrites what candidates without a variable left in its slots)
    TWR_EE_TILES(2)
    TWR_EE_TILES(1)
    TWR_EE_TILES(0)
#undef TWR_EE_TILES
#undef TWR_EE_TILE_F
#undef TWR_EE_TILE_M
#undef TWR_CODE_F
#undef TWR_CODE_M
  }
  // --- angular quantities (euler_converter.cc:58-83,133-166,207-221)
  double R[3][3];
  R[0][0] = cy * cz; R[0][1] = cz * sx * sy - cx * sz; R[0][2] = sx * sz + cx * cz * sy;
  R[1][0] = cy * sz; R[1][1] = cx * cz + sx * sy * sz; R[1][2] = cx * sy * sz - cz * sx;
  R[2][0] = -sy;     R[2][1] = cy * sx;                R[2][2] = cx * cy;
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
  const TWR_CONST DevStruct* H = cptr<DevStruct>(w.hdr);  // uniform per work item: scalar loads
  double Iw6[6];  // I_w = R I_b R^T (single_rigid_body_dynamics.cc:91), symmetric: (00,01,02,11,12,22)
  {
    double Ib[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) Ib[i] = H->Ib[i];
    double T[3][3];  // R I_b
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      T[i][0] = R[i][0] * Ib[0] + R[i][1] * Ib[1] + R[i][2] * Ib[2];
      T[i][1] = R[i][0] * Ib[1] + R[i][1] * Ib[3] + R[i][2] * Ib[4];
      T[i][2] = R[i][0] * Ib[2] + R[i][1] * Ib[4] + R[i][2] * Ib[5];
    }
    Iw6[0] = T[0][0] * R[0][0] + T[0][1] * R[0][1] + T[0][2] * R[0][2];
    Iw6[1] = T[0][0] * R[1][0] + T[0][1] * R[1][1] + T[0][2] * R[1][2];
    Iw6[2] = T[0][0] * R[2][0] + T[0][1] * R[2][1] + T[0][2] * R[2][2];
    Iw6[3] = T[1][0] * R[1][0] + T[1][1] * R[1][1] + T[1][2] * R[1][2];
    Iw6[4] = T[1][0] * R[2][0] + T[1][1] * R[2][1] + T[1][2] * R[2][2];
    Iw6[5] = T[2][0] * R[2][0] + T[2][1] * R[2][1] + T[2][2] * R[2][2];
  }
  double Iw_wd[3], Iw_w[3];
  symmul(Iw6, omd, Iw_wd);
  symmul(Iw6, om, Iw_w);
  const double m = H->mass;
  double wP[4], wV[4], wA[4];
  {
    double tb = nd.tb;
    asm volatile("" : "+v"(tb));   // a fresh evaluation: do not carry the front half's twelve weights across the copy-out
    hermite_all(tb, nd.iTb, wP, wV, wA);
  }
  char* row[3] = {nb, nb + nd.rs1, nb + nd.rs2};

  if (role == 3) {
    if (want_g) {  // GetDynamicViolation, single_rigid_body_dynamics.cc:76-101
      double wxIw[3];
      cross3(om, Iw_w, wxIw);
      double* go = gst + 6 * kk;  // staged in LDS, written out coalesced with the Jacobian slice
#pragma unroll
      for (int i = 0; i < 3; ++i) go[i] = Iw_wd[i] + wxIw[i] - tau[i];
      go[3] = m * cdd[0] - F[0];
      go[4] = m * cdd[1] - F[1];
      go[5] = m * cdd[2] - F[2] + m * H->gravity;
    }
  }
  if (want_j) {  // base-lin block: ang rows -sum_i [f_i]x J_pos, lin rows m J_acc (:103-121).  Every lane of the quad stores
                 // the nine values of ONE node value j = role (all four roles busy instead of role 3 storing all 36)
    const double wPj = role == 0 ? wP[0] : (role == 1 ? wP[1] : (role == 2 ? wP[2] : wP[3]));
    const double wAj = role == 0 ? wA[0] : (role == 1 ? wA[1] : (role == 2 ? wA[2] : wA[3]));
    const uint32_t o2 = 16u * (uint32_t)role, o1 = 8u * (uint32_t)role;
    lds_put(row[0], o2, -crs<0, 1>(F) * wPj);
    lds_put(row[0], o2 + 8, -crs<0, 2>(F) * wPj);
    lds_put(row[1], o2, -crs<1, 0>(F) * wPj);
    lds_put(row[1], o2 + 8, -crs<1, 2>(F) * wPj);
    lds_put(row[2], o2, -crs<2, 0>(F) * wPj);
    lds_put(row[2], o2 + 8, -crs<2, 1>(F) * wPj);
    const double ma = m * wAj;
#pragma unroll
    for (int d = 0; d < 3; ++d) lds_put(nb + nd.rl[d], o1, ma);
  }
  if (role != 3 && want_j) {
    // --- base-ang block (:123-165), Euler dimension d = role, factored (derivation: see pdyn_math)
    const double dMx_dy[3] = {-sy * cz, -sy * sz, -cy};
    const double dMx_dz[3] = {-cy * sz, cy * cz, 0.0};
    const double dMy_dz[3] = {-cz, -sz, 0.0};
    const double dMdx_dy[3] = {-cz * cy * yd + sy * sz * zd, -sy * cz * zd - cy * sz * yd, sy * yd};
    const double dMdx_dz[3] = {sz * sy * yd - cy * cz * zd, -cy * sz * zd - sy * cz * yd, 0.0};
    const double dMdy_dz[3] = {sz * zd, -cz * zd, 0.0};
    double Md[3], dwd_ed[3], dw[3], dwd[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Md[i] = sel3(role, Mx[i], My[i], i == 2 ? 1.0 : 0.0);  // column d of M (euler_converter.cc:133-148)
      dwd_ed[i] = sel3(role, Mdx[i], Mdy[i] + xd * dMx_dy[i], xd * dMx_dz[i] + yd * dMy_dz[i]);
      dw[i] = sel3(role, 0.0, xd * dMx_dy[i], xd * dMx_dz[i] + yd * dMy_dz[i]);
      dwd[i] = sel3(role, 0.0, xd * dMdx_dy[i] + edd[0] * dMx_dy[i],
                    xd * dMdx_dz[i] + yd * dMdy_dz[i] + edd[0] * dMx_dz[i] + edd[1] * dMy_dz[i]);
    }
    auto dIw = [&](const double v[3], const double Iwv[3], double o[3]) {
      double t1[3], t2[3], t3b[3];
      cross3(Md, Iwv, t1);
      cross3(v, Md, t2);
      symmul(Iw6, t2, t3b);
#pragma unroll
      for (int i = 0; i < 3; ++i) o[i] = t1[i] + t3b[i];
    };
    double A[3], B[3], C[3];
    symmul(Iw6, Md, C);
    {
      double t1[3], t2[3], t3b[3];
      symmul(Iw6, dwd_ed, t1);
      cross3(Md, Iw_w, t2);
      cross3(om, C, t3b);
#pragma unroll
      for (int i = 0; i < 3; ++i) B[i] = t1[i] + t2[i] + t3b[i];
    }
    {
      double t1[3], t2[3], t3b[3], t4[3], t5[3], t6[3], t7[3];
      dIw(omd, Iw_wd, t1);
      symmul(Iw6, dwd, t2);
      cross3(dw, Iw_w, t3b);
      dIw(om, Iw_w, t4);
      symmul(Iw6, dw, t5);
#pragma unroll
      for (int i = 0; i < 3; ++i) t6[i] = t4[i] + t5[i];
      cross3(om, t6, t7);
#pragma unroll
      for (int i = 0; i < 3; ++i) A[i] = t1[i] + t2[i] + t3b[i] + t7[i];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int j = 0; j < 4; ++j) lds_put(row[r], 8 * (8 + 3 * j + role), A[r] * wP[j] + B[r] * wV[j] + C[r] * wA[j]);
  }
}

// Shared by dyn_body and dyn_uniform_body.  The x gather of a slice: xp = x of its problem, m = XC 16-bit indices per lane
template <int XC>
TWR_DEV void dyn_gather_x(const double* xp, uint2 m, double xr[XC]) {
  xr[0] = xp[m.x & 0xFFFFu];
  xr[1] = xp[m.x >> 16];
  if (XC == 4) {
    xr[XC - 2] = xp[m.y & 0xFFFFu];
    xr[XC - 1] = xp[m.y >> 16];
  }
}
// image -> HBM; the constraint values (6 per time node, contiguous in g) with clamped lanes instead of predicates
template <bool WANT_G, bool WANT_J, bool NT>
TWR_DEV void dyn_copy_out(const double* stage, double* pdst, double* pg, int nvals, int cnt, int lane) {
  constexpr int NIT = (kDynImage + 2 + 127) / 128;
  const double* gst = stage + (WANT_J ? kDynG0 : 0);
  const int ppar = (int)((reinterpret_cast<uintptr_t>(pdst) >> 3) & 1);
  // (NT: batches of two -- with the non-temporal builtin the LDS reads of a batch keep registers of their own, and eight of
  // them in flight put 12 VGPRs into scratch; the plain form ends up serialised through one quad whatever the batch is)
  if (WANT_J) copy_out_fixed<NIT, NT ? 2 : kDynCopyBatch, NT>(pdst, stage, nvals, ppar, lane);
  if (WANT_G) {
    const int last = 6 * cnt - 1;
    pg[min(lane, last)] = gst[min(lane, last)];
    pg[min(lane + 64, last)] = gst[min(lane + 64, last)];
  }
}
// Loop of one persistent single-wave workgroup over its strided slices.  State at the top of iteration i: xs holds
// x(i); `xr` (registers) holds x(i+1), gathered one iteration ago; mapr holds the staging map of slice i+2;
// the front records of slice i and the record selectors (DynSel) of slices i and i+1 are in registers.
//   F  front(i): LDS reads of xs + the front records -> compact state
//   P  issue the loads of slice i's tile codes (needed by the back half only) and of slice i+1's front records (node,
//      polynomial and tile records, addressed through its selector, which arrived an iteration ago); they land during
//      the copy-out
//   O  copy-out(i-1): image -> HBM (one phase late: the x gathers of the previous iteration were issued before
//      these stores, so waiting for them never waits for a store)
//   B  back(i): Jacobian blocks -> image
//   S  xs <- xr (x(i+1));  then issue: selector of slice i+2, xr <- gather x(i+2), mapr <- map(i+3)
// (`stage`: kDynLds doubles of LDS owned by this wave; the wave takes slices i, i + stride, ...)
// WANT_G / WANT_J are compile-time, the first iteration copies the not-yet-filled image to a dump region instead of
// skipping the copy-out, and no store sits in a divergent branch: the number of vector-memory instructions between a
// prefetch and its use is then a constant on every path, and the compiler's counted waits stay counted.  (With run-time
// flags and `if (pending)` it had to assume the shortest path -- no stores at all -- and the wait for the put record in
// the middle of the loop drained the whole copy-out of the previous slice.)
// XC = 64-entry chunks of the staging map the slices of the batch use (2: every slice stages at most 128 doubles of x --
// true for all K = 200 problems, whose 12..15-node slices stage ~100 -- and reads the 256-byte form of its map; 4: the
// general 512-byte form).  A compile-time count: the x gather is XC loads per lane, the same on every path.
template <bool WANT_G, bool WANT_J, int XC, bool NT>
TWR_DEV void dyn_body(const DynWork* __restrict__ work, int n_work, const double* __restrict__ x, double* __restrict__ g,
                      double* __restrict__ jac, double* __restrict__ dump, double* stage, int lane, int i, int stride) {
  static_assert(XC == 2 || XC == 4, "staging map chunks");
  // (WANT_J false: no image -- the wave's LDS would be g + xs alone)
  constexpr int kG0 = WANT_J ? kDynG0 : 0, kX0 = kG0 + 96;
  double* gst = stage + kG0;
  char* xs = reinterpret_cast<char*>(stage + kX0);
  if (i >= n_work) return;
  if (lane < 2) stage[kX0 + lane] = 0.0;   // the zero pair
  auto load_map = [&](const DynWork& w) {   // XC 16-bit x indices per lane
    uint2 m;
    if (XC == 4) m = gptr<uint2>(w.map)[lane];
    else m = make_uint2(gptr<uint32_t>(w.map)[lane], 0u);
    return m;
  };
  auto stage_x = [&](const double xr[XC]) {
#pragma unroll
    for (int c = 0; c < XC; ++c)
      if (64 * c + lane < kDynXsCap) stage[kX0 + 2 + 64 * c + lane] = xr[c];
  };
  // Every prefetch is issued unconditionally, with the slice index clamped to this workgroup's last slice (a repeated load
  // of the last slice's records / x is harmless): no prefetched value goes through a phi or a conditional copy -- that is
  // what makes the compiler wait for a load right where it is issued (see rom_body) -- and the number of vector-memory
  // instructions per iteration is the same on every path.
  const int last = i + (n_work - 1 - i) / stride * stride;
  DynWork wp = work[i];   // slice whose image is waiting to be copied out
  // (nothing is pending in the first iteration: its copy-out goes to the dump region, same instruction count)
  double* pdst = dump;
  double* pg = dump + kDynImage + 2;
  DynWork w0 = wp, w1 = work[min(i + stride, last)], w2 = work[min(i + 2 * stride, last)];
  DynFrontRec fr0;
  double xr[XC];
  uint2 mapr = load_map(w0);
  uint32_t sel0 = dyn2_load_sel(w0, lane);
  dyn2_load_front(w0, sel0, lane, fr0);                  // (the only exposed record -> record dependency)
  dyn_gather_x<XC>(x + w0.x_off, mapr, xr);
  stage_x(xr);                                           // x(first slice): the only exposed gather
  mapr = load_map(w1);
  uint32_t sel1 = dyn2_load_sel(w1, lane);
  dyn_gather_x<XC>(x + w1.x_off, mapr, xr);
  mapr = load_map(w2);
  for (; i <= last; i += stride) {
    const DynWork w3 = work[min(i + 3 * stride, last)];
    double* dst = jac + w0.j_off;
    const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
    Dyn2Front S;
    dyn2_front(fr0, xs, lane, S);                                                            // F
    DynCodes cd;
    dyn2_load_codes(w0, sel0, cd);                                                           // P  (lands during the copy-out)
    DynFrontRec fr1;
    dyn2_load_front(w1, sel1, lane, fr1);                                                    //    front records of slice i+1
    // (the copy-out runs at raised wave priority: with two waves per SIMD a wave in its store phase then gets its LDS
    // reads and stores issued ahead of its neighbour's math, which keeps the store stream of the CU steadier -- A/B on one
    // box 0.602-0.608 -> 0.591-0.596 ms; raised priority around the prefetches as well, or in rom_kernel, which runs one
    // wave per SIMD, is neutral to slower)
    __builtin_amdgcn_s_setprio(3);
    dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wp.nvals, wp.cnt, lane);               // O
    __builtin_amdgcn_s_setprio(0);
    dyn2_back(w0, fr0, cd, S, gst, reinterpret_cast<char*>(stage + par), lane, WANT_G, WANT_J);   // B
    stage_x(xr);                                                                             // S
    const uint32_t sel2 = dyn2_load_sel(w2, lane);
    dyn_gather_x<XC>(x + w2.x_off, mapr, xr);
    mapr = load_map(w3);
    wp = w0;
    pdst = dst;
    pg = g + w0.g_off;
    w0 = w1; fr0 = fr1; sel0 = sel1;
    w1 = w2; sel1 = sel2;
    w2 = w3;
  }
  dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wp.nvals, wp.cnt, lane);   // last slice of this workgroup
}

template <bool WANT_G, bool WANT_J, int XC, bool NT>
__global__ __launch_bounds__(64, TWR_DYN_WAVES) void dyn_kernel(const DynWork* __restrict__ work, int n_work, const double* __restrict__ x,
                                                    double* __restrict__ g, double* __restrict__ jac, double* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) double stage[kDynLds];
  dyn_body<WANT_G, WANT_J, XC, NT>(work, n_work, x, g, jac, dump, stage, threadIdx.x, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------- dynamic, uniform list (dyn_uniform_kernel)
// Every problem of the batch is the same structure (device_tables.h DynUniform): the wave owns ONE slice kind, loads that
// kind's DynWork, selector, staging map, front records and tile codes once, before the loop, and then walks problems, not
// list positions.  Per iteration it gathers x of the problem after next, as dyn_body does, and forms the three offsets
// from the problem index; the 20 record loads of a dyn_body iteration (two of them dependent) are gone.  Same phases F O B
// S, the same single call sites of dyn2_front / dyn2_back / copy_out_fixed, the same clamped unconditional x prefetch and
// a constant count of vector-memory instructions per iteration.  Nothing of the image is kept from slice to slice: every
// value is recomputed and rewritten.
// Results are bit-identical to dyn_body's: the records pass through an empty asm at the top of every iteration, so the
// compiler sees fresh values there, exactly as after dyn_body's loads, and hoists no arithmetic on them out of the loop
// (a product of two record constants computed ahead of the loop could no longer contract into the FMA it forms in dyn_body).
TWR_DEV void dyn_fresh(double& v) { asm volatile("" : "+v"(v)); }
TWR_DEV void dyn_fresh(uint32_t& v) { asm volatile("" : "+v"(v)); }
template <bool WANT_G, bool WANT_J, int XC, bool NT>
TWR_DEV void dyn_uniform_body(const DynWork* __restrict__ work, const DynUniform u, const double* __restrict__ x,
                              double* __restrict__ g, double* __restrict__ jac, double* __restrict__ dump, double* stage, int lane,
                              int block) {
  static_assert(XC == 2 || XC == 4, "staging map chunks");
  constexpr int kG0 = WANT_J ? kDynG0 : 0, kX0 = kG0 + 96;
  double* gst = stage + kG0;
  char* xs = reinterpret_cast<char*>(stage + kX0);
  const DynUniformSlot sl = dyn_uniform_slot(u, block);
  if (sl.first >= u.n_problems) return;
  if (lane < 2) stage[kX0 + lane] = 0.0;   // the zero pair
  DynWork wt = work[sl.kind * u.first_stride];   // this kind's slice of problem 0
  uint2 mapr;
  if (XC == 4) mapr = gptr<uint2>(wt.map)[lane];
  else mapr = make_uint2(gptr<uint32_t>(wt.map)[lane], 0u);
  auto gather_x = [&](int p, double xr[XC]) { dyn_gather_x<XC>(x + wt.x_off + (int64_t)p * u.x_stride, mapr, xr); };
  auto stage_x = [&](const double xr[XC]) {
#pragma unroll
    for (int c = 0; c < XC; ++c)
      if (64 * c + lane < kDynXsCap) stage[kX0 + 2 + 64 * c + lane] = xr[c];
  };
  const int plast = sl.first + (u.n_problems - 1 - sl.first) / sl.step * sl.step;   // this wave's last problem
  const uint32_t sel = dyn2_load_sel(wt, lane);
  DynFrontRec fr;
  dyn2_load_front(wt, sel, lane, fr);
  DynCodes cd;
  dyn2_load_codes(wt, sel, cd);
  double xr[XC];
  gather_x(sl.first, xr);
  stage_x(xr);                                           // x(first problem): the only exposed gather
  gather_x(min(sl.first + sl.step, plast), xr);
  double* pdst = dump;                                   // (first iteration: nothing pending, same instruction count)
  double* pg = dump + kDynImage + 2;
  for (int p = sl.first; p <= plast; p += sl.step) {
    // (in place: the records stay in the registers they were loaded into, no copies)
    asm volatile("" : "+s"(wt.hdr));
    dyn_fresh(fr.nd.t); dyn_fresh(fr.nd.tb); dyn_fresh(fr.nd.iTb);
    dyn_fresh(fr.t0m); dyn_fresh(fr.iTm); dyn_fresh(fr.t0f); dyn_fresh(fr.iTf);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      dyn_fresh(fr.relm[q]); dyn_fresh(fr.presm[q]); dyn_fresh(fr.relf[q]); dyn_fresh(fr.presf[q]);
    }
    dyn_fresh(fr.flagsm); dyn_fresh(fr.flagsf);
#pragma unroll
    for (int q = 0; q < 5; ++q) dyn_fresh(fr.tl[q]);
#pragma unroll
    for (int q = 0; q < 6; ++q) dyn_fresh(cd.m[q]);
#pragma unroll
    for (int q = 0; q < 9; ++q) dyn_fresh(cd.f[q]);
    double* dst = jac + wt.j_off + (int64_t)p * u.j_stride;
    const int par = (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1);
    Dyn2Front S;
    dyn2_front(fr, xs, lane, S);                                                             // F
    __builtin_amdgcn_s_setprio(3);
    dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wt.nvals, wt.cnt, lane);               // O  (the kind's counts)
    __builtin_amdgcn_s_setprio(0);
    dyn2_back(wt, fr, cd, S, gst, reinterpret_cast<char*>(stage + par), lane, WANT_G, WANT_J);    // B
    stage_x(xr);                                                                             // S
    gather_x(min(p + 2 * sl.step, plast), xr);
    pdst = dst;
    pg = g + wt.g_off + (int64_t)p * u.g_stride;
  }
  dyn_copy_out<WANT_G, WANT_J, NT>(stage, pdst, pg, wt.nvals, wt.cnt, lane);   // last problem of this wave
}

template <bool WANT_G, bool WANT_J, int XC, bool NT>
__global__ __launch_bounds__(64, TWR_DYN_WAVES) void dyn_uniform_kernel(const DynWork* __restrict__ work, const DynUniform u,
                                                                        const double* __restrict__ x, double* __restrict__ g,
                                                                        double* __restrict__ jac, double* __restrict__ dump) {
  __shared__ __attribute__((aligned(16))) double stage[kDynLds];
  dyn_uniform_body<WANT_G, WANT_J, XC, NT>(work, u, x, g, jac, dump, stage, threadIdx.x, blockIdx.x);
}

// Values only (TWR_EVAL_VALUES: Ipopt's eval_g, a planner's scoring step): problems with fixed timings take the one-lane-per-
// time-node kernels below (eval_values_kernel); kDynValuesLds is what node_body needs of a wave's LDS there.
constexpr int kDynValuesLds = 96 + 2 + kDynXsCap;
}  // namespace twr
