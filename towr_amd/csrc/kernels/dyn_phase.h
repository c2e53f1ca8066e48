#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "async_pipe.h"
#include "common.h"
#include "spline_math.h"

namespace twr {
// ---- dynamic with optimised timings (dyn_phase_kernel)
// Persistent single-wave workgroups, software pipelined like rom_kernel.  The rows of "dynamic" now hold ALL variables
// of every ee set (C3: 1280 values = 10 KB per time node, ~75 % explicit zeros), so a work item is a "pass" of only FOUR
// consecutive time nodes (40 KB of Jacobian values) and a time node gets SIXTEEN lanes:
//   lane = 16 n + 4 e + j:   n = time node of the pass, e = end-effector, j = node value (p0, v0, p1, v1)
// Lane (n, e, j) loads the three dimensions of node value j of the base splines and of ee e's active polynomials and owns
// their Jacobian columns.  Spline points are sums over j (DPP quad sums), force / torque totals are sums over e (DPP row
// rotations by 4 and 8 lanes); the SRBD algebra is evaluated by every lane (the same instructions for all of them);
// lanes e < 3 produce Euler dimension e of the base-ang block, lanes e = 3 the base-lin block, the duration columns of
// ee e are spread over its four lanes.  What depends on x in the index work -- active polynomials, local times, current
// phase of every (time node, ee) -- comes from the pre-pass (phase_locate_kernel -> DynLoc); everything else is a
// constant of the structure: the byte offset of every value inside its time node is read off the CSR pattern on the
// host (PhasePutM / PhasePutF per polynomial, PhaseEe for the duration columns).  Per pass the wave clears the LDS image
// of the four expanded nodes, every lane stores its ~25 values at their final positions, and the wave streams the image
// to HBM with 16-byte coalesced stores: every byte of the Jacobian is written exactly once.
struct PDynRec {       // per lane: what depends on the work item only -- DynShared {tb, iTb, q6} and the DynLoc record,
                       // kept as whole dwords (unpacked with shifts where used)
  double tb, iTb;      // base spline: local time in the active polynomial, 1 / duration
  int32_t q6;
  double tm, Tm, tf, Tf;
  int32_t xbase_m, xbase_f;
  uint32_t slots_m[2], slots_f[2];
  uint32_t imjf;       // im | jf << 16
  uint32_t misc;       // cur | flags << 8 | np_m << 16 | np_f << 24
};
struct PDynIn {        // per lane: what depends on the record (second stage of the pipeline)
  double bl[3], ba[3], m[3], f[3];   // node value j (3 dimensions) of base-lin / base-ang and of ee e's polynomials
};
struct PDynPut {       // per lane: where its values go (loaded at the top of the pass, used at its end), whole dwords
  uint32_t pm[4], pf[6];             // 16-bit put offsets of candidates (j, D): index 2 D + r resp. 3 D + r
  int32_t ns, dur_ang[3], dur_lin[3];
  TWR_DEV uint32_t m(int q) const { return (pm[q >> 1] >> (16 * (q & 1))) & 0xFFFFu; }
  TWR_DEV uint32_t f(int q) const { return (pf[q >> 1] >> (16 * (q & 1))) & 0xFFFFu; }
};
struct ARec {          // record of a pass: DynShared {tb, iTb}, q6, DynLoc                 (6 loads)
  twr_v4f sh;
  uint32_t q6;
  twr_v4f lc[4];
};
struct AIn {           // x values of a pass                                               (12 loads)
  double v[12];
};
struct APut {          // put offsets of a pass: PhasePutM row j, PhasePutF row j, PhaseEe  (6 loads)
  twr_v4f pm;
  double pf[3];
  twr_v4f pe[2];
};
TWR_DEV void pdyn_issue_rec(uint64_t shared, uint64_t loc, int loc_stride, int cnt, int n_ee, int lane, ARec& a) {
  const int n = min(lane >> 4, cnt - 1), e = min((lane >> 2) & 3, n_ee - 1);   // (ee >= n_ee read ee n_ee-1 and are neutralised)
  const char* sh = reinterpret_cast<const char*>(shared) + sizeof(DynShared) * (size_t)n;
  const char* lc = reinterpret_cast<const char*>(loc) + (size_t)e * (size_t)loc_stride + sizeof(DynLoc) * (size_t)n;
  aload(a.sh, sh);
  aload(a.q6, sh + offsetof(DynShared, q6));
#pragma unroll
  for (int q = 0; q < 4; ++q) aload(a.lc[q], lc + 16 * q);
}
template <int N>
TWR_DEV void pdyn_wait_rec(ARec& a, PDynRec& r) {
  asm volatile("s_waitcnt %6" : "+a"(a.sh), "+a"(a.q6), "+a"(a.lc[0]), "+a"(a.lc[1]), "+a"(a.lc[2]), "+a"(a.lc[3]) : "n"(vmcnt_imm(N)) : "memory");
  static_assert(offsetof(DynLoc, xbase_m) == 32 && offsetof(DynLoc, slots_m) == 40 && offsetof(DynLoc, slots_f) == 48 &&
                offsetof(DynLoc, im) == 56 && offsetof(DynLoc, cur) == 60, "DynLoc dwords");
  r.tb = pdyn_f64(a.sh.x, a.sh.y);
  r.iTb = pdyn_f64(a.sh.z, a.sh.w);
  r.q6 = (int32_t)a.q6;
  r.tm = pdyn_f64(a.lc[0].x, a.lc[0].y);
  r.Tm = pdyn_f64(a.lc[0].z, a.lc[0].w);
  r.tf = pdyn_f64(a.lc[1].x, a.lc[1].y);
  r.Tf = pdyn_f64(a.lc[1].z, a.lc[1].w);
  r.xbase_m = (int32_t)__float_as_uint(a.lc[2].x);
  r.xbase_f = (int32_t)__float_as_uint(a.lc[2].y);
  r.slots_m[0] = __float_as_uint(a.lc[2].z);
  r.slots_m[1] = __float_as_uint(a.lc[2].w);
  r.slots_f[0] = __float_as_uint(a.lc[3].x);
  r.slots_f[1] = __float_as_uint(a.lc[3].y);
  r.imjf = __float_as_uint(a.lc[3].z);
  r.misc = __float_as_uint(a.lc[3].w);
}
TWR_DEV void pdyn_issue_in(const PDynWork& w, const PDynRec& r, const double* __restrict__ x, int lane, AIn& a) {
  const double* xp = x + w.x_off;
  const int j = lane & 3;
  const double* xl = xp + w.off_lin + r.q6 + 3 * j;
  const double* xa = xp + w.off_ang + r.q6 + 3 * j;
  const uint32_t sm = slots12(r.slots_m[0], r.slots_m[1], j), sf = slots12(r.slots_f[0], r.slots_f[1], j);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    aload(a.v[d], xl + d);
    aload(a.v[3 + d], xa + d);
    const uint32_t am = (sm >> (4 * d)) & 0xFu, af = (sf >> (4 * d)) & 0xFu;   // absent candidates read slot 0, weight 0
    aload(a.v[6 + d], xp + r.xbase_m + (am != 0xFu ? am : 0u));
    aload(a.v[9 + d], xp + r.xbase_f + (af != 0xFu ? af : 0u));
  }
}
template <int N>
TWR_DEV void pdyn_wait_in(AIn& a, PDynIn& in) {
  asm volatile("s_waitcnt %12" : "+a"(a.v[0]), "+a"(a.v[1]), "+a"(a.v[2]), "+a"(a.v[3]), "+a"(a.v[4]), "+a"(a.v[5]), "+a"(a.v[6]),
               "+a"(a.v[7]), "+a"(a.v[8]), "+a"(a.v[9]), "+a"(a.v[10]), "+a"(a.v[11]) : "n"(vmcnt_imm(N)) : "memory");
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    in.bl[d] = a.v[d];
    in.ba[d] = a.v[3 + d];
    in.m[d] = a.v[6 + d];
    in.f[d] = a.v[9 + d];
  }
}
TWR_DEV void pdyn_issue_put(const PDynWork& w, const PDynRec& r, int lane, APut& a) {
  const int ee = (lane >> 2) & 3, j = lane & 3;
  // an end-effector the robot does not have takes the structure's dummy records (every offset = its trash entry, no
  // duration columns): the select is on the index, nothing is done to the loaded values
  const bool has_ee = ee < w.n_ee;
  const uint32_t im = has_ee ? (r.imjf & 0xFFFFu) : (uint32_t)(w.n_mput + ee), jf = has_ee ? (r.imjf >> 16) : (uint32_t)(w.n_fput + ee);
  const char* pm = reinterpret_cast<const char*>(w.mput) + sizeof(PhasePutM) * (size_t)im + 16 * j;
  const char* pf = reinterpret_cast<const char*>(w.fput) + sizeof(PhasePutF) * (size_t)jf + 24 * j;
  const char* pe = reinterpret_cast<const char*>(w.ee) + sizeof(PhaseEe) * (size_t)ee;
  aload(a.pm, pm);
#pragma unroll
  for (int q = 0; q < 3; ++q) aload(a.pf[q], pf + 8 * q);
  aload(a.pe[0], pe);
  aload(a.pe[1], pe + 16);
}
template <int N>
TWR_DEV void pdyn_wait_put(APut& a, PDynPut& pu) {
  asm volatile("s_waitcnt %6" : "+a"(a.pm), "+a"(a.pf[0]), "+a"(a.pf[1]), "+a"(a.pf[2]), "+a"(a.pe[0]), "+a"(a.pe[1]) : "n"(vmcnt_imm(N)) : "memory");
  pu.pm[0] = __float_as_uint(a.pm.x); pu.pm[1] = __float_as_uint(a.pm.y); pu.pm[2] = __float_as_uint(a.pm.z); pu.pm[3] = __float_as_uint(a.pm.w);
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    pu.pf[2 * q] = (uint32_t)__double2loint(a.pf[q]);
    pu.pf[2 * q + 1] = (uint32_t)__double2hiint(a.pf[q]);
  }
  pu.ns = (int32_t)__float_as_uint(a.pe[0].x);
  pu.dur_ang[0] = (int32_t)__float_as_uint(a.pe[0].y); pu.dur_ang[1] = (int32_t)__float_as_uint(a.pe[0].z); pu.dur_ang[2] = (int32_t)__float_as_uint(a.pe[0].w);
  pu.dur_lin[0] = (int32_t)__float_as_uint(a.pe[1].x); pu.dur_lin[1] = (int32_t)__float_as_uint(a.pe[1].y); pu.dur_lin[2] = (int32_t)__float_as_uint(a.pe[1].z);
}
// One pass, first half: the math of lane (n, e, j); its share of the constraint values goes straight to global memory.
struct PDynVals {      // what the put half needs
  double wPj, wVj, wAj, wmj, wfj, f[3], rv[3];
  double F[3], mass;                     // e = 3: base-lin block
  double A[3], B[3], C[3];               // e < 3: base-ang factors of Euler dimension e
  double ap[3], ac[3], fprev[3], fcur[3];   // duration columns: angular rows (previous phases / current phase), forces
};
TWR_DEV void pdyn_math(const PDynWork& w, const PDynRec& r, const PDynIn& in, double* __restrict__ g, int lane, bool want_g,
                       PDynVals& V) {
  const int n = lane >> 4, ee = (lane >> 2) & 3, j = lane & 3;
  const bool live = n < w.cnt, has_ee = ee < w.n_ee;
  double (&f)[3] = V.f, (&rv)[3] = V.rv, (&F)[3] = V.F, (&fprev)[3] = V.fprev, (&fcur)[3] = V.fcur;
  double &wPj = V.wPj, &wVj = V.wVj, &wAj = V.wAj, &wmj = V.wmj, &wfj = V.wfj;
  {
    double wP[4], wV[4], wA[4];
    hermite_all(r.tb, r.iTb, wP, wV, wA);
    wPj = sel4(j, wP); wVj = sel4(j, wV); wAj = sel4(j, wA);
  }
  // base spline points (Spline::GetPoint in basis form): this lane's node value times its weight, summed over j
  double c[3], e[3], cdd[3], ed[3], edd[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c[d] = quad_sum(wPj * in.bl[d]);
    cdd[d] = quad_sum(wAj * in.bl[d]);
    e[d] = quad_sum(wPj * in.ba[d]);
    ed[d] = quad_sum(wVj * in.ba[d]);
    edd[d] = quad_sum(wAj * in.ba[d]);
  }
  // --- end-effector e: positions, forces, and the duration columns (PhaseSpline::GetJacobianOfPosWrtDurations,
  // phase_spline.cc:67-93, phase_durations.cc:126-154, polynomial.cc:236-257: dx/dT_poly is linear in the node values,
  // so it is a sum over j like the point itself)
  const uint32_t sm = slots12(r.slots_m[0], r.slots_m[1], j), sf = slots12(r.slots_f[0], r.slots_f[1], j);
  const bool shared = (r.misc >> 9) & 1, in_last = (r.misc >> 8) & 1;
  double xprev[3], xcur[3];
  auto ee_spline = [&](double t, double T, uint32_t slots, const double v[3], bool fold, double inner, double prevp, double& wj,
                       double pt[3], double prev[3], double cur[3]) {
    const double iT = 1.0 / T, iT2 = iT * iT, t2 = t * t, t3 = t2 * t;
    double wp[4], wv[4], wa[4], ct[4];
    hermite_all(t, iT, wp, wv, wa);
    // d pos / d T_poly = ct . (x0, v0, x1, v1)   (polynomial.cc:236-257, collected by node value)
    ct[0] = 6.0 * t2 * iT2 * iT - 6.0 * t3 * iT2 * iT2;
    ct[1] = 2.0 * t2 * iT2 - 2.0 * t3 * iT2 * iT;
    ct[2] = -ct[0];
    ct[3] = t2 * iT2 - 2.0 * t3 * iT2 * iT;
    if (fold) {   // stance ee-motion polynomial: p1 is the same variable as p0
      wp[0] += wp[2];
      wv[0] += wv[2];
      ct[0] += ct[2];
    }
    wj = sel4(j, wp);
    const double wvj = sel4(j, wv), ctj = sel4(j, ct);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double nv = ((slots >> (4 * d)) & 0xFu) != 0xFu ? v[d] : 0.0;
      pt[d] = quad_sum(wj * nv);
      const double vel = quad_sum(wvj * nv), dxdT = quad_sum(ctj * nv);
      const double dph = inner * (dxdT - prevp * vel);
      cur[d] = dph;
      prev[d] = -vel - (in_last ? dph : 0.0);
    }
  };
  {
    double p[3];
    ee_spline(r.tm, r.Tm, sm, in.m, shared, 1.0 / (double)((r.misc >> 16) & 0xF), (double)((r.misc >> 20) & 0xF), wmj, p, xprev, xcur);
    ee_spline(r.tf, r.Tf, sf, in.f, false, 1.0 / (double)((r.misc >> 24) & 0xF), (double)(r.misc >> 28), wfj, f, fprev, fcur);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      rv[d] = c[d] - p[d];
      if (!has_ee) f[d] = 0.0;
    }
  }
  // force and torque sums over the end-effectors (single_rigid_body_dynamics.cc:81-88): over the four quads of the row
  double tau[3];
  {
    double t3[3];
    cross3(f, rv, t3);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      F[d] = row4_sum(f[d]);
      tau[d] = row4_sum(t3[d]);
    }
  }
  // --- rotation: lanes j = 0..2 of a quad evaluate one sincos each and broadcast it (rotation_quad, written out: the call moves the assembly)
  double my_s, my_c;
  sincos_fast(sel3(j, e[0], e[1], e[2]), &my_s, &my_c);
  const double sx = quad_perm<0x00>(my_s), cx = quad_perm<0x00>(my_c);
  const double sy = quad_perm<0x55>(my_s), cy = quad_perm<0x55>(my_c);
  const double sz = quad_perm<0xAA>(my_s), cz = quad_perm<0xAA>(my_c);
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
    double Tm[3][3];  // R I_b
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
  double Iw_wd[3], Iw_w[3];
  symmul(Iw6, omd, Iw_wd);
  symmul(Iw6, om, Iw_w);
  const double m = H->mass;
  if (want_g && live && ee < 2 && j < 3) {  // GetDynamicViolation, single_rigid_body_dynamics.cc:76-101: one value per lane
    double wxIw[3];
    cross3(om, Iw_w, wxIw);
    const double ga = sel3(j, Iw_wd[0] + wxIw[0] - tau[0], Iw_wd[1] + wxIw[1] - tau[1], Iw_wd[2] + wxIw[2] - tau[2]);
    const double gl = sel3(j, m * cdd[0] - F[0], m * cdd[1] - F[1], m * cdd[2] - F[2] + m * H->gravity);
    g[w.g_off + 6 * n + 3 * ee + j] = ee == 0 ? ga : gl;
  }
  V.mass = m;
  {  // duration columns {[r]x J_f + [f]x J_p ; -J_f} of ee e (dynamic_constraint.cc:107-113)
    double t1[3], t2[3];
    cross3(rv, fprev, t1);
    cross3(f, xprev, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) V.ap[i] = t1[i] + t2[i];
    cross3(rv, fcur, t1);
    cross3(f, xcur, t2);
#pragma unroll
    for (int i = 0; i < 3; ++i) V.ac[i] = t1[i] + t2[i];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) V.A[i] = V.B[i] = V.C[i] = 0.0;
  if (ee < 3) {
    // --- base-ang block (:123-165), Euler dimension d = e, node value j, factored.
    // The columns of M are the rotation axes of the ZYX sequence, so dR/d e_d = [M_d]x R
    // (the cell-wise derivatives of euler_converter.cc:241-268 in closed form) and
    //   d(I_w v)/d e_d = R_d I_b R^T v + R I_b R_d^T v = M_d x (I_w v) + I_w (v x M_d)
    // (jac11+jac12 resp. jac21+jac22 of the reference) without ever forming R_d.
    const int role = ee;
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
      // d omega_dot / d edot_d
      dwd_ed[i] = sel3(role, Mdx[i], Mdy[i] + xd * dMx_dy[i], xd * dMx_dz[i] + yd * dMy_dz[i]);
      // d omega / d e_d , d omega_dot / d e_d   (roll: none)   (euler_converter.cc:168-198,270-304)
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
    double (&A)[3] = V.A, (&B)[3] = V.B, (&C)[3] = V.C;
    symmul(Iw6, Md, C);
    {  // B_d = I_w d(omega_dot)/d(edot_d) + M_d x (I_w omega) + omega x (I_w M_d)
      double t1[3], t2[3], t3b[3];
      symmul(Iw6, dwd_ed, t1);
      cross3(Md, Iw_w, t2);
      cross3(om, C, t3b);
#pragma unroll
      for (int i = 0; i < 3; ++i) B[i] = t1[i] + t2[i] + t3b[i];
    }
    {  // A_d = dI_w(omega_dot) + I_w d(omega_dot) + d(omega) x I_w omega + omega x (dI_w(omega) + I_w d(omega))
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
  }
}
// One pass, second half: the Jacobian values of lane (n, e, j) into the LDS image (`img`: byte address of the image's
// first value).
TWR_DEV void pdyn_puts(const PDynWork& w, const PDynRec& r, const PDynPut& pu, const PDynVals& V, char* __restrict__ img, int lane) {
  const int n = lane >> 4, ee = (lane >> 2) & 3, j = lane & 3;
  if (n >= w.cnt) return;
  const double (&f)[3] = V.f, (&rv)[3] = V.rv, (&F)[3] = V.F;
  const double wPj = V.wPj, wVj = V.wVj, wAj = V.wAj, wmj = V.wmj, wfj = V.wfj, m = V.mass;
  char* nb = img + (size_t)n * (size_t)w.node_vals * 8;   // first value of this time node
  // --- ee-motion block [f]x J_p (:181-192) and ee-force block {[r]x J_f ; -J_f} (:167-179), candidates (j, D), BEFORE
  // the base blocks: a candidate that is not a variable carries the offset of a base-ang entry of row AX, which the
  // base-ang stores below overwrite (same wave, program order)
#define TWR_EE_TILE3(D, R1, R2)                           \
  {                                                       \
    lds_put(nb, pu.m(2 * D + 0), crs<R1, D>(f) * wmj);    \
    lds_put(nb, pu.m(2 * D + 1), crs<R2, D>(f) * wmj);    \
    lds_put(nb, pu.f(3 * D + 0), crs<R1, D>(rv) * wfj);   \
    lds_put(nb, pu.f(3 * D + 1), crs<R2, D>(rv) * wfj);   \
    lds_put(nb, pu.f(3 * D + 2), -wfj);                   \
  }
  TWR_EE_TILE3(0, 1, 2)
  TWR_EE_TILE3(1, 2, 0)
  TWR_EE_TILE3(2, 0, 1)
#undef TWR_EE_TILE3
  {  // duration columns of ee e, phases p = j, j + 4, ...: `prev` for the phases before the current one, `cur` for it,
     // zero (the cleared image) after it
    const int cur = (int)(r.misc & 0xFF), n_dur = min(cur + 1, pu.ns);
    for (int p = j; p < n_dur; p += 4) {
      const bool is_cur = p == cur;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        lds_put(nb, (uint32_t)(pu.dur_ang[q] + 8 * p), is_cur ? V.ac[q] : V.ap[q]);
        lds_put(nb, (uint32_t)(pu.dur_lin[q] + 8 * p), is_cur ? -V.fcur[q] : -V.fprev[q]);
      }
    }
  }
  char* row[3] = {nb, nb + w.row_off[0], nb + w.row_off[1]};
  if (ee == 3) {   // base-lin block, node value j: ang rows -sum_i [f_i]x J_pos, lin rows m J_acc (:103-121)
    const uint32_t rl0 = w.row_off[2], rl1 = w.row_off[3], rl2 = w.row_off[4];
    lds_put(row[0], 8 * (2 * j + 0), -crs<0, 1>(F) * wPj);
    lds_put(row[0], 8 * (2 * j + 1), -crs<0, 2>(F) * wPj);
    lds_put(row[1], 8 * (2 * j + 0), -crs<1, 0>(F) * wPj);
    lds_put(row[1], 8 * (2 * j + 1), -crs<1, 2>(F) * wPj);
    lds_put(row[2], 8 * (2 * j + 0), -crs<2, 0>(F) * wPj);
    lds_put(row[2], 8 * (2 * j + 1), -crs<2, 1>(F) * wPj);
    lds_put(nb + rl0, 8 * j, m * wAj);
    lds_put(nb + rl1, 8 * j, m * wAj);
    lds_put(nb + rl2, 8 * j, m * wAj);
  } else {         // base-ang block, Euler dimension e, node value j
#pragma unroll
    for (int q = 0; q < 3; ++q) lds_put(row[q], 8 * (8 + 3 * j + ee), V.A[q] * wPj + V.B[q] * wVj + V.C[q] * wAj);
  }
}

// LDS: the image of one pass (dynamic size).  State at the top of iteration i: the record and the x values of pass i have
// landed.  Vector-memory operations of one iteration, in issue order (loads by hand, see aload):
//   P  put offsets of pass i (6 loads)        R  record of pass i+1 (6 loads)
//   .. clear the image, math of pass i ..     G  constraint values (1 store, WANT_G)
//   wait P (younger: R, G)  .. puts ..        wait R (younger: G)
//   X  x values of pass i+1 (12 loads)        S  copy-out of pass i (NIT stores + at most 2)
//   wait X (younger: S)
template <int NIT, bool WANT_G, bool WANT_J>   // NIT: store instructions of the copy-out (40: images of up to 40 KB, C3 sizes; 0: run-time)
__global__ __launch_bounds__(64, 1) void dyn_phase_kernel(const PDynWork* __restrict__ work, int n_work,
                                                          const double* __restrict__ x, double* __restrict__ g,
                                                          double* __restrict__ jac) {
  extern __shared__ __attribute__((aligned(16))) double pdyn_lds[];
  const int lane = threadIdx.x;
  const int stride = gridDim.x;
  int i = blockIdx.x;
  if (i >= n_work) return;
  PDynWork w0 = work[i], w1 = w0;
  const int n_ee = w0.n_ee;   // (all problems of a batch share n_ee)
  PDynRec r0;
  PDynIn in;
  {
    ARec ar;
    AIn ai;
    pdyn_issue_rec(w0.shared, w0.loc, w0.loc_stride, w0.cnt, n_ee, lane, ar);
    pdyn_wait_rec<0>(ar, r0);
    pdyn_issue_in(w0, r0, x, lane, ai);
    pdyn_wait_in<0>(ai, in);
  }
  for (; i < n_work; i += stride) {
    const bool has1 = i + stride < n_work;   // (the last pass of a workgroup prefetches itself once more: harmless)
    if (has1) w1 = work[i + stride];
    APut ap;
    ARec ar;
    AIn ai;
    if (WANT_J) pdyn_issue_put(w0, r0, lane, ap);                                   // P
    pdyn_issue_rec(w1.shared, w1.loc, w1.loc_stride, w1.cnt, n_ee, lane, ar);                      // R
    const int nv = w0.cnt * w0.node_vals;
    if (WANT_J) lds_clear(pdyn_lds, nv, lane);
    PDynVals V;
    pdyn_math(w0, r0, in, g, lane, WANT_G, V);                                      // (G inside)
    if (WANT_J) {
      PDynPut pu;
      pdyn_wait_put<6 + (WANT_G ? 1 : 0)>(ap, pu);
      pdyn_puts(w0, r0, pu, V, reinterpret_cast<char*>(pdyn_lds), lane);
    }
    PDynRec r1;
    pdyn_wait_rec<(WANT_G ? 1 : 0)>(ar, r1);
    pdyn_issue_in(w1, r1, x, lane, ai);                                             // X
    if (WANT_J) {                                                                   // S
      double* dst = jac + w0.j_off;
      stream_out<NIT>(dst, pdyn_lds, nv, (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1), lane);
    }
    pdyn_wait_in<(WANT_J ? (NIT < 63 ? NIT : 63) : 0)>(ai, in);   // (NIT = 0: drains the copy-out)
    w0 = w1;
    r0 = r1;
  }
}
}  // namespace twr
