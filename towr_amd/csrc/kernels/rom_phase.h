#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "async_pipe.h"
#include "common.h"
#include "spline_math.h"

namespace twr {
// rangeofmotion-<ee> with optimised timings (rom_phase_kernel): the same recipe as dyn_phase_kernel.  A pass is a run of
// up to SIXTEEN consecutive time nodes of one (problem, ee) -- their expanded rows [base-lin 12 | base-ang 12 (8) | all
// ee-motion_e variables | all durations] are one contiguous slice of the value array (C3: 182 values per node, 23 KB
// per pass) -- and a time node gets FOUR lanes:
//   lane = 4 n + j:   n = time node of the pass, j = node value (p0, v0, p1, v1)
// Lane (n, j) loads the three dimensions of node value j of the base splines and of the active ee-motion polynomial
// (9 values instead of 36) and owns their Jacobian columns; spline points are DPP quad sums, the rotation algebra is
// evaluated by all four lanes.  The wave clears the LDS image of the pass, every lane stores its ~26 values (+ its share
// of the duration columns) at their final positions, and the image goes to HBM with 16-byte coalesced stores.
// The x-dependent lookup comes from the pre-pass (RomRec); the pipeline is scheduled by hand like dyn_phase_kernel's.
struct ARomIn {        // x values of a pass (9 loads)
  double v[9];
};
struct RomPRec {       // the RomRec written by the pre-pass, whole dwords
  double tb, iTb, tm, iTm;
  int32_t q6, xbase;
  uint32_t slots[2], pad0, pad1;   // pad0 = base_all | current phase << 16 | in_last_phase << 24, pad1 = n_in_phase | poly_in_phase << 8
  uint32_t meta;
};
struct ARomRec {
  twr_v4f q[4];
};
TWR_DEV void romp_issue_rec(uint64_t recs, int cnt, int lane, ARomRec& a) {
  const char* p = reinterpret_cast<const char*>(recs) + sizeof(RomRec) * (size_t)min(lane >> 2, cnt - 1);
#pragma unroll
  for (int q = 0; q < 4; ++q) aload(a.q[q], p + 16 * q);
}
template <int N>
TWR_DEV void romp_wait_rec(ARomRec& a, RomPRec& r) {
  asm volatile("s_waitcnt %4" : "+a"(a.q[0]), "+a"(a.q[1]), "+a"(a.q[2]), "+a"(a.q[3]) : "n"(vmcnt_imm(N)) : "memory");
  static_assert(offsetof(RomRec, q6) == 32 && offsetof(RomRec, meta) == 44 && offsetof(RomRec, slots) == 48 && offsetof(RomRec, pad) == 56,
                "RomRec dwords");
  r.tb = pdyn_f64(a.q[0].x, a.q[0].y);
  r.iTb = pdyn_f64(a.q[0].z, a.q[0].w);
  r.tm = pdyn_f64(a.q[1].x, a.q[1].y);
  r.iTm = pdyn_f64(a.q[1].z, a.q[1].w);
  r.q6 = (int32_t)__float_as_uint(a.q[2].x);
  r.xbase = (int32_t)__float_as_uint(a.q[2].y);
  r.meta = __float_as_uint(a.q[2].w);
  r.slots[0] = __float_as_uint(a.q[3].x);
  r.slots[1] = __float_as_uint(a.q[3].y);
  r.pad0 = __float_as_uint(a.q[3].z);
  r.pad1 = __float_as_uint(a.q[3].w);
}
TWR_DEV void romp_issue_in(const RomPhaseWork& w, const RomPRec& r, const double* __restrict__ x, int lane, ARomIn& a) {
  const double* xp = x + w.x_off;
  const int j = lane & 3;
  const double* xl = xp + w.off_lin + r.q6 + 3 * j;
  const double* xa = xp + w.off_ang + r.q6 + 3 * j;
  const uint32_t sm = slots12(r.slots[0], r.slots[1], j);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    aload(a.v[d], xl + d);
    aload(a.v[3 + d], xa + d);
    const uint32_t am = (sm >> (4 * d)) & 0xFu;   // an absent candidate reads slot 0, weight 0
    aload(a.v[6 + d], xp + r.xbase + (am != 0xFu ? am : 0u));
  }
}
template <int N>
TWR_DEV void romp_wait_in(ARomIn& a, double in[9]) {
  asm volatile("s_waitcnt %9" : "+a"(a.v[0]), "+a"(a.v[1]), "+a"(a.v[2]), "+a"(a.v[3]), "+a"(a.v[4]), "+a"(a.v[5]), "+a"(a.v[6]),
               "+a"(a.v[7]), "+a"(a.v[8]) : "n"(vmcnt_imm(N)) : "memory");
#pragma unroll
  for (int q = 0; q < 9; ++q) in[q] = a.v[q];
}
// RangeOfMotionConstraint::{UpdateConstraintAtInstance, UpdateJacobianAtInstance} (range_of_motion_constraint.cc:58-109)
// with the PhaseSpline Jacobians (phase_spline.cc:44-93) for lane (n, j); `img`: byte address of the image.
TWR_DEV void romp_pass(const RomPhaseWork& w, const RomPRec& r, const double in[9], char* __restrict__ img, double* __restrict__ g,
                       int lane, bool want_g, bool want_j) {
  const int n = lane >> 2, j = lane & 3;
  const bool live = n < w.cnt;
  double wPj;
  {
    double wP[4];
    hermite_pos(r.tb, r.iTb, wP);
    wPj = sel4(j, wP);
  }
  double c[3], e[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c[d] = quad_sum(wPj * in[d]);
    e[d] = quad_sum(wPj * in[3 + d]);
  }
  // ee-motion point and the duration columns of PhaseSpline::GetJacobianOfPosWrtDurations (phase_spline.cc:67-93,
  // phase_durations.cc:126-154, polynomial.cc:236-257; dx/dT_poly collected by node value: a sum over j; twin of ee_spline, dyn_phase.h)
  const uint32_t sm = slots12(r.slots[0], r.slots[1], j);
  const bool shared = meta_shared(r.meta), in_last = (r.pad0 >> 24) & 1;
  double wmj, v[3], prev[3], cur[3];
  {
    const double t = r.tm, iT = r.iTm, iT2 = iT * iT, t2 = t * t, t3 = t2 * t;
    const double inner = 1.0 / (double)(r.pad1 & 0xFF), prevp = (double)((r.pad1 >> 8) & 0xFF);
    double wp[4], wv[4], wa[4], ct[4];
    hermite_all(t, iT, wp, wv, wa);
    ct[0] = 6.0 * t2 * iT2 * iT - 6.0 * t3 * iT2 * iT2;
    ct[1] = 2.0 * t2 * iT2 - 2.0 * t3 * iT2 * iT;
    ct[2] = -ct[0];
    ct[3] = t2 * iT2 - 2.0 * t3 * iT2 * iT;
    if (shared) {   // stance ee-motion polynomial: p1 is the same variable as p0
      wp[0] += wp[2];
      wv[0] += wv[2];
      ct[0] += ct[2];
    }
    wmj = sel4(j, wp);
    const double wvj = sel4(j, wv), ctj = sel4(j, ct);
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double nv = ((sm >> (4 * d)) & 0xFu) != 0xFu ? in[6 + d] : 0.0;
      v[d] = quad_sum(wmj * nv) - c[d];
      const double vel = quad_sum(wvj * nv), dxdT = quad_sum(ctj * nv);
      const double dph = inner * (dxdT - prevp * vel);
      cur[d] = dph;
      prev[d] = -vel - (in_last ? dph : 0.0);
    }
  }
  Rot ro;
  rotation_quad(j, e, ro);
  if (want_g && live && j < 3) {   // b_R_w (p - c): one value per lane
    double gv[3];
    matTvec(ro.R, v, gv);
    g[w.g_off + 3 * n + j] = sel3(j, gv[0], gv[1], gv[2]);
  }
  if (!want_j || !live) return;
  // DerivOfRotVecMult(t, v, inverse=true) = d(R^T v)/d e_d = R^T (v x M_d)  (euler_converter.cc:223-239, see rom_item)
  double ux[3], uy[3], uz[3];
  {
    const double Mx[3] = {ro.cy * ro.cz, ro.cy * ro.sz, -ro.sy}, My[3] = {-ro.sz, ro.cz, 0.0};
    double tx[3], ty[3];
    cross3(v, Mx, tx);
    cross3(v, My, ty);
    const double tz[3] = {v[1], -v[0], 0.0};  // v x e_z
    matTvec(ro.R, tx, ux);
    matTvec(ro.R, ty, uy);
    matTvec(ro.R, tz, uz);
  }
  const int base_all = r.pad0 & 0xFFFF, cur_ph = (r.pad0 >> 16) & 0xFF;
  const uint32_t len0 = 20u + (uint32_t)(w.msize + w.ns), len1 = len0 + 4u;
  char* nb = img + (size_t)n * (size_t)w.node_vals * 8;
  char* row[3] = {nb, nb + 8u * len0, nb + 8u * (len0 + len1)};
  const uint32_t mo[3] = {20u, 24u, 24u};
  // R^T J_p of candidates (j, D), BEFORE the base blocks: a candidate that is not a variable goes to the first value of
  // row 0, which the base-lin stores below overwrite (same wave, program order)
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const uint32_t sl = (sm >> (4 * d)) & 0xFu;
    const bool valid = sl != 0xFu;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      lds_put(valid ? row[q] + 8u * (mo[q] + (uint32_t)base_all + sl) : nb, 0, ro.R[d][q] * wmj);
  }
  {  // duration columns b_R_w * GetJacobianOfPosWrtDurations (range_of_motion_constraint.cc:106-108), phases p = j, j + 4, ..:
     // `prev` for the phases before the current one, `cur` for it, zero (the cleared image) after it
    double rp[3], rc[3];
    matTvec(ro.R, prev, rp);
    matTvec(ro.R, cur, rc);
    const int n_dur = min(cur_ph + 1, w.ns);
    for (int p = j; p < n_dur; p += 4) {
      const bool is_cur = p == cur_ph;
#pragma unroll
      for (int q = 0; q < 3; ++q) lds_put(row[q], 8u * (mo[q] + (uint32_t)w.msize + (uint32_t)p), is_cur ? rc[q] : rp[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int d = 0; d < 3; ++d) lds_put(row[q], 8 * (3 * j + d), -ro.R[d][q] * wPj);  // -R^T J_c
    if (q == 0) {  // row 0 of R^T v does not depend on roll
      lds_put(row[0], 8 * (12 + 2 * j + 0), wPj * uy[0]);
      lds_put(row[0], 8 * (12 + 2 * j + 1), wPj * uz[0]);
    } else {
      lds_put(row[q], 8 * (12 + 3 * j + 0), wPj * ux[q]);
      lds_put(row[q], 8 * (12 + 3 * j + 1), wPj * uy[q]);
      lds_put(row[q], 8 * (12 + 3 * j + 2), wPj * uz[q]);
    }
  }
}
// Vector-memory operations of one iteration, in issue order:  R record of pass i+1 (4 loads)  .. clear, math ..
//   G constraint values (1 store, WANT_G)  .. puts ..  wait R (younger: G)  X x values of pass i+1 (9 loads)
//   S copy-out of pass i (NIT stores + at most 2)   wait X (younger: S)
template <int NIT, bool WANT_G, bool WANT_J>
__global__ __launch_bounds__(64, 1) void rom_phase_kernel(const RomPhaseWork* __restrict__ work, int n_work,
                                                          const double* __restrict__ x, double* __restrict__ g,
                                                          double* __restrict__ jac) {
  extern __shared__ __attribute__((aligned(16))) double romp_lds[];
  const int lane = threadIdx.x;
  const int stride = gridDim.x;
  int i = blockIdx.x;
  if (i >= n_work) return;
  RomPhaseWork w0 = work[i], w1 = w0;
  RomPRec r0;
  double in[9];
  {
    ARomRec ar;
    ARomIn ai;
    romp_issue_rec(w0.recs, w0.cnt, lane, ar);
    romp_wait_rec<0>(ar, r0);
    romp_issue_in(w0, r0, x, lane, ai);
    romp_wait_in<0>(ai, in);
  }
  for (; i < n_work; i += stride) {
    const bool has1 = i + stride < n_work;   // (the last pass of a workgroup prefetches itself once more: harmless)
    if (has1) w1 = work[i + stride];
    ARomRec ar;
    ARomIn ai;
    romp_issue_rec(w1.recs, w1.cnt, lane, ar);                                       // R
    const int nv = w0.cnt * w0.node_vals;
    if (WANT_J) lds_clear(romp_lds, nv, lane);
    romp_pass(w0, r0, in, reinterpret_cast<char*>(romp_lds), g, lane, WANT_G, WANT_J);   // (G inside)
    RomPRec r1;
    romp_wait_rec<(WANT_G ? 1 : 0)>(ar, r1);
    romp_issue_in(w1, r1, x, lane, ai);                                              // X
    if (WANT_J) {                                                                    // S
      double* dst = jac + w0.j_off;
      __builtin_amdgcn_s_setprio(3);   // six workgroups per CU: as in dyn_kernel, the streaming wave goes first (-2 %)
      stream_out<NIT>(dst, romp_lds, nv, (int)((reinterpret_cast<uintptr_t>(dst) >> 3) & 1), lane);
      __builtin_amdgcn_s_setprio(0);
    }
    romp_wait_in<(WANT_J ? (NIT < 63 ? NIT : 63) : 0)>(ai, in);   // (NIT = 0: drains the copy-out)
    w0 = w1;
    r0 = r1;
  }
}
}  // namespace twr
