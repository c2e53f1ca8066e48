// HIP kernels (gfx950 / CDNA4) for towr's NLP constraint + Jacobian callback.
//
// Three launches per callback batch (dynamic, range of motion, node-based sets), one stream; batches of up to 8192
// rom slices run the same three bodies as block roles of ONE launch (eval_fused_kernel).
// A dyn/rom workgroup is one wavefront (64 lanes); it walks a strided list of work items, each one a
// *contiguous* slice of one problem's CSR value array.  Every lane computes its rows in registers (FP64, no MFMA: the
// work is 3x3 algebra), scatters the values into an LDS image of the slice at the CSR position they have in
// global memory, and the wave then streams the image out with 16-byte coalesced stores.
// x-independent index work (active polynomial, local time, node->column maps, CSR
// offsets) comes from the per-lane records of device_tables.h.  The dyn/rom kernels are
// software pipelined over their work list: while slice i is computed and stored, the record of
// slice i+2 and the x values of slice i+1 are already in flight, so the only exposed memory
// latency per slice is the LDS round trip.
//
// Math follows the reference line by line in meaning (citations per function); the
// arithmetic is re-associated (Hermite basis form, factored base-ang tile) and agrees
// with the reference formulas to rounding, tests/ pin that at <= 1e-9.
//
// kernels/*.h hold the kernels up to the values-only ones, each header with its own includes; this file includes them in the
// order of their definitions, still holds the optimised-timings and utility kernels, and names the instantiations:
//   common.h TWR_DEV, diagnostic puts, tbl / gptr / cptr      host_launch.h twr_launch, twr_first, pick (host only)
//   spline_math.h Hermite weights, candidates, sincos_fast, Rot, quad permutes     rom_item.h RomX, rom_item
//   terrain.h Terr, terrain_eval, gridmap_sample, force_core   copy_out.h copy_out, copy_out_fixed, the pipelining
//   dyn.h dyn_kernel, dyn_uniform_kernel                       rom.h rom_body (rom_kernel itself: rom_tu.hip)
//   node.h node_kernel, node_kernel2      node_chunk.h node_chunk_kernel      fused.h eval_fused_kernel
//   values.h eval_values_kernel, eval_scores_kernel, score_fold_kernel
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "launch.h"

#include "kernels/common.h"
#include "kernels/host_launch.h"
#include "kernels/spline_math.h"
#include "kernels/rom_item.h"
#include "kernels/terrain.h"
#include "kernels/copy_out.h"
#include "kernels/dyn.h"
#include "kernels/rom.h"
#include "kernels/node.h"
#include "kernels/node_chunk.h"
#include "kernels/fused.h"
#include "kernels/values.h"

namespace twr {

// ---------------------------------------------------------------- optimised timings (PhaseSpline) kernels
// With Parameters::OptimizePhaseDurations the active polynomial of every ee spline depends on x and every
// Jacobian row of an ee spline holds all variables of its set (phase_spline.cc:44-51), most of them
// explicit zeros; the duration columns come on top (dynamic_constraint.cc:107-113,
// range_of_motion_constraint.cc:106-108).  Three kernels: phase_locate_kernel resolves what depends on x in the index
// work (durations -> active polynomials, local times, current phase) into per-(time node, ee) records;
// dyn_phase_kernel and rom_phase_kernel then evaluate the same math as the fixed-timing kernels with more lanes per
// time node, assemble the EXPANDED rows of a few time nodes in LDS (clear, store every value at its final position)
// and stream them out, so every byte of the Jacobian -- zeros included -- is written to HBM exactly once.
// PhaseDurations::SetVariables (phase_durations.cc:77-103) + ConvertPhaseToPolyDurations
// (nodes_variables_phase_based.cc:73-84) of one ee, spread over the lanes of a wave: loads in parallel, only the
// duration sum is serial.
TWR_DEV void phase_poly_durations_wave(const PhaseTables* PT, const char* blob, const double* __restrict__ xp, int e,
                                       double* ph, double* md, int lane, int nthreads = 64) {
  const int ns = PT->n_phases[e] - 1;
  if (lane < ns) ph[lane] = xp[PT->off_sched[e] + lane];
  __syncthreads();
  if (lane == 0) {
    double sum = 0.0;
    for (int i = 0; i < ns; ++i) sum += ph[i];
    ph[ns] = PT->t_total[e] - sum;
  }
  __syncthreads();
  const PhasePoly* mp = tbl<PhasePoly>(blob, PT->o_mpoly[e]);
  for (int q = lane; q < PT->n_mpoly[e]; q += nthreads) md[q] = ph[mp[q].phase] / mp[q].n_in_phase;
  __syncthreads();
}

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
TWR_DEV double pdyn_f64(float lo, float hi) { return __hiloint2double((int)__float_as_uint(hi), (int)__float_as_uint(lo)); }
struct PDynIn {        // per lane: what depends on the record (second stage of the pipeline)
  double bl[3], ba[3], m[3], f[3];   // node value j (3 dimensions) of base-lin / base-ang and of ee e's polynomials
};
struct PDynPut {       // per lane: where its values go (loaded at the top of the pass, used at its end), whole dwords
  uint32_t pm[4], pf[6];             // 16-bit put offsets of candidates (j, D): index 2 D + r resp. 3 D + r
  int32_t ns, dur_ang[3], dur_lin[3];
  TWR_DEV uint32_t m(int q) const { return (pm[q >> 1] >> (16 * (q & 1))) & 0xFFFFu; }
  TWR_DEV uint32_t f(int q) const { return (pf[q >> 1] >> (16 * (q & 1))) & 0xFFFFu; }
};
TWR_DEV double sel4(int i, const double v[4]) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }
// sum over the four quads of a 16-lane row (lanes l, l-4, l-8, l-12 mod 16): DPP row_ror
TWR_DEV double row_perm_ror4(double v) { return quad_perm<0x124>(v); }
TWR_DEV double row_perm_ror8(double v) { return quad_perm<0x128>(v); }
TWR_DEV double row4_sum(double v) {
  v += row_perm_ror4(v);
  v += row_perm_ror8(v);
  return v;
}
// --- asynchronous loads.  The software pipeline of dyn_phase_kernel is scheduled by hand: its vector loads are issued
// as asm into AGPRs (free at one wave per SIMD) and waited for with explicit counted s_waitcnt, always inside the
// iteration that issued them.  Left to the compiler the prefetched values are shuffled between register files right
// after the loads are issued (which waits for them on the spot), and every wait behind the copy-out drains its stores.
// The compiler sees none of these loads; a value is used only through the wait that follows its load (`+a` operands),
// and the compiler's own waits (scalar loads, LDS) are unaffected.
typedef float twr_v4f __attribute__((ext_vector_type(4)));
TWR_DEV void aload(double& d, const void* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
TWR_DEV void aload(twr_v4f& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
TWR_DEV void aload(uint32_t& d, const void* p) { asm volatile("global_load_dword %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt / lgkmcnt fields left at "no wait")
constexpr int vmcnt_imm(int n) { return (n & 0xF) | (0x7 << 4) | (0xF << 8) | ((n >> 4) << 14); }
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
  const uint32_t sm = (uint32_t)((((uint64_t)r.slots_m[1] << 32) | r.slots_m[0]) >> (12 * j)) & 0xFFFu;
  const uint32_t sf = (uint32_t)((((uint64_t)r.slots_f[1] << 32) | r.slots_f[0]) >> (12 * j)) & 0xFFFu;
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
  const uint32_t sm = (uint32_t)((((uint64_t)r.slots_m[1] << 32) | r.slots_m[0]) >> (12 * j)) & 0xFFFu;
  const uint32_t sf = (uint32_t)((((uint64_t)r.slots_f[1] << 32) | r.slots_f[0]) >> (12 * j)) & 0xFFFu;
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
  // --- rotation: lanes j = 0..2 of a quad evaluate one sincos each and broadcast it
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
// zero [0, n) doubles of an LDS image (n rounded up to a pair): eight 16-byte stores per lane and round, lanes past the
// end re-clear the last pair
TWR_DEV void lds_clear(double* __restrict__ img, int n, int lane) {
  const double2 z = {0.0, 0.0};
  const int npairs = (n + 1) >> 1, nit = (npairs + 63) >> 6;
  for (int it0 = 0; it0 < nit; it0 += 8) {
#pragma unroll
    for (int b = 0; b < 8; ++b) reinterpret_cast<double2*>(img)[min(lane + 64 * (it0 + b), npairs - 1)] = z;
  }
}
// image -> HBM for a run-time length: batches of eight 16-byte LDS reads, then their eight stores; iterations past the
// end re-store the last complete pair (idempotent).  The image is NOT shifted by the parity of the destination (it fills
// the workgroup's LDS to the last byte): a 16-byte aligned global pair is read from an 8-byte aligned LDS address with
// ds_read2_b64.  The batch is staged in AGPRs (DS and vector-memory instructions take them as data operands; the kernel
// runs few waves per SIMD, so they are free), which leaves the arch VGPRs to the math -- left to the register
// allocator the eight reads end up serialised through one VGPR quad.  Written as asm for that reason; the waits are
// explicit (the compiler's own s_waitcnt counts stay conservative: unknown younger operations only make them stricter).
// NIT > 0: compile-time number of store instructions (the wait for the loads issued before them can then be counted);
// NIT = 0: run-time length (images larger than 40 KB).  At most two more stores follow (odd head / tail).
template <int NIT>
TWR_DEV void stream_out(double* __restrict__ dst, const double* __restrict__ stage, int n, int par, int lane) {
  char* al = reinterpret_cast<char*>(dst - par);  // 16-byte aligned; global pair t = image values 2t - par, 2t + 1 - par
  const int total = n + par;
  const uint32_t last = (uint32_t)((total >> 1) - 1) * 16u;
  const uint32_t first = (uint32_t)(par + lane) * 16u;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)stage - 8u * (uint32_t)par;
  constexpr int kB = 8;
  auto batch = [&](int it0) {
    uint32_t off[kB];
    twr_v4f v[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) {
      off[b] = min(first + 1024u * (uint32_t)(it0 + b), last);
      asm volatile("ds_read2_b64 %0, %1 offset1:1" : "=a"(v[b]) : "v"(lds0 + off[b]) : "memory");
    }
#pragma unroll
    for (int b = 0; b < kB; ++b) {
      switch (kB - 1 - b) {   // the b-th read has landed once at most kB-1-b younger ones are outstanding
        case 7: asm volatile("s_waitcnt lgkmcnt(7)" : "+a"(v[b])); break;
        case 6: asm volatile("s_waitcnt lgkmcnt(6)" : "+a"(v[b])); break;
        case 5: asm volatile("s_waitcnt lgkmcnt(5)" : "+a"(v[b])); break;
        case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+a"(v[b])); break;
        case 3: asm volatile("s_waitcnt lgkmcnt(3)" : "+a"(v[b])); break;
        case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+a"(v[b])); break;
        case 1: asm volatile("s_waitcnt lgkmcnt(1)" : "+a"(v[b])); break;
        default: asm volatile("s_waitcnt lgkmcnt(0)" : "+a"(v[b])); break;
      }
      asm volatile("global_store_dwordx4 %0, %1, %2" : : "v"(off[b]), "a"(v[b]), "s"(al) : "memory");
    }
  };
  if constexpr (NIT > 0) {
    static_assert(NIT % kB == 0, "whole batches");
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += kB) batch(it0);
  } else {
    const int nit = ((total >> 1) - par + 63) >> 6;
    for (int it0 = 0; it0 < nit; it0 += kB) batch(it0);
  }
  if (par && lane == 0 && n > 0) dst[0] = stage[0];
  if ((total & 1) && lane == 0 && total - 1 > par) dst[n - 1] = stage[n - 1];
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

// Optimised timings, pre-pass: one workgroup per (problem, ee) resolves the x-dependent part of every time node of
// the dynamic and the rangeofmotion-<ee> grids -- phase and polynomial durations, active polynomials, local times,
// current phase (PhaseDurations::SetVariables, ConvertPhaseToPolyDurations, Spline::GetSegmentID / GetLocalTime) -- into
// DynLoc / RomRec records in the batch's scratch buffer.  256 threads, one per time node: a lookup is a chain of ~60
// dependent LDS reads (the reference's sequential accumulation, kept bit for bit), so the kernel lives on waves in flight
// (one wave per workgroup, four time nodes per lane: 0.094 ms per 2048 C3 problems; this form: see DESIGN 6.0).
__global__ __launch_bounds__(kLocateThreads) void phase_locate_kernel(const LocWork* __restrict__ work, const double* __restrict__ x) {
  __shared__ double s_ph[TWR_MAX_PHASES_DEV], s_md[kMaxPhasePolys], s_fd[kMaxPhasePolys];
  // the records of one block of time nodes are staged in LDS and leave as one contiguous, fully coalesced stream
  // (a lane storing its own 64-byte record touches 32 lines per store instruction)
  __shared__ __attribute__((aligned(16))) char s_rec[kLocateThreads * 64];
  static_assert(sizeof(DynLoc) == 64 && sizeof(RomRec) == 64, "record staging");
  const LocWork lw = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(lw.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const PhaseTables* PT = tbl<PhaseTables>(blob, H->o_phase);
  const int lane = threadIdx.x, e = lw.ee;
  phase_poly_durations_wave(PT, blob, x + lw.x_off, e, s_ph, s_md, lane, kLocateThreads);
  const PhasePoly* mp = tbl<PhasePoly>(blob, PT->o_mpoly[e]);
  const int last_phase = PT->n_phases[e] - 1;
  auto flush = [&](char* dst, int n_recs) {   // s_rec[0 .. 64 n_recs) -> dst, 16 bytes per thread and round
    __syncthreads();
    for (int c = lane; c < 4 * n_recs; c += kLocateThreads)
      reinterpret_cast<uint4*>(dst)[c] = reinterpret_cast<const uint4*>(s_rec)[c];
    __syncthreads();
  };
  if (lw.dyn_loc) {
    const PhasePoly* fp = tbl<PhasePoly>(blob, PT->o_fpoly[e]);
    for (int q = lane; q < PT->n_fpoly[e]; q += kLocateThreads) s_fd[q] = s_ph[fp[q].phase] / fp[q].n_in_phase;
    __syncthreads();
    const double* tg = tbl<double>(blob, PT->o_tdyn);
    const int K = PT->k_dyn;
    for (int k0 = 0; k0 < K; k0 += kLocateThreads) {
      const int k = k0 + lane;
      if (k < K) {
        const double t = tg[k];
        double tlm, tlf, tlp;
        const int qm = locate_segment(s_md, PT->n_mpoly[e], t, tlm);
        const int qf = locate_segment(s_fd, PT->n_fpoly[e], t, tlf);
        const int cur = locate_segment(s_ph, PT->n_phases[e], t, tlp);
        const PhasePoly pm = mp[qm], pf = fp[qf];
        DynLoc o;
        o.tm = tlm; o.Tm = s_md[qm];
        o.tf = tlf; o.Tf = s_fd[qf];
        o.xbase_m = pm.xbase; o.xbase_f = pf.xbase;
        const uint64_t sm = slots_of(pm.cand), sf = slots_of(pf.cand);
        o.slots_m[0] = (uint32_t)sm; o.slots_m[1] = (uint32_t)(sm >> 32);
        o.slots_f[0] = (uint32_t)sf; o.slots_f[1] = (uint32_t)(sf >> 32);
        o.im = (uint16_t)(PT->mput_base[e] + qm); o.jf = (uint16_t)(PT->fput_base[e] + qf);
        o.cur = (uint8_t)cur;
        o.flags = (uint8_t)((cur == last_phase ? 1 : 0) | (meta_shared(pm.meta) ? 2 : 0));
        o.np_m = (uint8_t)(pm.n_in_phase | (pm.poly_in_phase << 4));
        o.np_f = (uint8_t)(pf.n_in_phase | (pf.poly_in_phase << 4));
        reinterpret_cast<DynLoc*>(s_rec)[lane] = o;
      }
      flush(reinterpret_cast<char*>(lw.dyn_loc) + sizeof(DynLoc) * (size_t)k0, min(kLocateThreads, K - k0));
    }
  }
  if (!lw.recs) return;
  const double* tg = tbl<double>(blob, PT->o_trom);
  const RomRec* base = tbl<RomRec>(blob, PT->o_rom_recs[e]);  // base-spline part (tb, iTb, q6) is x-independent
  const int K = PT->k_rom;
  for (int k0 = 0; k0 < K; k0 += kLocateThreads) {
    const int k = k0 + lane;
    if (k < K) {
      const double t = tg[k];
      double tlm, tlp;
      const int qm = locate_segment(s_md, PT->n_mpoly[e], t, tlm);
      const int cur = locate_segment(s_ph, PT->n_phases[e], t, tlp);
      const PhasePoly pm = mp[qm];
      RomRec r = base[k];
      r.tm = tlm;
      r.iTm = 1.0 / s_md[qm];
      r.xbase = pm.xbase;
      r.meta = pm.meta;
      const uint64_t slots = slots_of(pm.cand);
      r.slots[0] = (uint32_t)slots;
      r.slots[1] = (uint32_t)(slots >> 32);
      r.voff = 0;
      r.pad[0] = (uint32_t)pm.base_all | ((uint32_t)cur << 16) | ((cur == last_phase ? 1u : 0u) << 24);
      r.pad[1] = (uint32_t)pm.n_in_phase | ((uint32_t)pm.poly_in_phase << 8);
      reinterpret_cast<RomRec*>(s_rec)[lane] = r;
    }
    flush(reinterpret_cast<char*>(lw.recs) + sizeof(RomRec) * (size_t)k0, min(kLocateThreads, K - k0));
  }
}

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
  const uint32_t sm = (uint32_t)((((uint64_t)r.slots[1] << 32) | r.slots[0]) >> (12 * j)) & 0xFFFu;
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
  // phase_durations.cc:126-154, polynomial.cc:236-257; dx/dT_poly collected by node value: a sum over j)
  const uint32_t sm = (uint32_t)((((uint64_t)r.slots[1] << 32) | r.slots[0]) >> (12 * j)) & 0xFFFu;
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
  // rotation: lanes j = 0..2 of the quad evaluate one sincos each and broadcast it (euler_converter.cc:207-221)
  Rot ro;
  {
    double my_s, my_c;
    sincos_fast(sel3(j, e[0], e[1], e[2]), &my_s, &my_c);
    const double sx = quad_perm<0x00>(my_s), cx = quad_perm<0x00>(my_c);
    const double sy = quad_perm<0x55>(my_s), cy = quad_perm<0x55>(my_c);
    const double sz = quad_perm<0xAA>(my_s), cz = quad_perm<0xAA>(my_c);
    ro.sx = sx; ro.cx = cx; ro.sy = sy; ro.cy = cy; ro.sz = sz; ro.cz = cz;
    ro.R[0][0] = cy * cz; ro.R[0][1] = cz * sx * sy - cx * sz; ro.R[0][2] = sx * sz + cx * cz * sy;
    ro.R[1][0] = cy * sz; ro.R[1][1] = cx * cz + sx * sy * sz; ro.R[1][2] = cx * sy * sz - cz * sx;
    ro.R[2][0] = -sy;     ro.R[2][1] = cy * sx;                ro.R[2][2] = cx * cy;
  }
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

// ---------------------------------------------------------------- trajectory sampling
// fpowr::GetTrajectory (fpowr/include/fpowr/footstep_plan_extractor.h:19-53) for a batch of solutions: lane =
// sample.  Durations (constants of the structure, or recomputed from x with optimised timings) go to LDS once
// per workgroup; every lane accumulates its sample time like the reference (t += dt), locates the active
// polynomial of every spline and evaluates position / velocity / acceleration in Hermite basis form.
TWR_DEV void sample_spline(const double* __restrict__ xp, const PolyDesc& pd, double tl, double T, double p[3], double v[3],
                           double a[3]) {
  double X[12], nv[4][3], wp[4], wv[4], wa[4];
  gather12c(xp, pd.xbase, pd.cand, X);
  node_values(slots_of(pd.cand), meta_shared(pd.meta), X, nv);
  hermite_all(tl, 1.0 / T, wp, wv, wa);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p[d] = wp[0] * nv[0][d] + wp[1] * nv[1][d] + wp[2] * nv[2][d] + wp[3] * nv[3][d];
    v[d] = wv[0] * nv[0][d] + wv[1] * nv[1][d] + wv[2] * nv[2][d] + wv[3] * nv[3][d];
    a[d] = wa[0] * nv[0][d] + wa[1] * nv[1][d] + wa[2] * nv[2][d] + wa[3] * nv[3][d];
  }
}
// With `times` set the kernel is fpowr::ExtractInitialGuess (fpowr/include/fpowr/initial_guess_extractor.h:17-34)
// instead: sample s of every problem is taken at times[s] and the record is [ t | state: base-lin p, base-ang p (Euler
// angles), base-lin v, base-ang v (Euler rates) | controls (36): ee-motion acceleration of ee i at 3 i, twelve zeros
// ("joint torques"), ee-force of ee i at 24 + 3 i ] = 49 doubles.
__global__ __launch_bounds__(64) void sample_kernel(const SampleWork* __restrict__ work, const double* __restrict__ x,
                                                    double* __restrict__ out, double dt, const double* __restrict__ times) {
  __shared__ double s_bd[2 * kMaxPhasePolys], s_ph[kMaxEE][TWR_MAX_PHASES_DEV], s_md[kMaxEE][kMaxPhasePolys],
      s_fd[kMaxEE][kMaxPhasePolys];
  const SampleWork sw = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(sw.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const SampleTables* ST = tbl<SampleTables>(blob, H->o_sample);
  const double* xp = x + sw.x_off;
  const int lane = threadIdx.x, n_ee = H->n_ee;
  for (int q = lane; q < ST->n_base; q += 64) s_bd[q] = tbl<double>(blob, ST->o_bdur)[q];
  for (int e = 0; e < n_ee; ++e) {
    if (H->timings) {  // PhaseDurations::SetVariables + ConvertPhaseToPolyDurations (phase_durations.cc:77-103)
      const PhaseTables* PT = tbl<PhaseTables>(blob, H->o_phase);
      phase_poly_durations_wave(PT, blob, xp, e, s_ph[e], s_md[e], lane);
      const PhasePoly* fp = tbl<PhasePoly>(blob, PT->o_fpoly[e]);
      for (int q = lane; q < PT->n_fpoly[e]; q += 64) s_fd[e][q] = s_ph[e][fp[q].phase] / fp[q].n_in_phase;
    } else {
      for (int q = lane; q < ST->n_phases[e]; q += 64) s_ph[e][q] = tbl<double>(blob, ST->o_phdur[e])[q];
      for (int q = lane; q < ST->n_mpoly[e]; q += 64) s_md[e][q] = tbl<double>(blob, ST->o_mdur[e])[q];
      for (int q = lane; q < ST->n_fpoly[e]; q += 64) s_fd[e][q] = tbl<double>(blob, ST->o_fdur[e])[q];
    }
  }
  __syncthreads();
  if (lane >= sw.cnt) return;
  const int s_idx = sw.s0 + lane;
  double t = 0.0;
  if (times) t = times[s_idx];
  else for (int i = 0; i < s_idx; ++i) t += dt;   // the reference's accumulated sample time
  const int rec = times ? 49 : 20 + 13 * n_ee;
  double* o = out + sw.out_off + (int64_t)s_idx * rec;
  o[0] = t;
  // base-lin / base-ang (NodesVariablesAll: [p0 v0 p1 v1] x 3 of polynomial q at 6 q)
  double tl;
  const int qb = locate_segment(s_bd, ST->n_base, t, tl);
  double wp[4], wv[4], wa[4];
  hermite_all(tl, 1.0 / s_bd[qb], wp, wv, wa);
  const double* xl = xp + ST->off_lin + 6 * qb;
  const double* xa = xp + ST->off_ang + 6 * qb;
  double e3[3], ed[3], edd[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    o[1 + d] = wp[0] * xl[d] + wp[1] * xl[3 + d] + wp[2] * xl[6 + d] + wp[3] * xl[9 + d];
    o[4 + d] = wv[0] * xl[d] + wv[1] * xl[3 + d] + wv[2] * xl[6 + d] + wv[3] * xl[9 + d];
    o[7 + d] = wa[0] * xl[d] + wa[1] * xl[3 + d] + wa[2] * xl[6 + d] + wa[3] * xl[9 + d];
    e3[d] = wp[0] * xa[d] + wp[1] * xa[3 + d] + wp[2] * xa[6 + d] + wp[3] * xa[9 + d];
    ed[d] = wv[0] * xa[d] + wv[1] * xa[3 + d] + wv[2] * xa[6 + d] + wv[3] * xa[9 + d];
    edd[d] = wa[0] * xa[d] + wa[1] * xa[3 + d] + wa[2] * xa[6 + d] + wa[3] * xa[9 + d];
  }
  if (times) {   // ExtractInitialGuess record
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double lv = o[4 + d];
      o[4 + d] = e3[d];
      o[7 + d] = lv;
      o[10 + d] = ed[d];
    }
    for (int q = 13; q < 49; ++q) o[q] = 0.0;
    for (int e = 0; e < n_ee; ++e) {
      double tlm, tlf, p[3], v[3], a[3];
      const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
      const int qf = locate_segment(s_fd[e], ST->n_fpoly[e], t, tlf);
      sample_spline(xp, tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm], tlm, s_md[e][qm], p, v, a);
#pragma unroll
      for (int d = 0; d < 3; ++d) o[13 + 3 * e + d] = a[d];
      sample_spline(xp, tbl<PolyDesc>(blob, ST->o_fdesc[e])[qf], tlf, s_fd[e][qf], p, v, a);
#pragma unroll
      for (int d = 0; d < 3; ++d) o[37 + 3 * e + d] = p[d];
    }
    return;
  }
  Rot ro;
  rotation(e3, ro);
  {  // Eigen::Quaterniond(R) (euler_converter.cc:51-56; Eigen 3.3 Quaternion.h, quaternionbase_assign_impl)
    const double (&m)[3][3] = ro.R;
    double q[4];  // x y z w
    double tr = m[0][0] + m[1][1] + m[2][2];
    if (tr > 0) {
      tr = sqrt(tr + 1.0);
      q[3] = 0.5 * tr;
      tr = 0.5 / tr;
      q[0] = (m[2][1] - m[1][2]) * tr;
      q[1] = (m[0][2] - m[2][0]) * tr;
      q[2] = (m[1][0] - m[0][1]) * tr;
    } else {
      int i = 0;
      if (m[1][1] > m[0][0]) i = 1;
      if (m[2][2] > (i == 0 ? m[0][0] : m[1][1])) i = 2;
      const int j = (i + 1) % 3, k = (j + 1) % 3;
      auto M = [&](int r, int c) { return sel3(r, sel3(c, m[0][0], m[0][1], m[0][2]), sel3(c, m[1][0], m[1][1], m[1][2]),
                                               sel3(c, m[2][0], m[2][1], m[2][2])); };
      tr = sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
      const double qi = 0.5 * tr;
      tr = 0.5 / tr;
      const double qw = (M(k, j) - M(j, k)) * tr, qj = (M(j, i) + M(i, j)) * tr, qk = (M(k, i) + M(i, k)) * tr;
      q[3] = qw;
      q[0] = i == 0 ? qi : (j == 0 ? qj : qk);
      q[1] = i == 1 ? qi : (j == 1 ? qj : qk);
      q[2] = i == 2 ? qi : (j == 2 ? qj : qk);
    }
    o[10] = q[3]; o[11] = q[0]; o[12] = q[1]; o[13] = q[2];
  }
  {  // omega = M edot, omega_dot = Mdot edot + M eddot (euler_converter.cc:58-83,133-166)
    const double sy = ro.sy, cy = ro.cy, sz = ro.sz, cz = ro.cz;
    const double xd = ed[0], yd = ed[1], zd = ed[2];
    const double Mx[3] = {cy * cz, cy * sz, -sy}, My[3] = {-sz, cz, 0.0};
    const double Mdx[3] = {-cz * sy * yd - cy * sz * zd, cy * cz * zd - sy * sz * yd, -cy * yd};
    const double Mdy[3] = {-cz * zd, -sz * zd, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o[14 + i] = Mx[i] * xd + My[i] * yd + (i == 2 ? zd : 0.0);
      o[17 + i] = Mdx[i] * xd + Mdy[i] * yd + Mx[i] * edd[0] + My[i] * edd[1] + (i == 2 ? edd[2] : 0.0);
    }
  }
  for (int e = 0; e < n_ee; ++e) {
    double* oe = o + 20 + 13 * e;
    double tlp, tlm, tlf;
    const int phase = locate_segment(s_ph[e], ST->n_phases[e], t, tlp);   // PhaseDurations::IsContactPhase
    oe[0] = ((phase & 1) == 0) == (ST->contact0[e] != 0) ? 1.0 : 0.0;
    const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
    const int qf = locate_segment(s_fd[e], ST->n_fpoly[e], t, tlf);
    const PolyDesc pm = tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm];
    const PolyDesc pf = tbl<PolyDesc>(blob, ST->o_fdesc[e])[qf];
    double p[3], v[3], a[3];
    sample_spline(xp, pm, tlm, s_md[e][qm], p, v, a);
#pragma unroll
    for (int d = 0; d < 3; ++d) { oe[1 + d] = p[d]; oe[4 + d] = v[d]; oe[7 + d] = a[d]; }
    sample_spline(xp, pf, tlf, s_fd[e][qf], p, v, a);
#pragma unroll
    for (int d = 0; d < 3; ++d) oe[10 + d] = p[d];
  }
}
hipError_t launch_sample(const SampleWork* work, int n_work, const double* x, double* out, double dt, const double* times,
                         hipStream_t stream) {
  if (n_work <= 0) return hipSuccess;
  return twr_launch(sample_kernel, dim3(n_work), dim3(64), 0, stream, work, x, out, dt, times);
}

// ---------------------------------------------------------------- candidate scoring
// twr_batch_score: per problem and constraint family the inf- and 1-norm of the bound violation
// max(lower - g, g - upper, 0) over the family's rows (bounds of ConstraintSet::GetBounds, twr_structure_bounds).
// A sweep then returns 16 doubles per candidate instead of its Jacobian.
// (round 5: 256 threads per problem, row r = 256 k + thread, sixteen rows per thread; family slot and bounds of a row come
// from its 16-bit meta word and the structure's short table of distinct (lower, upper) pairs, device_tables.h ScoreTables.)
// Two dependent round trips: (1) the work item and its successor (row count = difference of their g offsets; the list
// carries an end entry), (2) the rows of g, the meta words of the rows AND the head of the score record (2 KB requested on spec:
// the pair table) -> LDS -- the record sits at a fixed offset of the blob (kScoreOff), no field of the header is needed.  The slot of a thread's rows never falls, so it keeps one
// running (max, sum) pair and hands it to its LDS cell when the slot moves on.  Round 4's kernel fetched a cold candidate's
// fields one s_load at a time and 16 bytes of bounds per row: 25 us for 128 candidates, 43 us for 1024.
__device__ __forceinline__ void best_of(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
__global__ __launch_bounds__(256) void score_kernel(const NodeWork* __restrict__ work, const double* __restrict__ g,
                                                    double* __restrict__ scores) {
  constexpr int kHeadDwords = kScoreHeadBytes / 4, kTabDwords = (int)(sizeof(ScoreTables) / 4);
  static_assert(kHeadDwords == 512 && kTabDwords + 4 * kScoreMaxPairs <= kHeadDwords, "the whole record within its head: two loads per thread");
  __shared__ __attribute__((aligned(16))) int32_t s_tab[kHeadDwords];   // the record as in the blob
  __shared__ double red[256 * 16 + 16 * 16];   // cell (2 slot + {max, sum}, thread), then the partial results of the fold
  const int tid = threadIdx.x;
  const NodeWork w = work[blockIdx.x];
  const int n_rows = (int)(work[blockIdx.x + 1].g_off - w.g_off);
  if (n_rows <= 0) {   // (uniform) a structure whose constraint sets have no rows: nothing is violated, nothing is read
    if (tid < 16) scores[16 * (size_t)blockIdx.x + tid] = 0.0;
    return;
  }
  const double* gp = g + w.g_off;
  const char* blob = reinterpret_cast<const char*>(w.blob);
#pragma unroll
  for (int c = 0; c < 16; ++c) red[c * 256 + tid] = 0.0;   // (a cell is written at most once more; own cells only: no barrier)
  int cur = 0;
  double cm = 0.0, cs = 0.0;
  for (int base = 0; base < n_rows; base += 16 * 256) {   // (one trip for structures of up to 4096 rows)
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = gp[min(base + 256 * k + tid, n_rows - 1)];
    const int32_t* Tw = reinterpret_cast<const int32_t*>(tbl<ScoreTables>(blob, kScoreOff));   // (fixed offset: no header field)
    const uint16_t* meta = reinterpret_cast<const uint16_t*>(blob + kScoreOff + kScoreHeadBytes);
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = meta[min(base + 256 * k + tid, n_rows - 1)];
    if (base == 0) {
      const int32_t a = Tw[tid], c = Tw[tid + 256];
      s_tab[tid] = a;
      s_tab[tid + 256] = c;
      __syncthreads();
    }
    const double* s_pairs = reinterpret_cast<const double*>(s_tab + kTabDwords);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (base + 256 * k < n_rows) {   // uniform
        const bool live = base + 256 * k + tid < n_rows;
        const int slot = (int)(m[k] >> 12), q = (int)(m[k] & 0xFFFu);
        const double lo = s_pairs[2 * q], up = s_pairs[2 * q + 1], val = v[k];
        // NaN-propagating: a non-finite constraint value makes the family's scores NaN instead of hiding in a max()
        double viol = fmax(fmax(lo - val, val - up), 0.0);
        if (val != val) viol = val;
        if (live && slot != cur) {   // the slot moved on: hand over the running pair (rare: a few times per thread)
          red[(2 * cur) * 256 + tid] = cm;
          red[(2 * cur + 1) * 256 + tid] = cs;
          cm = cs = 0.0;
          cur = slot;
        }
        if (live) {
          cm = nan_max(cm, viol);
          cs += viol;
        }
      }
    }
  }
  red[(2 * cur) * 256 + tid] = cm;
  red[(2 * cur + 1) * 256 + tid] = cs;
  // 256 threads x 16 cells -> 16 values, transposed: thread 16 c + j folds column j of threads c, c + 16, ..., then sixteen
  // threads fold the sixteen partial results of their column and store it at its FAMILY's place
  __syncthreads();
  {
    const int j = tid & 15, c = tid >> 4;   // column j (even: an inf-norm, odd: a 1-norm)
    double acc = red[j * 256 + c];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      const double o = red[j * 256 + c + 16 * i];
      acc = (j & 1) ? acc + o : nan_max(acc, o);
    }
    red[256 * 16 + c * 16 + j] = acc;
  }
  __syncthreads();
  if (tid < 16) {
    const int slot = reinterpret_cast<const int8_t*>(s_tab + 2)[tid >> 1];   // ScoreTables::slot_of_family[family tid / 2]
    double acc = 0.0;
    if (slot >= 0) {
      const int j = 2 * slot + (tid & 1);
      acc = red[256 * 16 + j];
      for (int c = 1; c < 16; ++c) {
        const double o = red[256 * 16 + c * 16 + j];
        acc = (tid & 1) ? acc + o : nan_max(acc, o);
      }
    }
    scores[16 * (size_t)blockIdx.x + tid] = acc;
  }
}
hipError_t launch_score(const NodeWork* work, int n_problems, const double* g, double* scores, hipStream_t stream) {
  return twr_launch(score_kernel, dim3(n_problems), dim3(256), 0, stream, work, g, scores);
}

// twr_batch_best: the planner's decision on the device -- arg-min over a score table of the summed inf-norm violations of
// the chosen constraint families (the table may be longer than this batch: after an all-gather it holds the candidates of
// every rank).  Same rule as towr_amd.dist.best_candidate: families summed in ascending order, NaN loses, first index wins
// a tie.  One launch: every block reduces its stride of candidates, the last block to finish reduces the blocks' results
// (threadfence + counter, reset for the next call) and writes best[0] = index, best[1] = its total.
__global__ __launch_bounds__(256) void best_kernel(const double* __restrict__ scores, int n, unsigned families, double* __restrict__ partial,
                                                   unsigned* __restrict__ counter, double* __restrict__ best, double index_offset) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  __shared__ bool s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double bv = __builtin_inf();
  int bi = 0x7fffffff;
  for (int c = blockIdx.x * 256 + tid; c < n; c += gridDim.x * 256) {
    const double* row = scores + 16 * (size_t)c;
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (families >> f & 1u) {
        t = first ? row[2 * f] : t + row[2 * f];
        first = false;
      }
    if (t != t) t = __builtin_inf();
    best_of(bv, bi, t, c);
  }
  auto block_reduce = [&]() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best_of(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
    if (lane == 0) {
      s_v[wave] = bv;
      s_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < 4; ++w) best_of(bv, bi, s_v[w], s_i[w]);
  };
  block_reduce();
  if (tid == 0) {
    partial[2 * blockIdx.x] = bv;
    partial[2 * blockIdx.x + 1] = (double)bi;
    __threadfence();
    s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  bv = __builtin_inf();
  bi = 0x7fffffff;
  for (int k = tid; k < (int)gridDim.x; k += 256)
    best_of(bv, bi, __builtin_nontemporal_load(partial + 2 * k), (int)__builtin_nontemporal_load(partial + 2 * k + 1));
  __syncthreads();
  block_reduce();
  if (tid == 0) {
    best[0] = index_offset + (double)(bi == 0x7fffffff ? 0 : bi);
    best[1] = bv;
    *counter = 0u;
  }
}
int best_max_blocks() { return 256; }
hipError_t launch_best(const double* scores, int n, unsigned families, double* partial, unsigned* counter, double* best, double index_offset,
                       hipStream_t stream) {
  int blocks = (n + 1023) / 1024;   // >= four candidates per thread before another block pays
  blocks = blocks < 1 ? 1 : (blocks > best_max_blocks() ? best_max_blocks() : blocks);
  return twr_launch(best_kernel, dim3(blocks), dim3(256), 0, stream, scores, n, families, partial, counter, best, index_offset);
}

// ---------------------------------------------------------------- contact plan
// fpowr::ExtractFootstepPlan (fpowr/include/fpowr/footstep_plan_extractor.h:69-133) minus the nearest-plane lookup
// (boost::geometry over ROS messages, left to the caller): the solution is sampled every dt like GetTrajectory
// (t accumulated), a footstep state is the first sample and every sample whose contact flags differ from the
// previous sample's (HasEndEffectorContactChanged, :55-67); its duration is the time to the next footstep state, the
// last one lasts until time_horizon (:121-128).  One wave per problem, lane = sample, 64 samples per round, footstep
// states compacted with a ballot.  Record: [ t | duration | contact per ee | ee-motion position (3) per ee ].
__global__ __launch_bounds__(64) void contact_plan_kernel(const NodeWork* __restrict__ work, const double* __restrict__ x,
                                                          double* __restrict__ out, int32_t* __restrict__ counts, double dt,
                                                          double time_horizon, int n_samples_max, int max_steps) {
  __shared__ double s_ph[kMaxEE][TWR_MAX_PHASES_DEV], s_md[kMaxEE][kMaxPhasePolys];
  const NodeWork w = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(w.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const SampleTables* ST = tbl<SampleTables>(blob, H->o_sample);
  const double* xp = x + w.x_off;
  const int lane = threadIdx.x, n_ee = H->n_ee;
  for (int e = 0; e < n_ee; ++e) {
    if (H->timings) {  // PhaseDurations::SetVariables + ConvertPhaseToPolyDurations (phase_durations.cc:77-103)
      phase_poly_durations_wave(tbl<PhaseTables>(blob, H->o_phase), blob, xp, e, s_ph[e], s_md[e], lane);
    } else {
      for (int q = lane; q < ST->n_phases[e]; q += 64) s_ph[e][q] = tbl<double>(blob, ST->o_phdur[e])[q];
      for (int q = lane; q < ST->n_mpoly[e]; q += 64) s_md[e][q] = tbl<double>(blob, ST->o_mdur[e])[q];
    }
  }
  __syncthreads();
  // GetTrajectory: while (t <= T + 1e-5) { ...; t += dt; }
  const double T = ST->t_total;
  const int rec = 2 + 4 * n_ee;
  double* o = out + (size_t)blockIdx.x * (size_t)max_steps * rec;
  int n_steps = 0;          // wave-uniform
  double t_carry = 0.0;     // t of the last footstep state of the previous round (wave-uniform)
  for (int s0 = 0; s0 < n_samples_max; s0 += 64) {
    const int s_idx = s0 + lane;
    double t = 0.0, tq = 0.0;   // this sample's and the previous sample's accumulated time (t += dt, like the reference)
    for (int i = 0; i < s_idx; ++i) {
      tq = t;
      t += dt;
    }
    const bool live = t <= T + 1e-5;
    unsigned mask = 0, mask_prev = 0;
    for (int e = 0; e < n_ee; ++e) {  // PhaseDurations::IsContactPhase (phase_durations.cc:118-124)
      double tl;
      const int ph = locate_segment(s_ph[e], ST->n_phases[e], t, tl);
      mask |= ((((ph & 1) == 0) == (ST->contact0[e] != 0)) ? 1u : 0u) << e;
      const int pq = locate_segment(s_ph[e], ST->n_phases[e], tq, tl);
      mask_prev |= ((((pq & 1) == 0) == (ST->contact0[e] != 0)) ? 1u : 0u) << e;
    }
    const bool step = live && (s_idx == 0 || mask != mask_prev);
    const uint64_t ball = __ballot(step);
    if (ball == 0) {
      if (!__any(live)) break;
      continue;
    }
    const uint64_t below = ball & ((1ull << lane) - 1ull);
    const uint64_t above = lane == 63 ? 0ull : (ball >> (lane + 1));
    const int my = n_steps + __popcll(below);
    // time of the footstep state before this one: the closest step lane below, or the previous round's last
    const double t_below = __shfl(t, below ? 63 - __clzll(below) : lane);
    const double t_prev = below ? t_below : t_carry;
    if (step && my < max_steps) {
      double* r = o + (size_t)my * rec;
      r[0] = t;
      if (!above) r[1] = time_horizon - t;   // last footstep state so far (:125-127); a later round may close it
      for (int e = 0; e < n_ee; ++e) {
        r[2 + e] = (mask >> e) & 1u ? 1.0 : 0.0;
        double tlm;
        const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
        const PolyDesc pm = tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm];
        double p[3], v[3], a[3];
        sample_spline(xp, pm, tlm, s_md[e][qm], p, v, a);
#pragma unroll
        for (int d = 0; d < 3; ++d) r[2 + n_ee + 3 * e + d] = p[d];
      }
    }
    // duration of the state before (:121-123) -- also when THIS state no longer fits the output (my == max_steps): the
    // last record that was kept still gets its duration
    if (step && my > 0 && my - 1 < max_steps) o[(size_t)(my - 1) * rec + 1] = t - t_prev;
    t_carry = __shfl(t, 63 - __clzll(ball));
    n_steps += __popcll(ball);
  }
  if (lane == 0) counts[blockIdx.x] = n_steps;
}
hipError_t launch_contact_plan(const NodeWork* work, int n_problems, const double* x, double* out, int32_t* counts, double dt,
                               double time_horizon, int n_samples_max, int max_steps, hipStream_t stream) {
  return twr_launch(contact_plan_kernel, dim3(n_problems), dim3(64), 0, stream, work, x, out, counts, dt, time_horizon,
                    n_samples_max, max_steps);
}

// ---------------------------------------------------------------- nearest plane of a footstep
// fpowr::NearestPlaneLookup::GetNearestPlaneIndex (nearest_plane_lookup.h:62-84) for every (problem, footstep state,
// end-effector) of a contact plan: boost::geometry::distance(point, polygon) restated from Boost 1.71 (winding
// strategy for covered_by, projected-point distance to the ring's consecutive points, no closing edge added; exact
// coordinate comparisons where boost allows a few ulp).  One thread per foot, polygons read from global memory.
TWR_DEV int ring_side(const double* __restrict__ xy, int n, double px, double py) {   // 1 inside, 0 boundary, -1 outside
  if (n < 4) return -1;
  int count = 0;
  for (int i = 0; i + 1 < n; ++i) {
    const double s1x = xy[2 * i], s1y = xy[2 * i + 1], s2x = xy[2 * i + 2], s2y = xy[2 * i + 3];
    const bool eq1 = s1x == px, eq2 = s2x == px;
    int c = 0;
    if (eq1 && eq2) {
      if ((s1y <= py && s2y >= py) || (s2y <= py && s1y >= py)) return 0;
    } else {
      c = eq1 ? (s2x > px ? 1 : -1) : eq2 ? (s1x > px ? -1 : 1) : (s1x < px && s2x > px) ? 2 : (s2x < px && s1x > px) ? -2 : 0;
    }
    if (c != 0) {
      int side;
      if (c == 1 || c == -1) {
        const double sey = eq1 ? s1y : s2y;
        side = py == sey ? 0 : (py < sey ? -c : c);
      } else {
        // (no FMA contraction: the sign of a tiny determinant must not depend on it)
        const double det = __dsub_rn(__dmul_rn(s2x - s1x, py - s1y), __dmul_rn(s2y - s1y, px - s1x));
        side = det > 0 ? 1 : (det < 0 ? -1 : 0);
      }
      if (side == 0) return 0;
      if (side * c > 0) count += c;
    }
  }
  return count == 0 ? -1 : 1;
}
TWR_DEV double ring_distance(const double* __restrict__ xy, int n, double px, double py) {
  if (n == 0) return 0.0;
  auto comparable = [&](double ax, double ay, double bx, double by) {
    const double vx = bx - ax, vy = by - ay, wx = px - ax, wy = py - ay;
    const double c1 = __dadd_rn(__dmul_rn(wx, vx), __dmul_rn(wy, vy));
    if (c1 <= 0) return __dadd_rn(__dmul_rn(wx, wx), __dmul_rn(wy, wy));
    const double c2 = __dadd_rn(__dmul_rn(vx, vx), __dmul_rn(vy, vy));
    if (c2 <= c1) return __dadd_rn(__dmul_rn(px - bx, px - bx), __dmul_rn(py - by, py - by));
    const double b = c1 / c2, qx = __dadd_rn(ax, __dmul_rn(b, vx)), qy = __dadd_rn(ay, __dmul_rn(b, vy));
    return __dadd_rn(__dmul_rn(px - qx, px - qx), __dmul_rn(py - qy, py - qy));
  };
  if (n == 1) return sqrt(comparable(xy[0], xy[1], xy[0], xy[1]));
  double best = comparable(xy[0], xy[1], xy[2], xy[3]);
  for (int i = 0; i + 1 < n; ++i) {
    const double c = comparable(xy[2 * i], xy[2 * i + 1], xy[2 * i + 2], xy[2 * i + 3]);
    if (c == 0.0) return 0.0;
    if (c < best) best = c;
  }
  return sqrt(best);
}
__global__ __launch_bounds__(256) void plane_kernel(const double* __restrict__ plan, const int32_t* __restrict__ counts,
                                                    const double* __restrict__ poly_xy, const int32_t* __restrict__ poly_start,
                                                    int n_polys, int n_problems, int max_steps, int n_ee,
                                                    int32_t* __restrict__ plane_index) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n_problems * max_steps * n_ee) return;
  const int e = (int)(id % n_ee), s = (int)((id / n_ee) % max_steps), p = (int)(id / ((int64_t)n_ee * max_steps));
  const double* rec = plan + ((int64_t)p * max_steps + s) * (2 + 4 * n_ee);
  int nearest = -1;
  if (s < counts[p] && rec[2 + e] != 0.0) {
    const double px = rec[2 + n_ee + 3 * e], py = rec[2 + n_ee + 3 * e + 1];
    double min_distance = 1.7976931348623157e308;
    for (int i = 0; i < n_polys; ++i) {
      const double* xy = poly_xy + 2 * poly_start[i];
      const int n = poly_start[i + 1] - poly_start[i];
      const double distance = ring_side(xy, n, px, py) >= 0 ? 0.0 : ring_distance(xy, n, px, py);
      if (distance < min_distance) {
        min_distance = distance;
        nearest = i;
      }
    }
  }
  plane_index[id] = nearest;
}
hipError_t launch_planes(const double* plan, const int32_t* counts, const double* poly_xy, const int32_t* poly_start, int n_polys,
                         int n_problems, int max_steps, int n_ee, int32_t* plane_index, hipStream_t stream) {
  const int64_t n = (int64_t)n_problems * max_steps * n_ee;
  if (n <= 0) return hipSuccess;
  return twr_launch(plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, plan, counts, poly_xy, poly_start, n_polys,
                    n_problems, max_steps, n_ee, plane_index);
}

// ---------------------------------------------------------------- TWR_EVAL_CHECK
// Per-problem non-finite flags (failure detection): a separate pass over the outputs of one
// evaluation, off the hot path (it re-reads g and jac once).  status[p] |= 1 if a constraint value of problem p is
// NaN/Inf, |= 2 if a Jacobian value is.  Sixteen workgroups per problem, each scanning a contiguous share.
constexpr int kCheckParts = 16;
TWR_DEV bool non_finite(double v) { return (__double2hiint(v) & 0x7ff00000) == 0x7ff00000; }
__global__ __launch_bounds__(256) void check_kernel(const int64_t* __restrict__ g_off, const int64_t* __restrict__ j_off,
                                                    const double* __restrict__ g, const double* __restrict__ jac,
                                                    int32_t* __restrict__ status, int flags) {
  const int p = blockIdx.x / kCheckParts, part = blockIdx.x % kCheckParts;
  int bad = 0;
  if (flags & 1) {
    const int64_t a = g_off[p], n = g_off[p + 1] - a;
    const int64_t lo = a + n * part / kCheckParts, hi = a + n * (part + 1) / kCheckParts;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) bad |= non_finite(g[i]) ? 1 : 0;
  }
  if (flags & 2) {
    const int64_t a = j_off[p], n = j_off[p + 1] - a;
    const int64_t lo = a + n * part / kCheckParts, hi = a + n * (part + 1) / kCheckParts;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) bad |= non_finite(jac[i]) ? 2 : 0;
  }
  if (bad) atomicOr(&status[p], bad);
}
hipError_t launch_check(int n_problems, const int64_t* g_off, const int64_t* j_off, const double* g, const double* jac,
                        int32_t* status, int flags, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n_problems, stream);
  if (e != hipSuccess) return e;
  return twr_launch(check_kernel, dim3(n_problems * kCheckParts), dim3(256), 0, stream, g_off, j_off, g, jac, status, flags);
}

// The instantiation lookups of the kernels launched by launch_eval (rom_kernel's: rom_kernel_fn).  A lookup returns the
// kernel's function pointer type, taken from one instantiation (every instantiation has the same one).
using DynFn = decltype(&dyn_kernel<true, true, 2, true>);
using DynUniformFn = decltype(&dyn_uniform_kernel<true, true, 2, true>);
using FusedFn = decltype(&eval_fused_kernel<34, true, true, 2, true>);
using PDynFn = decltype(&dyn_phase_kernel<40, true, true>);
using PRomFn = decltype(&rom_phase_kernel<24, true, true>);
using ChunkFn = decltype(&node_chunk_kernel<true, true>);
using ValuesFn = decltype(&eval_values_kernel<3>);
using ScoresFn = decltype(&eval_scores_kernel<3>);
static ChunkFn node_chunk_kernel_fn(const LaunchStep& p) {
  return pick<kStores>(p.store, [&](auto st) -> ChunkFn { return node_chunk_kernel<StoreG(st), StoreJ(st)>; });
}
static ValuesFn eval_values_kernel_fn(const LaunchStep& p) {
  return pick<kValuesNx>(p.xc, [&](auto nx) -> ValuesFn { return eval_values_kernel<nx>; });
}
static ScoresFn eval_scores_kernel_fn(const LaunchStep& p) {
  return pick<kValuesNx>(p.xc, [&](auto nx) -> ScoresFn { return eval_scores_kernel<nx>; });
}
static FusedFn fused_kernel_fn(const LaunchStep& p) {
  return pick<kDynXc>(p.xc, [&](auto xc) {
    return pick<kFusedNits>(p.nit, [&](auto nit) {
      return pick<kStoresNT>(p.store, [&](auto st) -> FusedFn { return eval_fused_kernel<nit, StoreG(st), StoreJ(st), xc, StoreNT(st)>; });
    });
  });
}
static DynFn dyn_kernel_fn(const LaunchStep& p) {
  return pick<kDynXc>(p.xc, [&](auto xc) {
    return pick<kStoresNT>(p.store, [&](auto st) -> DynFn { return dyn_kernel<StoreG(st), StoreJ(st), xc, StoreNT(st)>; });
  });
}
static DynUniformFn dyn_uniform_kernel_fn(const LaunchStep& p) {
  return pick<kDynXc>(p.xc, [&](auto xc) {
    return pick<kStoresNT>(p.store, [&](auto st) -> DynUniformFn { return dyn_uniform_kernel<StoreG(st), StoreJ(st), xc, StoreNT(st)>; });
  });
}
static PDynFn dyn_phase_kernel_fn(const LaunchStep& p) {
  return pick<kDynPhaseNits>(p.nit, [&](auto nit) {
    return pick<kStores>(p.store, [&](auto st) -> PDynFn { return dyn_phase_kernel<nit, StoreG(st), StoreJ(st)>; });
  });
}
static PRomFn rom_phase_kernel_fn(const LaunchStep& p) {
  return pick<kRomPhaseNits>(p.nit, [&](auto nit) {
    return pick<kStores>(p.store, [&](auto st) -> PRomFn { return rom_phase_kernel<nit, StoreG(st), StoreJ(st)>; });
  });
}

// Host side of one evaluation: the launches eval_plan.cc PlanEval plans (policy, thresholds and the measurements behind
// them are there), issued in order on one stream.  Every launch is issued; the first error is returned.
hipError_t launch_eval(const EvalShape& s, const EvalBuffers& b, hipStream_t stream, hipEvent_t* ev) {
  const EvalPlan plan = PlanEval(s);
  const int plan_flags = (s.flags & kEvalScores) ? 1 : s.flags & 3;   // what the node kernels write (a scoring request's fallback: g)
  hipError_t st = hipSuccess;
  for (int i = 0; i < plan.n; ++i) {
    const LaunchStep& p = plan.step[i];
    const dim3 grid(p.grid), block(p.block);
    const int* a = p.arg;
    switch (p.kernel) {
      case Launch::kEvent: (void)hipEventRecord(ev[a[0]], stream); break;
      case Launch::kDyn:
        if (p.uni.s > 0) st = twr_first(st, twr_launch(dyn_uniform_kernel_fn(p), grid, block, p.lds, stream, b.dyn, p.uni, b.x, b.g, b.jac, b.dump));
        else st = twr_first(st, twr_launch(dyn_kernel_fn(p), grid, block, p.lds, stream, b.dyn, s.dyn, b.x, b.g, b.jac, b.dump));
        break;
      case Launch::kRom: st = twr_first(st, twr_launch(rom_kernel_fn(p), grid, block, p.lds, stream, b.rom, s.rom, b.x, b.g, b.jac)); break;
      case Launch::kFused:
        st = twr_first(st, twr_launch(fused_kernel_fn(p), grid, block, p.lds, stream, b.rom, s.rom, a[0], b.dyn, s.dyn, a[1], b.node, b.x, b.g,
                                      b.jac, b.dump));
        break;
      case Launch::kLocate: st = twr_first(st, twr_launch(phase_locate_kernel, grid, block, p.lds, stream, b.ploc, b.x)); break;
      case Launch::kDynPhase: st = twr_first(st, twr_launch(dyn_phase_kernel_fn(p), grid, block, p.lds, stream, b.pdyn, s.pdyn, b.x, b.g, b.jac)); break;
      case Launch::kRomPhase: st = twr_first(st, twr_launch(rom_phase_kernel_fn(p), grid, block, p.lds, stream, b.prom, s.prom, b.x, b.g, b.jac)); break;
      case Launch::kNode: st = twr_first(st, twr_launch(node_kernel, grid, block, p.lds, stream, b.node, b.x, b.g, b.jac, plan_flags)); break;
      case Launch::kNode2: st = twr_first(st, twr_launch(node_kernel2, grid, block, p.lds, stream, b.node, b.x, b.g, b.jac, plan_flags)); break;
      case Launch::kChunk:
        st = twr_first(st, twr_launch(node_chunk_kernel_fn(p), grid, block, p.lds, stream, b.fam[0], s.fam[0], a[0], b.fam[1], s.fam[1], a[1],
                                      b.fam[2], s.fam[2], a[2], b.fam[3], s.fam[3], a[3], b.x, b.g, b.jac));
        break;
      case Launch::kValues:
        st = twr_first(st, twr_launch(eval_values_kernel_fn(p), grid, block, p.lds, stream, b.flat, a[0], a[2], b.node, a[1], b.x, b.g));
        break;
      case Launch::kScores:
        st = twr_first(st, twr_launch(eval_scores_kernel_fn(p), grid, block, p.lds, stream, b.flat, b.score_blob, a[0], a[2], b.node, a[1], b.x,
                                      b.slab));
        break;
      case Launch::kFold: st = twr_first(st, twr_launch(score_fold_kernel, grid, block, p.lds, stream, b.score_first, b.score_slot, b.slab, a[0], b.scores)); break;
      case Launch::kScoreG: st = twr_first(st, launch_score(b.node, a[0], b.g, b.scores, stream)); break;
      case Launch::kBest:
        st = twr_first(st, launch_best(b.scores, a[0], b.families, b.best_partial, b.best_counter, b.best, b.index_offset, stream));
        break;
    }
  }
  return st;
}

// Images of more than 64 KB need the dynamic-LDS limit of the run-time-length instantiations raised; done when a batch
// is created (on its device, always to the whole 160 KB of a CU), not at launch: an evaluation must stay capturable
// in a hipGraph.
hipError_t prepare_phase_kernels(int pdyn_img_cap, int prom_img_cap) {
  hipError_t st = hipSuccess;
  auto raise = [&](const void* fn) { st = twr_first(st, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); };
  LaunchStep p;   // (nit 0: the run-time length)
  for (int store : kStores) {
    p.store = store;
    if (pdyn_img_cap * sizeof(double) > 64 * 1024) raise(reinterpret_cast<const void*>(dyn_phase_kernel_fn(p)));
    if (prom_img_cap * sizeof(double) > 64 * 1024) raise(reinterpret_cast<const void*>(rom_phase_kernel_fn(p)));
  }
  return st;
}

}  // namespace twr
