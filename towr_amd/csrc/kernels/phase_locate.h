#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "phase_durations.h"
#include "spline_math.h"

namespace twr {
// Optimised timings (PhaseSpline): with Parameters::OptimizePhaseDurations the active polynomial of every ee spline depends on x and every
// Jacobian row of an ee spline holds all variables of its set (phase_spline.cc:44-51), most of them explicit zeros; the duration
// columns come on top (dynamic_constraint.cc:107-113, range_of_motion_constraint.cc:106-108).  Three kernels: phase_locate_kernel
// resolves what depends on x in the index work (durations -> active polynomials, local times, current phase) into per-(time node, ee) records;
// dyn_phase_kernel and rom_phase_kernel then evaluate the same math as the fixed-timing kernels with more lanes per
// time node, assemble the EXPANDED rows of a few time nodes in LDS (clear, store every value at its final position)
// and stream them out, so every byte of the Jacobian -- zeros included -- is written to HBM exactly once.

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
}  // namespace twr
