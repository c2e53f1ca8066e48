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
// kernels/*.h hold every kernel of this unit, each header with its own includes; this file includes them in the order of
// their definitions, names the instantiations (the lookups) and issues the launches of one evaluation (launch_eval):
//   common.h device-function macro, diagnostic puts, nan_max, tbl / gptr / cptr      host_launch.h twr_launch, twr_first, pick (host only)
//   spline_math.h Hermite weights, candidates, sincos_fast, Rot, quad permutes     rom_item.h RomX, rom_item
//   terrain.h Terr, terrain_eval, gridmap_sample, force_core   copy_out.h copy_out, copy_out_fixed, the pipelining
//   dyn.h dyn_kernel, dyn_uniform_kernel                       rom.h rom_body (rom_kernel itself: rom_tu.hip)
//   node.h node_kernel, node_kernel2      node_chunk.h node_chunk_kernel      fused.h eval_fused_kernel
//   values.h eval_values_kernel, eval_scores_kernel, score_fold_kernel
//   phase_durations.h phase_poly_durations_wave      async_pipe.h aload, vmcnt_imm, row4_sum, lds_clear, stream_out (both phase kernels)
//   dyn_phase.h dyn_phase_kernel      phase_locate.h phase_locate_kernel (their pre-pass)      rom_phase.h rom_phase_kernel
// Sibling units: rom_tu.hip (rom_kernel, with its own scheduling strategy) and util_tu.hip (sampling, score_kernel, best_kernel, contact
// plan, nearest plane, TWR_EVAL_CHECK, each with its launch_* function; launch_eval calls launch_score and launch_best through launch.h).
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
#include "kernels/phase_durations.h"
#include "kernels/async_pipe.h"
#include "kernels/dyn_phase.h"
#include "kernels/phase_locate.h"
#include "kernels/rom_phase.h"

namespace twr {

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
