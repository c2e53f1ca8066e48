// The launches of one evaluation (twr_batch_eval and the scoring entry points), planned on the host (no HIP): the shape of a
// call, the launch steps PlanEval makes of it and the names of the kernel instantiations.  eval_plan.cc.
#pragma once
#include <algorithm>
#include <cstddef>   // (device_tables.h uses offsetof)
#include <string>

#include "device_tables.h"

namespace twr {

// The launches of one evaluation (twr_batch_eval), planned on the host (no HIP) from the batch's list counts and policy:
// which kernels, which instantiation of each, their grids and LDS, and where the four profiling events go.
// Tuning knobs (include/towr_amd.h): 0 leaves the decision to the rules of PlanEval.
struct LaunchTuning {
  int dyn_bpc = 8, rom_bpc = 4;   // TWR_DYN_BPC, TWR_ROM_BPC: persistent workgroups per CU
  int node_bpc = 16;              // TWR_NODE_BPC: node_chunk_kernel's waves per CU, all families together
  int pdyn_bpc = 0, prom_bpc = 0; // TWR_PDYN_BPC, TWR_PROM_BPC
  int fused_max_rom = 0;          // TWR_FUSED_MAX_ROM
  int fused_split = 0;            // TWR_FUSED_SPLIT
  int fused_grom = 0, fused_gdyn = 0;   // TWR_FUSED_GROM, TWR_FUSED_GDYN
};
struct EvalShape {
  int n_cu = 0;
  int dyn = 0, rom = 0, node = 0, flat = 0, fam[4] = {0, 0, 0, 0}, pdyn = 0, ploc = 0, prom = 0;   // work items per list
  // what PlanBatch decided for the batch (BatchPlan)
  int rom_max_vals = 0, flat_max_x = 0, dyn_map_chunks = 2, node_families = 4, pdyn_img_cap = 0, prom_img_cap = 0;
  bool stream_nt = false;
  DynUniform dyn_uniform = {0, 0, 0, 0, 0, 0, 0, 0};   // BatchPlan::dyn_uniform (s = 0: the general dyn_kernel)
  int flags = 0;                  // TWR_EVAL_VALUES | TWR_EVAL_JACOBIAN, or kEvalScores (| kEvalBest)
  bool events = false;            // per-kernel profiling events are recorded
  bool score_fused = false;       // BatchPlan::score_fused
  LaunchTuning tuning;
};
// Internal requests of EvalShape::flags (not TWR_EVAL_* values): the score table of twr_batch_score (kEvalScores), then the
// arg-min of twr_batch_best over it (kEvalBest).  Fused (score_fused): the scoring launch and the fold; otherwise the
// values-only evaluation into g and score_kernel.  Neither records per-kernel events.
constexpr int kEvalScores = 1 << 8, kEvalBest = 1 << 9;
enum class Launch { kEvent, kDyn, kRom, kFused, kLocate, kDynPhase, kRomPhase, kNode, kNode2, kChunk, kValues, kScores, kFold, kScoreG, kBest };
// Outputs a launch writes: constraint values (G), Jacobian (J), and non-temporal copy-out stores (NT, only with J).
enum StoreVariant { kStoreG, kStoreJ, kStoreGJ, kStoreJNT, kStoreGJNT };
constexpr bool StoreG(int s) { return s == kStoreG || s == kStoreGJ || s == kStoreGJNT; }
constexpr bool StoreJ(int s) { return s != kStoreG; }
constexpr bool StoreNT(int s) { return s == kStoreJNT || s == kStoreGJNT; }
// The instantiations that exist: the key lists of the kernels' lookups (kernels.hip, rom_tu.hip), in the order the code
// objects lay them out.  NIT = store instructions of a copy-out (0: run-time length), XC = 64-entry chunks of dyn_kernel's
// staging maps, NX = doubles of x per thread of eval_values_kernel.
constexpr int kStoresNT[] = {kStoreGJNT, kStoreGJ, kStoreJNT, kStoreJ, kStoreG};   // dyn, rom, fused
constexpr int kStores[] = {kStoreGJ, kStoreJ, kStoreG};                            // phase kernels, chunks
constexpr int kDynXc[] = {2, 4};                                                   // dyn, fused
constexpr int kRomNits[] = {26, 30, 34, kRomNitMax};
constexpr int kFusedNits[] = {34, kRomNitMax};
constexpr int kDynPhaseNits[] = {40, 0};
constexpr int kRomPhaseNits[] = {24, 32, 40, 0};
constexpr int kValuesNx[] = {3, 5, 8};
struct LaunchStep {
  Launch kernel = Launch::kEvent;
  int store = kStoreG, nit = 0, xc = 0;   // instantiation (xc: NX of eval_values_kernel)
  int grid = 0, block = 0, lds = 0;       // lds: dynamic LDS bytes
  // kEvent: the event; kFused: rom and dyn blocks; kChunk: blocks per family; kValues, kScores: groups, node families, x bytes;
  // kFold, kScoreG, kBest: problems
  int arg[4] = {0, 0, 0, 0};
  // kDyn of a uniform list, when the grid rule of PlanEval holds: s > 0 selects dyn_uniform_kernel, cols is filled in
  DynUniform uni = {0, 0, 0, 0, 0, 0, 0, 0};
};
// Grid of a uniform dyn launch.  The persistent grid holds W0 = grid / 8 waves per XCD; every wave owns one of the s slice
// kinds, so the grid is trimmed to W = s * (W0 / s) waves per XCD, cols = W / s problems per XCD and iteration (no more
// columns than the batch has problems for: ceil(n / 8)).  Returns 0 -- keep the general kernel -- when the trimming would
// idle more than 1/32 of the residency (W0 - W > W0 / 32): s = 16 loses nothing of 256, s = 5 keeps 255, s = 6 keeps 252.
inline int DynUniformCols(int s, int n_problems, int resident_grid) {
  const int w0 = resident_grid / 8;
  if (s <= 0 || n_problems <= 0 || w0 < s) return 0;
  const int w = s * (w0 / s);
  if (w0 - w > w0 / 32) return 0;
  return std::min(w / s, (n_problems + 7) / 8);
}
struct EvalPlan {
  static constexpr int kMaxSteps = 10;
  int n = 0;
  LaunchStep step[kMaxSteps];
};
EvalPlan PlanEval(const EvalShape& shape);
// A step as the kernel it launches and the instantiation of it, spelled as the kernels' template lists are keyed:
//   dyn_kernel<GJ,xc2>  dyn_uniform_kernel<JNT,xc4>  rom_kernel<26,GJ>  eval_fused_kernel<34,xc2,GJNT>  dyn_phase_kernel<40,J>
//   rom_phase_kernel<0,GJ>  node_chunk_kernel<G>  eval_values_kernel<3>  eval_scores_kernel<8>
// and the plain names of the kernels that have one body (node_kernel, node_kernel2, phase_locate_kernel, score_fold_kernel,
// score_kernel, best_kernel).  "" for an event.
const char* StoreName(int store);
const char* KernelName(const LaunchStep& step);
std::string InstantiationName(const LaunchStep& step);

}  // namespace twr
