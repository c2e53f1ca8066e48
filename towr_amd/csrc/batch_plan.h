// A batch planned on the host (no HIP): which structure's layout tables a batch reads, its store policy, and everything
// twr_batch_create uploads besides the structures' tables (BatchPlan).  batch_plan.cc.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "eval_plan.h"
#include "structure.h"

namespace twr {

// Layout tables of dyn_kernel stored once per distinct CONTENT (device_tables.h): for every structure and every entry of its
// dyn_layout_tables, which structure's copy a batch reads -- the first one of the list with the same bytes (itself if none).
// Host logic only (no device): PlanBatch turns {owner, offset} into device addresses.
struct LayoutShare {
  struct Ref {
    int owner;          // index into the structure list
    uint32_t off;       // byte offset of the table inside the OWNER's blob
  };
  std::vector<std::vector<Ref>> of;     // [structure][i] for dyn_layout_tables[i]
  int64_t bytes_built = 0, bytes_distinct = 0;
};
LayoutShare ShareLayoutTables(const std::vector<const Structure*>& structs);
// Store policy of a batch (kernels/copy_out.h copy_out_fixed): non-temporal stores for SWEEP-LIKE batches -- fewer than
// four problems per structure on average, so that every evaluation re-reads tables and x that only one problem uses -- whose
// evaluation writes more than the Infinity Cache holds, so that plain stores would flush those tables out of it.
// The memory-side cache is a property of the DEVICE the batch lives on (HIP reports no field for it -- hipDeviceProp_t has
// l2CacheSize, the per-XCD L2 --, so it is a table by architecture name; a partitioned device, CPX / NPS4, sees its share):
//   gfx950 (MI350X / MI355X), gfx942 (MI300X / MI300A / MI325X): 256 MB;  anything else: eight times the L2 it reports
//   (a conservative stand-in: plain stores are the safe policy, they are never more than a few percent behind on a sweep,
//   while non-temporal stores cost rom_kernel 10-15 % where nothing needs protecting).
inline int64_t MemorySideCacheBytes(const char* gcn_arch_name, int64_t l2_bytes, int compute_partitions = 1) {
  const std::string arch = gcn_arch_name ? gcn_arch_name : "";
  int64_t bytes = 8 * l2_bytes;
  if (arch.rfind("gfx950", 0) == 0 || arch.rfind("gfx942", 0) == 0) bytes = (int64_t)256 << 20;
  return bytes / (compute_partitions > 0 ? compute_partitions : 1);
}
constexpr int64_t kInfinityCacheBytes = (int64_t)256 << 20;   // MI355X (what the measurements of DESIGN 6.R4 were taken on)
inline bool StreamNonTemporal(int structures_used, int n_problems, int64_t output_bytes_per_evaluation,
                              int64_t memory_side_cache_bytes = kInfinityCacheBytes) {
  return (int64_t)structures_used * 4 > n_problems && output_bytes_per_evaluation > memory_side_cache_bytes;
}
// Everything twr_batch_create uploads besides the structures' tables, planned on the host (no HIP): the offsets of every
// problem, every work list in launch order and the batch's policy decisions.  blob[i] is the device address of structure i's
// blob (BlobOffsets: one arena, every blob on a 256-byte line); the device enters as its CU count, its memory-side cache and
// the chunk length of node_chunk_kernel's force family (device_tables.h kForceChunk).
struct BatchPlan {
  std::vector<int64_t> x_off, g_off, j_off;   // n_problems + 1
  // what twr_batch_sample needs of every problem (the structures need not outlive the batch)
  std::vector<uint64_t> blob_of_problem;      // device blob address
  std::vector<double> t_total;                // Spline::GetTotalTime of base-lin
  std::vector<char> sample_ok;                // polynomial counts fit the sampling kernel's LDS tables
  struct Lists {
    std::vector<DynWork> dyn;                 // fixed timings; every slice of one problem on one XCD (Interleave)
    std::vector<RomWork> rom;                 // (same)
    std::vector<NodeWork> node;               // one per problem + one past the end that carries the totals
    std::vector<FlatWork> flat;               // groups of four per problem; empty when a problem cannot take the values-only path
    std::vector<FamWork> fam[4];              // chunk lists of node_chunk_kernel (large batches only)
    std::vector<PDynWork> pdyn;               // optimised timings (XCD order as dyn)
    std::vector<LocWork> ploc;
    std::vector<RomPhaseWork> prom;
    // candidate scoring without g (score_fused only; device_tables.h kScorePartial).  The scoring launch runs the flat groups
    // in the order of `flat`, then one workgroup per problem for the node-based sets; wave w of workgroup b writes partial
    // record 4 b + w of the slab.  Per problem, the fold reads score_slot[score_first[p] .. score_first[p + 1]) in that order:
    // its flat items in the order the structure lists them (empty items left out), then its node waves.
    std::vector<uint64_t> score_blob;         // per flat group: the blob of its problem (the score record, kScoreOff)
    std::vector<int32_t> score_first;         // n_problems + 1
    std::vector<int32_t> score_slot;
  } lists;
  // Scratch for the x-dependent DynLoc / RomRec records of the optimised-timings problems.  The lists hold byte offsets into it
  // until PlaceRecords(scratch address) turns them into addresses; LocWork::recs / dyn_loc store offset + 1 meanwhile, since
  // 0 there means "no such array".
  size_t records_bytes = 0;
  void PlaceRecords(uint64_t base);
  int rom_max_vals = 0;        // Jacobian values of the largest rom slice (picks the copy-out length)
  int flat_max_x = 0;          // variables of the largest problem of the values-only path (the LDS a wave stages x in)
  int dyn_map_chunks = 2;      // 2: every dyn slice of the batch stages <= 128 doubles of x (256-byte staging maps), else 4
  // Uniform dyn list (device_tables.h DynUniform): every problem references ONE structure with fixed timings, so the dyn list
  // holds the same s slices for every problem.  s = 0 otherwise; `cols` is left to PlanEval (it depends on the grid).  The
  // list itself is the same bytes either way: a uniform launch reads the records of problem 0 only.
  DynUniform dyn_uniform = {0, 0, 0, 0, 0, 0, 0, 0};
  int node_families = 4;       // 2 when no problem has more than terrain-* / force-* work for the node kernel
  int pdyn_img_cap = 0, prom_img_cap = 0;   // doubles of the LDS images of dyn_phase_kernel / rom_phase_kernel (largest pass)
  bool stream_nt = false;      // non-temporal copy-out stores (StreamNonTemporal)
  bool score_fused = false;    // every problem takes the values-only path: twr_batch_eval_scores writes no g
  int64_t score_slab = 0;      // partial records of the scoring launch (kScorePartial doubles each)
  int64_t dyn_layout_bytes = 0, dyn_layout_distinct_bytes = 0;   // dyn_kernel's layout tables: as built / after sharing
};
std::vector<size_t> BlobOffsets(const std::vector<const Structure*>& structs);   // n + 1 arena offsets
BatchPlan PlanBatch(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem,
                    const std::vector<uint64_t>& blob, int n_cu, int64_t cache_bytes, int force_chunk);

// twr_batch_start planned on the host (no HIP): the start tables of the batch's structures, byte-identical ones stored once,
// each on a 256-byte line of `tables` (device memory of its own: the blobs and the arena are not touched), and the work list --
// per problem, in problem order, its variables cut into runs of kStartItem; no item crosses a problem.  The list depends on the
// structures (table_of_struct[i]: Structure::start_table of structure i), the x offsets and the blob addresses only.
// StartWork::table holds the byte offset inside `tables` until Place(device address of tables).
struct StartPlan {
  std::vector<char> tables;
  std::vector<StartWork> work;
  int64_t bytes_built = 0, bytes_distinct = 0;   // start tables as the structures hold them / as stored
  void Place(uint64_t base);
};
StartPlan PlanStart(const std::vector<const std::vector<char>*>& table_of_struct, const std::vector<int32_t>& struct_of_problem,
                    const std::vector<int64_t>& x_off, const std::vector<uint64_t>& blob_of_problem);

// The shape of one call, assembled in ONE place for twr_batch_eval, the scoring entry points and twr_batch_eval_plan (and the
// host checks of the plans): the list counts as the batch holds them on the device, the policy PlanBatch decided, the request.
// `flags`: TWR_EVAL_* bits of an evaluation, or kEvalScores (| kEvalBest).  A scoring request records no per-kernel events and
// plans its fall-back evaluation without the uniform dyn list (its launches are the general kernels').
struct EvalCounts {
  int dyn = 0, rom = 0, node = 0, flat = 0, fam[4] = {0, 0, 0, 0}, pdyn = 0, ploc = 0, prom = 0;
};
EvalCounts CountsOf(const BatchPlan& plan);   // of a plan that still holds its lists (node: without the end entry)
EvalShape MakeEvalShape(const BatchPlan& plan, const EvalCounts& counts, int n_cu, int flags, bool events, const LaunchTuning& tuning);

}  // namespace twr
