// Host-side problem structure: everything about one candidate contact schedule that does
// not depend on x.  Built once (twr_structure_create); the reference spreads the same
// information over NlpFormulation::GetVariableSets/GetConstraints, NodesVariables*,
// SplineHolder and the constraint constructors (see citations in structure.cc).
#pragma once
#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/towr_amd.h"
#include "device_tables.h"

namespace twr {

struct SplineLayout {
  std::vector<double> durations;                 // per polynomial
  // x index (global, stacked) of node value (node, deriv, dim); -1 = not optimised (constant 0)
  std::vector<int> idx;                          // [node][deriv(2)][dim(3)]
  std::vector<char> node_constant;               // phase based sets only
  std::vector<int> poly_phase;                   // phase of each polynomial (phase based)
  int n_nodes = 0;
  int var_offset = 0, var_size = 0;
  int at(int node, int deriv, int dim) const { return idx[(node * 2 + deriv) * 3 + dim]; }
};

struct SetInfo {
  std::string name;
  int offset = 0, size = 0, nnz_offset = 0, nnz = 0;
};

struct TimeNode {  // result of Spline::GetLocalTime for one spline at one grid time
  int poly;
  double t_local;
};

struct TerrainGrid {   // HeightMapFromCSV (include/towr/terrain/height_map_from_csv.h) or Grid (grid_height_map.h)
  std::vector<double> heights;  // CSV: [y_cell * cols + x_cell]
  int rows = 0, cols = 0;       // CSV: rows x cols; grid_map: size_x x size_y cells
  double res = 0.17, eps = 0.17 / 50;  // CSV :112-115; grid_map: resolution, resolution / 6 (grid_height_map.h:25)
  bool grid_map = false;        // Grid: float elevation layer, column-major [i + j * size_x]
  std::vector<float> elevation;
  double pos_x = 0, pos_y = 0;  // GridMap::getPosition()
  double Height(double x, double y) const;
};

struct Structure {
  twr_model model;
  std::shared_ptr<const TerrainGrid> grid;  // TWR_TERRAIN_CSV_GRID only
  twr_schedule schedule;
  twr_params params;
  int n_ee = 0;
  double T = 0;

  SplineLayout base;  // durations shared by base-lin / base-ang; idx refers to base-lin
  int off_base_lin = 0, off_base_ang = 0;
  std::vector<SplineLayout> motion, force;
  std::vector<SetInfo> var_sets, con_sets;
  int n_vars = 0, n_rows = 0, nnz = 0;
  bool timings = false;             // TWR_SET_TOTAL_TIME: phase durations are variables
  int off_schedule[kMaxEE] = {0, 0, 0, 0};
  PhaseTables phase_tables;         // filled by BuildPattern / PackBlob when timings

  std::vector<double> grid_dyn, grid_rom, grid_bm;
  std::vector<TimeNode> dyn_base, rom_base, bm_base;
  std::vector<std::vector<TimeNode>> dyn_motion, dyn_force, rom_motion;  // [ee][k]
  std::vector<std::vector<PolyDesc>> mpoly, fpoly;                       // [ee][poly]
  std::vector<std::vector<ForceNode>> force_nodes;                       // [ee]
  std::vector<std::vector<TerrainRow>> terrain_rows;                     // [ee]
  std::vector<AccJunction> acc_junctions;                                // base spline junctions
  std::vector<std::vector<SwingNode>> swing_nodes;                       // [ee]

  std::vector<int32_t> row_ptr, col_idx;
  std::vector<double> lower, upper;

  std::vector<char> blob;  // packed DevStruct + tables (device_tables.h)
  // byte offsets of the per-lane record arrays inside the blob
  uint32_t off_dyn_shared = 0, off_dyn_lanes = 0;   // optimised timings: DynShared[k] (base-spline part)
  // fixed timings: slices of the dynamic set and their tables (device_tables.h DynNodeT / DynNodeL / DynSel / DynPolyT / DynPolyL / DynTile)
  struct DynSlice {
    int k0, cnt, nvals;
    uint32_t map;        // byte offset of the slice's staging map inside the blob: uint16[64][4], lane-transposed
    uint32_t map2;       // the two-chunk form uint16[64][2] of the same map (slices that stage <= 128 doubles; else = map)
    int poly0;           // index of the first DynPolyT / DynPolyL record the slice reads (DynSel::dm / df count from it)
  };
  std::vector<DynSlice> dyn_slices;
  int dyn_staged_max = 0;   // most doubles of x one slice stages (<= 128: the batch may use the two-chunk maps)
  uint32_t off_dyn_nodes_t = 0, off_dyn_nodes_l = 0, off_dyn_sel = 0, off_dyn_tile = 0, off_dyn_poly_t = 0, off_dyn_poly_l = 0;
  struct TableRef {
    uint32_t off, bytes;
  };
  std::vector<TableRef> dyn_layout_tables;   // the layout tables of dyn_kernel inside the blob (times excluded): what a batch may
                                             // share between structures when the bytes are identical
  uint32_t off_rom_recs[kMaxEE] = {0, 0, 0, 0};   // optimised timings: RomRec[k] templates (base-spline part)
  // fixed timings: slices of rangeofmotion-<ee> (device_tables.h RomNode / RomSeg)
  struct RomSlice {
    int k0, cnt, nvals;
    uint32_t segs;               // byte offset of the slice's RomSeg records inside the blob
    uint8_t first[kRomMaxSeg];   // first lane of every segment (255: none)
  };
  std::vector<std::vector<RomSlice>> rom_slices;   // [ee]
  uint32_t off_rom_nodes = 0;
  // values-only evaluation of dynamic / rangeofmotion-*, one lane per time node (device_tables.h FlatNode / FlatPoly /
  // FlatWork): blob offsets (0 = none) and the items of a problem of this structure (PlanBatch adds the problem's
  // addresses)
  struct FlatItem {
    int k0 = 0, cnt = 0;                 // time nodes [k0, k0 + cnt) of the grid
    uint64_t start[2] = {0, 0}, count = 0;   // FlatWork::start / count
    bool gather = false;                 // FlatWork::gather
  };
  uint32_t off_flat_polys = 0, off_flat_rom = 0, off_flat_dyn = 0;   // FlatPoly[] | FlatNode[] of the two grids
  int flat_row_dyn = 0, flat_row_rom[kMaxEE] = {0, 0, 0, 0};
  bool flat_with_rom = false;   // the two grids coincide: the "dynamic" items take the range-of-motion rows along
  std::vector<FlatItem> flat_items_rom, flat_items_dyn;

  const SetInfo* FindSet(const std::string& name) const;  // nullptr if the family is switched off
  void Build();            // throws std::runtime_error
  void BuildSizes();       // variables, time tables and CSR pattern only (n_vars / n_rows / nnz): no device tables
  void InitialGuess(const double* lin0, const double* ang0, const double* lin1, const double* ang1,
                    const double* ee0, double* x) const;
  int SampleCount(double dt) const;  // twr::SampleCount of the base spline's total time
  void VariableBounds(const double* init_base, const double* final_base, const double* ee0, double* lower,
                      double* upper) const;

 private:
  void BuildVariables();
  void BuildTimeTables();
  void BuildPattern();
  void PackBlob();
};

// gait tables
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
// Store policy of a batch (kernels.hip copy_out_fixed): non-temporal stores for SWEEP-LIKE batches -- fewer than
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
// The shape of one call, assembled in ONE place for twr_batch_eval, the scoring entry points and twr_batch_eval_plan (and the
// host checks of the plans): the list counts as the batch holds them on the device, the policy PlanBatch decided, the request.
// `flags`: TWR_EVAL_* bits of an evaluation, or kEvalScores (| kEvalBest).  A scoring request records no per-kernel events and
// plans its fall-back evaluation without the uniform dyn list (its launches are the general kernels').
struct EvalCounts {
  int dyn = 0, rom = 0, node = 0, flat = 0, fam[4] = {0, 0, 0, 0}, pdyn = 0, ploc = 0, prom = 0;
};
EvalCounts CountsOf(const BatchPlan& plan);   // of a plan that still holds its lists (node: without the end entry)
EvalShape MakeEvalShape(const BatchPlan& plan, const EvalCounts& counts, int n_cu, int flags, bool events, const LaunchTuning& tuning);
// A step as the kernel it launches and the instantiation of it, spelled as the kernels' template lists are keyed:
//   dyn_kernel<GJ,xc2>  dyn_uniform_kernel<JNT,xc4>  rom_kernel<26,GJ>  eval_fused_kernel<34,xc2,GJNT>  dyn_phase_kernel<40,J>
//   rom_phase_kernel<0,GJ>  node_chunk_kernel<G>  eval_values_kernel<3>  eval_scores_kernel<8>
// and the plain names of the kernels that have one body (node_kernel, node_kernel2, phase_locate_kernel, score_fold_kernel,
// score_kernel, best_kernel).  "" for an event.
const char* StoreName(int store);
const char* KernelName(const LaunchStep& step);
std::string InstantiationName(const LaunchStep& step);
// Products with a batch's Jacobian values (twr_jac_mul: y = J v, twr_jac_tmul: z = J^T w; jac_products.hip), planned on the host
// (no HIP).  The CSC view of a structure's CSR pattern: col_ptr[n + 1]; per entry its row and its position in the CSR value
// array, rows ascending within a column.  Throws when a row's columns do not ascend strictly (unsorted or duplicate entries)
// or leave [0, n_vars): the products rely on both.
struct CscPattern {
  std::vector<int32_t> col_ptr, row_idx, csr_pos;
};
CscPattern TransposePattern(const Structure& S);
// Work split of the two products (both: workgroups of kJacThreads lanes; every index from these tables, never from J, v or w).
//   J v:    blocks of consecutive rows, at most kJacMulRows rows and kJacMulNnz entries (a longer row is a block of its own).  The
//           block's entries are streamed with 16-byte loads, each multiplied by v[col] (v staged in LDS when n <= kJacLdsX, else
//           gathered from memory) into an LDS tile of kJacMulNnz products; the lane of a row then sums its products in column
//           order, across tiles for a longer row.
//   J^T w:  blocks of consecutive ENTRIES (rows need not be whole), at most kJacTNnz of them, kJacTCols distinct columns and rows
//           within a span of kJacTSpan.  The block's values are staged in LDS, every one multiplied by its row's w; the lane of a
//           column sums its products in row order (the block's map) into one partial of the slab; the fold then sums every
//           column's partials in block order (exact 0 for a column without entries).
// The order of every sum is a function of the pattern alone: not of the batch, the call or the device.
constexpr int kJacThreads = 256;
constexpr int kJacMulRows = 256, kJacMulNnz = 2048;
constexpr int kJacTNnz = 2048, kJacTCols = 256, kJacTSpan = 512;
constexpr int kJacLdsX = 6144;       // doubles of v jac_mul_kernel stages in LDS at most (48 KB; 64 KB with the products)
constexpr int kJacFoldCols = 256;    // columns of one fold item
// The work records (device layout; the table fields are byte offsets into JacOpsPlan::tables until Place() makes them addresses)
struct JacMulWork {     // rows [r0, r1) of one problem
  int64_t x_off, g_off, j_off;
  uint64_t col, row_ptr;           // the pattern's uint16 col[nnz], int32 row_ptr[m + 1]
  int32_t r0, r1, n, pad;          // n: variables (v is staged in LDS when n <= kJacLdsX)
};
struct JacTWork {       // entries [k0, k1) of one problem, rows [r_first, r_first + span)
  int64_t g_off, j_off, slab;      // slab: the block's first partial (its columns' partials follow in map order)
  uint64_t map, row_ptr;           // the block's uint16 lcol_ptr[ncols + 1], then uint16 pos[k1 - k0] (entry - k0, per column in
                                   // row order); the pattern's int32 row_ptr[m + 1]
  int32_t k0, k1, r_first, span, ncols, pad;
};
struct JacFoldWork {    // columns [c0, c1) of one problem
  int64_t x_off, slab;             // slab: the problem's first partial
  uint64_t ptr, slot;              // the pattern's int32 fold_ptr[n + 1], int32 fold_slot[]: column c sums
                                   // slab[fold_slot[fold_ptr[c] .. fold_ptr[c + 1])] in that order
  int32_t c0, c1;
};
struct JacOpsPlan {
  std::vector<int64_t> x_off, g_off, j_off;   // n_problems + 1: the layout of PlanBatch for the same arguments
  std::vector<char> tables;                   // every distinct pattern's tables, once (16-byte aligned)
  std::vector<int32_t> pattern_of_struct;     // the distinct pattern every structure reads
  int distinct_patterns = 0;
  std::vector<JacMulWork> mul;                // problem by problem, blocks in row order
  std::vector<JacTWork> tmul;                 // problem by problem, blocks in entry order
  std::vector<JacFoldWork> fold;
  int64_t slab = 0;                           // partials of one J^T w (doubles)
  int mul_lds_x = 0;                          // largest n <= kJacLdsX of the batch (the v jac_mul_kernel stages)
  int64_t table_bytes_mul = 0, table_bytes_tmul = 0;   // bytes of the distinct tables each product reads
  void Place(uint64_t base);                  // table offsets -> device addresses (base: where `tables` lives)
};
// (structs, struct_of_problem) as for twr_batch_create.  Byte-identical patterns (n, m, row_ptr, col_idx) share one set of tables.
JacOpsPlan PlanJacOps(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem);

// The one-pass normal product u = J^T (w o (J v)), y = J v (twr_jac_normal_mul; jac_products.hip jac_normal_kernel), planned on the
// host (no HIP): a plan of its own next to PlanJacOps, for the same arguments and in the same x / g / jac layout.
//   Blocks of consecutive WHOLE rows of one problem, at most kJacThreads rows and one tile of entries (kJacNormNnz).  The block's values are
//   streamed once into LDS, raw and multiplied by v[col]; the lane of a row sums its products in column order (y_r), forms
//   t_r = w_r y_r and multiplies the row's raw values by it; the column lanes then loop over the block's distinct columns (any
//   number of them), each summing its column's products in row order (the block's map, of the JacTWork kind) into one partial of
//   the slab; jac_fold_kernel sums every column's partials in block order (JacFoldWork, exact 0 for a column without entries).
//   A row of more than kJacNormNnz entries is a block of its own (long = 1): lane 0 sums its products tile by tile in column
//   order, then the tiles are streamed again and every entry times t_r is a partial of its own (a row's columns are distinct;
//   no map).
// The col / row_ptr tables are PlanJacOps's (offsets into JacOpsPlan::tables for the same arguments); the block maps and the
// fold tables live in `tables` here.  The order of every sum is a function of the pattern alone.
constexpr int kJacNormNnz = 2048;
struct JacNormalWork {  // rows [r0, r1) of one problem
  int64_t x_off, g_off, j_off, slab;   // slab: the block's first partial (its columns' partials follow in map order)
  uint64_t col, row_ptr;               // the pattern's tables in JacOpsPlan::tables
  uint64_t map;                        // the block's uint16 lcol_ptr[ncols + 1], then uint16 pos[entries] (entry - row_ptr[r0], per
                                       // column in row order); unused by a long row
  int32_t r0, r1, n, ncols, is_long, pad;   // ncols: partials the block writes
};
struct JacNormalPlan {
  std::vector<int64_t> x_off, g_off, j_off;   // n_problems + 1: the layout of PlanJacOps for the same arguments
  std::vector<char> tables;                   // every distinct pattern's block maps and fold tables, once (16-byte aligned)
  std::vector<JacNormalWork> work;            // problem by problem, blocks in row order
  std::vector<JacFoldWork> fold;
  int64_t slab = 0;                           // partials of one product (doubles)
  int lds_x = 0;                              // largest n <= kJacLdsX of the batch (the v the kernel stages)
  int tile = kJacNormNnz;                     // entries of one LDS tile: what the blocks were cut for
  // col / row_ptr -> addresses in the products' tables (ops_base), maps and fold tables -> addresses in `tables` (base)
  void Place(uint64_t ops_base, uint64_t base);
};
// Where the products' plan J (not yet placed) keeps the col / row_ptr tables of every distinct pattern (byte offsets into
// J.tables; 0 for a pattern without rows, which has no J v record to read them from), and the first structure that has it.
struct JacPatternPlace {
  int32_t first_struct;
  uint64_t col, row_ptr;
};
std::vector<JacPatternPlace> JacPatternPlaces(const JacOpsPlan& J, const std::vector<int32_t>& struct_of_problem);
// The plan from the distinct patterns (only n_vars, n_rows, nnz, row_ptr and col_idx of a Structure are read), the places of
// their tables and every problem's pattern: what a twr_jac_ops handle keeps.  tile: entries of one LDS tile, 1 .. kJacNormNnz
// (kJacNormNnz unless a test wants long rows out of short ones).
JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& patterns, const std::vector<JacPatternPlace>& places,
                            const std::vector<int32_t>& pattern_of_problem, int tile = kJacNormNnz);
// The same from the arguments of PlanJacOps, which it calls for the places: the unplaced JacOpsPlan of these arguments is the
// one whose tables the work records point into.
JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem,
                            int tile = kJacNormNnz);

// The Gram matrix N = J^T W J of every problem, formed once and kept (twr_jac_gram, twr_jac_gram_mul, twr_jac_lsq_solve_gram;
// jac_gram.hip), planned on the host (no HIP) for the arguments of PlanJacOps and in its x / g / jac layout.  Per distinct pattern:
//   the pattern of N = J^T J as full symmetric CSR -- int32 row_ptr[n + 1], uint16 col[nnz N], columns ascending.  Structural
//   only: an explicit zero of J counts, a column of J without entries gives an empty row and column.
//   the contribution table of the LOWER triangle (i >= j; the kernel writes the sum to (i, j) and to (j, i), so both carry the
//   same bits): the lower entries are sorted by the length of their lists, longest first (ties in CSR order), and cut into
//   slices of kGramSlice entries, one lane each.  Per sorted entry: int32 pos[] (its place in the problem's values), int32
//   mirror[] (the place of (j, i); == pos on the diagonal), int32 cnt[] (its terms).  Per slice int32 slice_ptr[]: where its
//   words start; term t of lane l is word[slice_ptr[s] + t * kGramSlice + l] (lanes of a slice read consecutive words; the
//   slice is as wide as its first, longest list, shorter lists are padded with kGramPad), terms in ascending row r:
//       word = r << 48 | position of J_ri in the CSR values << 24 | position of J_rj
//   hence the limits of the packing: at most kGramMaxRows rows and kGramMaxNnz Jacobian entries per problem.  A lane adds its
//   terms in table order: the order of every sum is a function of the pattern alone, and no list is split.
// The values of problem p start at gram_off[p] of one value array (doubles; every start on a 16-byte boundary).
// The solve keeps six vectors of n doubles and its reduction scratch in one workgroup's LDS (kGramLdsBytes, the most a single
// workgroup may have on gfx950): at most kGramMaxVars variables per problem.
// Whatever passes one of these limits makes PlanJacGram throw JacGramUnsupported (TWR_ERR_UNSUPPORTED at the C ABI).
constexpr int kGramThreads = 256;
constexpr int kGramSlice = 64;                  // lanes of one slice: a wave
constexpr int kGramRowLanes = 16;               // lanes that share a row of N in the products
constexpr int kGramMaxRows = 1 << 16;
constexpr int kGramMaxNnz = 1 << 24;
constexpr uint64_t kGramPad = ~0ull;
constexpr int kGramLdsBytes = 160 * 1024;
constexpr int kGramSolveVectors = 6;            // e, s, p, c, c o p and N (c o p)
constexpr int kGramRed = 2 * (kGramThreads / 64);   // doubles of reduction scratch
constexpr int kGramPlanThreads = 16;              // host threads PlanJacGram plans distinct patterns with, at most
constexpr int kGramMaxVars = (kGramLdsBytes / 8 - kGramRed) / kGramSolveVectors;
struct JacGramUnsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct JacGramWork {    // sorted lower entries [e0, e1) of one problem: kGramThreads / kGramSlice slices at most
  int64_t g_off, j_off, gram_off;
  uint64_t pos, mirror, cnt, slice_ptr, words;   // the pattern's tables (slice_ptr indexed by e / kGramSlice)
  int32_t e0, e1;
};
struct JacGramMulWork { // rows [r0, r1) of N of one problem
  int64_t x_off, gram_off;
  uint64_t row_ptr, col;
  int32_t r0, r1;
};
struct JacGramSolveWork {   // one problem
  int64_t x_off, gram_off;
  uint64_t row_ptr, col;
  int32_t n, pad;
};
struct JacGramPattern { // one distinct pattern: byte offsets into JacGramPlan::tables, and its sizes
  uint64_t row_ptr = 0, col = 0, pos = 0, mirror = 0, cnt = 0, slice_ptr = 0, words = 0;
  int32_t n = 0, nnz = 0, lower = 0, slices = 0;
  int64_t n_words = 0, products = 0;            // padded table words; terms of the lower triangle
};
struct JacGramPlan {
  std::vector<int64_t> x_off, g_off, j_off;   // n_problems + 1: the layout of PlanJacOps for the same arguments
  std::vector<int64_t> gram_off;              // n_problems + 1: into the value array (doubles), every one even
  std::vector<char> tables;                   // every distinct pattern's tables, once (16-byte aligned)
  std::vector<JacGramPattern> patterns;
  std::vector<int32_t> pattern_of_struct;
  std::vector<JacGramWork> form;              // problem by problem, slices in sorted order
  std::vector<JacGramMulWork> mul;            // problem by problem, kGramThreads rows each
  std::vector<JacGramSolveWork> solve;        // one per problem
  int max_n = 0;                              // the largest n of the batch (sizes the solve's LDS)
  void Place(uint64_t base);                  // table offsets -> device addresses (base: where `tables` lives)
};
JacGramPlan PlanJacGram(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem);
// One structure's pattern of N alone (twr_structure_gram_pattern): row_ptr[n + 1], col_idx[nnz N]
void GramPattern(const Structure& S, std::vector<int32_t>* row_ptr, std::vector<int32_t>* col_idx);

// The damped weighted least-squares step with a batch's Jacobian (twr_jac_lsq_solve, twr_jac_violation, twr_jac_dot; jac_lsq.hip),
// planned on the host (no HIP): one work record per problem, the solver's workspace and the per-row bound tables.
//   workspace (doubles, every segment starts on a 16-byte boundary): p and z in the x layout, q, r and t in the g layout, then
//   kLsqRec doubles of scalars per problem.  A vector of problem p lives at segment + x_off[p] / g_off[p], as in the batch.
//   The Marquardt-scaled solve (twr_jac_lsq_solve_scaled) adds two vectors in the x layout, planned as a workspace of their
//   own (ws2_*) that the handle allocates only when that solve is used; the one-pass solve (twr_jac_lsq_solve_onepass) adds
//   two more (ws3_*: the recurred s, and u), allocated only when that solve is used.
//   bounds: per distinct (lower, upper) table lower[m] then upper[m], 16-byte aligned; structures whose tables are
//   byte-identical share one copy.  These are the structures' own per-row bounds (Structure::lower / upper), any number of
//   distinct pairs: nothing here reads PackBlob's compact score record.
// Every sum of the kernels is taken by kLsqThreads lanes over aligned index pairs: lane t adds the elements of the pairs
// {2j, 2j + 1}, j = t, t + kLsqThreads, ... in index order, then a fixed tree over the wave, then the waves' partials in wave
// order: a function of the vector's length alone.
constexpr int kLsqThreads = 256;
constexpr int kLsqRec = 4;    // per-problem scalars: the slots below
enum { kLsqGamma = 0, kLsqGamma0 = 1, kLsqIters = 2, kLsqState = 3 };   // state: kLsqRunning, or the status the problem stopped with
constexpr double kLsqRunning = -1.0;
struct JacLsqWork {     // one problem (device layout; lower / upper are byte offsets into JacLsqPlan::bounds until Place())
  int64_t x_off, g_off;
  uint64_t lower, upper;           // double[m] each
  int32_t n, m;
};
struct JacLsqPlan {
  std::vector<int64_t> x_off, g_off;          // n_problems + 1: the layout of PlanBatch / PlanJacOps for the same arguments
  std::vector<JacLsqWork> work;               // problem by problem
  std::vector<char> bounds;                   // every distinct bound table, once
  std::vector<int32_t> bounds_of_struct;      // the distinct table every structure reads
  int distinct_bounds = 0;
  int64_t ws_p = 0, ws_z = 0, ws_q = 0, ws_r = 0, ws_t = 0, ws_rec = 0;   // segment starts (doubles)
  int64_t ws_doubles = 0;                     // the whole workspace
  int64_t ws2_e = 0, ws2_cp = 0;              // the scaled solve's own workspace, a second allocation made on first use
  int64_t ws2_doubles = 0;                    // (twr_jac_lsq_reserve_scaled): e = d / c and c o p in the x layout, segment starts
  int64_t ws3_s = 0, ws3_u = 0;               // the one-pass solve's own workspace, a third allocation made on first use
  int64_t ws3_doubles = 0;                    // (twr_jac_lsq_solve_onepass): the recurred s and u = J^T(w o (J p)) in the x layout
  int lds_x = 0;                              // largest n <= kJacLdsX of the batch (the s the direction kernel keeps in LDS)
  void Place(uint64_t base);                  // bound offsets -> device addresses (base: where `bounds` lives)
};
JacLsqPlan PlanJacLsq(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem);

// The bound-constrained Levenberg-Marquardt driver (twr_jac_lm_*; jac_lm.hip), planned on the host (no HIP): the workspace of a
// twr_jac_lm handle in the x / g layout of PlanJacLsq for the same arguments (only n_vars and n_rows of a Structure are read).
//   workspace (doubles, every segment starts on a 16-byte boundary):
//     x layout: xt (the trial point), d (the step), z = J^T(w o b), colsq, colmax (the running maximum), c (the Marquardt scale),
//               cf (c with an exact 0 for every fixed / blocked variable);
//     g layout: r (the violation), b = -r, wa (the active-set weights), gt and rt (values and violation at the trial point);
//     per problem: kLmRec doubles of state (the record twr_jac_lm_state copies out), mu, the trial merit, the merit of the
//               linearisation, the free count, the 4 doubles of the solve's info.
//   The power iteration of twr_jac_lm_start borrows d (v), xt (cf o v), z (u) and gt (y): nothing of its own.
constexpr int kLmRec = 8;   // the record of a problem: the slots below
enum { kLmMerit0 = 0, kLmMerit = 1, kLmMu = 2, kLmSteps = 3, kLmAccepted = 4, kLmFree = 5, kLmCgIters = 6, kLmState = 7 };
constexpr double kLmRunning = 0.0, kLmDone = 1.0, kLmBad = 2.0;   // kLmState
struct JacLmPlan {
  std::vector<int64_t> x_off, g_off;   // n_problems + 1: the layout of PlanBatch / PlanJacOps / PlanJacLsq for the same arguments
  int64_t ws_xt = 0, ws_d = 0, ws_z = 0, ws_colsq = 0, ws_colmax = 0, ws_c = 0, ws_cf = 0;   // segment starts (doubles)
  int64_t ws_r = 0, ws_b = 0, ws_wa = 0, ws_gt = 0, ws_rt = 0;
  int64_t ws_rec = 0, ws_mu = 0, ws_merit_t = 0, ws_merit_lin = 0, ws_nfree = 0, ws_info = 0;
  int64_t ws_doubles = 0;              // the whole workspace
};
JacLmPlan PlanJacLm(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem);

// fpowr GetTrajectory (fpowr/include/fpowr/footstep_plan_extractor.h:19-53): samples while t <= t_total + 1e-5, t accumulated
int SampleCount(double t_total, double dt);
void GaitCombo(int n_ee, int combo, double t_total, double swing_scale, twr_schedule* out);
void ModelPreset(int robot, int terrain, twr_model* out);
double TerrainHeightHost(const twr_model& m, const TerrainGrid* grid, double x, double y);

}  // namespace twr
