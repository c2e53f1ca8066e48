// The Jacobian linear algebra planned on the host (no HIP): products with a batch's Jacobian values, the one-pass normal
// product, the Gram matrix, the least-squares step and the LM driver's workspace.  jac_plan.cc.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "structure.h"

namespace twr {

// Products with a batch's Jacobian values (twr_jac_mul: y = J v, twr_jac_tmul: z = J^T w; jac/products.h), planned on the host
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

// The one-pass normal product u = J^T (w o (J v)), y = J v (twr_jac_normal_mul; jac/products.h jac_normal_kernel), planned on the
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
// jac/gram.h), planned on the host (no HIP) for the arguments of PlanJacOps and in its x / g / jac layout.  Per distinct pattern:
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

// The damped weighted least-squares step with a batch's Jacobian (twr_jac_lsq_solve, twr_jac_violation, twr_jac_dot; jac/lsq.h),
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

// The bound-constrained Levenberg-Marquardt driver (twr_jac_lm_*; jac/lm.h), planned on the host (no HIP): the workspace of a
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

}  // namespace twr
