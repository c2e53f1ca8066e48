// The plans of the Jacobian linear algebra on the host (no HIP): the products with J, the one-pass normal product, the Gram
// matrix, the least-squares step and the LM driver's workspace (jac_plan.h).
#include "jac_plan.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <utility>

namespace twr {

// ---------------------------------------------------------------- products with the Jacobian values (jac/products.h)
namespace {
void CheckPattern(const Structure& S) {
  const int n = S.n_vars, m = S.n_rows;
  if ((int)S.row_ptr.size() != m + 1 || (int)S.col_idx.size() != S.nnz || S.row_ptr[0] != 0 || S.row_ptr[m] != S.nnz)
    throw std::runtime_error("CSR pattern does not match its sizes");
  if (n > 65536) throw std::runtime_error("more than 65536 variables: column indices do not fit 16 bits");
  for (int r = 0; r < m; ++r) {
    if (S.row_ptr[r + 1] < S.row_ptr[r]) throw std::runtime_error("row_ptr descends");
    for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
      const int c = S.col_idx[k];
      if (c < 0 || c >= n) throw std::runtime_error("column index outside [0, n_vars)");
      if (k > S.row_ptr[r] && c <= S.col_idx[k - 1])
        throw std::runtime_error("row " + std::to_string(r) + ": column indices not strictly ascending (unsorted or duplicate entries)");
    }
  }
}

template <class T>
uint64_t AppendTable(std::vector<char>& out, const T* data, size_t count) {
  const size_t at = (out.size() + 15) / 16 * 16;
  out.resize(at + count * sizeof(T));
  if (count) std::memcpy(out.data() + at, data, count * sizeof(T));
  return at;
}

uint64_t HashWords(uint64_t h, const void* data, size_t bytes) {   // FNV-1a over 8-byte words (a bucket key only)
  const char* p = static_cast<const char*>(data);
  size_t i = 0;
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, p + i, 8);
    h = (h ^ w) * 1099511628211ull;
    h ^= h >> 29;
  }
  for (; i < bytes; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
  return h;
}

// The distinct sparsity patterns of a batch's structures, every one checked: byte-identical (n, row_ptr, col_idx) is one
// pattern, numbered in the order the structures first show it.
struct DistinctPatterns {
  std::vector<int32_t> pattern_of_struct;
  std::vector<const Structure*> first;   // the first structure of every distinct pattern
};
DistinctPatterns FindDistinctPatterns(const std::vector<const Structure*>& structs) {
  DistinctPatterns d;
  std::unordered_map<uint64_t, std::vector<int>> by_hash;
  for (const Structure* sp : structs) {
    const Structure& S = *sp;
    CheckPattern(S);
    uint64_t h = HashWords(1469598103934665603ull ^ (uint64_t)S.n_vars, S.row_ptr.data(), S.row_ptr.size() * sizeof(int32_t));
    h = HashWords(h, S.col_idx.data(), S.col_idx.size() * sizeof(int32_t));
    std::vector<int>& bucket = by_hash[h];
    int pid = -1;
    for (int q : bucket)
      if (d.first[q]->n_vars == S.n_vars && d.first[q]->row_ptr == S.row_ptr && d.first[q]->col_idx == S.col_idx) pid = q;
    if (pid < 0) {
      pid = (int)d.first.size();
      bucket.push_back(pid);
      d.first.push_back(&S);
    }
    d.pattern_of_struct.push_back(pid);
  }
  return d;
}

// The layout of a batch: prefix sums of the problems' variables, rows and (j_off, unless null) Jacobian entries, n_problems + 1
// each.  Throws "<what> out of range" for a problem that names no structure.
void Layout(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem, const char* what,
            std::vector<int64_t>* x_off, std::vector<int64_t>* g_off, std::vector<int64_t>* j_off) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  x_off->assign(n_problems + 1, 0);
  g_off->assign(n_problems + 1, 0);
  if (j_off) j_off->assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error(std::string(what) + " out of range");
    (*x_off)[p + 1] = (*x_off)[p] + structs[si]->n_vars;
    (*g_off)[p + 1] = (*g_off)[p] + structs[si]->n_rows;
    if (j_off) (*j_off)[p + 1] = (*j_off)[p] + structs[si]->nnz;
  }
}

struct JacTables {   // one distinct pattern: byte offsets into JacOpsPlan::tables, its blocks, partials per problem
  uint64_t col = 0, row_ptr = 0, fold_ptr = 0, fold_slot = 0;
  std::vector<std::pair<int, int>> rows;   // J v blocks [r0, r1)
  struct TBlock {
    int k0, k1, r_first, span, ncols;
    uint64_t map;
    int64_t slot;                          // first partial, relative to the problem's
  };
  std::vector<TBlock> tblocks;
  int64_t slots = 0;
};

JacTables BuildJacTables(const Structure& S, JacOpsPlan& J) {
  const int n = S.n_vars, m = S.n_rows, nnz = S.nnz;
  JacTables P;
  const std::vector<uint16_t> col(S.col_idx.begin(), S.col_idx.end());   // < 65536: CheckPattern
  P.col = AppendTable(J.tables, col.data(), col.size());
  P.row_ptr = AppendTable(J.tables, S.row_ptr.data(), S.row_ptr.size());
  J.table_bytes_mul += 2 * (int64_t)nnz + 4 * (int64_t)(m + 1);
  for (int r0 = 0; r0 < m;) {
    int r1 = r0 + 1;
    while (r1 < m && r1 - r0 < kJacMulRows && S.row_ptr[r1 + 1] - S.row_ptr[r0] <= kJacMulNnz) ++r1;
    P.rows.push_back({r0, r1});
    r0 = r1;
  }
  std::vector<int> row_of(nnz);
  for (int r = 0; r < m; ++r) std::fill(row_of.begin() + S.row_ptr[r], row_of.begin() + S.row_ptr[r + 1], r);
  std::vector<int> stamp(n, -1);
  std::vector<std::vector<int32_t>> slots_of(n);   // the partials of every column, in block order
  int64_t tbytes = 4 * (int64_t)(m + 1);
  for (int k0 = 0; k0 < nnz;) {
    const int b = (int)P.tblocks.size();
    int k1 = k0, ncols = 0;
    while (k1 < nnz && k1 - k0 < kJacTNnz && row_of[k1] - row_of[k0] < kJacTSpan) {
      const int c = S.col_idx[k1];
      if (stamp[c] != b) {
        if (ncols == kJacTCols) break;
        stamp[c] = b;
        ++ncols;
      }
      ++k1;
    }
    std::vector<std::pair<int, int>> e;   // (column, entry - k0), sorted: the block's columns ascending, each in row order
    for (int k = k0; k < k1; ++k) e.push_back({S.col_idx[k], k - k0});
    std::sort(e.begin(), e.end());
    std::vector<uint16_t> map(ncols + 1 + e.size());
    int j = -1;
    for (size_t i = 0; i < e.size(); ++i) {
      if (i == 0 || e[i].first != e[i - 1].first) {
        map[++j] = (uint16_t)i;
        slots_of[e[i].first].push_back((int32_t)(P.slots + j));
      }
      map[ncols + 1 + i] = (uint16_t)e[i].second;
    }
    map[ncols] = (uint16_t)e.size();
    const uint64_t at = AppendTable(J.tables, map.data(), map.size());
    tbytes += 2 * (int64_t)map.size();
    P.tblocks.push_back({k0, k1, row_of[k0], row_of[k1 - 1] - row_of[k0] + 1, ncols, at, P.slots});
    P.slots += ncols;
    k0 = k1;
  }
  std::vector<int32_t> fptr(n + 1, 0), fslot;
  for (int c = 0; c < n; ++c) {
    fslot.insert(fslot.end(), slots_of[c].begin(), slots_of[c].end());
    fptr[c + 1] = (int32_t)fslot.size();
  }
  P.fold_ptr = AppendTable(J.tables, fptr.data(), fptr.size());
  P.fold_slot = AppendTable(J.tables, fslot.data(), fslot.size());
  J.table_bytes_tmul += tbytes + 4 * (int64_t)(fptr.size() + fslot.size());
  return P;
}
}  // namespace

CscPattern TransposePattern(const Structure& S) {
  CheckPattern(S);
  CscPattern t;
  t.col_ptr.assign(S.n_vars + 1, 0);
  for (int k = 0; k < S.nnz; ++k) ++t.col_ptr[S.col_idx[k] + 1];
  for (int c = 0; c < S.n_vars; ++c) t.col_ptr[c + 1] += t.col_ptr[c];
  t.row_idx.resize(S.nnz);
  t.csr_pos.resize(S.nnz);
  std::vector<int32_t> next(t.col_ptr.begin(), t.col_ptr.end() - 1);
  for (int r = 0; r < S.n_rows; ++r)
    for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
      const int q = next[S.col_idx[k]]++;
      t.row_idx[q] = r;
      t.csr_pos[q] = k;
    }
  return t;
}

void JacOpsPlan::Place(uint64_t base) {
  for (auto& w : mul) w.col += base, w.row_ptr += base;
  for (auto& w : tmul) w.map += base, w.row_ptr += base;
  for (auto& w : fold) w.ptr += base, w.slot += base;
}

JacOpsPlan PlanJacOps(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_problems = (int)struct_of_problem.size();
  JacOpsPlan J;
  DistinctPatterns d = FindDistinctPatterns(structs);
  std::vector<JacTables> pats;
  for (const Structure* S : d.first) pats.push_back(BuildJacTables(*S, J));
  J.pattern_of_struct = std::move(d.pattern_of_struct);
  J.distinct_patterns = (int)pats.size();
  Layout(structs, struct_of_problem, "struct_of_problem", &J.x_off, &J.g_off, &J.j_off);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    const Structure& S = *structs[si];
    const JacTables& P = pats[J.pattern_of_struct[si]];
    for (const auto& rb : P.rows) J.mul.push_back({J.x_off[p], J.g_off[p], J.j_off[p], P.col, P.row_ptr, rb.first, rb.second, S.n_vars, 0});
    for (const auto& tb : P.tblocks)
      J.tmul.push_back({J.g_off[p], J.j_off[p], J.slab + tb.slot, tb.map, P.row_ptr, tb.k0, tb.k1, tb.r_first, tb.span, tb.ncols, 0});
    for (int c0 = 0; c0 < S.n_vars; c0 += kJacFoldCols)
      J.fold.push_back({J.x_off[p], J.slab, P.fold_ptr, P.fold_slot, c0, std::min(S.n_vars, c0 + kJacFoldCols)});
    J.slab += P.slots;
    if (S.n_vars <= kJacLdsX) J.mul_lds_x = std::max(J.mul_lds_x, S.n_vars);
  }
  return J;
}

// ---------------------------------------------------------------- the one-pass normal product (jac/products.h jac_normal_kernel)
namespace {
struct JacNormalTables {   // one distinct pattern: byte offsets into JacNormalPlan::tables, its blocks, partials per problem
  uint64_t fold_ptr = 0, fold_slot = 0;
  struct Block {
    int r0, r1, ncols, is_long;
    uint64_t map;
    int64_t slot;   // first partial, relative to the problem's
  };
  std::vector<Block> blocks;
  int64_t slots = 0;
};

JacNormalTables BuildJacNormalTables(const Structure& S, JacNormalPlan& N, int tile) {
  const int n = S.n_vars, m = S.n_rows;
  JacNormalTables P;
  std::vector<std::vector<int32_t>> slots_of(n);   // the partials of every column, in block order
  for (int r0 = 0; r0 < m;) {
    int r1 = r0 + 1;
    while (r1 < m && r1 - r0 < kJacThreads && S.row_ptr[r1 + 1] - S.row_ptr[r0] <= tile) ++r1;
    const int k0 = S.row_ptr[r0], k1 = S.row_ptr[r1];
    if (k1 - k0 > tile) {   // one long row: a partial per entry, in column order
      for (int k = k0; k < k1; ++k) slots_of[S.col_idx[k]].push_back((int32_t)(P.slots + (k - k0)));
      P.blocks.push_back({r0, r1, k1 - k0, 1, 0, P.slots});
      P.slots += k1 - k0;
    } else if (k1 > k0) {
      std::vector<std::pair<int, int>> e;   // (column, entry - k0), sorted: the block's columns ascending, each in row order
      for (int k = k0; k < k1; ++k) e.push_back({S.col_idx[k], k - k0});
      std::sort(e.begin(), e.end());
      int ncols = 0;
      for (size_t i = 0; i < e.size(); ++i) ncols += i == 0 || e[i].first != e[i - 1].first;
      std::vector<uint16_t> map(ncols + 1 + e.size());
      int j = -1;
      for (size_t i = 0; i < e.size(); ++i) {
        if (i == 0 || e[i].first != e[i - 1].first) {
          map[++j] = (uint16_t)i;
          slots_of[e[i].first].push_back((int32_t)(P.slots + j));
        }
        map[ncols + 1 + i] = (uint16_t)e[i].second;
      }
      map[ncols] = (uint16_t)e.size();
      P.blocks.push_back({r0, r1, ncols, 0, AppendTable(N.tables, map.data(), map.size()), P.slots});
      P.slots += ncols;
    } else {
      P.blocks.push_back({r0, r1, 0, 0, 0, P.slots});   // rows without entries: y = 0 is still theirs to write
    }
    r0 = r1;
  }
  std::vector<int32_t> fptr(n + 1, 0), fslot;
  for (int c = 0; c < n; ++c) {
    fslot.insert(fslot.end(), slots_of[c].begin(), slots_of[c].end());
    fptr[c + 1] = (int32_t)fslot.size();
  }
  P.fold_ptr = AppendTable(N.tables, fptr.data(), fptr.size());
  P.fold_slot = AppendTable(N.tables, fslot.data(), fslot.size());
  return P;
}
}  // namespace

void JacNormalPlan::Place(uint64_t ops_base, uint64_t base) {
  for (auto& w : work) w.col += ops_base, w.row_ptr += ops_base, w.map += base;
  for (auto& w : fold) w.ptr += base, w.slot += base;
}

std::vector<JacPatternPlace> JacPatternPlaces(const JacOpsPlan& J, const std::vector<int32_t>& struct_of_problem) {
  std::vector<JacPatternPlace> at(J.distinct_patterns, JacPatternPlace{-1, 0, 0});
  size_t k = 0;
  for (size_t p = 0; p < struct_of_problem.size(); ++p) {   // J.mul is problem by problem; a problem without rows has no record
    while (k < J.mul.size() && J.mul[k].x_off < J.x_off[p]) ++k;
    JacPatternPlace& a = at[J.pattern_of_struct[struct_of_problem[p]]];
    if (a.first_struct >= 0) continue;
    a.first_struct = struct_of_problem[p];
    if (k < J.mul.size() && J.mul[k].x_off == J.x_off[p]) a.col = J.mul[k].col, a.row_ptr = J.mul[k].row_ptr;
  }
  return at;
}

JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& patterns, const std::vector<JacPatternPlace>& places,
                            const std::vector<int32_t>& pattern_of_problem, int tile) {
  const int n_problems = (int)pattern_of_problem.size();
  if (tile < 1 || tile > kJacNormNnz) throw std::runtime_error("the one-pass tile is 1 .. kJacNormNnz entries");
  if (places.size() != patterns.size()) throw std::runtime_error("one place per pattern");
  JacNormalPlan N;
  N.tile = tile;
  std::vector<JacNormalTables> npats;
  for (const Structure* S : patterns) {
    CheckPattern(*S);
    npats.push_back(BuildJacNormalTables(*S, N, tile));
  }
  Layout(patterns, pattern_of_problem, "pattern_of_problem", &N.x_off, &N.g_off, &N.j_off);
  for (int p = 0; p < n_problems; ++p) {
    const int q = pattern_of_problem[p];
    const Structure& S = *patterns[q];
    const JacNormalTables& Q = npats[q];
    for (const auto& b : Q.blocks)
      N.work.push_back({N.x_off[p], N.g_off[p], N.j_off[p], N.slab + b.slot, places[q].col, places[q].row_ptr, b.map, b.r0, b.r1,
                        S.n_vars, b.ncols, b.is_long, 0});
    for (int c0 = 0; c0 < S.n_vars; c0 += kJacFoldCols)
      N.fold.push_back({N.x_off[p], N.slab, Q.fold_ptr, Q.fold_slot, c0, std::min(S.n_vars, c0 + kJacFoldCols)});
    N.slab += Q.slots;
    if (S.n_vars <= kJacLdsX) N.lds_x = std::max(N.lds_x, S.n_vars);
  }
  return N;
}

JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem, int tile) {
  const JacOpsPlan J = PlanJacOps(structs, struct_of_problem);   // (checks the patterns and struct_of_problem)
  const std::vector<JacPatternPlace> places = JacPatternPlaces(J, struct_of_problem);
  std::vector<const Structure*> patterns(places.size(), nullptr);   // (a pattern no problem has is still a structure's)
  for (size_t i = 0; i < structs.size(); ++i)
    if (!patterns[J.pattern_of_struct[i]]) patterns[J.pattern_of_struct[i]] = structs[i];
  std::vector<int32_t> pattern_of_problem;
  for (int32_t si : struct_of_problem) pattern_of_problem.push_back(J.pattern_of_struct[si]);
  return PlanJacNormal(patterns, places, pattern_of_problem, tile);
}

// ---------------------------------------------------------------- the Gram matrix N = J^T W J (jac/gram.h)
void GramPattern(const Structure& S, std::vector<int32_t>* row_ptr, std::vector<int32_t>* col_idx) {
  const CscPattern T = TransposePattern(S);   // (checks the pattern)
  const int n = S.n_vars;
  row_ptr->assign(n + 1, 0);
  col_idx->clear();
  std::vector<int> stamp(n, -1);
  std::vector<int32_t> cols;
  for (int i = 0; i < n; ++i) {   // row i of N: the columns of every row of J that has an entry in column i
    cols.clear();
    for (int q = T.col_ptr[i]; q < T.col_ptr[i + 1]; ++q) {
      const int r = T.row_idx[q];
      for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
        const int c = S.col_idx[k];
        if (stamp[c] != i) stamp[c] = i, cols.push_back(c);
      }
    }
    std::sort(cols.begin(), cols.end());
    if (col_idx->size() + cols.size() > (size_t)INT32_MAX) throw JacGramUnsupported("the Gram matrix has more than 2^31 - 1 entries");
    col_idx->insert(col_idx->end(), cols.begin(), cols.end());
    (*row_ptr)[i + 1] = (int32_t)col_idx->size();
  }
}

namespace {
// One pattern's tables, appended to `tables` (offsets into it)
JacGramPattern BuildGramTables(const Structure& S, std::vector<char>& tables) {
  const int n = S.n_vars;
  if (S.n_rows > kGramMaxRows)
    throw JacGramUnsupported("the Gram tables hold a row of J in 16 bits: " + std::to_string(S.n_rows) + " rows, at most " + std::to_string(kGramMaxRows));
  if (S.nnz > kGramMaxNnz)
    throw JacGramUnsupported("the Gram tables hold a position in J in 24 bits: " + std::to_string(S.nnz) + " entries, at most " + std::to_string(kGramMaxNnz));
  if (n > kGramMaxVars)
    throw JacGramUnsupported("the Gram solve keeps " + std::to_string(kGramSolveVectors) + " vectors of n doubles in one workgroup's LDS (" +
                             std::to_string(kGramLdsBytes) + " bytes): " + std::to_string(n) + " variables, at most " + std::to_string(kGramMaxVars));
  JacGramPattern P;
  std::vector<int32_t> rp, ci;
  GramPattern(S, &rp, &ci);
  const CscPattern T = TransposePattern(S);
  P.n = n;
  P.nnz = (int32_t)ci.size();
  // the lower entries in CSR order, and every one's terms in ascending row
  std::vector<int32_t> lpos, lmirror;
  std::vector<std::vector<uint64_t>> terms;
  std::vector<int32_t> where(n, -1);   // column -> lower entry of the row in hand
  for (int i = 0; i < n; ++i) {
    for (int e = rp[i]; e < rp[i + 1] && ci[e] <= i; ++e) {
      const int j = ci[e];
      where[j] = (int32_t)lpos.size();
      lpos.push_back(e);
      lmirror.push_back((int32_t)(std::lower_bound(ci.begin() + rp[j], ci.begin() + rp[j + 1], i) - ci.begin()));
      terms.emplace_back();
    }
    for (int q = T.col_ptr[i]; q < T.col_ptr[i + 1]; ++q) {
      const int r = T.row_idx[q];
      for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1] && S.col_idx[k] <= i; ++k)
        terms[where[S.col_idx[k]]].push_back((uint64_t)r << 48 | (uint64_t)T.csr_pos[q] << 24 | (uint64_t)k);
    }
  }
  P.lower = (int32_t)lpos.size();
  std::vector<int32_t> order(P.lower);
  for (int e = 0; e < P.lower; ++e) order[e] = e;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return terms[a].size() > terms[b].size(); });
  P.slices = (P.lower + kGramSlice - 1) / kGramSlice;
  std::vector<int32_t> pos(P.lower), mirror(P.lower), cnt(P.lower), slice_ptr(P.slices + 1, 0);
  std::vector<uint64_t> words;
  for (int s = 0; s < P.slices; ++s) {
    const int e0 = s * kGramSlice, e1 = std::min(P.lower, e0 + kGramSlice);
    const size_t width = terms[order[e0]].size(), at = words.size();
    if (at + width * kGramSlice > (size_t)INT32_MAX) throw JacGramUnsupported("the Gram contribution table has more than 2^31 - 1 words");
    words.resize(at + width * kGramSlice, kGramPad);
    for (int e = e0; e < e1; ++e) {
      const std::vector<uint64_t>& t = terms[order[e]];
      pos[e] = lpos[order[e]], mirror[e] = lmirror[order[e]], cnt[e] = (int32_t)t.size();
      for (size_t k = 0; k < t.size(); ++k) words[at + k * kGramSlice + (e - e0)] = t[k];
      P.products += (int64_t)t.size();
    }
    slice_ptr[s + 1] = (int32_t)words.size();
  }
  P.n_words = (int64_t)words.size();
  std::vector<uint16_t> col(ci.begin(), ci.end());
  P.row_ptr = AppendTable(tables, rp.data(), rp.size());
  P.col = AppendTable(tables, col.data(), col.size());
  P.pos = AppendTable(tables, pos.data(), pos.size());
  P.mirror = AppendTable(tables, mirror.data(), mirror.size());
  P.cnt = AppendTable(tables, cnt.data(), cnt.size());
  P.slice_ptr = AppendTable(tables, slice_ptr.data(), slice_ptr.size());
  P.words = AppendTable(tables, words.data(), words.size());
  return P;
}
}  // namespace

void JacGramPlan::Place(uint64_t base) {
  for (auto& w : form) w.pos += base, w.mirror += base, w.cnt += base, w.slice_ptr += base, w.words += base;
  for (auto& w : mul) w.row_ptr += base, w.col += base;
  for (auto& w : solve) w.row_ptr += base, w.col += base;
}

JacGramPlan PlanJacGram(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_problems = (int)struct_of_problem.size();
  JacGramPlan G;
  DistinctPatterns d = FindDistinctPatterns(structs);
  const std::vector<const Structure*>& first = d.first;
  G.pattern_of_struct = std::move(d.pattern_of_struct);
  G.patterns = std::vector<JacGramPattern>(first.size());
  // The distinct patterns are planned side by side (a sweep has a thousand of them at a third of a second each), every one into
  // tables of its own, which are then laid end to end in pattern order: the plan does not depend on the number of threads.
  const int n_pat = (int)first.size();
  std::vector<std::vector<char>> local(n_pat);
  std::vector<std::exception_ptr> failed(n_pat);
  std::atomic<int> next{0};
  const auto worker = [&] {
    for (int q = next++; q < n_pat; q = next++) {
      try {
        G.patterns[q] = BuildGramTables(*first[q], local[q]);
      } catch (...) {
        failed[q] = std::current_exception();
      }
    }
  };
  const int n_threads = std::max(1, std::min({n_pat, kGramPlanThreads, (int)std::thread::hardware_concurrency()}));
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) pool.emplace_back(worker);
  worker();
  for (std::thread& t : pool) t.join();
  for (int q = 0; q < n_pat; ++q)
    if (failed[q]) std::rethrow_exception(failed[q]);   // the first pattern that failed, whatever thread had it
  for (int q = 0; q < n_pat; ++q) {
    const uint64_t base = AppendTable(G.tables, local[q].data(), local[q].size());
    JacGramPattern& P = G.patterns[q];
    P.row_ptr += base, P.col += base, P.pos += base, P.mirror += base, P.cnt += base, P.slice_ptr += base, P.words += base;
    std::vector<char>().swap(local[q]);
  }
  Layout(structs, struct_of_problem, "struct_of_problem", &G.x_off, &G.g_off, &G.j_off);
  G.gram_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    const Structure& S = *structs[si];
    const JacGramPattern& P = G.patterns[G.pattern_of_struct[si]];
    G.gram_off[p + 1] = G.gram_off[p] + (P.nnz + 1) / 2 * 2;
    for (int e0 = 0; e0 < P.lower; e0 += kGramThreads)
      G.form.push_back({G.g_off[p], G.j_off[p], G.gram_off[p], P.pos, P.mirror, P.cnt, P.slice_ptr, P.words, e0, std::min(P.lower, e0 + kGramThreads)});
    for (int r0 = 0; r0 < S.n_vars; r0 += kGramThreads)
      G.mul.push_back({G.x_off[p], G.gram_off[p], P.row_ptr, P.col, r0, std::min(S.n_vars, r0 + kGramThreads)});
    G.solve.push_back({G.x_off[p], G.gram_off[p], P.row_ptr, P.col, S.n_vars, 0});
    G.max_n = std::max(G.max_n, S.n_vars);
  }
  return G;
}

void JacLsqPlan::Place(uint64_t base) {
  for (auto& w : work) w.lower += base, w.upper += base;
}

JacLsqPlan PlanJacLsq(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  JacLsqPlan L;
  struct Table {
    const Structure* first;
    uint64_t lower, upper;
  };
  std::vector<Table> tabs;
  std::unordered_map<uint64_t, std::vector<int>> by_hash;
  L.bounds_of_struct.resize(n_structs);
  for (int i = 0; i < n_structs; ++i) {
    const Structure& S = *structs[i];
    if ((int)S.lower.size() != S.n_rows || (int)S.upper.size() != S.n_rows) throw std::runtime_error("bounds do not match the rows");
    uint64_t h = HashWords(1469598103934665603ull ^ (uint64_t)S.n_rows, S.lower.data(), S.lower.size() * sizeof(double));
    h = HashWords(h, S.upper.data(), S.upper.size() * sizeof(double));
    std::vector<int>& bucket = by_hash[h];
    const size_t bytes = (size_t)S.n_rows * sizeof(double);
    int tid = -1;
    for (int q : bucket) {   // byte-identical, not ==: -0.0 and 0.0 are different tables, NaN bounds equal themselves
      const Structure& F = *tabs[q].first;
      if (F.n_rows == S.n_rows && (bytes == 0 || (std::memcmp(F.lower.data(), S.lower.data(), bytes) == 0 &&
                                                  std::memcmp(F.upper.data(), S.upper.data(), bytes) == 0)))
        tid = q;
    }
    if (tid < 0) {
      tid = (int)tabs.size();
      bucket.push_back(tid);
      const uint64_t lo = AppendTable(L.bounds, S.lower.data(), S.lower.size());
      tabs.push_back({&S, lo, AppendTable(L.bounds, S.upper.data(), S.upper.size())});
    }
    L.bounds_of_struct[i] = tid;
  }
  L.distinct_bounds = (int)tabs.size();
  Layout(structs, struct_of_problem, "struct_of_problem", &L.x_off, &L.g_off, nullptr);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    const Structure& S = *structs[si];
    const Table& T = tabs[L.bounds_of_struct[si]];
    L.work.push_back({L.x_off[p], L.g_off[p], T.lower, T.upper, S.n_vars, S.n_rows});
    if (S.n_vars <= kJacLdsX) L.lds_x = std::max(L.lds_x, S.n_vars);
  }
  const auto even = [](int64_t v) { return (v + 1) / 2 * 2; };
  const int64_t X = even(L.x_off[n_problems]), G = even(L.g_off[n_problems]);
  L.ws_p = 0;
  L.ws_z = L.ws_p + X;
  L.ws_q = L.ws_z + X;
  L.ws_r = L.ws_q + G;
  L.ws_t = L.ws_r + G;
  L.ws_rec = L.ws_t + G;
  L.ws_doubles = L.ws_rec + (int64_t)kLsqRec * n_problems;
  L.ws2_e = 0;
  L.ws2_cp = L.ws2_e + X;
  L.ws2_doubles = L.ws2_cp + X;
  L.ws3_s = 0;
  L.ws3_u = L.ws3_s + X;
  L.ws3_doubles = L.ws3_u + X;
  return L;
}

JacLmPlan PlanJacLm(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_problems = (int)struct_of_problem.size();
  JacLmPlan L;
  Layout(structs, struct_of_problem, "struct_of_problem", &L.x_off, &L.g_off, nullptr);
  const auto even = [](int64_t v) { return (v + 1) / 2 * 2; };
  const int64_t X = even(L.x_off[n_problems]), G = even(L.g_off[n_problems]), P = even(n_problems);
  int64_t at = 0;
  const auto take = [&](int64_t& seg, int64_t len) { seg = at, at += len; };
  for (int64_t* s : {&L.ws_xt, &L.ws_d, &L.ws_z, &L.ws_colsq, &L.ws_colmax, &L.ws_c, &L.ws_cf}) take(*s, X);
  for (int64_t* s : {&L.ws_r, &L.ws_b, &L.ws_wa, &L.ws_gt, &L.ws_rt}) take(*s, G);
  take(L.ws_rec, even((int64_t)kLmRec * n_problems));
  for (int64_t* s : {&L.ws_mu, &L.ws_merit_t, &L.ws_merit_lin, &L.ws_nfree}) take(*s, P);
  take(L.ws_info, even((int64_t)4 * n_problems));
  L.ws_doubles = at;
  return L;
}

}  // namespace twr
