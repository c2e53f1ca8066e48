// Checks of the product plans (twr_jac_mul / twr_jac_tmul) on the host: the tables and work lists twr::PlanJacOps builds, and the
// CSC view twr::TransposePattern.  Built and run by tests/test_jac_plan.py (g++ against the host planner, no HIP).
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../towr_amd/csrc/batch_plan.h"
#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

template <class T>
static const T* table(const twr::JacOpsPlan& J, uint64_t off) {
  return reinterpret_cast<const T*>(J.tables.data() + off);
}

// The terms of every output of problem p, in the order the kernels add them (CSR positions), with the per-problem parts of the
// work records that decide it: what must depend on the structure alone.
struct Order {
  std::vector<std::vector<int>> y, z;   // [row] / [column] -> CSR positions in summation order
  std::vector<int64_t> shape;           // the work records relative to the problem
  bool operator==(const Order& o) const { return y == o.y && z == o.z && shape == o.shape; }
};

// Coverage of one problem: every entry once in J v and once in J^T w, every row and column written once, term order.
static Order check_problem(const char* name, const twr::JacOpsPlan& J, const twr::Structure& S, int p,
                           const std::vector<const twr::JacMulWork*>& mul, const std::vector<const twr::JacTWork*>& tmul,
                           const std::vector<const twr::JacFoldWork*>& fold) {
  const int n = S.n_vars, m = S.n_rows, nnz = S.nnz;
  Order o;
  o.y.assign(m, {});
  o.z.assign(n, {});
  std::vector<int> row_hit(m, 0), mul_entry(nnz, 0), tmul_entry(nnz, 0), col_hit(n, 0);
  for (const twr::JacMulWork* w : mul) {
    CHECK(w->x_off == J.x_off[p] && w->g_off == J.g_off[p] && w->j_off == J.j_off[p] && w->n == n, "%s: mul offsets of problem %d", name, p);
    CHECK(0 <= w->r0 && w->r0 < w->r1 && w->r1 <= m && w->r1 - w->r0 <= twr::kJacMulRows, "%s: mul rows [%d, %d)", name, w->r0, w->r1);
    const int32_t* rp = table<int32_t>(J, w->row_ptr);
    const uint16_t* col = table<uint16_t>(J, w->col);
    CHECK(std::memcmp(rp, S.row_ptr.data(), S.row_ptr.size() * 4) == 0, "%s: row_ptr table", name);
    for (int k = 0; k < nnz; ++k) CHECK(col[k] == S.col_idx[k], "%s: col table at %d", name, k);
    const int e = rp[w->r1] - rp[w->r0];
    CHECK(e <= twr::kJacMulNnz || w->r1 - w->r0 == 1, "%s: mul block of %d entries over %d rows", name, e, w->r1 - w->r0);
    o.shape.insert(o.shape.end(), {1, w->r0, w->r1});
    for (int r = w->r0; r < w->r1; ++r) {
      ++row_hit[r];
      for (int k = rp[r]; k < rp[r + 1]; ++k) {
        ++mul_entry[k];
        o.y[r].push_back(k);
      }
    }
  }
  std::map<int64_t, std::vector<int>> slot_terms;   // partial (relative to the problem's first) -> CSR positions in order
  int64_t slab0 = fold.empty() ? -1 : fold[0]->slab;
  int next_k = 0;
  for (const twr::JacTWork* t : tmul) {
    CHECK(t->g_off == J.g_off[p] && t->j_off == J.j_off[p], "%s: tmul offsets of problem %d", name, p);
    CHECK(t->k0 == next_k && t->k0 < t->k1 && t->k1 <= nnz, "%s: tmul block [%d, %d) after %d", name, t->k0, t->k1, next_k);
    next_k = t->k1;
    CHECK(t->k1 - t->k0 <= twr::kJacTNnz && t->ncols >= 1 && t->ncols <= twr::kJacTCols && t->span >= 1 && t->span <= twr::kJacTSpan,
          "%s: tmul block limits", name);
    CHECK(S.row_ptr[t->r_first] <= t->k0 && t->k0 < S.row_ptr[t->r_first + 1], "%s: tmul r_first", name);
    CHECK(S.row_ptr[t->r_first + t->span - 1] < t->k1 && t->k1 <= S.row_ptr[t->r_first + t->span], "%s: tmul span", name);
    CHECK(table<int32_t>(J, t->row_ptr)[m] == nnz, "%s: tmul row_ptr table", name);
    const uint16_t* map = table<uint16_t>(J, t->map);
    const uint16_t* pos = map + t->ncols + 1;
    CHECK(map[0] == 0 && map[t->ncols] == t->k1 - t->k0, "%s: map ends", name);
    o.shape.insert(o.shape.end(), {2, t->k0, t->k1, t->r_first, t->span, t->ncols, t->slab - slab0});
    int prev_col = -1;
    for (int j = 0; j < t->ncols; ++j) {
      CHECK(map[j] < map[j + 1], "%s: empty column %d of a block", name, j);
      const int c = S.col_idx[t->k0 + pos[map[j]]];
      CHECK(c > prev_col, "%s: block columns not ascending", name);
      prev_col = c;
      std::vector<int>& terms = slot_terms[t->slab - slab0 + j];
      CHECK(terms.empty(), "%s: partial %lld written twice", name, (long long)(t->slab - slab0 + j));
      for (int i = map[j]; i < map[j + 1]; ++i) {
        const int k = t->k0 + pos[i];
        CHECK(S.col_idx[k] == c, "%s: map entry of another column", name);
        CHECK(terms.empty() || k > terms.back(), "%s: column terms not in row order", name);
        ++tmul_entry[k];
        terms.push_back(k);
      }
    }
  }
  CHECK(next_k == nnz, "%s: tmul blocks end at %d of %d", name, next_k, nnz);
  int next_c = 0;
  for (const twr::JacFoldWork* f : fold) {
    CHECK(f->x_off == J.x_off[p] && f->slab == slab0, "%s: fold offsets of problem %d", name, p);
    CHECK(f->c0 == next_c && f->c0 < f->c1 && f->c1 <= n && f->c1 - f->c0 <= twr::kJacFoldCols, "%s: fold columns", name);
    next_c = f->c1;
    const int32_t* ptr = table<int32_t>(J, f->ptr);
    const int32_t* slot = table<int32_t>(J, f->slot);
    o.shape.insert(o.shape.end(), {3, f->c0, f->c1});
    for (int c = f->c0; c < f->c1; ++c) {
      ++col_hit[c];
      for (int i = ptr[c]; i < ptr[c + 1]; ++i) {
        auto it = slot_terms.find(slot[i]);
        CHECK(it != slot_terms.end(), "%s: column %d folds an unwritten partial", name, c);
        if (it == slot_terms.end()) continue;
        for (int k : it->second) CHECK(S.col_idx[k] == c, "%s: column %d folds another column's partial", name, c);
        o.z[c].insert(o.z[c].end(), it->second.begin(), it->second.end());
        slot_terms.erase(it);   // folded once
      }
    }
  }
  CHECK(next_c == n, "%s: fold columns end at %d of %d", name, next_c, n);
  CHECK(slot_terms.empty(), "%s: %zu partials nobody folds", name, slot_terms.size());
  int bad = 0;
  for (int r = 0; r < m; ++r) bad += row_hit[r] != 1;
  for (int c = 0; c < n; ++c) bad += col_hit[c] != 1;
  for (int k = 0; k < nnz; ++k) bad += mul_entry[k] != 1 || tmul_entry[k] != 1;
  CHECK(bad == 0, "%s: problem %d: %d rows / columns / entries not covered exactly once", name, p, bad);
  // J^T w adds a column's terms in row order: the CSC order of the transposed pattern
  const twr::CscPattern T = twr::TransposePattern(S);
  for (int c = 0; c < n; ++c) {
    const std::vector<int> want(T.csr_pos.begin() + T.col_ptr[c], T.csr_pos.begin() + T.col_ptr[c + 1]);
    CHECK(o.z[c] == want, "%s: column %d not summed in row order", name, c);
  }
  return o;
}

static std::vector<Order> plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop,
                                    int want_distinct) {
  const twr::JacOpsPlan J = twr::PlanJacOps(sp, sop), K = twr::PlanJacOps(sp, sop);
  CHECK(same_bytes(J.tables, K.tables) && same_bytes(J.mul, K.mul) && same_bytes(J.tmul, K.tmul) && same_bytes(J.fold, K.fold) &&
            J.slab == K.slab && J.pattern_of_struct == K.pattern_of_struct,
        "%s: planning twice differs", name);
  CHECK(J.distinct_patterns == want_distinct, "%s: %d distinct patterns, want %d", name, J.distinct_patterns, want_distinct);
  const twr::BatchPlan B = twr::PlanBatch(sp, sop, blob_at(sp.size()), 256, (int64_t)256 << 20, twr::kForceChunk);
  CHECK(J.x_off == B.x_off && J.g_off == B.g_off && J.j_off == B.j_off, "%s: layout differs from PlanBatch", name);
  const int n = (int)sop.size();
  // the problem of a work record: by x_off (every structure has variables), by j_off for J^T w (only problems with entries
  // have its records, and their j_off differ)
  std::map<int64_t, int> problem_of_x, problem_of_j;
  for (int p = 0; p < n; ++p) {
    problem_of_x[J.x_off[p]] = p;
    if (J.j_off[p + 1] > J.j_off[p]) problem_of_j[J.j_off[p]] = p;
  }
  std::vector<std::vector<const twr::JacMulWork*>> mul(n);
  std::vector<std::vector<const twr::JacTWork*>> tmul(n);
  std::vector<std::vector<const twr::JacFoldWork*>> fold(n);
  for (const auto& w : J.mul) mul[problem_of_x.at(w.x_off)].push_back(&w);
  for (const auto& t : J.tmul) tmul[problem_of_j.at(t.j_off)].push_back(&t);
  for (const auto& f : J.fold) fold[problem_of_x.at(f.x_off)].push_back(&f);
  std::vector<int> slab_owner(J.slab, -1);
  for (int p = 0; p < n; ++p)
    for (const twr::JacTWork* t : tmul[p])
      for (int j = 0; j < t->ncols; ++j) {
        const int64_t s = t->slab + j;
        CHECK(s >= 0 && s < J.slab && slab_owner[s] < 0, "%s: partial %lld outside the slab or shared", name, (long long)s);
        if (s >= 0 && s < J.slab) slab_owner[s] = p;
      }
  std::vector<Order> orders;
  for (int p = 0; p < n; ++p) orders.push_back(check_problem(name, J, *sp[sop[p]], p, mul[p], tmul[p], fold[p]));
  // the order of terms is the structure's: the same in a one-problem plan of that structure
  for (int p = 0; p < n; ++p) {
    const twr::Structure* S = sp[sop[p]];
    const twr::JacOpsPlan A = twr::PlanJacOps({S}, {0});
    std::vector<const twr::JacMulWork*> am;
    std::vector<const twr::JacTWork*> at_;
    std::vector<const twr::JacFoldWork*> af;
    for (const auto& w : A.mul) am.push_back(&w);
    for (const auto& t : A.tmul) at_.push_back(&t);
    for (const auto& f : A.fold) af.push_back(&f);
    CHECK(check_problem(name, A, *S, 0, am, at_, af) == orders[p], "%s: problem %d sums in another order than alone", name, p);
  }
  std::printf("jac plan %-10s %4d problems: %d distinct patterns, %zu mul / %zu tmul / %zu fold items, slab %lld, tables %zu B\n", name, n,
              J.distinct_patterns, J.mul.size(), J.tmul.size(), J.fold.size(), (long long)J.slab, J.tables.size());
  return orders;
}

int main() {
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63, 1.0, 200), c3_hot = build(3, 0, 1, 2.0, 27, 1.0, 200), c3_twin = build(3, 0, 1, 2.0, 27, 1.0, 200);
  const twr::Structure every = build(3, 2, 0, 2.4, 255, 1.1, 200);   // every family, optimised timings, base_z_init set
  plan_case("C3x16", {&c3_hot}, std::vector<int32_t>(16, 0), 1);
  plan_case("twins", {&c3_hot, &c3_twin}, {0, 1, 1, 0}, 1);   // two structures from identical inputs: one pattern
  plan_case("every", {&every, &c3}, {0, 1, 0}, 2);
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 6; ++i) ss.push_back(build(i % 2 ? 2 : 1, 4, i % 3, 1.2 + 0.3 * i, i % 2 ? 27 : 63, 0.9, 200));
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 3, 1, 1, 0}, 6);
  auto grid = std::make_shared<twr::TerrainGrid>();
  grid->rows = 40;
  grid->cols = 60;
  for (int i = 0; i < grid->rows * grid->cols; ++i) grid->heights.push_back(0.05 * ((i * 7919) % 13) / 13.0);
  const twr::Structure g1 = build(3, 7, 1, 2.0, 63, 1.0, 200, grid);
  plan_case("grid", {&g1, &c3_hot}, {1, 0, 0}, 2);
  const twr::Structure wide = build(3, 0, 1, 2.0, 27, 1.0, 200, nullptr, 0.003);   // J v gathers v from memory
  CHECK(wide.n_vars > twr::kJacLdsX, "the wide structure has %d variables", wide.n_vars);
  plan_case("wide", {&wide, &c3_hot}, {0, 1}, 2);
  // the invariant the products rely on is checked, not assumed
  twr::Structure dup = c3_hot;
  dup.col_idx[1] = dup.col_idx[0];
  bool threw = false;
  try {
    twr::TransposePattern(dup);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a duplicate entry was accepted");
  threw = false;
  try {
    twr::PlanJacOps({&dup}, {0});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a plan over a duplicate entry was accepted");
  std::printf("jac_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
