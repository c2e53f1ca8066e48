// Checks of the Gram matrix's plan (twr_jac_gram, twr_jac_gram_mul, twr_jac_lsq_solve_gram) on the host: the tables and work lists
// twr::PlanJacGram builds.  Built and run by tests/test_jac_gram_plan.py (tests/host_build.py: g++ against the host planner
// under ASan + UBSan, no HIP).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

// towr/test/hopper_example.cc:67-68: the monoped of BASELINE's C1 (tests/common.py hopper_schedule), towr's default time steps
static twr::Structure hopper(int sets) {
  twr::Structure S;
  twr::ModelPreset(0, 0, &S.model);
  std::memset(&S.schedule, 0, sizeof S.schedule);
  const double d[7] = {0.4, 0.2, 0.4, 0.2, 0.4, 0.2, 0.2};
  S.schedule.n_ee = 1;
  S.schedule.n_phases[0] = 7;
  for (int i = 0; i < 7; ++i) S.schedule.phase_durations[0][i] = d[i];
  S.schedule.in_contact_at_start[0] = 1;
  twr_params& p = S.params;   // twr_params_default
  p.dt_dynamic = 0.1, p.dt_rom = 0.08, p.duration_base_poly = 0.1;
  p.polys_per_swing = 2, p.polys_per_stance_force = 3;
  p.constraint_sets = sets;
  p.reserved_ = 0;
  p.dt_base_motion = 0.025;
  p.base_z_init = -S.model.nominal_stance[0][2];
  S.Build();
  return S;
}

// One distinct pattern's tables against the structure they were made from
static void check_pattern(const char* name, const twr::JacGramPlan& G, const twr::JacGramPattern& P, const twr::Structure& S) {
  const int n = S.n_vars, m = S.n_rows;
  // the structural P^T P, naively
  std::vector<char> dense((size_t)n * n, 0);
  for (int r = 0; r < m; ++r)
    for (int a = S.row_ptr[r]; a < S.row_ptr[r + 1]; ++a)
      for (int b = S.row_ptr[r]; b < S.row_ptr[r + 1]; ++b) dense[(size_t)S.col_idx[a] * n + S.col_idx[b]] = 1;
  int64_t want = 0;
  for (char v : dense) want += v;
  CHECK(P.n == n && P.nnz == want, "%s: n %d nnz %d, want %d and %lld", name, P.n, P.nnz, n, (long long)want);
  const int32_t* rp = table<int32_t>(name, G.tables, P.row_ptr, n + 1);
  const uint16_t* col = table<uint16_t>(name, G.tables, P.col, P.nnz);
  if (!rp || !col || P.nnz != want) return;
  CHECK(rp[0] == 0 && rp[n] == P.nnz, "%s: row_ptr ends", name);
  for (int i = 0; i < n; ++i) {
    CHECK(rp[i] <= rp[i + 1], "%s: row_ptr descends at %d", name, i);
    int cnt = 0;
    for (int j = 0; j < n; ++j) cnt += dense[(size_t)i * n + j];
    CHECK(rp[i + 1] - rp[i] == cnt, "%s: row %d has %d entries, want %d", name, i, rp[i + 1] - rp[i], cnt);
    for (int e = rp[i]; e < rp[i + 1]; ++e) {
      CHECK(col[e] < n && dense[(size_t)i * n + col[e]], "%s: entry (%d, %d) is not in P^T P", name, i, col[e]);
      CHECK(e == rp[i] || col[e] > col[e - 1], "%s: row %d columns do not ascend", name, i);
      CHECK(dense[(size_t)col[e] * n + i], "%s: (%d, %d) has no mirror", name, i, col[e]);   // symmetric
    }
  }
  std::vector<int32_t> rp2, ci2;
  twr::GramPattern(S, &rp2, &ci2);
  CHECK((int)ci2.size() == P.nnz && std::memcmp(rp2.data(), rp, 4 * (n + 1)) == 0, "%s: GramPattern differs from the plan's tables", name);
  for (int e = 0; e < P.nnz && e < (int)ci2.size(); ++e) CHECK(ci2[e] == col[e], "%s: GramPattern column %d", name, e);
  // the lower triangle's entries, the mirrors, the slices and every term
  int64_t lower = 0;
  for (int i = 0; i < n; ++i)
    for (int e = rp[i]; e < rp[i + 1]; ++e) lower += col[e] <= i;
  CHECK(P.lower == lower && P.slices == (lower + twr::kGramSlice - 1) / twr::kGramSlice, "%s: %d lower entries in %d slices, want %lld", name,
        P.lower, P.slices, (long long)lower);
  const int32_t* pos = table<int32_t>(name, G.tables, P.pos, P.lower);
  const int32_t* mirror = table<int32_t>(name, G.tables, P.mirror, P.lower);
  const int32_t* cnt = table<int32_t>(name, G.tables, P.cnt, P.lower);
  const int32_t* sptr = table<int32_t>(name, G.tables, P.slice_ptr, P.slices + 1);
  if (!pos || !mirror || !cnt || !sptr || P.lower != lower) return;
  CHECK(sptr[0] == 0 && sptr[P.slices] == P.n_words, "%s: slice_ptr ends", name);
  const uint64_t* words = table<uint64_t>(name, G.tables, P.words, (size_t)P.n_words);
  if (!words) return;
  std::vector<int> row_of(P.nnz);
  for (int i = 0; i < n; ++i) std::fill(row_of.begin() + rp[i], row_of.begin() + rp[i + 1], i);
  std::vector<int> jrow(S.nnz);
  for (int r = 0; r < m; ++r) std::fill(jrow.begin() + S.row_ptr[r], jrow.begin() + S.row_ptr[r + 1], r);
  std::vector<char> written(P.nnz, 0);
  // what every lower entry must add, from the rows of J: (r, position of J_ri, position of J_rj), r ascending
  std::vector<std::vector<uint64_t>> want_of(P.nnz);
  for (int r = 0; r < m; ++r)
    for (int a = S.row_ptr[r]; a < S.row_ptr[r + 1]; ++a)
      for (int b = S.row_ptr[r]; b <= a; ++b) {   // columns ascend: col[b] <= col[a]
        const int i = S.col_idx[a], j = S.col_idx[b];
        const int at = (int)(std::lower_bound(col + rp[i], col + rp[i + 1], (uint16_t)j) - col);
        want_of[at].push_back((uint64_t)r << 48 | (uint64_t)a << 24 | (uint64_t)b);
      }
  int64_t products = 0;
  for (int e = 0; e < P.lower; ++e) {
    const int s = e / twr::kGramSlice, lane = e % twr::kGramSlice;
    CHECK(e == 0 || cnt[e] <= cnt[e - 1], "%s: lists not sorted by length at %d", name, e);
    CHECK(pos[e] >= 0 && pos[e] < P.nnz && mirror[e] >= 0 && mirror[e] < P.nnz, "%s: entry %d outside N", name, e);
    if (!(pos[e] >= 0 && pos[e] < P.nnz && mirror[e] >= 0 && mirror[e] < P.nnz)) continue;
    const int i = row_of[pos[e]], j = col[pos[e]];
    CHECK(i >= j && row_of[mirror[e]] == j && col[mirror[e]] == i, "%s: entry %d = (%d, %d), mirror (%d, %d)", name, e, i, j, row_of[mirror[e]],
          col[mirror[e]]);
    CHECK(!written[pos[e]] && (mirror[e] == pos[e] || !written[mirror[e]]), "%s: (%d, %d) written twice", name, i, j);
    CHECK((mirror[e] == pos[e]) == (i == j), "%s: mirror of (%d, %d)", name, i, j);
    written[pos[e]] = written[mirror[e]] = 1;
    const int64_t width = (sptr[s + 1] - sptr[s]) / twr::kGramSlice;
    CHECK((sptr[s + 1] - sptr[s]) % twr::kGramSlice == 0 && cnt[e] >= 1 && cnt[e] <= width, "%s: entry %d has %d terms in a slice %lld wide", name, e,
          cnt[e], (long long)width);
    if (cnt[e] > width) continue;
    if (lane == 0) CHECK(cnt[e] == width, "%s: slice %d is wider than its first list", name, s);
    // every product J_ri J_rj of every row, exactly once, in ascending r
    const std::vector<uint64_t>& want_terms = want_of[pos[e]];
    CHECK((int)want_terms.size() == cnt[e], "%s: (%d, %d) has %d terms, the rows give %zu", name, i, j, cnt[e], want_terms.size());
    for (int t = 0; t < cnt[e] && t < (int)want_terms.size(); ++t) {
      const uint64_t w = words[sptr[s] + (int64_t)t * twr::kGramSlice + lane];
      const int wr = (int)(w >> 48), wa = (int)((w >> 24) & 0xffffff), wb = (int)(w & 0xffffff);
      CHECK(w == want_terms[t], "%s: term %d of (%d, %d) is (%d, %d, %d)", name, t, i, j, wr, wa, wb);
      CHECK(wa < S.nnz && wb < S.nnz && jrow[wa] == wr && jrow[wb] == wr && S.col_idx[wa] == i && S.col_idx[wb] == j,
            "%s: term %d of (%d, %d) is outside its row of J or names other columns", name, t, i, j);
    }
    for (int64_t u = cnt[e]; u < width; ++u)
      CHECK(words[sptr[s] + u * twr::kGramSlice + lane] == twr::kGramPad, "%s: padding of entry %d", name, e);
    products += cnt[e];
  }
  for (int e = P.lower; e < P.slices * twr::kGramSlice; ++e) {   // the lanes behind the last entry: padding alone
    const int s = e / twr::kGramSlice, lane = e % twr::kGramSlice;
    for (int64_t u = 0; u < (sptr[s + 1] - sptr[s]) / twr::kGramSlice; ++u)
      CHECK(words[sptr[s] + u * twr::kGramSlice + lane] == twr::kGramPad, "%s: padding behind the last entry", name);
  }
  for (int e = 0; e < P.nnz; ++e) CHECK(written[e], "%s: value %d of N is never written", name, e);
  CHECK(products == P.products, "%s: %lld products, the plan says %lld", name, (long long)products, (long long)P.products);
  int64_t lower_products = 0;
  for (int r = 0; r < m; ++r) {
    const int64_t len = S.row_ptr[r + 1] - S.row_ptr[r];
    lower_products += len * (len + 1) / 2;
  }
  CHECK(products == lower_products, "%s: %lld products, the rows of J give %lld", name, (long long)products, (long long)lower_products);
}

// Everything PlanJacGram returns, as one number
static uint64_t gram_fingerprint(const twr::JacGramPlan& G) {
  Fnv f;
  f.vec64(G.x_off), f.vec64(G.g_off), f.vec64(G.j_off), f.vec64(G.gram_off), f.vec64(G.tables), f.vec64(G.patterns);
  f.vec64(G.pattern_of_struct), f.vec64(G.form), f.vec64(G.mul), f.vec64(G.solve), f.i64(G.max_n);
  return f.h;
}
static_assert(sizeof(twr::JacGramPattern) == 88 && sizeof(twr::JacGramWork) == 72 && sizeof(twr::JacGramMulWork) == 40 &&
                  sizeof(twr::JacGramSolveWork) == 40,
              "hashed as bytes: no padding");

// Recorded from the commit before the planner was cut into units (this driver with -DTWR_RECORD_PARENT): the plan before
// and after Place.
static const ParentRecord<2> kParent[] = {
    {"hopper_all", {0x78885fe5fd7f6a9dull, 0x8d2d9e53793387b7ull}},
    {"twins", {0xfe647b65299b3bfcull, 0xb2f96087f081483aull}},
    {"mixed", {0x5ec1f26ba9ccbac5ull, 0xe9310c4b7fbb3c27ull}},
};

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, int want_distinct,
                      bool recorded = false) {
  const twr::JacGramPlan G = twr::PlanJacGram(sp, sop), H = twr::PlanJacGram(sp, sop);
  if (recorded) {
    twr::JacGramPlan placed = G;
    placed.Place(0x7e0000000000ull);
    const uint64_t hash[2] = {gram_fingerprint(G), gram_fingerprint(placed)};
    parent_record(kParent, name, hash);
  }
  const twr::JacOpsPlan J = twr::PlanJacOps(sp, sop);
  CHECK(same_bytes(G.tables, H.tables) && same_bytes(G.form, H.form) && same_bytes(G.mul, H.mul) && same_bytes(G.solve, H.solve) &&
            G.gram_off == H.gram_off,
        "%s: planning twice differs", name);
  CHECK(G.x_off == J.x_off && G.g_off == J.g_off && G.j_off == J.j_off, "%s: layout differs from PlanJacOps", name);
  CHECK(G.pattern_of_struct == J.pattern_of_struct && (int)G.patterns.size() == J.distinct_patterns, "%s: patterns are not shared as PlanJacOps shares them",
        name);
  CHECK((int)G.patterns.size() == want_distinct, "%s: %zu distinct patterns, want %d", name, G.patterns.size(), want_distinct);
  const int n = (int)sop.size();
  std::vector<char> seen(G.patterns.size(), 0);
  for (size_t i = 0; i < sp.size(); ++i) {
    const int q = G.pattern_of_struct[i];
    if (seen[q]) continue;
    seen[q] = 1;
    check_pattern(name, G, G.patterns[q], *sp[i]);
  }
  // gram_off: monotone, 16-byte aligned, room for every problem's values
  CHECK((int)G.gram_off.size() == n + 1 && G.gram_off[0] == 0, "%s: gram_off", name);
  int max_n = 0;
  size_t fi = 0, mi = 0;
  for (int p = 0; p < n; ++p) {
    const twr::Structure& S = *sp[sop[p]];
    const twr::JacGramPattern& P = G.patterns[G.pattern_of_struct[sop[p]]];
    CHECK(G.gram_off[p] % 2 == 0 && G.gram_off[p + 1] >= G.gram_off[p] + P.nnz && G.gram_off[p + 1] <= G.gram_off[p] + P.nnz + 1,
          "%s: gram_off of problem %d", name, p);
    max_n = std::max(max_n, S.n_vars);
    // every sorted entry in exactly one formation item, every row of N in exactly one product item, in order
    int next = 0;
    for (; fi < G.form.size() && G.form[fi].gram_off == G.gram_off[p] && G.form[fi].j_off == G.j_off[p] && next < P.lower; ++fi) {
      const twr::JacGramWork& w = G.form[fi];
      CHECK(w.e0 == next && w.e1 > w.e0 && w.e1 - w.e0 <= twr::kGramThreads && w.e0 % twr::kGramSlice == 0 && w.e1 <= P.lower,
            "%s: formation item [%d, %d) of problem %d after %d", name, w.e0, w.e1, p, next);
      CHECK(w.g_off == G.g_off[p] && w.pos == P.pos && w.mirror == P.mirror && w.cnt == P.cnt && w.slice_ptr == P.slice_ptr && w.words == P.words,
            "%s: formation item of problem %d reads other tables", name, p);
      next = w.e1;
    }
    CHECK(next == P.lower, "%s: problem %d forms %d of %d entries", name, p, next, P.lower);
    next = 0;
    for (; mi < G.mul.size() && G.mul[mi].x_off == G.x_off[p] && next < S.n_vars; ++mi) {
      const twr::JacGramMulWork& w = G.mul[mi];
      CHECK(w.r0 == next && w.r1 > w.r0 && w.r1 - w.r0 <= twr::kGramThreads && w.r1 <= S.n_vars && w.gram_off == G.gram_off[p] &&
                w.row_ptr == P.row_ptr && w.col == P.col,
            "%s: product item [%d, %d) of problem %d", name, w.r0, w.r1, p);
      next = w.r1;
    }
    CHECK(next == S.n_vars, "%s: problem %d multiplies %d of %d rows", name, p, next, S.n_vars);
    CHECK((int)G.solve.size() == n && G.solve[p].x_off == G.x_off[p] && G.solve[p].gram_off == G.gram_off[p] && G.solve[p].n == S.n_vars &&
              G.solve[p].row_ptr == P.row_ptr && G.solve[p].col == P.col,
          "%s: solve item of problem %d", name, p);
  }
  CHECK(fi == G.form.size() && mi == G.mul.size(), "%s: work items of no problem", name);
  CHECK(G.max_n == max_n, "%s: max_n %d, want %d", name, G.max_n, max_n);
  int64_t words = 0, nnz = 0;
  for (const auto& P : G.patterns) words += P.n_words, nnz += P.nnz;
  std::printf("gram plan %-10s %4d problems, %zu patterns: nnz N %lld, %lld table words, %zu + %zu work items, tables %zu B\n", name, n,
              G.patterns.size(), (long long)nnz, (long long)words, G.form.size(), G.mul.size(), G.tables.size());
}

template <class F>
static void expect_unsupported(const char* what, F f) {
  bool threw = false;
  try {
    f();
  } catch (const twr::JacGramUnsupported& e) {
    threw = std::strlen(e.what()) > 0;
  } catch (const std::exception&) {
  }
  CHECK(threw, "%s: not refused as unsupported", what);
}

int main() {
  const twr::Structure c1 = hopper(27), hopper_all = hopper(127), biped_all = build(1, 0, 0, 2.0, 127, 1.0, 40);
  const twr::Structure anymal = build(3, 0, 1, 2.0, 27, 1.0, 21), anymal_twin = build(3, 0, 1, 2.0, 27, 1.0, 21);
  plan_case("C1", {&c1}, {0}, 1);
  plan_case("hopper_all", {&hopper_all}, {0, 0, 0}, 1, true);
  plan_case("biped_all", {&biped_all}, {0}, 1);
  plan_case("anymal", {&anymal}, {0, 0}, 1);
  plan_case("twins", {&anymal, &anymal_twin, &c1}, {0, 1, 2, 1, 0}, 2, true);   // byte-identical patterns share tables
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 6; ++i) ss.push_back(build(i % 2 ? 2 : 1, 4, i % 3, 1.2 + 0.3 * i, i % 3 == 2 ? 127 : (i % 2 ? 27 : 63), 0.9, 14 + 3 * i));
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 3, 1, 1, 0}, 6);
  // no rows: N has no entries; an empty column between full ones; explicit structure made by hand
  const twr::Structure empty = pattern(7, {}, {}, 1), holes = pattern(9, {0, 2, 5, 0}, {2, 3, 2, 0}, 2);
  plan_case("no rows", {&empty}, {0, 0, 0}, 1);
  plan_case("mixed", {&empty, &holes, &c1}, {1, 0, 2, 0, 1}, 3, true);
  {
    const twr::JacGramPlan G = twr::PlanJacGram({&empty}, {0, 0});
    CHECK(G.gram_off.back() == 0 && G.form.empty() && G.patterns[0].nnz == 0 && G.solve.size() == 2, "no rows: N is not empty");
  }
  // the limits of the packing and of the solve's LDS
  CHECK(twr::kGramMaxVars == 3412 && (size_t)8 * (twr::kGramSolveVectors * twr::kGramMaxVars + twr::kGramRed) <= (size_t)twr::kGramLdsBytes,
        "kGramMaxVars %d", twr::kGramMaxVars);
  const twr::Structure fits = pattern(twr::kGramMaxVars, {0, 5}, {3, 2}, 1), wide = pattern(twr::kGramMaxVars + 1, {0, 5}, {3, 2}, 1);
  plan_case("widest", {&fits}, {0}, 1);
  expect_unsupported("more variables than the LDS holds", [&] { twr::PlanJacGram({&c1, &wide}, {0, 1}); });
  const twr::Structure tall = pattern(4, std::vector<int>(twr::kGramMaxRows + 1, 1), std::vector<int>(twr::kGramMaxRows + 1, 1), 1);
  expect_unsupported("more rows than 16 bits hold", [&] { twr::PlanJacGram({&tall}, {0}); });
  const twr::Structure tallest = pattern(4, std::vector<int>(twr::kGramMaxRows, 1), std::vector<int>(twr::kGramMaxRows, 2), 1);
  {
    const twr::JacGramPlan G = twr::PlanJacGram({&tallest}, {0});   // the last row the packing holds
    const uint64_t* words = table<uint64_t>("tallest", G.tables, G.patterns[0].words, (size_t)G.patterns[0].n_words);
    const int32_t* cnt = table<int32_t>("tallest", G.tables, G.patterns[0].cnt, 3);
    CHECK(G.patterns[0].lower == 3 && cnt && cnt[0] == twr::kGramMaxRows, "tallest: lists");
    if (words && cnt) CHECK((int)(words[(int64_t)(cnt[0] - 1) * twr::kGramSlice] >> 48) == twr::kGramMaxRows - 1, "tallest: the last row's index");
  }
  const twr::Structure fat = pattern(300, std::vector<int>(twr::kGramMaxRows, 0), std::vector<int>(twr::kGramMaxRows, 257), 1);
  CHECK(fat.nnz > twr::kGramMaxNnz, "the fat pattern has %d entries", fat.nnz);
  expect_unsupported("more Jacobian entries than 24 bits hold", [&] { twr::PlanJacGram({&fat}, {0}); });
  // the invariants the kernels rely on are checked, not assumed
  twr::Structure dup = c1;
  dup.col_idx[1] = dup.col_idx[0];
  bool threw = false;
  try {
    twr::PlanJacGram({&dup}, {0});
  } catch (const twr::JacGramUnsupported&) {
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a plan over a duplicate entry was accepted");
  threw = false;
  try {
    twr::PlanJacGram({&c1}, {0, 1});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a struct_of_problem out of range was accepted");
  std::printf("jac_gram_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
