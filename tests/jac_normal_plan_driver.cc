// Checks of the one-pass normal product's plan (twr_jac_normal_mul) on the host: the tables and work lists twr::PlanJacNormal
// builds, and that twr::PlanJacOps still gives what it gave.  Built and run by tests/test_jac_normal_plan.py
// (tests/host_build.py: g++ against the host planner, no HIP).  With a directory as argument, every case's emulation of the plan's summation order on a
// random matrix is written there for the test to hold against scipy.  -DOPS_ONLY leaves out everything PlanJacNormal: the
// program then only prints the fingerprints of PlanJacOps (how the ones in the test were taken from the commit before).
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

// Everything PlanJacOps returns, as one number
static uint64_t ops_fingerprint(const twr::JacOpsPlan& J) {
  Fnv f;
  f.vec64(J.x_off), f.vec64(J.g_off), f.vec64(J.j_off), f.vec64(J.tables), f.vec64(J.pattern_of_struct);
  f.vec64(J.mul), f.vec64(J.tmul), f.vec64(J.fold);
  for (int64_t v : {(int64_t)J.distinct_patterns, J.slab, (int64_t)J.mul_lds_x, J.table_bytes_mul, J.table_bytes_tmul}) f.i64(v);
  return f.h;
}

#ifndef OPS_ONLY
// Everything PlanJacNormal returns
static uint64_t normal_fingerprint(const twr::JacNormalPlan& N) {
  Fnv f;
  f.vec64(N.x_off), f.vec64(N.g_off), f.vec64(N.j_off), f.vec64(N.tables), f.vec64(N.work), f.vec64(N.fold);
  f.i64(N.slab), f.i64(N.lds_x), f.i64(N.tile);
  return f.h;
}

// Recorded from the commit before the planner was cut into units (this driver with -DTWR_RECORD_PARENT): the products' plan
// after Place (before it: OPS_FINGERPRINTS of tests/test_jac_normal_plan.py), the one-pass plan at tiles of 256 and 1024
// entries before and after Place.
// {PlanJacOps placed; PlanJacNormal at a tile of 256, placed, at 1024, placed}
static const ParentRecord<5> kParent[] = {
    {"C3x16", {0x8e2becdde03d5e1eull, 0x8071889574083d95ull, 0xa89ea3d7852fe679ull, 0x81b73abadd89f034ull, 0xbf975fc11cff7a90ull}},
    {"twins", {0xc0650b918436d2b1ull, 0xa7ca115457f5a065ull, 0x289f102421911eedull, 0xf7927d2d6e533d1aull, 0xb3043811888e4abeull}},
    {"every", {0x3fc121df9bd4e0ffull, 0x7300c98e216ed2edull, 0x96d5ad51ae228ef5ull, 0xced325113e59cc41ull, 0x9c57fa596e99ef3eull}},
    {"ragged", {0x78e115d51d01f5adull, 0x5645be43d402c5efull, 0x55ce00823feb4c77ull, 0xd060b78b4750edebull, 0x4574397672168224ull}},
    {"grid", {0xdb169c20c50b6089ull, 0x30145d001c681739ull, 0x8187c221485f1c5eull, 0xabefaefddf0f163eull, 0xd8f7f9a80d119cdeull}},
    {"wide", {0x6d2c011f92496debull, 0xbb8971a5f900a5d7ull, 0x5aac340088141f1bull, 0xc96cb970e2759ab4ull, 0x748570666619dc0cull}},
    {"longrow", {0x4a47bf587cede2c9ull, 0x09fd84d2760dd97cull, 0x87cf897ad5044217ull, 0x10441f2ccd0979a1ull, 0x7e601572474bf245ull}},
};
static const uint64_t kOpsBase = 0x7e0000000000ull, kNormalBase = 0x7d0000000000ull;
#endif

#ifndef OPS_ONLY
struct Shape {   // one problem's work records relative to the problem, and the order of the terms of every partial and column
  std::vector<int64_t> shape;
  std::vector<std::vector<int>> partial;   // [slot] -> CSR positions in summation order
  std::vector<std::vector<int>> fold;      // [column] -> slots in summation order
  bool operator==(const Shape& o) const { return shape == o.shape && partial == o.partial && fold == o.fold; }
};

static Shape check_problem(const char* name, const twr::JacNormalPlan& N, const twr::JacOpsPlan& J, const twr::Structure& S, int p,
                           const std::vector<const twr::JacNormalWork*>& work, const std::vector<const twr::JacFoldWork*>& fold,
                           int64_t slab0, int64_t slab1) {
  const int n = S.n_vars, m = S.n_rows, nnz = S.nnz;
  Shape o;
  o.partial.assign(slab1 - slab0, {});
  o.fold.assign(n, {});
  std::vector<int> entry_hit(nnz, 0), slot_block(slab1 - slab0, -1), slot_col(slab1 - slab0, -1);
  int next_r = 0, b = 0;
  for (const twr::JacNormalWork* w : work) {
    CHECK(w->x_off == N.x_off[p] && w->g_off == N.g_off[p] && w->j_off == N.j_off[p] && w->n == n, "%s: offsets of problem %d", name, p);
    CHECK(w->r0 == next_r && w->r0 < w->r1 && w->r1 <= m, "%s: rows [%d, %d) after %d", name, w->r0, w->r1, next_r);   // whole rows, in order
    next_r = w->r1;
    // the pattern's tables are the ones PlanJacOps made for the same arguments
    const int32_t* rp = table<int32_t>(name, J.tables, w->row_ptr, m + 1);
    const uint16_t* col = table<uint16_t>(name, J.tables, w->col, nnz);
    if (!rp || !col) continue;
    CHECK(std::memcmp(rp, S.row_ptr.data(), S.row_ptr.size() * 4) == 0, "%s: row_ptr table", name);
    for (int k = 0; k < nnz; ++k) CHECK(col[k] == S.col_idx[k], "%s: col table at %d", name, k);
    const int k0 = rp[w->r0], k1 = rp[w->r1], e = k1 - k0;
    CHECK(w->slab >= slab0 && w->slab + w->ncols <= slab1, "%s: partials of block %d outside the problem's slab", name, b);
    o.shape.insert(o.shape.end(), {w->r0, w->r1, w->ncols, w->is_long, w->slab - slab0});
    if (w->slab < slab0 || w->slab + w->ncols > slab1) continue;
    for (int k = k0; k < k1; ++k) ++entry_hit[k];
    if (w->is_long) {
      CHECK(w->r1 - w->r0 == 1 && e > twr::kJacNormNnz && w->ncols == e, "%s: long block of %d rows, %d entries", name, w->r1 - w->r0, e);
      for (int i = 0; i < e; ++i) {
        const int64_t s = w->slab - slab0 + i;
        CHECK(slot_block[s] < 0, "%s: partial %lld written twice", name, (long long)s);
        slot_block[s] = b, slot_col[s] = S.col_idx[k0 + i];
        o.partial[s] = {k0 + i};
      }
    } else {
      CHECK(w->r1 - w->r0 <= twr::kJacThreads && e <= twr::kJacNormNnz, "%s: block of %d rows, %d entries", name, w->r1 - w->r0, e);
      if (e == 0) {
        CHECK(w->ncols == 0, "%s: an empty block with columns", name);
      } else {
        const uint16_t* map = table<uint16_t>(name, N.tables, w->map, (size_t)w->ncols + 1 + e);
        if (!map) continue;
        const uint16_t* pos = map + w->ncols + 1;
        CHECK(w->ncols >= 1 && map[0] == 0 && map[w->ncols] == e, "%s: map ends", name);
        int prev_col = -1;
        for (int j = 0; j < w->ncols; ++j) {
          CHECK(map[j] < map[j + 1] && map[j + 1] <= e, "%s: column %d of block %d", name, j, b);
          if (!(map[j] < map[j + 1] && map[j + 1] <= e)) break;
          const int64_t s = w->slab - slab0 + j;
          CHECK(slot_block[s] < 0, "%s: partial %lld written twice", name, (long long)s);
          CHECK(pos[map[j]] < e, "%s: map entry outside the block", name);
          const int c = S.col_idx[k0 + pos[map[j]] % e];
          CHECK(c > prev_col, "%s: block columns not ascending", name);
          prev_col = c;
          slot_block[s] = b, slot_col[s] = c;
          for (int i = map[j]; i < map[j + 1]; ++i) {
            CHECK(pos[i] < e, "%s: map entry outside the block", name);
            const int k = k0 + pos[i] % e;
            CHECK(S.col_idx[k] == c, "%s: map entry of another column", name);
            CHECK(o.partial[s].empty() || k > o.partial[s].back(), "%s: column terms not in row order", name);
            o.partial[s].push_back(k);
          }
        }
      }
    }
    ++b;
  }
  CHECK(next_r == m, "%s: blocks end at row %d of %d", name, next_r, m);
  std::vector<int> term_hit(nnz, 0);
  for (const auto& t : o.partial)
    for (int k : t) ++term_hit[k];
  int bad = 0;
  for (int k = 0; k < nnz; ++k) bad += entry_hit[k] != 1 || term_hit[k] != 1;
  CHECK(bad == 0, "%s: problem %d: %d entries not in exactly one block and one partial", name, p, bad);
  for (size_t s = 0; s < slot_block.size(); ++s) CHECK(slot_block[s] >= 0, "%s: partial %zu of the slab is nobody's", name, s);
  std::vector<int> slot_folded(slab1 - slab0, 0);
  int next_c = 0;
  for (const twr::JacFoldWork* f : fold) {
    CHECK(f->x_off == N.x_off[p] && f->slab == slab0, "%s: fold offsets of problem %d", name, p);
    CHECK(f->c0 == next_c && f->c0 < f->c1 && f->c1 <= n && f->c1 - f->c0 <= twr::kJacFoldCols, "%s: fold columns", name);
    next_c = f->c1;
    const int32_t* ptr = table<int32_t>(name, N.tables, f->ptr, n + 1);
    if (!ptr) continue;
    CHECK(ptr[0] == 0 && ptr[n] == slab1 - slab0, "%s: fold_ptr ends", name);
    const int32_t* slot = table<int32_t>(name, N.tables, f->slot, (size_t)std::max(0, ptr[n]));
    if (!slot) continue;
    for (int c = f->c0; c < f->c1; ++c) {
      int prev_block = -1;
      for (int i = ptr[c]; i < ptr[c + 1]; ++i) {
        const int s = slot[i];
        CHECK(s >= 0 && s < slab1 - slab0, "%s: column %d folds a partial outside the problem's slab", name, c);
        if (s < 0 || s >= slab1 - slab0) continue;
        CHECK(slot_col[s] == c, "%s: column %d folds a partial of column %d", name, c, slot_col[s]);
        CHECK(slot_block[s] > prev_block, "%s: column %d not folded in block order", name, c);
        prev_block = slot_block[s];
        ++slot_folded[s];
        o.fold[c].push_back(s);
      }
    }
  }
  CHECK(next_c == n, "%s: fold columns end at %d of %d", name, next_c, n);
  for (size_t s = 0; s < slot_folded.size(); ++s) CHECK(slot_folded[s] == 1, "%s: partial %zu folded %d times", name, s, slot_folded[s]);
  return o;
}

// y = J v and u = J^T (w o y) of one problem in the order the kernels add: a row's products in column order, a partial's terms
// in the order of the block's map, a column's partials in the order of the fold table.
static void emulate(const twr::Structure& S, const Shape& o, std::FILE* out) {
  const int n = S.n_vars, m = S.n_rows, nnz = S.nnz;
  std::mt19937_64 rng(12345 + 31 * n + m);
  std::normal_distribution<double> nd;
  std::uniform_real_distribution<double> ud(0.1, 3.0);
  std::vector<double> a(nnz), v(n), w(m), y(m, 0.0), u(n, 0.0);
  for (auto& x : a) x = nd(rng) * std::exp(3.0 * nd(rng));
  for (auto& x : v) x = nd(rng);
  for (auto& x : w) x = ud(rng);
  std::vector<int> row_of(nnz);
  for (int r = 0; r < m; ++r) {
    for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
      y[r] += a[k] * v[S.col_idx[k]];
      row_of[k] = r;
    }
  }
  std::vector<double> part(o.partial.size(), 0.0);
  for (size_t s = 0; s < o.partial.size(); ++s)
    for (int k : o.partial[s]) part[s] += a[k] * (w[row_of[k]] * y[row_of[k]]);
  for (int c = 0; c < n; ++c)
    for (int s : o.fold[c]) u[c] += part[s];
  const int64_t head[3] = {n, m, nnz};
  std::fwrite(head, sizeof head, 1, out);
  std::fwrite(S.row_ptr.data(), 4, m + 1, out);
  std::fwrite(S.col_idx.data(), 4, nnz, out);
  std::fwrite(a.data(), 8, nnz, out);
  std::fwrite(v.data(), 8, n, out);
  std::fwrite(w.data(), 8, m, out);
  std::fwrite(y.data(), 8, m, out);
  std::fwrite(u.data(), 8, n, out);
}
#endif   // OPS_ONLY

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, const char* dir) {
  const twr::JacOpsPlan J = twr::PlanJacOps(sp, sop);
  std::printf("opsplan %s %016llx\n", name, (unsigned long long)ops_fingerprint(J));
#ifndef OPS_ONLY
  twr::JacOpsPlan placed = J;
  placed.Place(kOpsBase);
  uint64_t hash[5] = {ops_fingerprint(placed)};
  for (int t = 0; t < 2; ++t) {
    twr::JacNormalPlan T = twr::PlanJacNormal(sp, sop, t ? 1024 : 256);
    hash[1 + 2 * t] = normal_fingerprint(T);
    T.Place(kOpsBase, kNormalBase);
    hash[2 + 2 * t] = normal_fingerprint(T);
  }
  parent_record(kParent, name, hash);
  const twr::JacNormalPlan N = twr::PlanJacNormal(sp, sop), M = twr::PlanJacNormal(sp, sop);
  CHECK(same_bytes(N.tables, M.tables) && same_bytes(N.work, M.work) && same_bytes(N.fold, M.fold) && N.slab == M.slab,
        "%s: planning twice differs", name);
  CHECK(ops_fingerprint(twr::PlanJacOps(sp, sop)) == ops_fingerprint(J), "%s: PlanJacOps differs after PlanJacNormal", name);
  CHECK(N.x_off == J.x_off && N.g_off == J.g_off && N.j_off == J.j_off, "%s: layout differs from PlanJacOps", name);
  const int n = (int)sop.size();
  int lds_x = 0;
  for (int p = 0; p < n; ++p)
    if (sp[sop[p]]->n_vars <= twr::kJacLdsX) lds_x = std::max(lds_x, sp[sop[p]]->n_vars);
  CHECK(N.lds_x == lds_x, "%s: lds_x %d, want %d", name, N.lds_x, lds_x);
  // work records are problem by problem: split them by x_off (every structure has variables)
  std::map<int64_t, int> problem_of_x;
  for (int p = 0; p < n; ++p) problem_of_x[N.x_off[p]] = p;
  std::vector<std::vector<const twr::JacNormalWork*>> work(n);
  std::vector<std::vector<const twr::JacFoldWork*>> fold(n);
  int last = 0;
  for (const auto& w : N.work) {
    const int p = problem_of_x.count(w.x_off) ? problem_of_x[w.x_off] : -1;
    CHECK(p >= last, "%s: work records not problem by problem", name);
    if (p < 0) continue;
    last = p;
    work[p].push_back(&w);
  }
  for (const auto& f : N.fold) {
    CHECK(problem_of_x.count(f.x_off) == 1, "%s: fold record of no problem", name);
    if (problem_of_x.count(f.x_off)) fold[problem_of_x[f.x_off]].push_back(&f);
  }
  // the problems' partials tile the slab in problem order
  std::vector<int64_t> slab_at(n + 1, 0);
  for (int p = 0; p < n; ++p) {
    int64_t cnt = 0;
    for (const auto* w : work[p]) cnt += w->ncols;
    slab_at[p + 1] = slab_at[p] + cnt;
  }
  CHECK(slab_at[n] == N.slab, "%s: slab %lld, the blocks write %lld", name, (long long)N.slab, (long long)slab_at[n]);
  std::vector<Shape> shapes;
  for (int p = 0; p < n; ++p) shapes.push_back(check_problem(name, N, J, *sp[sop[p]], p, work[p], fold[p], slab_at[p], slab_at[p + 1]));
  // the order of terms is the structure's: the same in a one-problem plan of that structure
  std::FILE* out = nullptr;
  if (dir) {
    out = std::fopen((std::string(dir) + "/" + name + ".bin").c_str(), "wb");
    CHECK(out != nullptr, "%s: cannot write to %s", name, dir);
  }
  std::vector<char> done(sp.size(), 0);
  size_t long_blocks = 0;
  for (const auto& w : N.work) long_blocks += w.is_long;
  for (int p = 0; p < n; ++p) {
    if (done[sop[p]]) {
      for (int q = 0; q < p; ++q)
        if (sop[q] == sop[p]) {
          CHECK(shapes[q] == shapes[p], "%s: problems %d and %d of one structure sum in different orders", name, q, p);
          break;
        }
      continue;
    }
    done[sop[p]] = 1;
    const twr::Structure* S = sp[sop[p]];
    const twr::JacNormalPlan A = twr::PlanJacNormal({S}, {0});
    const twr::JacOpsPlan AJ = twr::PlanJacOps({S}, {0});
    std::vector<const twr::JacNormalWork*> aw;
    std::vector<const twr::JacFoldWork*> af;
    for (const auto& w : A.work) aw.push_back(&w);
    for (const auto& f : A.fold) af.push_back(&f);
    CHECK(check_problem(name, A, AJ, *S, 0, aw, af, 0, A.slab) == shapes[p], "%s: problem %d sums in another order than alone", name, p);
    if (out) emulate(*S, shapes[p], out);
  }
  if (out) std::fclose(out);
  std::printf("normal plan %-10s %4d problems: %zu blocks (%zu long) / %zu fold items, slab %lld, tables %zu B\n", name, n, N.work.size(),
              long_blocks, N.fold.size(), (long long)N.slab, N.tables.size());
#else
  (void)dir;
#endif
}

int main(int argc, char** argv) {
  const char* dir = argc > 1 ? argv[1] : nullptr;
  // the six batches of tests/jac_plan_driver.cc
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63, 1.0, 200), c3_hot = build(3, 0, 1, 2.0, 27, 1.0, 200), c3_twin = build(3, 0, 1, 2.0, 27, 1.0, 200);
  const twr::Structure every = build(3, 2, 0, 2.4, 255, 1.1, 200);   // every family, optimised timings, base_z_init set
  plan_case("C3x16", {&c3_hot}, std::vector<int32_t>(16, 0), dir);
  plan_case("twins", {&c3_hot, &c3_twin}, {0, 1, 1, 0}, dir);
  plan_case("every", {&every, &c3}, {0, 1, 0}, dir);
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 6; ++i) ss.push_back(build(i % 2 ? 2 : 1, 4, i % 3, 1.2 + 0.3 * i, i % 2 ? 27 : 63, 0.9, 200));
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 3, 1, 1, 0}, dir);
  auto grid = std::make_shared<twr::TerrainGrid>();
  grid->rows = 40;
  grid->cols = 60;
  for (int i = 0; i < grid->rows * grid->cols; ++i) grid->heights.push_back(0.05 * ((i * 7919) % 13) / 13.0);
  const twr::Structure g1 = build(3, 7, 1, 2.0, 63, 1.0, 200, grid);
  plan_case("grid", {&g1, &c3_hot}, {1, 0, 0}, dir);
  const twr::Structure wide = build(3, 0, 1, 2.0, 27, 1.0, 200, nullptr, 0.003);   // v is gathered from memory
  CHECK(wide.n_vars > twr::kJacLdsX, "the wide structure has %d variables", wide.n_vars);
  plan_case("wide", {&wide, &c3_hot}, {0, 1}, dir);
  // rows longer than one tile: between short rows, first, last, next to an empty row, two in a row; one exactly a tile long
  const int T = 2048;   // twr::kJacNormNnz (checked below)
  const twr::Structure longrow = pattern(3 * T + 7, {0, 5, 0, 1, 0, 9, 2, 0, 3}, {3 * T + 7, 40, 0, T + 1, 2 * T + 5, 17, T, 300, T + 2}, 1);
  const twr::Structure strided = pattern(7000, {0, 1, 2, 3}, {300, 2333, 5, 2300}, 3);   // n > kJacLdsX with long rows
  CHECK(strided.n_vars > twr::kJacLdsX, "the strided pattern has %d variables", strided.n_vars);
  plan_case("longrow", {&longrow, &c3_hot, &strided}, {1, 0, 2, 0}, dir);
#ifndef OPS_ONLY
  CHECK(T == twr::kJacNormNnz, "the long rows were made for a tile of %d entries", T);
  {
    const twr::JacNormalPlan N = twr::PlanJacNormal({&longrow}, {0});
    size_t longs = 0;
    for (const auto& w : N.work) longs += w.is_long;
    CHECK(longs == 4, "the long-row pattern has %zu long blocks, want 4", longs);
  }
  // the invariant the products rely on is checked, not assumed
  twr::Structure dup = c3_hot;
  dup.col_idx[1] = dup.col_idx[0];
  bool threw = false;
  try {
    twr::PlanJacNormal({&dup}, {0});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a plan over a duplicate entry was accepted");
  threw = false;
  try {
    twr::PlanJacNormal({&c3_hot}, {0, 1});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a struct_of_problem out of range was accepted");
#endif
  std::printf("jac_normal_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
