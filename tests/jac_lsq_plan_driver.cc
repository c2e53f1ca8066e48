// Checks of the least-squares plan (twr_jac_lsq_*) on the host: the work records, the workspace segments and the bound tables
// twr::PlanJacLsq builds.  Built and run by tests/test_jac_lsq_plan.py (tests/host_build.py: g++ against the host planner under
// ASan + UBSan, no HIP).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

static bool same_bounds(const twr::Structure& a, const twr::Structure& b) {
  const size_t bytes = a.lower.size() * sizeof(double);
  return a.lower.size() == b.lower.size() && a.upper.size() == b.upper.size() &&
         (bytes == 0 || (std::memcmp(a.lower.data(), b.lower.data(), bytes) == 0 && std::memcmp(a.upper.data(), b.upper.data(), bytes) == 0));
}

// Everything PlanJacLsq returns, as one number
static uint64_t lsq_fingerprint(const twr::JacLsqPlan& L) {
  Fnv f;
  f.vec64(L.x_off), f.vec64(L.g_off), f.vec64(L.work), f.vec64(L.bounds), f.vec64(L.bounds_of_struct);
  for (int64_t v : {(int64_t)L.distinct_bounds, L.ws_p, L.ws_z, L.ws_q, L.ws_r, L.ws_t, L.ws_rec, L.ws_doubles, L.ws2_e, L.ws2_cp, L.ws2_doubles,
                    L.ws3_s, L.ws3_u, L.ws3_doubles, (int64_t)L.lds_x})
    f.i64(v);
  return f.h;
}
static_assert(sizeof(twr::JacLsqWork) == 40, "hashed as bytes: no padding");

// Recorded from the commit before the planner was cut into units (this driver with -DTWR_RECORD_PARENT): the plan before
// and after Place.
static const ParentRecord<2> kParent[] = {
    {"twins", {0x4502fb002bb309d5ull, 0x11aa9304196727b5ull}},
    {"every", {0x840001f8bca32d82ull, 0x0229a978e9e73ff6ull}},
    {"per-row", {0x88195663af5b544cull, 0x431510b258405ad4ull}},
};

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, int want_distinct,
                      bool recorded = false) {
  const twr::JacLsqPlan L = twr::PlanJacLsq(sp, sop), K = twr::PlanJacLsq(sp, sop);
  if (recorded) {
    twr::JacLsqPlan placed = L;
    placed.Place(0x7e0000000000ull);
    const uint64_t hash[2] = {lsq_fingerprint(L), lsq_fingerprint(placed)};
    parent_record(kParent, name, hash);
  }
  CHECK(same_bytes(L.work, K.work) && same_bytes(L.bounds, K.bounds) && L.bounds_of_struct == K.bounds_of_struct &&
            L.ws_doubles == K.ws_doubles && L.ws_rec == K.ws_rec,
        "%s: planning twice differs", name);
  const twr::JacOpsPlan J = twr::PlanJacOps(sp, sop);
  CHECK(L.x_off == J.x_off && L.g_off == J.g_off, "%s: layout differs from PlanJacOps", name);
  CHECK(L.lds_x == J.mul_lds_x, "%s: lds_x %d, the products stage %d", name, L.lds_x, J.mul_lds_x);
  const int n = (int)sop.size(), ns = (int)sp.size();
  const int64_t X = L.x_off[n], G = L.g_off[n];
  // the workspace: five vector segments and the scalar records, disjoint, in the allocation, on 16-byte boundaries
  std::vector<std::pair<int64_t, int64_t>> seg = {{L.ws_p, X}, {L.ws_z, X}, {L.ws_q, G}, {L.ws_r, G}, {L.ws_t, G},
                                                  {L.ws_rec, (int64_t)twr::kLsqRec * n}};
  for (const auto& s : seg) {
    CHECK(s.first >= 0 && s.first % 2 == 0 && s.first + s.second <= L.ws_doubles, "%s: segment [%lld, +%lld) outside %lld or odd", name,
          (long long)s.first, (long long)s.second, (long long)L.ws_doubles);
  }
  std::sort(seg.begin(), seg.end());
  for (size_t i = 0; i + 1 < seg.size(); ++i)
    CHECK(seg[i].first + seg[i].second <= seg[i + 1].first, "%s: workspace segments %zu and %zu overlap", name, i, i + 1);
  CHECK(twr::kLsqRec > std::max({(int)twr::kLsqGamma, (int)twr::kLsqGamma0, (int)twr::kLsqIters, (int)twr::kLsqState}),
        "%s: a scalar slot outside the record", name);
  // every problem's record: its own offsets and sizes, its structure's bounds
  CHECK((int)L.work.size() == n, "%s: %zu records for %d problems", name, L.work.size(), n);
  for (int p = 0; p < n && p < (int)L.work.size(); ++p) {
    const twr::Structure& S = *sp[sop[p]];
    const twr::JacLsqWork& w = L.work[p];
    CHECK(w.x_off == L.x_off[p] && w.g_off == L.g_off[p] && w.n == S.n_vars && w.m == S.n_rows, "%s: record of problem %d", name, p);
    CHECK(w.x_off + w.n == L.x_off[p + 1] && w.g_off + w.m == L.g_off[p + 1], "%s: problem %d reaches into its neighbour", name, p);
    const size_t bytes = (size_t)S.n_rows * sizeof(double);
    const bool in = w.lower % 16 == 0 && w.upper % 16 == 0 && w.lower + bytes <= L.bounds.size() && w.upper + bytes <= L.bounds.size();
    CHECK(in, "%s: bound tables of problem %d outside the blob or misaligned", name, p);
    if (in && bytes)
      CHECK(std::memcmp(L.bounds.data() + w.lower, S.lower.data(), bytes) == 0 && std::memcmp(L.bounds.data() + w.upper, S.upper.data(), bytes) == 0,
            "%s: bound tables of problem %d are not its structure's", name, p);
    CHECK(w.lower + bytes <= w.upper || w.upper + bytes <= w.lower, "%s: lower and upper of problem %d overlap", name, p);
  }
  // shared exactly when byte-identical, and every distinct table stored once
  CHECK((int)L.bounds_of_struct.size() == ns, "%s: bounds_of_struct", name);
  int distinct = 0;
  size_t want_bytes = 0;
  for (int i = 0; i < ns; ++i) {
    bool seen = false;
    for (int j = 0; j < i; ++j) {
      const bool same = same_bounds(*sp[i], *sp[j]);
      seen |= same;
      CHECK((L.bounds_of_struct[i] == L.bounds_of_struct[j]) == same, "%s: structures %d and %d: shared %d, identical %d", name, i, j,
            L.bounds_of_struct[i] == L.bounds_of_struct[j], (int)same);
    }
    if (!seen) {
      ++distinct;
      want_bytes += 2 * ((sp[i]->lower.size() * sizeof(double) + 15) / 16 * 16);
    }
  }
  CHECK(L.distinct_bounds == distinct && distinct == want_distinct, "%s: %d distinct bound tables, counted %d, want %d", name,
        L.distinct_bounds, distinct, want_distinct);
  CHECK(L.bounds.size() <= want_bytes, "%s: bound blob of %zu bytes, %zu would do", name, L.bounds.size(), want_bytes);
  // Place() moves the table fields and nothing else
  twr::JacLsqPlan P = L;
  const uint64_t base = 0x7f0000001000ull;
  P.Place(base);
  for (int p = 0; p < n; ++p)
    CHECK(P.work[p].lower == L.work[p].lower + base && P.work[p].upper == L.work[p].upper + base && P.work[p].x_off == L.work[p].x_off &&
              P.work[p].g_off == L.work[p].g_off && P.work[p].n == L.work[p].n && P.work[p].m == L.work[p].m,
          "%s: Place() on problem %d", name, p);
  // the record of a problem is its structure's: the same in a one-problem plan, up to the offsets
  for (int p = 0; p < n; ++p) {
    const twr::JacLsqPlan A = twr::PlanJacLsq({sp[sop[p]]}, {0});
    CHECK(A.work.size() == 1 && A.work[0].n == L.work[p].n && A.work[0].m == L.work[p].m && A.work[0].x_off == 0 && A.work[0].g_off == 0,
          "%s: problem %d alone", name, p);
  }
  std::printf("lsq plan %-10s %4d problems: %d distinct bound tables in %zu B, workspace %lld doubles, lds_x %d\n", name, n, L.distinct_bounds,
              L.bounds.size(), (long long)L.ws_doubles, L.lds_x);
}

int main() {
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63, 1.0, 200), c3_hot = build(3, 0, 1, 2.0, 27, 1.0, 200), c3_twin = build(3, 0, 1, 2.0, 27, 1.0, 200);
  const twr::Structure every = build(3, 2, 0, 2.4, 255, 1.1, 200);   // every family, optimised timings, base_z_init set
  plan_case("C3x16", {&c3_hot}, std::vector<int32_t>(16, 0), 1);
  plan_case("twins", {&c3_hot, &c3_twin}, {0, 1, 1, 0}, 1, true);   // two structures from identical inputs: one table
  plan_case("every", {&every, &c3}, {0, 1, 0}, 2, true);
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
  plan_case("grid", {&g1, &c3_hot}, {1, 0, 0}, same_bounds(g1, c3_hot) ? 1 : 2);
  const twr::Structure wide = build(3, 0, 1, 2.0, 27, 1.0, 200, nullptr, 0.003);   // s does not fit the LDS copy
  CHECK(wide.n_vars > twr::kJacLdsX, "the wide structure has %d variables", wide.n_vars);
  plan_case("wide", {&wide, &c3_hot}, {0, 1}, 1);   // another pattern, the same rows and bounds: one table
  // per-row bounds of any kind: one changed bound, a zero of the other sign and more distinct pairs than a compact score record
  // holds (127) each make a table of their own
  CHECK(c3_hot.n_rows > 400, "C3 has %d rows", c3_hot.n_rows);
  twr::Structure moved = c3_hot, negzero = c3_hot, many = c3_hot;
  moved.upper[moved.n_rows / 2] += 0.125;
  int zero_at = -1;
  for (int r = 0; r < negzero.n_rows && zero_at < 0; ++r)
    if (negzero.lower[r] == 0.0 && !std::signbit(negzero.lower[r])) zero_at = r;
  CHECK(zero_at >= 0, "C3 has no row with a lower bound of 0");
  if (zero_at >= 0) negzero.lower[zero_at] = -0.0;
  for (int r = 0; r < 400; ++r) many.lower[r] = -1.0 - r, many.upper[r] = 2.0 + 0.5 * r;
  plan_case("per-row", {&c3_hot, &moved, &negzero, &many, &c3_twin}, {0, 1, 2, 3, 4, 3, 2, 1, 0}, 4, true);
  bool threw = false;
  try {
    twr::PlanJacLsq({&c3_hot}, {0, 1});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a struct_of_problem entry out of range was accepted");
  threw = false;
  twr::Structure torn = c3_hot;
  torn.upper.pop_back();
  try {
    twr::PlanJacLsq({&torn}, {0});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "bounds shorter than the rows were accepted");
  std::printf("jac_lsq_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
