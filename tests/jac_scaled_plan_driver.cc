// Checks of the scaled solve's part of the least-squares plan (twr_jac_lsq_solve_scaled) on the host: the second workspace
// twr::PlanJacLsq plans (ws2_*: e and c o p in the x layout), and that the first workspace keeps the formula it had before the
// scaled solve existed.  Built and run by tests/test_jac_scaled_plan.py (g++ against the host planner under ASan + UBSan,
// no HIP).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <utility>
#include <vector>

#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop) {
  const twr::JacLsqPlan L = twr::PlanJacLsq(sp, sop), K = twr::PlanJacLsq(sp, sop);
  CHECK(L.ws2_e == K.ws2_e && L.ws2_cp == K.ws2_cp && L.ws2_doubles == K.ws2_doubles && L.ws_doubles == K.ws_doubles,
        "%s: planning twice differs", name);
  const int n = (int)sop.size();
  int64_t X = 0, G = 0;   // the layout, summed here from the structures
  for (int p = 0; p < n; ++p) X += sp[sop[p]]->n_vars, G += sp[sop[p]]->n_rows;
  CHECK(L.x_off[n] == X && L.g_off[n] == G, "%s: layout", name);
  // the second allocation: two x-layout segments on 16-byte boundaries, disjoint, inside it, and no larger than two padded vectors
  std::vector<std::pair<int64_t, int64_t>> seg = {{L.ws2_e, X}, {L.ws2_cp, X}};
  for (const auto& s : seg)
    CHECK(s.first >= 0 && s.first % 2 == 0 && s.first + s.second <= L.ws2_doubles, "%s: segment [%lld, +%lld) outside %lld or odd", name,
          (long long)s.first, (long long)s.second, (long long)L.ws2_doubles);
  std::sort(seg.begin(), seg.end());
  CHECK(seg[0].first + seg[0].second <= seg[1].first, "%s: e and c o p overlap", name);
  CHECK(L.ws2_doubles <= 2 * ((X + 1) / 2 * 2), "%s: second workspace of %lld doubles for two vectors of %lld", name,
        (long long)L.ws2_doubles, (long long)X);
  // the first allocation: the formula it had without the scaled solve (p, z; q, r, t; the records), every segment padded to even
  const int64_t Xe = (X + 1) / 2 * 2, Ge = (G + 1) / 2 * 2;
  CHECK(L.ws_p == 0 && L.ws_z == Xe && L.ws_q == 2 * Xe && L.ws_r == 2 * Xe + Ge && L.ws_t == 2 * Xe + 2 * Ge &&
            L.ws_rec == 2 * Xe + 3 * Ge && L.ws_doubles == 2 * Xe + 3 * Ge + (int64_t)twr::kLsqRec * n,
        "%s: the first workspace changed: %lld doubles", name, (long long)L.ws_doubles);
  CHECK((int)L.work.size() == n && sizeof(twr::JacLsqWork) == 40, "%s: work records", name);
  std::printf("scaled plan %-8s %4d problems: workspace %lld doubles, second workspace %lld doubles (e at %lld, c o p at %lld)\n", name, n,
              (long long)L.ws_doubles, (long long)L.ws2_doubles, (long long)L.ws2_e, (long long)L.ws2_cp);
}

int main() {
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63, 1.0, 200), c3_hot = build(3, 0, 1, 2.0, 27, 1.0, 200);
  const twr::Structure every = build(3, 2, 0, 2.4, 255, 1.1, 200);
  plan_case("C3x16", {&c3_hot}, std::vector<int32_t>(16, 0));
  plan_case("every", {&every, &c3}, {0, 1, 0});
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 6; ++i) ss.push_back(build(i % 2 ? 2 : 1, 4, i % 3, 1.2 + 0.3 * i, i % 2 ? 27 : 63, 0.9, 200));
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 3, 1, 1, 0});
  plan_case("one", sp, {3});
  const twr::Structure wide = build(3, 0, 1, 2.0, 27, 1.0, 200, nullptr, 0.003);
  CHECK(wide.n_vars > twr::kJacLdsX, "the wide structure has %d variables", wide.n_vars);
  plan_case("wide", {&wide, &c3_hot}, {0, 1, 0});
  // an odd number of variables in all: the segments still start on 16-byte boundaries
  bool odd = false;
  for (size_t i = 0; i < ss.size() && !odd; ++i)
    if (ss[i].n_vars % 2) {
      plan_case("odd", {&ss[i]}, {0});
      plan_case("odd x3", {&ss[i]}, {0, 0, 0});
      odd = true;
    }
  if (!odd) std::printf("scaled plan: no structure with an odd variable count among the ragged ones\n");
  std::printf("jac_scaled_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
