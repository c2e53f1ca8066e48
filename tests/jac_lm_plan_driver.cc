// Checks of the bounded LM driver's plan (twr_jac_lm_*) on the host: the workspace segments twr::PlanJacLm lays out.  Built and run
// by tests/test_jac_lm_plan.py (tests/host_build.py: g++ against the host planner under ASan + UBSan, no HIP).
#include <algorithm>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../towr_amd/csrc/jac_plan.h"
#include "plan_driver_common.h"

static twr::Structure sizes_only(int n, int m) {   // the plan reads n_vars and n_rows alone
  twr::Structure S;
  S.n_vars = n, S.n_rows = m;
  return S;
}

// Everything PlanJacLm returns, as one number (the plan has nothing to Place)
static uint64_t lm_fingerprint(const twr::JacLmPlan& L) {
  Fnv f;
  f.vec64(L.x_off), f.vec64(L.g_off);
  for (int64_t v : {L.ws_xt, L.ws_d, L.ws_z, L.ws_colsq, L.ws_colmax, L.ws_c, L.ws_cf, L.ws_r, L.ws_b, L.ws_wa, L.ws_gt, L.ws_rt, L.ws_rec, L.ws_mu,
                    L.ws_merit_t, L.ws_merit_lin, L.ws_nfree, L.ws_info, L.ws_doubles})
    f.i64(v);
  return f.h;
}

// Recorded from the commit before the planner was cut into units (this driver with -DTWR_RECORD_PARENT).
static const ParentRecord<1> kParent[] = {
    {"hopper x3", {0xb14ce8bbecf3c627ull}},
    {"ragged", {0x3bf30e0547ad490full}},
    {"odd", {0xa57699bdf4af0eddull}},
};

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, bool recorded = false) {
  const twr::JacLmPlan L = twr::PlanJacLm(sp, sop), K = twr::PlanJacLm(sp, sop);
  if (recorded) {
    const uint64_t hash[1] = {lm_fingerprint(L)};
    parent_record(kParent, name, hash);
  }
  const int n = (int)sop.size();
  CHECK(L.x_off == K.x_off && L.g_off == K.g_off && L.ws_doubles == K.ws_doubles && L.ws_info == K.ws_info && L.ws_rec == K.ws_rec,
        "%s: planning twice differs", name);
  bool built = true;   // (hand-made structures have no bound tables for PlanJacLsq to read)
  for (const twr::Structure* s : sp) built = built && (int)s->lower.size() == s->n_rows;
  if (built) {
    const twr::JacLsqPlan Q = twr::PlanJacLsq(sp, sop);
    CHECK(L.x_off == Q.x_off && L.g_off == Q.g_off, "%s: layout differs from PlanJacLsq", name);
  }
  CHECK((int)L.x_off.size() == n + 1 && (int)L.g_off.size() == n + 1, "%s: offsets", name);
  for (int p = 0; p < n; ++p)
    CHECK(L.x_off[p + 1] - L.x_off[p] == sp[sop[p]]->n_vars && L.g_off[p + 1] - L.g_off[p] == sp[sop[p]]->n_rows, "%s: problem %d", name, p);
  const int64_t X = L.x_off[n], G = L.g_off[n];
  std::vector<std::pair<int64_t, int64_t>> seg = {
      {L.ws_xt, X}, {L.ws_d, X}, {L.ws_z, X}, {L.ws_colsq, X}, {L.ws_colmax, X}, {L.ws_c, X}, {L.ws_cf, X},
      {L.ws_r, G},  {L.ws_b, G}, {L.ws_wa, G}, {L.ws_gt, G},   {L.ws_rt, G},
      {L.ws_rec, (int64_t)twr::kLmRec * n}, {L.ws_mu, n}, {L.ws_merit_t, n}, {L.ws_merit_lin, n}, {L.ws_nfree, n}, {L.ws_info, 4 * (int64_t)n}};
  for (const auto& s : seg)
    CHECK(s.first >= 0 && s.first % 2 == 0 && s.first + s.second <= L.ws_doubles, "%s: segment [%lld, +%lld) outside %lld or odd", name,
          (long long)s.first, (long long)s.second, (long long)L.ws_doubles);
  std::sort(seg.begin(), seg.end());
  for (size_t i = 0; i + 1 < seg.size(); ++i)
    CHECK(seg[i].first + seg[i].second <= seg[i + 1].first, "%s: workspace segments %zu and %zu overlap", name, i, i + 1);
  int64_t need = 0;
  for (const auto& s : seg) need += (s.second + 1) / 2 * 2;
  CHECK(L.ws_doubles == need, "%s: workspace of %lld doubles, %lld would do", name, (long long)L.ws_doubles, (long long)need);
  CHECK(twr::kLmRec > std::max({(int)twr::kLmMerit0, (int)twr::kLmMerit, (int)twr::kLmMu, (int)twr::kLmSteps, (int)twr::kLmAccepted,
                                (int)twr::kLmFree, (int)twr::kLmCgIters, (int)twr::kLmState}),
        "%s: a slot outside the record", name);
  std::printf("lm plan %-10s %4d problems: X %lld, G %lld, workspace %lld doubles\n", name, n, (long long)X, (long long)G,
              (long long)L.ws_doubles);
}

int main() {
  const twr::Structure hopper = build(0, 0, 0, 2.0, 27, 1.0, 40), hopper_all = build(0, 0, 0, 2.0, 127, 1.0, 40), biped_all = build(1, 0, 0, 2.0, 127, 1.0, 40);
  const twr::Structure anymal = build(3, 0, 1, 2.0, 27, 1.0, 40);
  const twr::Structure odd = sizes_only(339, 273), empty = sizes_only(7, 0), one = sizes_only(1, 1);
  plan_case("hopper", {&hopper}, {0});
  plan_case("hopper x3", {&hopper}, {0, 0, 0}, true);
  plan_case("ragged", {&hopper, &hopper_all, &biped_all, &anymal}, {0, 1, 2, 3, 2, 1, 0, 0, 3}, true);
  plan_case("odd", {&odd, &one}, {0, 1, 0, 0, 1}, true);            // odd n and m: odd totals, odd problem counts
  plan_case("no rows", {&empty}, {0, 0, 0});                   // G = 0: empty g segments
  plan_case("mixed", {&empty, &odd, &anymal}, {1, 0, 2, 0, 1});
  CHECK(hopper.n_vars % 2 == 1 || hopper_all.n_vars % 2 == 1 || odd.n_vars % 2 == 1, "no odd n among the cases");
  bool threw = false;
  try {
    twr::PlanJacLm({&hopper}, {0, 1});
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw, "a struct_of_problem entry out of range was accepted");
  std::printf("jac_lm_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
