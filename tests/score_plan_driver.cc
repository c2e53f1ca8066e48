// Checks of the scoring plan (twr_batch_eval_scores) on the host: the lists twr::PlanBatch builds for the fold
// (score_blob / score_first / score_slot, score_slab) and the steps twr::PlanEval plans for a scoring request (kEvalScores).
// Built and run by tests/test_score_plan.py (g++ against the host planner, no HIP).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../towr_amd/csrc/batch_plan.h"
#include "plan_driver_common.h"

static twr::EvalShape shape_of(const twr::BatchPlan& B, int n_cu, int flags, bool events = false) {
  const auto& L = B.lists;
  twr::EvalShape s;
  s.n_cu = n_cu;
  s.dyn = (int)L.dyn.size(), s.rom = (int)L.rom.size(), s.node = (int)L.node.size() - 1, s.flat = (int)L.flat.size();
  for (int f = 0; f < 4; ++f) s.fam[f] = (int)L.fam[f].size();
  s.pdyn = (int)L.pdyn.size(), s.ploc = (int)L.ploc.size(), s.prom = (int)L.prom.size();
  s.rom_max_vals = B.rom_max_vals, s.flat_max_x = B.flat_max_x, s.dyn_map_chunks = B.dyn_map_chunks, s.node_families = B.node_families;
  s.pdyn_img_cap = B.pdyn_img_cap, s.prom_img_cap = B.prom_img_cap, s.stream_nt = B.stream_nt;
  s.flags = flags;
  s.events = events;
  s.score_fused = B.score_fused;
  return s;
}

static bool same_step(const twr::LaunchStep& a, const twr::LaunchStep& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// every row of every problem is covered exactly once by the problem's partial records; slots are in the slab and belong to
// one problem each
static void check_coverage(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop,
                           const twr::BatchPlan& B) {
  const auto& L = B.lists;
  const int n = (int)sop.size(), n_groups = (int)L.flat.size() / twr::kFlatGroup;
  CHECK((int)L.score_first.size() == n + 1 && L.score_first[0] == 0 && L.score_first[n] == (int)L.score_slot.size(),
        "%s: score_first", name);
  CHECK((int)L.score_blob.size() == n_groups, "%s: score_blob has %zu entries for %d groups", name, L.score_blob.size(), n_groups);
  CHECK(B.score_slab == (int64_t)twr::kFlatGroup * (n_groups + n), "%s: slab %lld", name, (long long)B.score_slab);
  std::vector<int> owner(B.score_slab, -1);
  for (int p = 0; p < n; ++p) {
    const twr::Structure& S = *sp[sop[p]];
    const auto* H = reinterpret_cast<const twr::DevStruct*>(S.blob.data());
    const int m = (int)(B.g_off[p + 1] - B.g_off[p]);
    std::vector<int> hits(m, 0);
    auto cover = [&](int r0, int count) {
      for (int r = r0; r < r0 + count; ++r) {
        if (r < 0 || r >= m) {
          CHECK(false, "%s: problem %d row %d outside [0, %d)", name, p, r, m);
          return;
        }
        ++hits[r];
      }
    };
    for (int k = L.score_first[p]; k < L.score_first[p + 1]; ++k) {
      const int s = L.score_slot[k];
      if (s < 0 || s >= B.score_slab) {
        CHECK(false, "%s: slot %d outside the slab", name, s);
        continue;
      }
      CHECK(owner[s] < 0, "%s: slot %d of problem %d already belongs to problem %d", name, s, p, owner[s]);
      owner[s] = p;
      const int b = s / twr::kFlatGroup, w = s % twr::kFlatGroup;
      if (b < n_groups) {
        const twr::FlatWork& it = L.flat[s];
        CHECK(it.cnt > 0 && it.g_off == B.g_off[p] && L.score_blob[b] == B.blob_of_problem[p], "%s: flat slot %d of problem %d", name, s, p);
        if (it.dynamic) cover(it.row_dyn + 6 * it.k0, 6 * it.cnt);
        if (!it.dynamic || it.with_rom)
          for (int e = 0; e < it.n_ee; ++e) cover(it.row_rom[e] + 3 * it.k0, 3 * it.cnt);
      } else {
        CHECK(b - n_groups == p && w < B.node_families, "%s: node slot %d of problem %d", name, s, p);
        if (w == 0) cover(H->row_terrain, H->n_terrain_rows);
        if (w == 1) cover(H->row_force, 5 * H->n_force_nodes);
        if (w == 2) {
          cover(H->row_acc, 6 * H->n_junctions);
          cover(H->row_bm, 6 * H->n_bm_nodes);
        }
        if (w == 3) cover(H->row_swing, 4 * H->n_swing_nodes);
      }
    }
    int bad = 0;
    for (int r = 0; r < m; ++r) bad += hits[r] != 1;
    CHECK(bad == 0, "%s: problem %d: %d of %d rows not covered exactly once", name, p, bad, m);
  }
  // every flat item with work is some problem's slot
  for (size_t i = 0; i < L.flat.size(); ++i)
    if (L.flat[i].cnt > 0) CHECK(owner[i] >= 0, "%s: flat item %zu is in no problem's fold", name, i);
}

static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, bool fused) {
  const int n_cu = 256;
  const std::vector<uint64_t> at = blob_at(sp.size());
  const twr::BatchPlan B = twr::PlanBatch(sp, sop, at, n_cu, (int64_t)256 << 20, twr::kForceChunk);
  const twr::BatchPlan C = twr::PlanBatch(sp, sop, at, n_cu, (int64_t)256 << 20, twr::kForceChunk);
  CHECK(B.score_fused == fused, "%s: score_fused %d, want %d", name, (int)B.score_fused, (int)fused);
  CHECK(same_bytes(B.lists.score_blob, C.lists.score_blob) && same_bytes(B.lists.score_first, C.lists.score_first) &&
            same_bytes(B.lists.score_slot, C.lists.score_slot) && B.score_slab == C.score_slab,
        "%s: planning twice differs", name);
  const int n = (int)sop.size();
  if (fused) check_coverage(name, sp, sop, B);
  else CHECK(B.lists.score_slot.empty() && B.lists.score_first.empty() && B.score_slab == 0, "%s: scoring lists without the fused path", name);
  // the scoring plans
  for (int best = 0; best < 2; ++best) {
    const int flags = twr::kEvalScores | (best ? twr::kEvalBest : 0);
    const twr::EvalPlan P = twr::PlanEval(shape_of(B, n_cu, flags, true));   // (events requested: a scoring plan records none)
    int k = 0;
    if (fused) {
      const int n_groups = (int)B.lists.flat.size() / twr::kFlatGroup;
      CHECK(P.n == 2 + best, "%s: %d steps", name, P.n);
      const twr::LaunchStep& s = P.step[0];
      CHECK(s.kernel == twr::Launch::kScores && s.grid == n_groups + n && s.block == 64 * twr::kFlatGroup &&
                s.lds == twr::flat_lds_bytes(B.flat_max_x) && s.arg[0] == n_groups && s.arg[1] == B.node_families &&
                s.arg[2] == twr::flat_x_bytes(B.flat_max_x),
            "%s: scoring launch", name);
      const int nx = (B.flat_max_x + 255) / 256;
      CHECK(s.xc == (nx <= 3 ? 3 : nx <= 5 ? 5 : 8), "%s: NX %d", name, s.xc);
      CHECK(P.step[1].kernel == twr::Launch::kFold && P.step[1].grid == (16 * n + 255) / 256 && P.step[1].block == 256 &&
                P.step[1].arg[0] == n,
            "%s: fold", name);
      k = 2;
    } else {   // exactly the values-only evaluation, then score_kernel
      const twr::EvalPlan V = twr::PlanEval(shape_of(B, n_cu, 1));
      CHECK(P.n == V.n + 1 + best, "%s: fallback %d steps, values %d", name, P.n, V.n);
      for (int i = 0; i < V.n && i < P.n; ++i) CHECK(same_step(P.step[i], V.step[i]), "%s: fallback step %d", name, i);
      k = V.n;
      CHECK(k < P.n && P.step[k].kernel == twr::Launch::kScoreG && P.step[k].grid == n && P.step[k].arg[0] == n, "%s: score_kernel", name);
      ++k;
    }
    for (int i = 0; i < P.n; ++i) CHECK(P.step[i].kernel != twr::Launch::kEvent, "%s: an event in a scoring plan", name);
    if (best) {
      const int blocks = std::max(1, std::min((n + 1023) / 1024, 256));
      CHECK(k < P.n && P.step[k].kernel == twr::Launch::kBest && P.step[k].grid == blocks && P.step[k].arg[0] == n, "%s: best", name);
    }
  }
  // the plans of the existing flags do not see the scoring fields
  for (int flags = 1; flags <= 3; ++flags)
    for (int ev = 0; ev < 2; ++ev) {
      twr::EvalShape a = shape_of(B, n_cu, flags, ev), b = a;
      b.score_fused = !a.score_fused;
      const twr::EvalPlan pa = twr::PlanEval(a), pb = twr::PlanEval(b);
      bool same = pa.n == pb.n;
      for (int i = 0; same && i < pa.n; ++i) same = same_step(pa.step[i], pb.step[i]);
      CHECK(same, "%s: flags %d events %d: the plan depends on score_fused", name, flags, ev);
      for (int i = 0; i < pa.n; ++i)
        CHECK(pa.step[i].kernel != twr::Launch::kScores && pa.step[i].kernel != twr::Launch::kFold && pa.step[i].kernel != twr::Launch::kScoreG &&
                  pa.step[i].kernel != twr::Launch::kBest,
              "%s: flags %d: a scoring launch in an evaluation", name, flags);
    }
  std::printf("score plan %-10s %5d problems: fused %d, %zu groups, %zu slots, slab %lld\n", name, n, (int)B.score_fused,
              B.lists.score_blob.size(), B.lists.score_slot.size(), (long long)B.score_slab);
}

int main() {
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63, 1.0, 200), c3_timings = build(3, 0, 1, 2.0, 127, 1.0, 200), c3_hot = build(3, 0, 1, 2.0, 27, 1.0, 200);
  plan_case("C3x2048", {&c3}, std::vector<int32_t>(2048, 0), true);   // the values path would chunk the node sets here
  plan_case("C3x200", {&c3}, std::vector<int32_t>(200, 0), true);
  plan_case("single", {&c3_hot}, {0}, true);
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 11; ++i)
    ss.push_back(build(2, 4, i == 10 ? 3 : 1, i < 8 ? 1.2 + 0.2 * i : 2.0, 27, i < 8 ? 0.80 : 0.80 + 0.016 * (i - 7), 200));
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 3, 5, 5, 0}, true);
  auto grid = std::make_shared<twr::TerrainGrid>();
  grid->rows = 40;
  grid->cols = 60;
  for (int i = 0; i < grid->rows * grid->cols; ++i) grid->heights.push_back(0.05 * ((i * 7919) % 13) / 13.0);
  const twr::Structure g1 = build(3, 7, 1, 2.0, 63, 1.0, 200, grid), g2 = build(3, 7, 0, 2.4, 27, 1.0, 120, grid);
  plan_case("grid", {&g1, &g2}, {0, 1, 1, 0, 0, 1, 0}, true);
  const twr::Structure all = build(3, 2, 0, 2.4, 191, 1.1, 200);   // every family but totalduration, baseMotion included
  plan_case("all-sets", {&all, &c3}, {0, 1, 0}, true);
  // the fallbacks: optimised timings, fixed and optimised timings mixed, more than 2046 variables
  plan_case("timings", {&c3_timings}, {0, 0}, false);
  plan_case("mixed", {&c3, &c3_timings}, {0, 1, 0}, false);
  const twr::Structure wide = build(3, 0, 1, 2.0, 63, 1.0, 200, nullptr, 0.01);
  CHECK(wide.n_vars > 2046, "the wide structure has %d variables", wide.n_vars);
  plan_case("wide", {&wide, &c3}, {0, 1}, false);
  std::printf("score_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
