// The start table of a structure (towr_amd/csrc/start_table.h, Structure::BuildStartTable), its host executor
// (Structure::StartHost, what twr_structure_start_host calls) and the work list of twr_batch_start (twr::PlanStart), checked on the
// host.  A stand-alone program built by tests/host_build.py with g++ under AddressSanitizer + UndefinedBehaviorSanitizer against
// the host sources; no HIP, nothing loaded into Python.
//   tables:  one record per variable, each naming a node value that IS that variable and the LATEST node that is; bound targets
//            are exactly the optimised ones of the reference's AddStartBound / AddFinalBound lists; durations and their box
//   host:    StartHost == InitialGuess + VariableBounds bit for bit (robots x gait combos x fixed / optimised timings x
//            terrains x yaws x goals on terrain breakpoints), each output alone as well
//   planner: six batch shapes covered exactly once inside every problem, identical tables stored once, the list a function of
//            structures and offsets alone
#include <cmath>
#include <map>

#include "../towr_amd/csrc/batch_plan.h"
#include "plan_driver_common.h"

using twr::kMaxEE;
using twr::StartHeader;
using twr::StartRec;
using twr::Structure;

static const twr::SplineLayout& spline_of(const Structure& S, int spline, int& delta) {
  delta = 0;
  if (spline == 0) return delta = S.off_base_lin, S.base;
  if (spline == 1) return delta = S.off_base_ang, S.base;
  if (spline < 2 + kMaxEE) return S.motion[spline - 2];
  return S.force[spline - 2 - kMaxEE];
}

static void table_case(const Structure& S, const char* name) {
  CHECK(S.start_table != nullptr, "%s: no start table", name);
  if (!S.start_table) return;
  const std::vector<char>& t = *S.start_table;
  const StartHeader* h = table<StartHeader>(name, t, 0, 1);
  if (!h) return;
  CHECK(h->n_vars == S.n_vars && h->n_ee == S.n_ee && h->T == S.T, "%s: header sizes", name);
  const double* dur = table<double>(name, t, h->o_dur, h->n_dur);
  const StartRec* rec = table<StartRec>(name, t, h->o_rec, h->n_vars);
  if (!rec || (h->n_dur && !dur)) return;
  CHECK(t.size() == h->o_rec + (size_t)h->n_vars * sizeof(StartRec), "%s: exactly one record per variable", name);
  CHECK(h->nm1[0] == S.base.n_nodes - 1 && h->nm1[1] == S.base.n_nodes - 1, "%s: base nodes", name);
  for (int e = 0; e < kMaxEE; ++e) {
    CHECK(h->nm1[2 + e] == (e < S.n_ee ? S.motion[e].n_nodes - 1 : 0), "%s: ee-motion %d nodes", name, e);
    CHECK(h->nm1[2 + kMaxEE + e] == (e < S.n_ee ? S.force[e].n_nodes - 1 : 0), "%s: ee-force %d nodes", name, e);
    for (int d = 0; d < 3; ++d) CHECK(h->stance[e][d] == (e < S.n_ee ? S.model.nominal_stance[e][d] : 0.0), "%s: stance", name);
  }
  // the variables a spline node owns, and the last node that owns each
  std::map<int, int> last_node[twr::kStartSplines];
  int n_node_vars = 0;
  for (int sp = 0; sp < twr::kStartSplines; ++sp) {
    if ((sp >= 2 + S.n_ee && sp < 2 + kMaxEE) || sp >= 2 + kMaxEE + S.n_ee) continue;
    int delta;
    const twr::SplineLayout& L = spline_of(S, sp, delta);
    for (int n = 0; n < L.n_nodes; ++n)
      for (int c = 0; c < 6; ++c)
        if (L.at(n, c / 3, c % 3) >= 0) last_node[sp][L.at(n, c / 3, c % 3) + delta] = n;
    n_node_vars += (int)last_node[sp].size();
  }
  int n_dur_vars = 0, n_fixed = 0;
  for (int i = 0; i < h->n_vars; ++i) {
    const StartRec r = rec[i];
    if (r.value == twr::kStartNode) {
      const bool ok = r.spline < twr::kStartSplines && r.comp < 6 && last_node[r.spline].count(i);
      CHECK(ok, "%s: variable %d names spline %d, which has no node value there", name, i, r.spline);
      if (!ok) continue;
      int delta;
      const twr::SplineLayout& L = spline_of(S, r.spline, delta);
      CHECK((int)r.node < L.n_nodes && L.at(r.node, r.comp / 3, r.comp % 3) + delta == i, "%s: variable %d is not node %d comp %d of spline %d",
            name, i, r.node, r.comp, r.spline);
      CHECK(last_node[r.spline][i] == (int)r.node, "%s: variable %d names node %d, the later node is %d", name, i, r.node, last_node[r.spline][i]);
      CHECK(r.bound == twr::kStartNoBound || r.bound == twr::kStartFixed, "%s: variable %d: a node with a duration box", name, i);
    } else if (r.value == twr::kStartDuration) {
      ++n_dur_vars;
      CHECK(S.timings && (int)r.node < h->n_dur && r.bound == twr::kStartDurationBox, "%s: variable %d: duration record", name, i);
    } else {
      CHECK(false, "%s: variable %d has no source (every variable of the reference's sets is a node value or a duration)", name, i);
    }
    if (r.bound == twr::kStartFixed) {
      ++n_fixed;
      CHECK(r.slot < twr::kStartRequest, "%s: slot", name);
    }
  }
  CHECK(n_node_vars + n_dur_vars == h->n_vars, "%s: node variables %d + durations %d != %d", name, n_node_vars, n_dur_vars, h->n_vars);
  // the durations in the order of PhaseDurations::GetValues
  if (S.timings) {
    int k = 0;
    for (int e = 0; e < S.n_ee; ++e)
      for (int i = 0; i < S.schedule.n_phases[e] - 1; ++i, ++k) {
        const StartRec r = rec[S.off_schedule[e] + i];
        CHECK(r.value == twr::kStartDuration && dur[r.node] == S.schedule.phase_durations[e][i], "%s: duration %d of foot %d", name, i, e);
      }
    CHECK(k == h->n_dur && k == n_dur_vars, "%s: duration count", name);
  } else {
    CHECK(h->n_dur == 0, "%s: durations without optimised timings", name);
  }
  // bound targets (nlp_formulation.cc:109-122,151 with parameters.cc:65-69): the optimised ones, each with its slot; a target that is
  // no variable (a stance foot's velocity, ...) leaves nothing
  std::map<int, int> want;   // variable -> slot
  auto target = [&](const twr::SplineLayout& L, int delta, int node, int deriv, int dim, int slot) {
    const int i = L.at(node, deriv, dim);
    if (i >= 0) want[i + delta] = slot;
  };
  const int last = S.base.n_nodes - 1;
  for (int d = 0; d < 3; ++d) {
    target(S.base, S.off_base_lin, 0, 0, d, d);
    target(S.base, S.off_base_lin, 0, 1, d, 3 + d);
    if (d != 2) target(S.base, S.off_base_lin, last, 0, d, 12 + d);
    target(S.base, S.off_base_lin, last, 1, d, 15 + d);
    target(S.base, S.off_base_ang, 0, 0, d, 6 + d);
    target(S.base, S.off_base_ang, 0, 1, d, 9 + d);
    target(S.base, S.off_base_ang, last, 0, d, 18 + d);
    target(S.base, S.off_base_ang, last, 1, d, 21 + d);
    for (int e = 0; e < S.n_ee; ++e) target(S.motion[e], 0, 0, 0, d, 24 + 3 * e + d);
  }
  CHECK((int)want.size() == n_fixed, "%s: %d fixed records, %zu optimised bound targets", name, n_fixed, want.size());
  for (const auto& w : want)
    CHECK(rec[w.first].bound == twr::kStartFixed && rec[w.first].slot == w.second, "%s: variable %d should be fixed to slot %d", name, w.first, w.second);
  // no ee-force variable and no ee-motion variable past node 0's position is ever a bound target
  for (int i = 0; i < h->n_vars; ++i)
    if (rec[i].bound == twr::kStartFixed && rec[i].value == twr::kStartNode && rec[i].spline >= 2)
      CHECK(rec[i].spline < 2 + kMaxEE && rec[i].comp < 3 && S.motion[rec[i].spline - 2].at(0, 0, rec[i].comp) == i, "%s: variable %d bound", name, i);
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) { return same_bytes(a, b); }

static int host_case(const Structure& S, const char* name) {
  const double yaws[] = {0.0, 0.3, -2.0, 1.5707963267948966, -0.0};
  const double goals[][2] = {{1.0, 0.0},  {std::nextafter(1.0, 0.0), 0.1}, {1.4, -0.2}, {std::nextafter(1.4, 2.0), 0.05}, {0.77, 0.13},
                             {2.0, 0.3},  {3.0, -0.4},                     {1.5, 0.5},  {0.17 * 3, 0.17 * 2},            {-0.3, -0.2}};
  int n = 0;
  std::vector<double> x(S.n_vars), lo(S.n_vars), up(S.n_vars), x2(S.n_vars), lo2(S.n_vars), up2(S.n_vars);
  for (double yaw : yaws)
    for (const auto& g : goals) {
      double rq[twr::kStartRequest];
      for (int i = 0; i < twr::kStartRequest; ++i) rq[i] = 0.01 * ((i * 37 + n * 11) % 23) - 0.1;   // non-zero velocities included
      rq[2] = 0.5;
      rq[12] = g[0], rq[13] = g[1], rq[14] = 0.5;
      rq[20] = yaw;
      S.InitialGuess(rq, rq + 6, rq + 12, rq + 18, rq + 24, x.data());
      S.VariableBounds(rq, rq + 12, rq + 24, lo.data(), up.data());
      S.StartHost(rq, x2.data(), lo2.data(), up2.data());
      CHECK(same_bits(x, x2) && same_bits(lo, lo2) && same_bits(up, up2), "%s: StartHost differs from InitialGuess / VariableBounds (yaw %g goal %g %g)",
            name, yaw, g[0], g[1]);
      if (n % 7 == 0) {   // each output alone
        std::vector<double> a(S.n_vars, -7.0), b(S.n_vars, -7.0), c(S.n_vars, -7.0);
        S.StartHost(rq, a.data(), nullptr, nullptr);
        S.StartHost(rq, nullptr, b.data(), nullptr);
        S.StartHost(rq, nullptr, nullptr, c.data());
        CHECK(same_bits(x, a) && same_bits(lo, b) && same_bits(up, c), "%s: single outputs", name);
      }
      ++n;
    }
  return n;
}

static void plan_case(const char* name, const std::vector<const Structure*>& structs, const std::vector<int32_t>& sop) {
  std::vector<int64_t> x_off(1, 0);
  for (int32_t s : sop) x_off.push_back(x_off.back() + structs[s]->n_vars);
  const std::vector<uint64_t> at = blob_at(structs.size());
  std::vector<uint64_t> blob;
  for (int32_t s : sop) blob.push_back(at[s]);
  std::vector<const std::vector<char>*> tables;
  for (const Structure* s : structs) tables.push_back(s->start_table.get());
  const twr::StartPlan plan = twr::PlanStart(tables, sop, x_off, blob);
  CHECK(plan.tables.size() % 256 == 0 && !plan.work.empty(), "%s: tables on 256-byte lines", name);
  std::vector<int> seen(x_off.back(), 0);
  int32_t prev_problem = 0;
  for (const twr::StartWork& w : plan.work) {
    const bool in = w.problem >= 0 && w.problem < (int)sop.size() && w.problem >= prev_problem;
    CHECK(in, "%s: item of problem %d", name, w.problem);
    if (!in) continue;
    prev_problem = w.problem;
    const Structure& S = *structs[sop[w.problem]];
    CHECK(w.cnt >= 1 && w.cnt <= twr::kStartItem && w.v0 >= 0 && w.v0 + w.cnt <= S.n_vars, "%s: item [%d, +%d) leaves problem %d (%d variables)", name,
          w.v0, w.cnt, w.problem, S.n_vars);
    CHECK(w.x_off == x_off[w.problem] && w.blob == blob[w.problem] && w.pad == 0, "%s: item addresses", name);
    const bool placed = w.table % 256 == 0 && w.table + S.start_table->size() <= plan.tables.size();
    CHECK(placed, "%s: table outside", name);
    if (placed) CHECK(std::memcmp(plan.tables.data() + w.table, S.start_table->data(), S.start_table->size()) == 0, "%s: table bytes", name);
    for (int v = std::max(w.v0, 0); v < std::min(w.v0 + w.cnt, S.n_vars); ++v) ++seen[x_off[w.problem] + v];
  }
  int bad = 0;
  for (int c : seen) bad += c != 1;
  CHECK(bad == 0, "%s: %d variables not covered exactly once", name, bad);
  // byte-identical tables once
  std::map<std::string, int> distinct;
  int64_t built = 0, stored = 0;
  for (const Structure* s : structs) {
    built += (int64_t)s->start_table->size();
    if (distinct.emplace(std::string(s->start_table->begin(), s->start_table->end()), 0).second) stored += (int64_t)s->start_table->size();
  }
  CHECK(plan.bytes_built == built && plan.bytes_distinct == stored, "%s: bytes built %lld distinct %lld", name, (long long)plan.bytes_built,
        (long long)plan.bytes_distinct);
  CHECK(plan.tables.size() <= (size_t)stored + 256 * distinct.size(), "%s: %zu table bytes for %lld distinct", name, plan.tables.size(), (long long)stored);
  // a function of structures and offsets alone: the same again; other blob addresses move the blob fields only; Place adds the base
  const twr::StartPlan again = twr::PlanStart(tables, sop, x_off, blob);
  CHECK(same_bytes(plan.tables, again.tables) && same_bytes(plan.work, again.work), "%s: planning twice differs", name);
  std::vector<uint64_t> blob2 = blob;
  for (uint64_t& a : blob2) a += 0x4000;
  twr::StartPlan moved = twr::PlanStart(tables, sop, x_off, blob2);
  CHECK(same_bytes(plan.tables, moved.tables) && moved.work.size() == plan.work.size(), "%s: tables depend on blob addresses", name);
  for (size_t i = 0; i < moved.work.size() && i < plan.work.size(); ++i) {
    twr::StartWork w = moved.work[i];
    CHECK(w.blob == plan.work[i].blob + 0x4000, "%s: moved blob", name);
    w.blob = plan.work[i].blob;
    CHECK(std::memcmp(&w, &plan.work[i], sizeof(w)) == 0, "%s: item %zu depends on more than the blob address", name, i);
  }
  moved.Place(0x7e0000000000ull);
  for (size_t i = 0; i < moved.work.size() && i < plan.work.size(); ++i)
    CHECK(moved.work[i].table == plan.work[i].table + 0x7e0000000000ull, "%s: Place", name);
}

int main() {
  int structures = 0, requests = 0;
  auto csv = std::make_shared<twr::TerrainGrid>();
  csv->rows = 12;
  csv->cols = 20;
  for (int i = 0; i < csv->rows * csv->cols; ++i) csv->heights.push_back(0.05 * ((i * 7919) % 13) / 13.0);
  auto gm = std::make_shared<twr::TerrainGrid>();
  gm->grid_map = true;
  gm->rows = 47;
  gm->cols = 37;
  gm->res = 0.1;
  gm->eps = 0.1 / 6;
  gm->pos_x = 1.0;
  gm->pos_y = 0.05;
  for (int i = 0; i < gm->rows * gm->cols; ++i) gm->elevation.push_back(0.3f * (float)((i * 7919) % 31) / 31.0f);
  const int terrains[] = {TWR_TERRAIN_FLAT, TWR_TERRAIN_STAIRS, TWR_TERRAIN_GAP, TWR_TERRAIN_SLOPE, TWR_TERRAIN_CSV_GRID, TWR_TERRAIN_GRID_MAP};
  const int robots[] = {0, 1, 3, 4};   // monoped, biped, ANYmal, Go1
  for (int robot : robots)
    for (int combo = 0; combo < 5; ++combo)     // every gait combo of the sanitizer tier (oracle/asan_driver.cc)
      for (int timings = 0; timings < 2; ++timings)
        for (int ti = 0; ti < 6; ++ti) {
          if ((robot + combo + timings + ti) % 2 != 0 && !(combo == 1 && timings == 0)) continue;   // half the product, every factor with every other
          const int terrain = terrains[ti];
          std::shared_ptr<const twr::TerrainGrid> grid = terrain == TWR_TERRAIN_CSV_GRID ? csv : terrain == TWR_TERRAIN_GRID_MAP ? gm : nullptr;
          const Structure S = build(robot, terrain, combo, 1.4 + 0.2 * combo, timings ? 27 | 64 : 63, 1.0, 40, grid);
          char name[96];
          std::snprintf(name, sizeof(name), "robot %d combo %d timings %d terrain %d", robot, combo, timings, terrain);
          table_case(S, name);
          requests += host_case(S, name);
          ++structures;
        }
  // the planner: six batch shapes
  const Structure a = build(4, TWR_TERRAIN_STAIRS, 1, 2.0, 63, 1.0, 40), b = build(4, TWR_TERRAIN_STAIRS, 2, 1.8, 27 | 64, 1.0, 40),
                  c = build(4, TWR_TERRAIN_STAIRS, 0, 2.4, 27, 0.9, 40), a2 = build(4, TWR_TERRAIN_STAIRS, 1, 2.0, 63, 1.0, 40);
  const Structure tiny = build(0, TWR_TERRAIN_FLAT, 0, 0.8, 27, 1.0, 20, nullptr, 0.5);
  CHECK(tiny.n_vars < twr::kStartItem, "the small structure has %d variables (wanted fewer than one item)", tiny.n_vars);
  CHECK(a.n_vars % twr::kStartItem != 0 && a.n_vars > twr::kStartItem, "a: %d variables (wanted several items and a tail)", a.n_vars);
  CHECK(a.n_vars != b.n_vars && b.n_vars != c.n_vars && a.n_vars != c.n_vars, "the ragged mix needs three sizes: %d %d %d", a.n_vars, b.n_vars, c.n_vars);
  plan_case("one", {&a}, {0});
  plan_case("three", {&a}, std::vector<int32_t>(3, 0));
  plan_case("sixty-seven", {&a}, std::vector<int32_t>(67, 0));
  plan_case("ragged", {&a, &b, &c}, {0, 1, 2, 2, 1, 0, 1, 1, 2, 0, 0});
  plan_case("tail", {&b, &a2, &a}, {0, 1, 2, 1});   // (a and a2: byte-identical tables, stored once)
  plan_case("small", {&tiny, &a}, {0, 0, 1, 0});
  std::printf("start_plan_driver: %d structures, %d requests, %d failures\n", structures, requests, fails);
  return fails ? 1 : 0;
}
