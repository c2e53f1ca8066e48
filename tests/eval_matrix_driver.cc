// The evaluation-kernel instantiation matrix (tests/eval_matrix.py), checked on the host: every row's batch is built and
// planned by the product's own planner (twr::PlanBatch, twr::MakeEvalShape, twr::PlanEval) for every flag set, with and
// without per-kernel events, and for the two scoring requests; each row must reach the instantiations it claims, and the
// claims of all rows plus the exclusion list must be exactly the set of instantiations that exist -- enumerated here from the
// key lists of structure.h, so a new instantiation without a row fails.
// Built and run by tests/test_eval_matrix_plan.py (g++ against the host planner, no HIP); the matrix text comes in
// as a file (argv[1]), the same text tests/test_eval_matrix.py builds its device batches from.  The device enters as 256 CUs
// and a 256 MB memory-side cache (an MI355X); the GPU test holds the rows to the plan of the device it runs on.
// With --print the plan of every call is listed (how the rows were found).  With --partial the text is a set of rows of its own
// (tests/test_eval_edges.py): every row must reach what it claims, and the rows need not cover every instantiation.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include "../towr_amd/csrc/batch_plan.h"
#include "plan_driver_common.h"

static const int kCu = 256;
static const int64_t kCache = (int64_t)256 << 20;
static const int kMaxExclusions = 8;

using Fields = std::map<std::string, std::string>;

static std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  std::string cur;
  for (char c : s) {
    if (c == sep) {
      if (!cur.empty()) out.push_back(cur);
      cur.clear();
    } else {
      cur += c;
    }
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

static std::string get(const Fields& f, const std::string& key, const std::string& dflt) {
  const auto it = f.find(key);
  return it == f.end() ? dflt : it->second;
}

static const std::map<std::string, int> kRobots = {{"monoped", 0}, {"biped", 1}, {"hyq", 2}, {"anymal", 3}, {"go1", 4}};
static const std::map<std::string, int> kTerrains = {{"flat", 0}, {"block", 1}, {"stairs", 2}, {"gap", 3}, {"slope", 4}, {"chimney", 5},
                                                    {"chimney_lr", 6}, {"csv", 7}, {"grid_map", 8}};

// the structure of a `struct` line: the same fields, defaults and formulas as tests/eval_matrix.py make_case
static twr::Structure build(const Fields& f) {
  twr::Structure S;
  const double T = std::stod(get(f, "T", "2.0"));
  const int K = std::stoi(get(f, "K", "40"));
  const int terrain = kTerrains.at(get(f, "terrain", "flat"));
  twr::ModelPreset(kRobots.at(get(f, "robot", "anymal")), terrain, &S.model);
  if (terrain >= 7) {   // gridded terrains: the plan depends on the map's presence, not on its cells
    auto g = std::make_shared<twr::TerrainGrid>();
    g->rows = 7, g->cols = 9;
    g->grid_map = terrain == 8;
    if (g->grid_map) g->elevation.assign(63, 0.0f), g->res = 0.05, g->eps = 0.05 / 6.0;
    else g->heights.assign(63, 0.0);
    S.grid = g;
  }
  twr::GaitCombo(S.model.n_ee, std::stoi(get(f, "combo", "1")), T, std::stod(get(f, "swing", "1.0")), &S.schedule);
  twr_params& p = S.params;
  p.dt_dynamic = p.dt_rom = T / (K - 1.5);
  p.duration_base_poly = std::stod(get(f, "dbp", "0.1"));
  p.polys_per_swing = std::stoi(get(f, "pps", "2"));
  p.polys_per_stance_force = std::stoi(get(f, "ppf", "3"));
  p.constraint_sets = std::stoi(get(f, "sets", "27"));
  p.reserved_ = 0;
  p.dt_base_motion = std::stod(get(f, "dbm", "0.025"));
  p.base_z_init = -S.model.nominal_stance[0][2];
  S.Build();
  return S;
}

// a claim with its store wildcard filled in for a call: '*' -> G / J / GJ, + NT where the row streams and the kernel can
static std::string expand(const std::string& claim, int flags, bool nt) {
  const size_t at = claim.find('*');
  if (at == std::string::npos) return claim;
  const bool can_nt = claim.rfind("dyn_kernel", 0) == 0 || claim.rfind("dyn_uniform_kernel", 0) == 0 || claim.rfind("rom_kernel", 0) == 0 ||
                      claim.rfind("eval_fused_kernel", 0) == 0;
  std::string st = flags == 1 ? "G" : flags == 2 ? "J" : "GJ";
  if (nt && can_nt && (flags & 2)) st += "NT";
  return claim.substr(0, at) + st + claim.substr(at + 1);
}

static std::set<std::string> complete_set() {
  std::set<std::string> all;
  twr::LaunchStep p;
  auto put = [&](twr::Launch k, int store, int nit, int xc, int uni) {
    p = twr::LaunchStep();
    p.kernel = k, p.store = store, p.nit = nit, p.xc = xc, p.uni.s = uni;
    all.insert(twr::InstantiationName(p));
  };
  for (int st : twr::kStoresNT)
    for (int xc : twr::kDynXc) put(twr::Launch::kDyn, st, 0, xc, 0), put(twr::Launch::kDyn, st, 0, xc, 1);
  for (int st : twr::kStoresNT)
    for (int nit : twr::kRomNits) put(twr::Launch::kRom, st, nit, 0, 0);
  for (int st : twr::kStoresNT)
    for (int nit : twr::kFusedNits)
      for (int xc : twr::kDynXc) put(twr::Launch::kFused, st, nit, xc, 0);
  for (int st : twr::kStores) {
    for (int nit : twr::kDynPhaseNits) put(twr::Launch::kDynPhase, st, nit, 0, 0);
    for (int nit : twr::kRomPhaseNits) put(twr::Launch::kRomPhase, st, nit, 0, 0);
    put(twr::Launch::kChunk, st, 0, 0, 0);
  }
  for (int nx : twr::kValuesNx) put(twr::Launch::kValues, 0, 0, nx, 0), put(twr::Launch::kScores, 0, 0, nx, 0);
  return all;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::fprintf(stderr, "usage: eval_matrix_driver MATRIX.txt [--print] [--partial]\n");
    return 2;
  }
  bool print = false, partial = false;
  for (int i = 2; i < argc; ++i) {
    print = print || std::string(argv[i]) == "--print";
    partial = partial || std::string(argv[i]) == "--partial";
  }
  std::ifstream in(argv[1]);
  std::map<std::string, twr::Structure> structs;
  std::set<std::string> reached, excluded;
  const std::set<std::string> all = complete_set();
  CHECK(all.size() == 87, "%zu instantiations enumerated from the key lists, the matrix was written for 87", all.size());
  int n_rows = 0;
  std::string line;
  while (std::getline(in, line)) {
    const std::vector<std::string> tok = split(line, ' ');
    if (tok.empty() || tok[0][0] == '#') continue;
    if (tok[0] == "exclude") {   // exclude <instantiation> <the rule, free text>
      CHECK(tok.size() > 2, "exclusion of %s quotes no rule", tok.size() > 1 ? tok[1].c_str() : "?");
      if (tok.size() > 1) CHECK(excluded.insert(tok[1]).second, "%s excluded twice", tok[1].c_str());
      continue;
    }
    Fields f;
    for (size_t i = 2; i < tok.size(); ++i) {
      const size_t eq = tok[i].find('=');
      CHECK(eq != std::string::npos, "%s: field '%s'", tok[1].c_str(), tok[i].c_str());
      if (eq != std::string::npos) f[tok[i].substr(0, eq)] = tok[i].substr(eq + 1);
    }
    const std::string name = tok.size() > 1 ? tok[1] : "";
    if (tok[0] == "struct") {
      try {
        const twr::Structure& S = structs.emplace(name, build(f)).first->second;
        if (print)
          std::printf("struct %-12s n %d m %d nnz %d, %zu dyn slices staging <= %d doubles\n", name.c_str(), S.n_vars, S.n_rows, S.nnz,
                      S.dyn_slices.size(), S.dyn_staged_max);
      } catch (const std::exception& e) {
        CHECK(false, "struct %s: %s", name.c_str(), e.what());
      }
      continue;
    }
    CHECK(tok[0] == "row", "unknown line '%s'", tok[0].c_str());
    if (tok[0] != "row") continue;
    ++n_rows;
    // the batch: structs=a,b*3 (b three times: three tables in the arena), order=0,1,1 or cycle:N (problem p -> p % structures)
    std::vector<const twr::Structure*> sp;
    bool ok = true;
    for (const std::string& item : split(get(f, "structs", ""), ',')) {
      const size_t star = item.find('*');
      const std::string sn = item.substr(0, star);
      const int count = star == std::string::npos ? 1 : std::stoi(item.substr(star + 1));
      if (!structs.count(sn)) {
        CHECK(false, "row %s: no struct %s", name.c_str(), sn.c_str());
        ok = false;
        continue;
      }
      for (int i = 0; i < count; ++i) sp.push_back(&structs.at(sn));
    }
    std::vector<int32_t> sop;
    const std::string order = get(f, "order", "");
    if (order.rfind("cycle:", 0) == 0) {
      const int n = std::stoi(order.substr(6));
      for (int p = 0; p < n; ++p) sop.push_back(p % (int)sp.size());
    } else {
      for (const std::string& o : split(order, ',')) sop.push_back(std::stoi(o));
    }
    for (int si : sop) ok = ok && si >= 0 && si < (int)sp.size();
    CHECK(ok && !sop.empty() && !sp.empty(), "row %s: structures / order", name.c_str());
    if (!ok || sop.empty() || sp.empty()) continue;
    const std::string kind = get(f, "kind", "cheap");
    const bool nt = get(f, "nt", "0") == "1";
    if (kind == "cheap") {
      bool small = sop.size() <= 8;
      for (const twr::Structure* S : sp) small = small && (int)S->grid_dyn.size() <= 200;
      CHECK(small, "row %s: a cheap row has at most 8 problems of K <= 200", name.c_str());
    }
    const std::vector<size_t> off = twr::BlobOffsets(sp);
    std::vector<uint64_t> blob;
    for (size_t i = 0; i < sp.size(); ++i) blob.push_back(0x7f0000000000ull + off[i]);
    const twr::BatchPlan B = twr::PlanBatch(sp, sop, blob, kCu, kCache, twr::kForceChunk);
    const twr::EvalCounts counts = twr::CountsOf(B);
    CHECK(B.stream_nt == nt, "row %s: nt=%d but the batch %s (%.1f MB of output, %zu structures, %zu problems)", name.c_str(), (int)nt,
          B.stream_nt ? "streams" : "does not stream", 8e-6 * (double)(B.g_off.back() + B.j_off.back()), sp.size(), sop.size());
    if (kind == "chunk") {
      CHECK((int)sop.size() >= 8 * kCu && counts.fam[0] + counts.fam[1] + counts.fam[2] + counts.fam[3] > 0,
            "row %s: a chunk row has at least %d problems and chunk lists", name.c_str(), 8 * kCu);
    }
    if (kind == "nt") CHECK(4 * sp.size() > sop.size(), "row %s: 4 x structures > problems", name.c_str());
    struct Call {
      const char* key;
      int flags;
      bool events;
    };
    const Call calls[] = {{"val_off", 1, false}, {"val_on", 1, true}, {"jac_off", 2, false}, {"jac_on", 2, true}, {"jac_off", 3, false},
                          {"jac_on", 3, true}, {"scores", twr::kEvalScores, false}, {"scores", twr::kEvalScores | twr::kEvalBest, false}};
    for (const Call& c : calls) {
      const twr::EvalPlan P = twr::PlanEval(twr::MakeEvalShape(B, counts, kCu, c.flags, c.events, twr::LaunchTuning()));
      std::set<std::string> planned;
      std::string listing;
      for (int i = 0; i < P.n; ++i) {
        if (P.step[i].kernel == twr::Launch::kEvent) continue;
        planned.insert(twr::InstantiationName(P.step[i]));
        listing += " " + twr::InstantiationName(P.step[i]);
      }
      if (print) std::printf("%-22s flags %3d events %d:%s\n", name.c_str(), c.flags, (int)c.events, listing.c_str());
      std::vector<std::string> claims = split(get(f, c.key, ""), ';');
      if (c.flags & twr::kEvalBest) claims.push_back("best_kernel");
      for (const std::string& raw : claims) {
        const std::string want = expand(raw, c.flags & 3, nt);
        CHECK(planned.count(want), "row %s, flags %d, events %d: claims %s, planned:%s", name.c_str(), c.flags, (int)c.events, want.c_str(),
              listing.c_str());
        if (planned.count(want) && all.count(want)) reached.insert(want);
      }
    }
    if (print)
      std::printf("%-22s rom_max_vals %d flat_max_x %d chunks %d pdyn_img %d prom_img %d uniform %d, %.1f MB out\n", name.c_str(), B.rom_max_vals,
                  B.flat_max_x, B.dyn_map_chunks, B.pdyn_img_cap, B.prom_img_cap, B.dyn_uniform.s, 8e-6 * (double)(B.g_off.back() + B.j_off.back()));
  }
  CHECK(n_rows > 0, "no rows read from %s", argv[1]);
  CHECK((int)excluded.size() <= kMaxExclusions, "%zu exclusions, at most %d are allowed", excluded.size(), kMaxExclusions);
  for (const std::string& e : excluded) {
    CHECK(all.count(e), "exclusion %s is not an instantiation", e.c_str());
    CHECK(!reached.count(e), "exclusion %s is reached by a row", e.c_str());
  }
  if (!partial)
    for (const std::string& a : all) CHECK(reached.count(a) || excluded.count(a), "no row reaches %s and no rule excludes it", a.c_str());
  std::printf("eval_matrix_driver: %d rows, %zu of %zu instantiations reached, %zu excluded, %d failures\n", n_rows, reached.size(), all.size(),
              excluded.size(), fails);
  return fails ? 1 : 0;
}
