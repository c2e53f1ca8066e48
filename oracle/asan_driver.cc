// TEST INFRASTRUCTURE ONLY -- sanitizer driver ("-fsanitize=address,undefined build of the
// CPU oracle"; extended to the product's host-side structure builder, which contains no HIP).
// Built by `make -C oracle asan` with -fsanitize=address,undefined and run by tests/test_sanitizers.py: walks
// robots x gait combos x constraint-set masks (incl. optimised timings and baseMotion) through
//   twr::Structure::Build / InitialGuess / VariableBounds   (towr_amd/csrc/structure.cc, presets.cc)
//   twr::ShareLayoutTables / PlanBatch (what twr_batch_create uploads; batch_plan.cc)
//   twr::PlanEval (the launches of one twr_batch_eval; eval_plan.cc)
//   orc_create / orc_eval / orc_bounds / orc_sample_trajectory (oracle/towr_oracle.cc)
// and cross-checks sizes and the CSR pattern of the two, so that every table write and every row of the
// pattern builders executes under the sanitizers.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../towr_amd/csrc/batch_plan.h"
#include "towr_oracle.h"

static int fails = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      std::fprintf(stderr, __VA_ARGS__);  \
      std::fprintf(stderr, "\n");         \
      ++fails;                            \
    }                                     \
  } while (0)

static void one_case(int robot, int terrain, int combo, double T, int sets, double dt) {
  twr_model m;
  twr::ModelPreset(robot, terrain, &m);
  twr_schedule s;
  twr::GaitCombo(m.n_ee, combo, T, 1.0, &s);
  twr_params p;
  p.dt_dynamic = dt;
  p.dt_rom = dt * 0.8;
  p.duration_base_poly = 0.1;
  p.polys_per_swing = 2;
  p.polys_per_stance_force = 3;
  p.constraint_sets = sets;
  p.reserved_ = 0;
  p.dt_base_motion = 0.025;
  p.base_z_init = -m.nominal_stance[0][2];
  twr::Structure S;
  S.model = m;
  S.schedule = s;
  S.params = p;
  S.Build();

  std::vector<int> n_ph(m.n_ee), con(m.n_ee);
  std::vector<double> pd;
  for (int e = 0; e < m.n_ee; ++e) {
    n_ph[e] = s.n_phases[e];
    con[e] = s.in_contact_at_start[e];
    for (int i = 0; i < s.n_phases[e]; ++i) pd.push_back(s.phase_durations[e][i]);
  }
  orc_problem* P = orc_create(robot, terrain, m.n_ee, n_ph.data(), pd.data(), con.data(), p.dt_dynamic, p.dt_rom,
                              p.duration_base_poly, p.polys_per_swing, p.polys_per_stance_force, m.force_limit, sets,
                              p.dt_base_motion, p.base_z_init, nullptr, 0, 0);
  CHECK(P != nullptr, "orc_create failed (robot %d combo %d sets %d)", robot, combo, sets);
  if (!P) return;
  CHECK(orc_n_vars(P) == S.n_vars, "n_vars %d vs %d", orc_n_vars(P), S.n_vars);
  CHECK(orc_n_rows(P) == S.n_rows, "n_rows %d vs %d", orc_n_rows(P), S.n_rows);

  // initial guess of both, then one full callback of the oracle on it
  std::vector<double> x(S.n_vars), xo(S.n_vars), ee(3 * m.n_ee);
  for (int e = 0; e < m.n_ee; ++e) {
    ee[3 * e] = m.nominal_stance[e][0];
    ee[3 * e + 1] = m.nominal_stance[e][1];
    ee[3 * e + 2] = 0.0;
  }
  const double z = -m.nominal_stance[0][2];
  const double lin0[3] = {0, 0, z}, ang0[3] = {0, 0, 0}, lin1[3] = {1.5, 0.1, z}, ang1[3] = {0, 0, 0.2};
  S.InitialGuess(lin0, ang0, lin1, ang1, ee.data(), x.data());
  orc_initial_guess(P, lin0, ang0, lin1, ang1, ee.data(), xo.data());
  for (int i = 0; i < S.n_vars; ++i) CHECK(std::fabs(x[i] - xo[i]) <= 1e-12 * (1 + std::fabs(xo[i])), "x0[%d] %g vs %g", i, x[i], xo[i]);

  const int nnz = orc_eval(P, x.data(), nullptr, nullptr, nullptr, nullptr);
  CHECK(nnz == S.nnz, "nnz %d vs %d (robot %d combo %d sets %d)", nnz, S.nnz, robot, combo, sets);
  std::vector<double> g(S.n_rows), v(nnz), lo(S.n_rows), up(S.n_rows);
  std::vector<int> rp(S.n_rows + 1), ci(nnz);
  orc_eval(P, x.data(), g.data(), rp.data(), ci.data(), v.data());
  if (nnz == S.nnz) {
    for (int r = 0; r <= S.n_rows; ++r) CHECK(rp[r] == S.row_ptr[r], "row_ptr[%d]", r);
    for (int i = 0; i < nnz; ++i) CHECK(ci[i] == S.col_idx[i], "col_idx[%d]", i);
  }
  for (double gv : g) CHECK(std::isfinite(gv), "non-finite g");
  orc_bounds(P, lo.data(), up.data());
  for (int r = 0; r < S.n_rows; ++r) CHECK(lo[r] == S.lower[r] && up[r] == S.upper[r], "bounds row %d", r);

  std::vector<double> vl(S.n_vars), vu(S.n_vars), ol(S.n_vars), ou(S.n_vars);
  double ib[12] = {0, 0, z, 0, 0, 0, 0, 0, 0, 0, 0, 0}, fb[12] = {1.5, 0.1, z, 0, 0, 0, 0, 0, 0.2, 0, 0, 0};
  S.VariableBounds(ib, fb, ee.data(), vl.data(), vu.data());
  orc_variable_bounds(P, ib, fb, ee.data(), ol.data(), ou.data());
  for (int i = 0; i < S.n_vars; ++i) CHECK(vl[i] == ol[i] && vu[i] == ou[i], "variable bound %d", i);

  const int ns = orc_sample_trajectory(P, x.data(), 0.05, nullptr, 0);
  CHECK(ns == S.SampleCount(0.05), "sample count %d vs %d", ns, S.SampleCount(0.05));
  std::vector<double> traj((size_t)ns * (20 + 13 * m.n_ee));
  orc_sample_trajectory(P, x.data(), 0.05, traj.data(), ns);
  orc_destroy(P);
}

// a structure as the sweeps of BASELINE build them: K time nodes of dynamic / range of motion
static twr::Structure build(int robot, int terrain, int combo, double T, int sets, double scale = 1.0, int K = 200,
                            std::shared_ptr<const twr::TerrainGrid> grid = nullptr) {
  twr::Structure S;
  twr::ModelPreset(robot, terrain, &S.model);
  twr::GaitCombo(S.model.n_ee, combo, T, scale, &S.schedule);
  twr_params& p = S.params;
  p.dt_dynamic = p.dt_rom = T / (K - 1.5);
  p.duration_base_poly = 0.1;
  p.polys_per_swing = 2;
  p.polys_per_stance_force = 3;
  p.constraint_sets = sets;
  p.reserved_ = 0;
  p.dt_base_motion = 0.025;
  p.base_z_init = -S.model.nominal_stance[0][2];
  S.grid = grid;
  S.Build();
  return S;
}

// the candidates of a sweep at K = 200 (hyq on the slope): T-siblings, swing-scale siblings and one other gait
static std::vector<twr::Structure> sweep_structures() {
  std::vector<twr::Structure> ss;
  for (int i = 0; i < 11; ++i)
    ss.push_back(build(2, 4, i == 10 ? 3 : 1, i < 8 ? 1.2 + 0.2 * i : 2.0, 27, i < 8 ? 0.80 : 0.80 + 0.016 * (i - 7)));
  return ss;
}

// twr::ShareLayoutTables (what twr::PlanBatch merges): T-siblings of a sweep at K = 200 share selector / polynomial-layout /
// tile tables, every reference points at bytes identical to the structure's own table, owners own themselves, and the
// byte counts add up.
static void sharing_case() {
  const std::vector<twr::Structure> ss = sweep_structures();
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  sp.push_back(&ss[3]);   // the same structure twice: shares everything with its first occurrence
  const twr::LayoutShare sh = twr::ShareLayoutTables(sp);
  int64_t built = 0, distinct = 0;
  for (size_t i = 0; i < sp.size(); ++i) {
    const auto& tabs = sp[i]->dyn_layout_tables;
    CHECK(sh.of[i].size() == tabs.size() && !tabs.empty(), "sharing: table count of structure %zu", i);
    for (size_t t = 0; t < tabs.size(); ++t) {
      const twr::LayoutShare::Ref r = sh.of[i][t];
      CHECK(r.owner >= 0 && r.owner <= (int)i, "sharing: owner after its user");
      const twr::Structure& O = *sp[r.owner];
      CHECK((size_t)r.off + tabs[t].bytes <= O.blob.size() && std::memcmp(O.blob.data() + r.off, sp[i]->blob.data() + tabs[t].off, tabs[t].bytes) == 0,
            "sharing: structure %zu table %zu reads other bytes", i, t);
      built += tabs[t].bytes;
      if (r.owner == (int)i && r.off == tabs[t].off) distinct += tabs[t].bytes;
    }
  }
  CHECK(built == sh.bytes_built && distinct == sh.bytes_distinct, "sharing: byte counts %lld / %lld vs %lld / %lld", (long long)built,
        (long long)distinct, (long long)sh.bytes_built, (long long)sh.bytes_distinct);
  CHECK(sh.bytes_distinct < sh.bytes_built * 85 / 100 && sh.bytes_distinct > sh.bytes_built / 3, "sharing: %lld of %lld bytes distinct",
        (long long)sh.bytes_distinct, (long long)sh.bytes_built);
  for (size_t t = 0; t < sh.of[11].size(); ++t) CHECK(sh.of[11][t].owner <= 3, "sharing: a repeated structure owns a table");
}

// the store policy of a batch (batch_plan.h): the measured cases of DESIGN 6.R4
static void policy_case() {
  const int64_t per = 859216;   // bytes per callback of a K = 200 quadruped candidate
  CHECK(twr::StreamNonTemporal(1024, 1024, 1024 * per), "policy: the 1024-candidate sweep streams");
  CHECK(twr::StreamNonTemporal(384, 384, 384 * per), "policy: 384 candidates stream");
  CHECK(!twr::StreamNonTemporal(256, 256, 256 * per), "policy: 256 candidates (220 MB) keep plain stores");
  CHECK(!twr::StreamNonTemporal(64, 64, 64 * per), "policy: 64 candidates keep plain stores");
  CHECK(!twr::StreamNonTemporal(1, 8192, 8192 * per), "policy: one structure for 8192 problems keeps plain stores");
  CHECK(!twr::StreamNonTemporal(1024, 4096, 4096 * per), "policy: four problems per structure keep plain stores");
  CHECK(twr::StreamNonTemporal(1024, 2048, 2048 * per), "policy: two problems per structure stream");
  // the threshold is the device's memory-side cache, by architecture name: MI355X / MI300X 256 MB, a CPX
  // partition its share, an unknown device eight times its L2 -- where a 384-candidate sweep keeps plain stores
  CHECK(twr::MemorySideCacheBytes("gfx950:sramecc+:xnack-", 4 << 20) == ((int64_t)256 << 20), "cache: gfx950");
  CHECK(twr::MemorySideCacheBytes("gfx942", 4 << 20, 8) == ((int64_t)32 << 20), "cache: a CPX partition of gfx942");
  CHECK(twr::MemorySideCacheBytes("gfx90a", 8 << 20) == ((int64_t)64 << 20), "cache: unknown architecture");
  CHECK(twr::StreamNonTemporal(128, 128, 128 * per, twr::MemorySideCacheBytes("gfx90a", 8 << 20)), "policy: follows the device's cache");
  CHECK(!twr::StreamNonTemporal(256, 256, 256 * per, twr::MemorySideCacheBytes("gfx950", 4 << 20)), "policy: MI355X as measured");
}

// a copy of list `a` with every non-zero address field (byte offsets `addr`) moved by `delta` must be `b`, byte for byte
template <class W>
static void check_moved(const char* what, const std::vector<W>& a, const std::vector<W>& b, std::initializer_list<size_t> addr,
                        uint64_t delta) {
  CHECK(a.size() == b.size(), "plan: %s has %zu vs %zu items", what, a.size(), b.size());
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) {
    char want[sizeof(W)];
    std::memcpy(want, &a[i], sizeof(W));
    for (size_t off : addr) {
      uint64_t v;
      std::memcpy(&v, want + off, 8);
      if (v) v += delta;
      std::memcpy(want + off, &v, 8);
    }
    if (std::memcmp(want, &b[i], sizeof(W)) != 0) {
      CHECK(false, "plan: %s[%zu] differs (blob delta %llu)", what, i, (unsigned long long)delta);
      return;
    }
  }
}


// twr::PlanEval (the launches of one evaluation).  A plan as text, one token per step: "e<i>" for an event, else the kernel
// and its instantiation (n = NIT, x = XC / NX, store variant), grid x block, dynamic LDS when there is any, then the role
// grids (fused, chunks) or groups / node families (values).
static const char* const kKernelName[] = {"e", "dyn", "rom", "fused", "ploc", "pdyn", "prom", "node", "node2", "chunk", "values"};
static const char* const kStoreName[] = {"G", "J", "GJ", "J+NT", "GJ+NT"};
static std::string describe(const twr::EvalPlan& plan, bool full = true) {
  std::string out;
  char buf[160];
  for (int i = 0; i < plan.n; ++i) {
    const twr::LaunchStep& p = plan.step[i];
    if (p.kernel == twr::Launch::kEvent) {
      std::snprintf(buf, sizeof buf, "%se%d", i ? " " : "", p.arg[0]);
    } else if (!full) {
      std::snprintf(buf, sizeof buf, "%s%s", i ? " " : "", kKernelName[(int)p.kernel]);
    } else {
      int n = std::snprintf(buf, sizeof buf, "%s%s", i ? " " : "", kKernelName[(int)p.kernel]);
      if (p.nit || p.kernel == twr::Launch::kDynPhase || p.kernel == twr::Launch::kRomPhase) n += std::snprintf(buf + n, sizeof buf - n, " n%d", p.nit);
      if (p.xc) n += std::snprintf(buf + n, sizeof buf - n, " x%d", p.xc);
      n += std::snprintf(buf + n, sizeof buf - n, " %s %dx%d", kStoreName[p.store], p.grid, p.block);
      if (p.lds) n += std::snprintf(buf + n, sizeof buf - n, " lds%d", p.lds);
      if (p.kernel == twr::Launch::kFused) n += std::snprintf(buf + n, sizeof buf - n, " [%d %d]", p.arg[0], p.arg[1]);
      if (p.kernel == twr::Launch::kChunk) n += std::snprintf(buf + n, sizeof buf - n, " [%d %d %d %d]", p.arg[0], p.arg[1], p.arg[2], p.arg[3]);
      if (p.kernel == twr::Launch::kValues) std::snprintf(buf + n, sizeof buf - n, " [%d %d %d]", p.arg[0], p.arg[1], p.arg[2]);
    }
    out += buf;
    if (full && p.kernel != twr::Launch::kEvent) out += ";";
  }
  return out;
}
static void expect_plan(const char* what, const twr::EvalShape& s, const char* want) {
  const std::string got = describe(twr::PlanEval(s));
  CHECK(got == want, "eval plan %s:\n  got  %s\n  want %s", what, got.c_str(), want);
}
template <size_t N>
static bool listed(const int (&keys)[N], int v) {
  return std::find(keys, keys + N, v) != keys + N;
}

// Both sides of every threshold of PlanEval on synthetic shapes of a 256-CU device (rom residency 4 x 256 = 1024 slices);
// the expected plans are worked out by hand from the rules, not by the planner's formulas.
static twr::EvalShape shape(int dyn, int rom, int node, int flags = 3) {
  twr::EvalShape s;
  s.n_cu = 256;
  s.dyn = dyn, s.rom = rom, s.node = node, s.flags = flags;
  s.rom_max_vals = 4000;   // copy-out 32 -> NIT 34 for rom and fused
  return s;
}
static void eval_threshold_cases() {
  // fused up to 20 rounds of rom residency; the split of the residency at 8 n_rom = 34 cap (5/8 for rom, then 4/8)
  expect_plan("fused at 20 rounds", shape(4000, 20480, 300), "fused n34 x2 GJ 1624x128 [512 512];");
  expect_plan("separate past 20 rounds", shape(4000, 20481, 300), "dyn x2 GJ 2048x64; rom n34 GJ 1024x64; node GJ 300x256;");
  expect_plan("split 5/8 at 34/8 rounds", shape(4096, 4352, 300), "fused n34 x2 GJ 1624x128 [640 384];");
  expect_plan("split 4/8 past 34/8 rounds", shape(4096, 4353, 300), "fused n34 x2 GJ 1624x128 [512 512];");
  expect_plan("roles that fit stay whole", shape(200, 300, 300), "fused n34 x2 GJ 996x128 [300 96];");
  expect_plan("g_dyn below 8", shape(13, 100, 10), "fused n34 x2 GJ 127x128 [100 7];");
  expect_plan("g_dyn at 8", shape(16, 100, 10), "fused n34 x2 GJ 128x128 [100 8];");
  expect_plan("g_dyn rounded to 8", shape(19, 100, 10), "fused n34 x2 GJ 128x128 [100 8];");
  // copy-out lengths: rom 26 / 30 / 34 / 38, fused 34 / 38 (whole store instructions of 128 doubles past a parity pair and one)
  const int rom_nit[][2] = {{3325, 26}, {3326, 30}, {3837, 30}, {3838, 34}, {4349, 34}, {4350, 38}, {twr::kRomStage, 38}};
  for (const auto& c : rom_nit) {
    twr::EvalShape s = shape(0, 1000, 0);
    s.rom_max_vals = c[0];
    const std::string want = "rom n" + std::to_string(c[1]) + " GJ 1000x64;";
    expect_plan(("rom copy-out of " + std::to_string(c[0])).c_str(), s, want.c_str());
  }
  twr::EvalShape f = shape(100, 100, 0);
  f.rom_max_vals = 4349;
  expect_plan("fused copy-out 34", f, "fused n34 x2 GJ 148x128 [100 48];");
  f.rom_max_vals = 4350;
  f.dyn_map_chunks = 4;
  expect_plan("fused copy-out 38", f, "fused n38 x4 GJ 148x128 [100 48];");
  // phase kernels: copy-out length and residency from the LDS image (dyn_phase_kernel at most 4 per CU, rom_phase_kernel 8)
  const int pdyn[][2] = {{1000, 0}, {5120, 0}, {5121, 0}, {8200, 0}};
  const char* const pdyn_want[] = {"pdyn n40 GJ 1024x64 lds8000;", "pdyn n40 GJ 1024x64 lds40960;", "pdyn n0 GJ 768x64 lds40976;",
                                   "pdyn n0 GJ 512x64 lds65600;"};
  for (int i = 0; i < 4; ++i) {
    twr::EvalShape s = shape(0, 0, 0);
    s.pdyn = 2000, s.pdyn_img_cap = pdyn[i][0];
    expect_plan(("pdyn image " + std::to_string(pdyn[i][0])).c_str(), s, pdyn_want[i]);
  }
  const int prom[] = {100, 3072, 3073, 4096, 4097, 5120, 5121, 8193};
  const char* const prom_want[] = {"prom n24 GJ 2048x64 lds800;",    "prom n24 GJ 1536x64 lds24576;", "prom n32 GJ 1536x64 lds24592;",
                                   "prom n32 GJ 1280x64 lds32768;",  "prom n40 GJ 1024x64 lds32784;", "prom n40 GJ 1024x64 lds40960;",
                                   "prom n0 GJ 768x64 lds40976;",    "prom n0 GJ 512x64 lds65552;"};
  for (int i = 0; i < 8; ++i) {
    twr::EvalShape s = shape(0, 0, 0);
    s.prom = 3000, s.prom_img_cap = prom[i];
    expect_plan(("prom image " + std::to_string(prom[i])).c_str(), s, prom_want[i]);
  }
  // values only: NX 3 / 5 / 8 for up to 3 / 5 / 8 x 256 variables; the node families ride along without events and chunks
  const int flat_x[] = {768, 769, 1280, 1281};
  const char* const flat_want[] = {"values x3 G 200x256 lds24592 [100 4 6160];", "values x5 G 200x256 lds24608 [100 4 6176];",
                                   "values x5 G 200x256 lds28688 [100 4 10256];", "values x8 G 200x256 lds28704 [100 4 10272];"};
  for (int i = 0; i < 4; ++i) {
    twr::EvalShape s = shape(1600, 1600, 100, 1);
    s.flat = 400, s.flat_max_x = flat_x[i];
    expect_plan(("values of " + std::to_string(flat_x[i]) + " variables").c_str(), s, flat_want[i]);
  }
  twr::EvalShape v = shape(1600, 1600, 100, 1);
  v.flat = 400, v.flat_max_x = 768, v.events = true;
  expect_plan("values with events", v, "e0 values x3 G 100x256 lds24592 [100 0 6160]; e1 e2 node G 100x256; e3");
  v.events = false, v.fam[1] = 100, v.fam[3] = 50;
  expect_plan("values with chunk lists", v, "values x3 G 100x256 lds24592 [100 0 6160]; chunk G 150x64 [0 100 0 50];");
  v.fam[1] = 0, v.fam[3] = 0, v.flags = 3;
  expect_plan("values and Jacobian", v, "fused n34 x2 GJ 1224x128 [640 384];");
  // chunk shares: one that rounds to 0 gets one block, none gets more than its chunks
  twr::EvalShape c = shape(0, 0, 2048);
  c.fam[0] = 100000, c.fam[1] = 1, c.fam[3] = 5000;
  expect_plan("chunk shares rounding to 0", c, "chunk GJ 4096x64 [3900 1 0 195];");
  c.fam[0] = 10, c.fam[1] = 20, c.fam[2] = 30, c.fam[3] = 40;
  expect_plan("chunk shares past the chunks", c, "chunk GJ 100x64 [10 20 30 40];");
  twr::EvalShape n2 = shape(0, 0, 300, 2);
  n2.node_families = 2;
  expect_plan("two node families", n2, "node2 J 300x128;");
  // every list with events, non-temporal stores (Jacobian only: the values-only store variant stays G)
  twr::EvalShape all = shape(100, 100, 10, 2);
  all.ploc = 4, all.pdyn = 50, all.prom = 60, all.pdyn_img_cap = 1000, all.prom_img_cap = 1000, all.dyn_map_chunks = 4;
  all.stream_nt = true, all.events = true;
  expect_plan("all lists, events", all, "e0 dyn x4 J+NT 100x64; ploc J 4x256; pdyn n40 J 50x64 lds8000; e1 prom n24 J 60x64 lds8000; "
              "rom n34 J+NT 100x64; e2 node J 10x256; e3");
  twr::EvalShape g = shape(100, 100, 10, 1);
  g.stream_nt = true;
  expect_plan("values with non-temporal stores", g, "fused n34 x2 G 168x128 [100 48];");
  g.flags = 3;
  expect_plan("both with non-temporal stores", g, "fused n34 x2 GJ+NT 168x128 [100 48];");

  // tuning knobs: split 8 = unsplit, explicit role grids clamped to the work, the residency counts
  twr::EvalShape k = shape(4096, 4352, 300);
  k.tuning.fused_split = 8;
  expect_plan("knob: split 8", k, "fused n34 x2 GJ 2648x128 [1024 1024];");
  k.tuning.fused_split = 6;
  expect_plan("knob: split 6", k, "fused n34 x2 GJ 1624x128 [768 256];");
  k = shape(4000, 3000, 0);
  k.tuning.fused_grom = 5000, k.tuning.fused_gdyn = 5000;
  expect_plan("knob: role grids clamped", k, "fused n34 x2 GJ 5000x128 [3000 2000];");
  k.tuning.fused_grom = 100, k.tuning.fused_gdyn = 13;
  expect_plan("knob: role grids", k, "fused n34 x2 GJ 108x128 [100 8];");
  k = shape(4000, 25000, 0);
  k.tuning.fused_max_rom = 30000;
  expect_plan("knob: fused up to more", k, "fused n34 x2 GJ 1024x128 [512 512];");
  k = shape(4000, 101, 0);
  k.tuning.fused_max_rom = 100;
  expect_plan("knob: fused up to less", k, "dyn x2 GJ 2048x64; rom n34 GJ 101x64;");
  k = shape(4000, 30000, 0);
  k.tuning.dyn_bpc = 4, k.tuning.rom_bpc = 2;
  expect_plan("knob: dyn / rom residency", k, "dyn x2 GJ 1024x64; rom n34 GJ 512x64;");
  k = shape(0, 0, 100);
  k.fam[0] = 1000, k.fam[1] = 1000, k.tuning.node_bpc = 1;
  expect_plan("knob: chunk residency", k, "chunk GJ 256x64 [128 128 0 0];");
  k = shape(0, 0, 0);
  k.pdyn = 2000, k.prom = 2000, k.pdyn_img_cap = 1000, k.prom_img_cap = 1000, k.tuning.pdyn_bpc = 2, k.tuning.prom_bpc = 3;
  expect_plan("knob: phase residency", k, "pdyn n40 GJ 512x64 lds8000; prom n24 GJ 768x64 lds8000;");
}

// Invariants of the plans of a PlanBatch result, for V, J and VJ with and without events: every list is launched exactly once
// (dyn and rom rows by their own kernels, the fused launch or the values-only launch; the node families by the node kernels,
// the chunk kernel, the fused launch's node role or the values-only launch), grids inside 1..items, copy-outs covering the
// largest slice, LDS within a CU, instantiations that exist, non-temporal stores only with the Jacobian, events in place.
static void eval_invariants(const char* name, const twr::BatchPlan& B, int n_cu) {
  const twr::BatchPlan::Lists& L = B.lists;
  for (int flags : {1, 2, 3})
    for (bool events : {false, true}) {
      twr::EvalShape s;
      s.n_cu = n_cu;
      s.dyn = (int)L.dyn.size(); s.rom = (int)L.rom.size(); s.node = (int)L.node.size() - 1; s.flat = (int)L.flat.size();
      s.pdyn = (int)L.pdyn.size(); s.ploc = (int)L.ploc.size(); s.prom = (int)L.prom.size();
      for (int f = 0; f < 4; ++f) s.fam[f] = (int)L.fam[f].size();
      s.rom_max_vals = B.rom_max_vals; s.flat_max_x = B.flat_max_x; s.dyn_map_chunks = B.dyn_map_chunks; s.node_families = B.node_families;
      s.pdyn_img_cap = B.pdyn_img_cap; s.prom_img_cap = B.prom_img_cap; s.stream_nt = B.stream_nt;
      s.flags = flags;
      s.events = events;
      const twr::EvalPlan plan = twr::PlanEval(s);
      const std::string text = describe(plan);
      const char* what = text.c_str();
      int dyn = 0, rom = 0, node = 0, pdyn = 0, ploc = 0, prom = 0, launches = 0, chunks = 0;
      for (int f = 0; f < 4; ++f) chunks += s.fam[f];
      for (int i = 0; i < plan.n; ++i) {
        const twr::LaunchStep& p = plan.step[i];
        if (p.kernel == twr::Launch::kEvent) continue;
        ++launches;
        int items = 0;
        bool key = true;
        const bool has_store = p.kernel != twr::Launch::kLocate && p.kernel != twr::Launch::kNode && p.kernel != twr::Launch::kNode2 &&
                               p.kernel != twr::Launch::kValues;
        switch (p.kernel) {
          case twr::Launch::kDyn: ++dyn; items = s.dyn; key = listed(twr::kDynXc, p.xc) && listed(twr::kStoresNT, p.store); break;
          case twr::Launch::kRom: ++rom; items = s.rom; key = listed(twr::kRomNits, p.nit) && listed(twr::kStoresNT, p.store); break;
          case twr::Launch::kFused:
            ++dyn, ++rom, ++node;
            items = s.rom + (s.dyn + 1) / 2 + 2 * s.node;
            key = listed(twr::kFusedNits, p.nit) && listed(twr::kDynXc, p.xc) && listed(twr::kStoresNT, p.store);
            CHECK(p.arg[0] >= 1 && p.arg[0] <= s.rom && p.arg[1] >= 1 && p.arg[1] <= (s.dyn + 1) / 2 && p.grid == p.arg[0] + p.arg[1] + 2 * s.node,
                  "%s: fused role grids in %s", name, what);
            break;
          case twr::Launch::kLocate: ++ploc; items = s.ploc; break;
          case twr::Launch::kDynPhase: ++pdyn; items = s.pdyn; key = listed(twr::kDynPhaseNits, p.nit) && listed(twr::kStores, p.store); break;
          case twr::Launch::kRomPhase: ++prom; items = s.prom; key = listed(twr::kRomPhaseNits, p.nit) && listed(twr::kStores, p.store); break;
          case twr::Launch::kNode: case twr::Launch::kNode2: ++node; items = s.node; break;
          case twr::Launch::kChunk:
            ++node;
            items = chunks;
            key = listed(twr::kStores, p.store);
            for (int f = 0; f < 4; ++f)
              CHECK(s.fam[f] ? p.arg[f] >= 1 && p.arg[f] <= s.fam[f] : p.arg[f] == 0, "%s: chunk grid of family %d in %s", name, f, what);
            CHECK(p.grid == p.arg[0] + p.arg[1] + p.arg[2] + p.arg[3], "%s: chunk grid in %s", name, what);
            break;
          case twr::Launch::kValues:
            ++dyn, ++rom, node += p.arg[1] > 0;
            items = s.flat / 4 + (p.arg[1] > 0 ? s.node : 0);
            key = listed(twr::kValuesNx, p.xc) && p.xc * 64 * twr::kFlatGroup >= s.flat_max_x;
            CHECK(p.arg[0] == s.flat / 4 && (p.arg[1] == 0 || p.arg[1] == s.node_families), "%s: values groups in %s", name, what);
            break;
          case twr::Launch::kEvent: break;
        }
        CHECK(p.grid >= 1 && p.grid <= items, "%s: grid %d of %d items in %s", name, p.grid, items, what);
        CHECK(key, "%s: an instantiation that does not exist in %s", name, what);
        CHECK(p.lds >= 0 && p.lds <= 160 * 1024, "%s: LDS in %s", name, what);
        if (has_store)
          CHECK(twr::StoreG(p.store) == (bool)(flags & 1) && twr::StoreJ(p.store) == (bool)(flags & 2) &&
                    (!twr::StoreNT(p.store) || s.stream_nt),
                "%s: store variant in %s", name, what);
        if (p.kernel == twr::Launch::kRom || p.kernel == twr::Launch::kFused)
          CHECK(p.nit * 128 >= s.rom_max_vals + 3, "%s: rom copy-out of %d in %s", name, s.rom_max_vals, what);
        if (p.kernel == twr::Launch::kDynPhase || p.kernel == twr::Launch::kRomPhase) {
          const int img = p.kernel == twr::Launch::kDynPhase ? s.pdyn_img_cap : s.prom_img_cap;
          CHECK(p.nit == 0 || p.nit * 128 >= img, "%s: phase copy-out of %d in %s", name, img, what);
          CHECK(p.lds >= 8 * img, "%s: phase image in %s", name, what);
        }
      }
      const bool values = (flags == 1) && s.flat > 0 && s.pdyn + s.ploc + s.prom == 0;
      CHECK(dyn == (s.dyn > 0 || values) && rom == (s.rom > 0 || values) && node == (s.node > 0) && pdyn == (s.pdyn > 0) &&
                ploc == (s.ploc > 0) && prom == (s.prom > 0),
            "%s: flags %d events %d: a list launched twice or not at all: %s", name, flags, events, what);
      // events: ev0 | launch | ev1 ev2 | nodes | ev3 (values only), ev0 | dyn ploc pdyn | ev1 | prom rom | ev2 | nodes | ev3
      std::vector<std::string> tok;
      const std::string seq = describe(plan, false);
      for (size_t a = 0, b; a < seq.size(); a = b + 1) {
        b = seq.find(' ', a);
        if (b == std::string::npos) b = seq.size();
        tok.push_back(seq.substr(a, b - a));
      }
      const char* const between[3] = {values ? " values " : " dyn ploc pdyn ", values ? " " : " prom rom ", " node node2 chunk "};
      int ev = 0;
      for (size_t t = 0; t < tok.size(); ++t) {
        if (tok[t][0] == 'e' && tok[t].size() == 2) {
          CHECK(events && tok[t][1] == '0' + ev && (ev > 0 || t == 0), "%s: events at %s", name, seq.c_str());
          ++ev;
        } else if (events) {
          CHECK(ev >= 1 && ev <= 3 && std::string(between[ev - 1]).find(" " + tok[t] + " ") != std::string::npos, "%s: events at %s", name,
                seq.c_str());
        }
      }
      CHECK(ev == (events ? 4 : 0) && (!events || tok.back() == "e3"), "%s: events at %s", name, seq.c_str());
      if (values && events) CHECK(seq.compare(0, 15, "e0 values e1 e2") == 0, "%s: events at %s", name, seq.c_str());
      if (seq.find("fused") != std::string::npos) CHECK(!events && launches == 1, "%s: the fused launch is not alone: %s", name, seq.c_str());
    }
}

// twr::PlanBatch (what twr_batch_create uploads besides the tables), on fake blob addresses: every row of dynamic,
// rangeofmotion-* and the chunked node families is written by exactly one work item at the g / Jacobian offsets of the
// CSR pattern, every list keeps each problem's items in order, the XCD order, whole flat groups of one problem, every
// address inside the blob it belongs to, and a plan that depends on nothing but its inputs (twice the same bytes; moving
// the blobs moves the addresses and nothing else).
static void plan_case(const char* name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop) {
  const int n_cu = 256, chunk = 32, P = (int)sop.size();
  const std::vector<size_t> off = twr::BlobOffsets(sp);
  std::vector<uint64_t> at(sp.size());
  for (size_t i = 0; i < sp.size(); ++i) {
    CHECK(off[i] % 256 == 0 && off[i + 1] >= off[i] + sp[i]->blob.size(), "%s: blob %zu placed at %zu", name, i, off[i]);
    at[i] = 0x7f0000000000ull + off[i];
  }
  twr::BatchPlan B = twr::PlanBatch(sp, sop, at, n_cu, (int64_t)256 << 20, chunk);
  const twr::BatchPlan::Lists& L = B.lists;
  auto in_blob = [&](uint64_t a, int si) { return a >= at[si] && a < at[si] + sp[si]->blob.size(); };
  auto in_any = [&](uint64_t a) {
    for (size_t i = 0; i < sp.size(); ++i)
      if (in_blob(a, (int)i)) return true;
    return false;
  };
  auto problem_of = [&](int64_t g) { return (int)(std::upper_bound(B.g_off.begin(), B.g_off.end(), g) - B.g_off.begin()) - 1; };
  CHECK((int)B.x_off.size() == P + 1 && (int)L.node.size() == P + 1 && L.node[P].blob == 0 && L.node[P].g_off == B.g_off[P] &&
            L.node[P].j_off == B.j_off[P] && L.node[P].x_off == B.x_off[P], "%s: offsets / node end entry", name);
  // rows written by the item lists: hits[p][row]
  std::vector<std::vector<int>> hits(P);
  for (int p = 0; p < P; ++p) {
    const twr::Structure& S = *sp[sop[p]];
    CHECK(B.x_off[p + 1] - B.x_off[p] == S.n_vars && B.g_off[p + 1] - B.g_off[p] == S.n_rows && B.j_off[p + 1] - B.j_off[p] == S.nnz,
          "%s: offsets of problem %d", name, p);
    CHECK(L.node[p].blob == at[sop[p]] && B.blob_of_problem[p] == at[sop[p]] && L.node[p].g_off == B.g_off[p], "%s: node item %d", name, p);
    hits[p].assign(S.n_rows, 0);
  }
  int bad = 0;
  auto rows = [&](const char* what, int64_t x_off, int64_t g_off, int64_t j_off, int n_rows, uint64_t own_addr) {
    const int p = problem_of(g_off);
    if (p < 0 || p >= P) {
      CHECK(false, "%s: %s item outside every problem", name, what);
      return;
    }
    const twr::Structure& S = *sp[sop[p]];
    const int r0 = (int)(g_off - B.g_off[p]);
    const bool ok = x_off == B.x_off[p] && r0 + n_rows <= S.n_rows && j_off - B.j_off[p] == S.row_ptr[r0] &&
                    (!own_addr || in_blob(own_addr, sop[p]));
    if (!ok && bad++ < 5) CHECK(false, "%s: %s item of problem %d at row %d", name, what, p, r0);
    for (int r = r0; r < std::min(r0 + n_rows, S.n_rows); ++r) hits[p][r]++;
  };
  for (const auto& w : L.dyn) {
    rows("dyn", w.x_off, w.g_off, w.j_off, 6 * w.cnt, w.nodes_t);
    for (uint64_t a : {w.nodes_l, w.sel, w.tile, w.poly_l, w.map, w.hdr}) CHECK(in_any(a), "%s: dyn layout address", name);
    CHECK(in_blob(w.poly_t, sop[problem_of(w.g_off)]), "%s: dyn poly_t", name);
  }
  for (const auto& w : L.rom) {
    rows("rom", w.x_off, w.g_off, w.j_off, 3 * w.cnt, w.nodes);
    CHECK(in_blob(w.segs, sop[problem_of(w.g_off)]), "%s: rom segs", name);
  }
  for (const auto& w : L.pdyn) {
    rows("pdyn", w.x_off, w.g_off, w.j_off, 6 * w.cnt, w.shared);
    for (uint64_t a : {w.hdr, w.mput, w.fput, w.ee}) CHECK(in_blob(a, sop[problem_of(w.g_off)]), "%s: pdyn address", name);
    CHECK(w.loc < B.records_bytes, "%s: pdyn scratch", name);
  }
  for (const auto& w : L.prom) {
    rows("prom", w.x_off, w.g_off, w.j_off, 3 * w.cnt, 0);
    CHECK(w.recs + sizeof(twr::RomRec) * w.cnt <= B.records_bytes, "%s: prom scratch", name);
  }
  for (const auto& w : L.ploc) {
    CHECK(in_any(w.blob) && w.recs <= B.records_bytes && w.dyn_loc <= B.records_bytes && (w.recs || w.dyn_loc), "%s: ploc item", name);
  }
  const int fam_rows[4] = {1, 5, 1, 4};
  for (int f = 0; f < 4; ++f)
    for (const auto& w : L.fam[f]) {
      rows("fam", w.x_off, w.g_off, w.j_off, fam_rows[f] * w.cnt, w.table);
      CHECK(w.blob == B.blob_of_problem[problem_of(w.g_off)] && w.cnt <= (f == 1 ? chunk : 64), "%s: fam %d item", name, f);
    }
  // exactly once: every row of dynamic / rangeofmotion-*, and the node families when there are chunk lists
  bool chunked = false;
  for (int f = 0; f < 4; ++f) chunked = chunked || !L.fam[f].empty();
  for (int p = 0; p < P; ++p) {
    const twr::Structure& S = *sp[sop[p]];
    const twr::DevStruct* H = reinterpret_cast<const twr::DevStruct*>(S.blob.data());
    std::vector<std::pair<int, int>> want;   // [first, end) row ranges
    for (const twr::SetInfo& cs : S.con_sets)
      if (cs.name == "dynamic" || cs.name.rfind("rangeofmotion-", 0) == 0) want.push_back({cs.offset, cs.offset + cs.size});
    if (chunked) {
      want.push_back({H->row_terrain, H->row_terrain + H->n_terrain_rows});
      want.push_back({H->row_force, H->row_force + 5 * H->n_force_nodes});
      want.push_back({H->row_acc, H->row_acc + 6 * H->n_junctions});
      want.push_back({H->row_swing, H->row_swing + 4 * H->n_swing_nodes});
    }
    std::vector<char> covered(S.n_rows, 0);
    for (const auto& w : want)
      for (int r = w.first; r < w.second; ++r) covered[r] = 1;
    for (int r = 0; r < S.n_rows; ++r)
      if (hits[p][r] != covered[r] && bad++ < 5) CHECK(false, "%s: problem %d row %d written %d times", name, p, r, hits[p][r]);
  }
  // each problem's items in their order (rows ascending); equal item counts: position j holds a problem = j mod 8
  auto order = [&](const char* what, const std::vector<int64_t>& g) {
    std::vector<int64_t> last(P, -1);
    std::vector<int> count(P, 0);
    for (int64_t x : g) {
      const int p = problem_of(x);
      CHECK(x > last[p], "%s: %s items of problem %d out of order", name, what, p);
      last[p] = x;
      count[p]++;
    }
    if (std::count(count.begin(), count.end(), count[0]) == P)
      for (size_t j = 0; j < (size_t)(P / 8 * 8) * count[0]; ++j)
        CHECK(problem_of(g[j]) % 8 == (int)(j % 8), "%s: %s position %zu on the wrong XCD", name, what, j);
  };
  std::vector<int64_t> gd, gr, gp;
  for (const auto& w : L.dyn) gd.push_back(w.g_off);
  for (const auto& w : L.rom) gr.push_back(w.g_off);
  for (const auto& w : L.pdyn) gp.push_back(w.g_off);
  order("dyn", gd);
  order("rom", gr);
  order("pdyn", gp);
  // flat: whole groups of four of one problem each, nothing when a problem has optimised timings
  bool timings = false;
  for (int si : sop) timings = timings || sp[si]->timings;
  CHECK(L.flat.size() % 4 == 0 && (!timings || L.flat.empty()), "%s: flat list of %zu items", name, L.flat.size());
  for (size_t i = 0; i < L.flat.size(); ++i) {
    const auto& w = L.flat[i];
    CHECK(w.x_off == L.flat[i & ~(size_t)3].x_off && w.n_x == L.flat[i & ~(size_t)3].n_x, "%s: flat group %zu of two problems", name, i / 4);
    if (w.cnt) CHECK(in_any(w.nodes) && in_any(w.polys), "%s: flat addresses", name);
  }
  // the same inputs plan the same bytes; moved blobs move every address and nothing else; the scratch placed
  const uint64_t delta = 0x12345600;
  std::vector<uint64_t> moved(at);
  for (auto& a : moved) a += delta;
  for (uint64_t d : {(uint64_t)0, delta}) {
    const twr::BatchPlan C = twr::PlanBatch(sp, sop, d ? moved : at, n_cu, (int64_t)256 << 20, chunk);
    const twr::BatchPlan::Lists& M = C.lists;
    check_moved("dyn", L.dyn, M.dyn, {offsetof(twr::DynWork, nodes_t), offsetof(twr::DynWork, nodes_l), offsetof(twr::DynWork, sel),
                                      offsetof(twr::DynWork, tile), offsetof(twr::DynWork, poly_t), offsetof(twr::DynWork, poly_l),
                                      offsetof(twr::DynWork, map), offsetof(twr::DynWork, hdr)}, d);
    check_moved("rom", L.rom, M.rom, {offsetof(twr::RomWork, nodes), offsetof(twr::RomWork, segs)}, d);
    check_moved("node", L.node, M.node, {offsetof(twr::NodeWork, blob)}, d);
    check_moved("flat", L.flat, M.flat, {offsetof(twr::FlatWork, nodes), offsetof(twr::FlatWork, polys)}, d);
    for (int f = 0; f < 4; ++f) check_moved("fam", L.fam[f], M.fam[f], {offsetof(twr::FamWork, blob), offsetof(twr::FamWork, table)}, d);
    check_moved("pdyn", L.pdyn, M.pdyn, {offsetof(twr::PDynWork, hdr), offsetof(twr::PDynWork, shared), offsetof(twr::PDynWork, mput),
                                         offsetof(twr::PDynWork, fput), offsetof(twr::PDynWork, ee)}, d);
    check_moved("ploc", L.ploc, M.ploc, {offsetof(twr::LocWork, blob)}, d);
    check_moved("prom", L.prom, M.prom, {}, d);
    check_moved("blob_of_problem", B.blob_of_problem, C.blob_of_problem, {0}, d);
    CHECK(C.x_off == B.x_off && C.j_off == B.j_off && C.t_total == B.t_total && C.sample_ok == B.sample_ok &&
              C.records_bytes == B.records_bytes && C.stream_nt == B.stream_nt && C.dyn_map_chunks == B.dyn_map_chunks &&
              C.node_families == B.node_families && C.rom_max_vals == B.rom_max_vals && C.flat_max_x == B.flat_max_x &&
              C.pdyn_img_cap == B.pdyn_img_cap && C.prom_img_cap == B.prom_img_cap && C.dyn_layout_bytes == B.dyn_layout_bytes,
          "%s: plan scalars differ", name);
  }
  const uint64_t base = 0x7e0000000000ull;
  B.PlaceRecords(base);
  for (const auto& w : L.ploc)
    CHECK((!w.recs || (w.recs >= base && w.recs < base + B.records_bytes)) && (!w.dyn_loc || (w.dyn_loc >= base && w.dyn_loc < base + B.records_bytes)),
          "%s: placed LocWork", name);
  for (const auto& w : L.prom) CHECK(w.recs >= base && w.recs < base + B.records_bytes, "%s: placed RomPhaseWork", name);
  for (const auto& w : L.pdyn) CHECK(w.loc >= base && w.loc < base + B.records_bytes, "%s: placed PDynWork", name);
  eval_invariants(name, B, n_cu);
  std::printf("plan %-9s %5d problems: dyn %zu rom %zu flat %zu fam %zu/%zu/%zu/%zu pdyn %zu ploc %zu prom %zu\n", name, P, L.dyn.size(),
              L.rom.size(), L.flat.size(), L.fam[0].size(), L.fam[1].size(), L.fam[2].size(), L.fam[3].size(), L.pdyn.size(),
              L.ploc.size(), L.prom.size());
}

static void plan_cases() {
  const twr::Structure c3 = build(3, 0, 1, 2.0, 63), c3_timings = build(3, 0, 1, 2.0, 127), c3_hot = build(3, 0, 1, 2.0, 27);
  plan_case("C3x2048", {&c3}, std::vector<int32_t>(2048, 0));   // 8 problems per CU: chunk lists
  plan_case("C3x200", {&c3}, std::vector<int32_t>(200, 0));
  plan_case("single", {&c3_hot}, {0});
  std::vector<twr::Structure> ss = sweep_structures();
  std::vector<const twr::Structure*> sp;
  for (const auto& s : ss) sp.push_back(&s);
  plan_case("ragged", sp, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 3, 5, 5, 0});
  const twr::Structure gap_timings = build(3, 3, 2, 1.8, 127, 0.9), stairs_all = build(3, 2, 0, 2.4, 255, 1.1);
  plan_case("mixed", {&c3, &gap_timings, &stairs_all, &c3_timings, &c3_hot}, {0, 1, 2, 1, 3, 2, 2, 1, 0, 1, 4, 4, 1, 2, 2, 3, 1, 0, 2, 1, 4});
  auto grid = std::make_shared<twr::TerrainGrid>();
  grid->rows = 40;
  grid->cols = 60;
  for (int i = 0; i < grid->rows * grid->cols; ++i) grid->heights.push_back(0.05 * ((i * 7919) % 13) / 13.0);
  const twr::Structure g1 = build(3, 7, 1, 2.0, 63, 1.0, 200, grid), g2 = build(3, 7, 0, 2.4, 27, 1.0, 120, grid);
  plan_case("grid", {&g1, &g2}, {0, 1, 1, 0, 0, 1, 0});
}

int main() {
  sharing_case();
  policy_case();
  eval_threshold_cases();
  plan_cases();
  int cases = 0;
  const int masks[] = {27, 63, 127, 255, 2, 8 | 64, 1 | 16};
  for (int robot = 0; robot < 5; ++robot) {
    const int n_ee = robot == 0 ? 1 : (robot == 1 ? 2 : 4);
    for (int combo = 0; combo < 5; ++combo)
      for (int mi = 0; mi < 7; ++mi) {
        if ((combo + mi + robot) % 3 != 0 && !(combo == 1 && mi < 4)) continue;  // a spread, not the full product
        const int terrain = (robot + combo + mi) % 7;
        (void)n_ee;
        one_case(robot, terrain, combo, 1.4 + 0.2 * combo, masks[mi], 0.1 - 0.01 * mi);
        ++cases;
      }
  }
  std::printf("asan_driver: %d cases, %d failures\n", cases, fails);
  return fails ? 1 : 0;
}
