// Checks of the uniform dyn plan on the host: twr::PlanBatch's detection of a batch whose problems all reference one
// structure (BatchPlan::dyn_uniform), twr::PlanEval's grid rule for dyn_uniform_kernel (DynUniformCols) and the schedule
// the kernel runs (device_tables.h dyn_uniform_slot, the same function the kernel calls).
// Built and run by tests/test_dyn_uniform_plan.py (g++ against towr_amd/csrc/structure.cc, no HIP).
// With -DTWR_RECORD_PARENT the driver builds against a tree without the uniform plan and only prints the hashes of the
// lists and plans: that is how the values of kParent below were taken from the parent commit.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../towr_amd/csrc/structure.h"

static int fails = 0;
#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      std::fprintf(stderr, __VA_ARGS__);  \
      std::fprintf(stderr, "\n");         \
      ++fails;                            \
    }                                     \
  } while (0)

static twr::Structure build(int K, int sets, double T = 2.0) {
  twr::Structure S;
  twr::ModelPreset(3, 0, &S.model);   // ANYmal, flat ground
  twr::GaitCombo(S.model.n_ee, 1, T, 1.0, &S.schedule);
  twr_params& p = S.params;
  p.dt_dynamic = p.dt_rom = T / (K - 1.5);
  p.duration_base_poly = 0.1;
  p.polys_per_swing = 2;
  p.polys_per_stance_force = 3;
  p.constraint_sets = sets;
  p.reserved_ = 0;
  p.dt_base_motion = 0.025;
  p.base_z_init = -S.model.nominal_stance[0][2];
  S.Build();
  return S;
}

static twr::EvalShape shape_of(const twr::BatchPlan& B, int n_cu, int flags, bool events) {
  const auto& L = B.lists;
  twr::EvalShape s;
  s.n_cu = n_cu;
  s.dyn = (int)L.dyn.size(), s.rom = (int)L.rom.size(), s.node = (int)L.node.size() - 1, s.flat = (int)L.flat.size();
  for (int f = 0; f < 4; ++f) s.fam[f] = (int)L.fam[f].size();
  s.pdyn = (int)L.pdyn.size(), s.ploc = (int)L.ploc.size(), s.prom = (int)L.prom.size();
  s.rom_max_vals = B.rom_max_vals, s.flat_max_x = B.flat_max_x, s.dyn_map_chunks = B.dyn_map_chunks, s.node_families = B.node_families;
  s.pdyn_img_cap = B.pdyn_img_cap, s.prom_img_cap = B.prom_img_cap, s.stream_nt = B.stream_nt;
#ifndef TWR_RECORD_PARENT
  s.dyn_uniform = B.dyn_uniform;
#endif
  s.flags = flags;
  s.events = events;
  s.score_fused = B.score_fused;
  return s;
}

struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  }
  void i32(int v) { bytes(&v, sizeof(v)); }
  template <class T>
  void vec(const std::vector<T>& v) {
    i32((int)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};
// every work list and policy field of a plan as the parent commit had them
static uint64_t hash_lists(const twr::BatchPlan& B) {
  Fnv f;
  const auto& L = B.lists;
  f.vec(B.x_off), f.vec(B.g_off), f.vec(B.j_off);
  f.vec(L.dyn), f.vec(L.rom), f.vec(L.node), f.vec(L.flat), f.vec(L.pdyn), f.vec(L.ploc), f.vec(L.prom);
  for (int q = 0; q < 4; ++q) f.vec(L.fam[q]);
  f.vec(L.score_blob), f.vec(L.score_first), f.vec(L.score_slot);
  f.i32(B.rom_max_vals), f.i32(B.flat_max_x), f.i32(B.dyn_map_chunks), f.i32(B.node_families), f.i32(B.pdyn_img_cap), f.i32(B.prom_img_cap);
  f.i32(B.stream_nt), f.i32(B.score_fused);
  return f.h;
}
// the steps of every evaluation plan of the batch, field by field.  skip_dyn_grid: leave out the grid of the dyn launch (the
// one field the uniform plan changes in a uniform batch's plans; everything else must stay)
static uint64_t hash_plans(const twr::BatchPlan& B, int n_cu, bool skip_dyn_grid) {
  Fnv f;
  for (int flags = 1; flags <= 3; ++flags)
    for (int ev = 0; ev < 2; ++ev) {
      const twr::EvalPlan P = twr::PlanEval(shape_of(B, n_cu, flags, ev));
      f.i32(P.n);
      for (int i = 0; i < P.n; ++i) {
        const twr::LaunchStep& s = P.step[i];
        f.i32((int)s.kernel), f.i32(s.store), f.i32(s.nit), f.i32(s.xc), f.i32(s.block), f.i32(s.lds);
        if (!(skip_dyn_grid && s.kernel == twr::Launch::kDyn)) f.i32(s.grid);
        for (int a : s.arg) f.i32(a);
      }
    }
  return f.h;
}

// Recorded from the parent commit (this driver with -DTWR_RECORD_PARENT against its structure.cc).
struct Parent {
  const char* name;
  uint64_t lists, plans;
};
#ifndef TWR_RECORD_PARENT
static const Parent kParent[] = {
    {"K200x1", 0xd38c8f7ad5a4121bull, 0x255f7c84f401bde0ull},
    {"K200x5", 0xd835bec3e1fb0d34ull, 0xeda9422890f105b0ull},
    {"K200x8", 0x846b71163fa71a63ull, 0xc1264773840c9562ull},
    {"K200x400", 0xb464a77e2d66a3b6ull, 0x5fc99441df2a3027ull},
    {"K200x1603", 0xe810565d5662a24cull, 0xcc7130770930a308ull},
    {"K52x1", 0x228fb8eed1ecd6f0ull, 0xc35ad3f99a4a03e0ull},
    {"K52x5", 0x8416a04d93a4ab58ull, 0xd47b339591cc7e30ull},
    {"K52x8", 0x63733ea4575729faull, 0x479423f43aeec962ull},
    {"K52x400", 0xeac6f3f92aecd0adull, 0x933f8d5c7f6b644full},
    {"K52x1603", 0x07c8f4ac0b48e150ull, 0x31974f1269602548ull},
    {"K40x1", 0xe00ca2e72dd82730ull, 0x7c104ac951160a60ull},
    {"K40x5", 0xf889855899a46fd9ull, 0xd47b339591cc7e30ull},
    {"K40x8", 0xf7ef4e7cb3f76bddull, 0x479423f43aeec962ull},
    {"K40x400", 0x4482f12e51b3096eull, 0x933f8d5c7f6b644full},
    {"K40x1603", 0x300efbc2be74351dull, 0x31974f1269602548ull},
    {"two-structures", 0xd119c7155fcdc376ull, 0x35ecee3772865ae7ull},
    {"one-of-two", 0x5d1071de088ff67full, 0x4ede985ac0a66baaull},
    {"ragged", 0x5c8694222d84ccfbull, 0x832e05c9f9c19c0cull},
    {"timings", 0x6e953c77b35ddcd3ull, 0x57faed0562ce9373ull},
};
#endif

static std::vector<uint64_t> blob_at(size_t n) {
  std::vector<uint64_t> at;
  for (size_t i = 0; i < n; ++i) at.push_back(0x7f0000000000ull + 0x100000ull * i);
  return at;
}

static const int kCu = 256;

static void parent_case(const std::string& name, const twr::BatchPlan& B, bool uniform) {
  const uint64_t hl = hash_lists(B), hp = hash_plans(B, kCu, uniform);
#ifdef TWR_RECORD_PARENT
  std::printf("{\"%s\", 0x%016llxull, 0x%016llxull},\n", name.c_str(), (unsigned long long)hl, (unsigned long long)hp);
#else
  const Parent* q = nullptr;
  for (const Parent& e : kParent)
    if (name == e.name) q = &e;
  CHECK(q != nullptr, "%s: no parent record", name.c_str());
  if (!q) return;
  CHECK(q->lists == hl, "%s: the work lists differ from the parent's (%016llx, parent %016llx)", name.c_str(), (unsigned long long)hl,
        (unsigned long long)q->lists);
  CHECK(q->plans == hp, "%s: the evaluation plans differ from the parent's (%016llx, parent %016llx)", name.c_str(),
        (unsigned long long)hp, (unsigned long long)q->plans);
#endif
}

#ifndef TWR_RECORD_PARENT
template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static const twr::LaunchStep* dyn_step(const twr::EvalPlan& P) {
  for (int i = 0; i < P.n; ++i)
    if (P.step[i].kernel == twr::Launch::kDyn) return &P.step[i];
  return nullptr;
}

// the schedule of a uniform launch against the batch's list
static void check_schedule(const std::string& name, const twr::Structure& S, const twr::BatchPlan& B, int n, const twr::LaunchStep& st) {
  const auto& L = B.lists.dyn;
  const twr::DynUniform& u = st.uni;
  const int s = (int)S.dyn_slices.size();
  CHECK(u.s == s && u.n_problems == n && u.first_stride == std::min(8, n) && u.x_stride == S.n_vars && u.g_stride == S.n_rows &&
            u.j_stride == S.nnz,
        "%s: DynUniform {%d %d %d %d %d %d %d}", name.c_str(), u.s, u.cols, u.first_stride, u.n_problems, u.x_stride, u.g_stride, u.j_stride);
  // the grid rule
  const int w0 = 8 * kCu / 8, w = s * (w0 / s);
  CHECK(w0 - w <= w0 / 32, "%s: uniform although %d of %d waves per XCD would idle", name.c_str(), w0 - w, w0);
  CHECK(u.cols == std::min(w / s, (n + 7) / 8) && st.grid == 8 * s * u.cols && st.grid % 8 == 0 && st.block == 64,
        "%s: cols %d grid %d", name.c_str(), u.cols, st.grid);
  CHECK(st.grid <= 8 * kCu, "%s: grid %d exceeds the residency", name.c_str(), st.grid);
  std::map<int64_t, int> at;   // first Jacobian value -> list position
  for (size_t i = 0; i < L.size(); ++i) at[L[i].j_off] = (int)i;
  CHECK(at.size() == L.size() && (int)L.size() == s * n, "%s: %zu list entries", name.c_str(), L.size());
  std::vector<int> hits(L.size(), 0), xcd_of(n, -1), iter_of(n, -1);
  int bad_rec = 0, bad_kind = 0, bad_place = 0, active = 0;
  for (int b = 0; b < st.grid; ++b) {
    const twr::DynUniformSlot sl = twr::dyn_uniform_slot(u, b);
    CHECK(sl.kind >= 0 && sl.kind < s && sl.first >= 0 && sl.step == 8 * u.cols, "%s: block %d slot", name.c_str(), b);
    const size_t ti = (size_t)sl.kind * u.first_stride;
    if (ti >= L.size()) {
      CHECK(false, "%s: block %d reads list position %zu of %zu", name.c_str(), b, ti, L.size());
      continue;
    }
    const twr::DynWork& tmpl = L[ti];   // what the wave loads once
    CHECK(tmpl.x_off == 0, "%s: the record slice of kind %d is not problem 0's", name.c_str(), sl.kind);
    active += sl.first < n;
    int t = 0;
    for (int p = sl.first; p < n; p += sl.step, ++t) {
      twr::DynWork e = tmpl;   // the slice the wave evaluates in iteration t, as the kernel forms it
      e.x_off = tmpl.x_off + (int64_t)p * u.x_stride;
      e.g_off = tmpl.g_off + (int64_t)p * u.g_stride;
      e.j_off = tmpl.j_off + (int64_t)p * u.j_stride;
      const auto it = at.find(e.j_off);
      if (it == at.end() || std::memcmp(&e, &L[it->second], sizeof(e)) != 0) {   // records, counts and offsets: all bytes
        ++bad_rec;
        continue;
      }
      ++hits[it->second];
      bad_kind += L[it->second].nodes_t != tmpl.nodes_t;   // one kind per wave
      CHECK(e.x_off == B.x_off[p], "%s: x of problem %d", name.c_str(), p);
      if (xcd_of[p] < 0) xcd_of[p] = b & 7, iter_of[p] = t;
      bad_place += xcd_of[p] != (b & 7) || iter_of[p] != t;
    }
  }
  int bad_hits = 0;
  for (int h : hits) bad_hits += h != 1;
  CHECK(bad_rec == 0, "%s: %d scheduled slices are not list entries", name.c_str(), bad_rec);
  CHECK(bad_hits == 0, "%s: %d of %zu slices not evaluated exactly once", name.c_str(), bad_hits, L.size());
  CHECK(bad_kind == 0, "%s: %d slices of another kind than their wave's", name.c_str(), bad_kind);
  CHECK(bad_place == 0, "%s: %d slices away from their problem's XCD or iteration", name.c_str(), bad_place);
  std::printf("uniform %-14s s %2d cols %3d grid %4d, %d active waves, %zu slices\n", name.c_str(), s, u.cols, st.grid, active, L.size());
}

static void uniform_case(const std::string& name, const twr::Structure& S, int n, int want_s) {
  const std::vector<const twr::Structure*> sp = {&S};
  const std::vector<int32_t> sop(n, 0);
  const twr::BatchPlan B = twr::PlanBatch(sp, sop, blob_at(1), kCu, (int64_t)256 << 20, twr::kForceChunk);
  const twr::BatchPlan C = twr::PlanBatch(sp, sop, blob_at(1), kCu, (int64_t)256 << 20, twr::kForceChunk);
  CHECK((int)S.dyn_slices.size() == want_s, "%s: %zu dyn slices per problem, expected %d", name.c_str(), S.dyn_slices.size(), want_s);
  CHECK(same_bytes(B.lists.dyn, C.lists.dyn) && same_bytes(B.lists.rom, C.lists.rom) &&
            std::memcmp(&B.dyn_uniform, &C.dyn_uniform, sizeof(B.dyn_uniform)) == 0 && hash_lists(B) == hash_lists(C),
        "%s: planning twice differs", name.c_str());
  parent_case(name, B, true);
  CHECK(B.dyn_uniform.s == want_s && B.dyn_uniform.cols == 0, "%s: dyn_uniform.s %d", name.c_str(), B.dyn_uniform.s);
  for (int flags = 2; flags <= 3; ++flags) {
    // per-kernel events: three launches whatever the batch size (without them a batch this small takes the fused launch)
    const twr::EvalPlan P = twr::PlanEval(shape_of(B, kCu, flags, true)), Q = twr::PlanEval(shape_of(B, kCu, flags, true));
    const twr::LaunchStep* st = dyn_step(P);
    CHECK(st && st->uni.s > 0, "%s: flags %d: no uniform dyn launch", name.c_str(), flags);
    CHECK(P.n == Q.n && std::memcmp(P.step, Q.step, sizeof(P.step)) == 0, "%s: planning the evaluation twice differs", name.c_str());
    if (st && st->uni.s > 0) check_schedule(name, S, B, n, *st);
    // the fused launch keeps the general dyn role
    const twr::EvalPlan F = twr::PlanEval(shape_of(B, kCu, flags, false));
    for (int i = 0; i < F.n; ++i) CHECK(F.step[i].uni.s == 0 || F.step[i].kernel == twr::Launch::kDyn, "%s: uniform fields outside the dyn launch", name.c_str());
  }
  // the fallback: a residency the kinds do not divide (32 waves per XCD, s = 5 would idle 2 > 32 / 32) keeps the parent's launch
  twr::EvalShape a = shape_of(B, kCu, 3, true), g = a;
  a.tuning.dyn_bpc = 1;
  g.tuning.dyn_bpc = 1;
  g.dyn_uniform = twr::DynUniform{0, 0, 0, 0, 0, 0, 0, 0};
  const twr::EvalPlan Pa = twr::PlanEval(a), Pg = twr::PlanEval(g);
  const int w0 = kCu / 8, idle = w0 - want_s * (w0 / want_s);
  const twr::LaunchStep* sa = dyn_step(Pa);
  CHECK(sa && (sa->uni.s > 0) == (idle <= w0 / 32), "%s: one workgroup per CU: uniform %d with %d idle of %d", name.c_str(),
        sa ? sa->uni.s : -1, idle, w0);
  if (sa && sa->uni.s == 0) CHECK(Pa.n == Pg.n && std::memcmp(Pa.step, Pg.step, sizeof(Pa.step)) == 0, "%s: the fallback is not the general plan", name.c_str());
}

static void general_case(const std::string& name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop) {
  const twr::BatchPlan B = twr::PlanBatch(sp, sop, blob_at(sp.size()), kCu, (int64_t)256 << 20, twr::kForceChunk);
  CHECK(B.dyn_uniform.s == 0, "%s: taken for uniform", name.c_str());
  parent_case(name, B, false);
  for (int flags = 1; flags <= 3; ++flags)
    for (int ev = 0; ev < 2; ++ev) {
      const twr::EvalPlan P = twr::PlanEval(shape_of(B, kCu, flags, ev));
      for (int i = 0; i < P.n; ++i) CHECK(P.step[i].uni.s == 0, "%s: a uniform launch", name.c_str());
    }
  std::printf("general %-14s %zu dyn slices\n", name.c_str(), B.lists.dyn.size());
}
#endif

int main() {
  const twr::Structure k200 = build(200, 27), k52 = build(52, 27), k40 = build(40, 27), k200b = build(200, 27), timings = build(200, 91);
  struct {
    const char* name;
    const twr::Structure* S;
    int s;
  } kinds[] = {{"K200", &k200, 16}, {"K52", &k52, 5}, {"K40", &k40, 4}};
  const int sizes[] = {1, 5, 8, 400, 1603};
  const std::vector<const twr::Structure*> two = {&k200, &k200b}, mixed = {&k200, &k52, &k40}, tm = {&timings};
  std::vector<int32_t> alt(400), rag;
  for (int i = 0; i < 400; ++i) alt[i] = i & 1;
  for (int i = 0; i < 37; ++i) rag.push_back(i % 3);
#ifdef TWR_RECORD_PARENT
  for (const auto& k : kinds)
    for (int n : sizes) {
      const std::vector<const twr::Structure*> sp = {k.S};
      parent_case(std::string(k.name) + "x" + std::to_string(n), twr::PlanBatch(sp, std::vector<int32_t>(n, 0), blob_at(1), kCu, (int64_t)256 << 20, twr::kForceChunk), true);
    }
  parent_case("two-structures", twr::PlanBatch(two, alt, blob_at(2), kCu, (int64_t)256 << 20, twr::kForceChunk), false);
  parent_case("one-of-two", twr::PlanBatch(two, {1, 0}, blob_at(2), kCu, (int64_t)256 << 20, twr::kForceChunk), false);
  parent_case("ragged", twr::PlanBatch(mixed, rag, blob_at(3), kCu, (int64_t)256 << 20, twr::kForceChunk), false);
  parent_case("timings", twr::PlanBatch(tm, std::vector<int32_t>(5, 0), blob_at(1), kCu, (int64_t)256 << 20, twr::kForceChunk), false);
#else
  for (const auto& k : kinds)
    for (int n : sizes) uniform_case(std::string(k.name) + "x" + std::to_string(n), *k.S, n, k.s);
  general_case("two-structures", two, alt);     // two separately built equal structures, alternating
  general_case("one-of-two", two, {1, 0});
  general_case("ragged", mixed, rag);
  general_case("timings", tm, std::vector<int32_t>(5, 0));   // optimised phase durations: no DynWork at all
  // the grid rule on its own: 256 waves per XCD
  CHECK(twr::DynUniformCols(16, 8192, 2048) == 16 && twr::DynUniformCols(5, 8192, 2048) == 51 && twr::DynUniformCols(6, 8192, 2048) == 42,
        "DynUniformCols at 256 waves per XCD");
  CHECK(twr::DynUniformCols(13, 8192, 2048) == 0 && twr::DynUniformCols(300, 8192, 2048) == 0 && twr::DynUniformCols(0, 8192, 2048) == 0,
        "DynUniformCols fallback");   // 13: 247 of 256, nine idle > 8
  CHECK(twr::DynUniformCols(16, 5, 2048) == 1 && twr::DynUniformCols(16, 400, 2048) == 16 && twr::DynUniformCols(5, 1603, 2048) == 51,
        "DynUniformCols of small batches");
#endif
  std::printf("dyn_uniform_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
