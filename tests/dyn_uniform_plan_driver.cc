// Checks of the uniform dyn plan on the host: twr::PlanBatch's detection of a batch whose problems all reference one
// structure (BatchPlan::dyn_uniform), twr::PlanEval's grid rule for dyn_uniform_kernel (DynUniformCols) and the schedule
// the kernel runs (device_tables.h dyn_uniform_slot, the same function the kernel calls).
// Built and run by tests/test_dyn_uniform_plan.py (tests/host_build.py: g++ against the host planner, no HIP).
// The lists and plans of every batch are held against hashes recorded from earlier commits: kParent from the commit before
// the uniform plan existed, kParentWide -- every field of BatchPlan, every plan the product makes, and the lists after
// PlaceRecords, also for batches that reach the chunk lists, four node families, mixed timings, one leg, four-chunk staging
// maps and non-temporal stores -- from the commit before the planner was cut into units.  With -DTWR_RECORD_PARENT the driver
// prints the kParentWide records instead of comparing them.
#include <map>
#include <string>
#include <vector>

#include "../towr_amd/csrc/batch_plan.h"
#include "plan_driver_common.h"

static twr::Structure build(int K, int sets, double T = 2.0) { return build(3, 0, 1, T, sets, 1.0, K); }   // ANYmal, flat ground

static twr::EvalShape shape_of(const twr::BatchPlan& B, int n_cu, int flags, bool events) {
  const auto& L = B.lists;
  twr::EvalShape s;
  s.n_cu = n_cu;
  s.dyn = (int)L.dyn.size(), s.rom = (int)L.rom.size(), s.node = (int)L.node.size() - 1, s.flat = (int)L.flat.size();
  for (int f = 0; f < 4; ++f) s.fam[f] = (int)L.fam[f].size();
  s.pdyn = (int)L.pdyn.size(), s.ploc = (int)L.ploc.size(), s.prom = (int)L.prom.size();
  s.rom_max_vals = B.rom_max_vals, s.flat_max_x = B.flat_max_x, s.dyn_map_chunks = B.dyn_map_chunks, s.node_families = B.node_families;
  s.pdyn_img_cap = B.pdyn_img_cap, s.prom_img_cap = B.prom_img_cap, s.stream_nt = B.stream_nt;
  s.dyn_uniform = B.dyn_uniform;
  s.flags = flags;
  s.events = events;
  s.score_fused = B.score_fused;
  return s;
}

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

// Recorded from the commit before the uniform plan (shapes without dyn_uniform; hence skip_dyn_grid).
struct Parent {
  const char* name;
  uint64_t lists, plans;
};
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

// the fields of BatchPlan hash_lists leaves out
static uint64_t hash_rest(const twr::BatchPlan& B) {
  Fnv f;
  f.vec(B.blob_of_problem), f.vec(B.t_total), f.vec(B.sample_ok);
  f.i64((int64_t)B.records_bytes), f.bytes(&B.dyn_uniform, sizeof(B.dyn_uniform));
  f.i64(B.score_slab), f.i64(B.dyn_layout_bytes), f.i64(B.dyn_layout_distinct_bytes);
  return f.h;
}
// every step, all bytes, of every plan the product makes for the batch: MakeEvalShape of its own counts for the three flag
// sets with and without events and for the two scoring requests
static uint64_t hash_all_plans(const twr::BatchPlan& B, int n_cu) {
  Fnv f;
  const twr::EvalCounts counts = twr::CountsOf(B);
  f.bytes(&counts, sizeof(counts));
  const int requests[] = {1, 2, 3, twr::kEvalScores, twr::kEvalScores | twr::kEvalBest};
  for (int flags : requests)
    for (int ev = 0; ev < 2; ++ev) {
      const twr::EvalPlan P = twr::PlanEval(twr::MakeEvalShape(B, counts, n_cu, flags, ev, twr::LaunchTuning()));
      f.i32(P.n);
      f.bytes(P.step, sizeof(twr::LaunchStep) * P.n);
    }
  return f.h;
}
static_assert(sizeof(twr::LaunchStep) == 19 * sizeof(int) && sizeof(twr::EvalCounts) == 11 * sizeof(int), "hashed as bytes: no padding");

// Recorded from the commit before the planner was cut into units (this driver with -DTWR_RECORD_PARENT).
// {lists, rest, plans, placed}
static const ParentRecord<4> kParentWide[] = {
    {"K200x1", {0xd38c8f7ad5a4121bull, 0x04b49bab4c05d851ull, 0x5f196f51efbffe75ull, 0xb0c0d10d3cdcbc69ull}},
    {"K200x5", {0xd835bec3e1fb0d34ull, 0x04cd81a14e2c4161ull, 0xb730afdbbab22369ull, 0x4d9a0c42318f74efull}},
    {"K200x8", {0x846b71163fa71a63ull, 0x033b25b3638591b4ull, 0x525c4a4cdc3b72daull, 0x7debfb581230068bull}},
    {"K200x400", {0xb464a77e2d66a3b6ull, 0xfd7333d1455cd028ull, 0x9d700e5541cd0352ull, 0xf4799452237f46f9ull}},
    {"K200x1603", {0xe810565d5662a24cull, 0x4a67e91fa5736564ull, 0xed66fc168ea4ba32ull, 0x809554945551c1f8ull}},
    {"K52x1", {0x228fb8eed1ecd6f0ull, 0xaac6c43da8f90f3bull, 0x53702f68cdb4a01cull, 0x6d5ff94211c687e3ull}},
    {"K52x5", {0x8416a04d93a4ab58ull, 0x3c3a1bf72c3553ebull, 0xf776f7ca6f5af8b4ull, 0xb2c8f4bc5748adffull}},
    {"K52x8", {0x63733ea4575729faull, 0x4159cbce2a19c4baull, 0xae486a0b17809372ull, 0xd353b6ab9c1e0374ull}},
    {"K52x400", {0xeac6f3f92aecd0adull, 0x6d0a61b5238d8302ull, 0x012cd756113a0d93ull, 0xc2733b8f4b0a27ccull}},
    {"K52x1603", {0x07c8f4ac0b48e150ull, 0xf53fa87fe7a89096ull, 0x3777f4706e0b4312ull, 0xd936f181c1c4b24cull}},
    {"K40x1", {0xe00ca2e72dd82730ull, 0x4ab4f2e4a2d9602full, 0x81a43028584af855ull, 0xdd2dfeb9b09619ecull}},
    {"K40x5", {0xf889855899a46fd9ull, 0x4d1141213862d95full, 0xd30d28a37d692389ull, 0xaf92c6ca854a0ed8ull}},
    {"K40x8", {0xf7ef4e7cb3f76bddull, 0xf58f103b3676eec6ull, 0x8c7e6d70aaa0a386ull, 0x5e96ab090e164662ull}},
    {"K40x400", {0x4482f12e51b3096eull, 0x3863c08206db8fb2ull, 0x0236a9990a36f698ull, 0xe865974b49b831faull}},
    {"K40x1603", {0x300efbc2be74351dull, 0x5147b22f5422166aull, 0x174d9367a0d355c7ull, 0xde1f43df27416219ull}},
    {"two-structures", {0xd119c7155fcdc376ull, 0x17f90878ee6532daull, 0xb6f813833a522dcaull, 0x86557d0a0acef799ull}},
    {"one-of-two", {0x5d1071de088ff67full, 0xbdd06f7ef2d64b61ull, 0xe4b32b4fc7031e48ull, 0x21c8675630521f87ull}},
    {"ragged", {0x5c8694222d84ccfbull, 0x68aeafee547dd0a5ull, 0x98a1fafc9d8587cdull, 0x2bc6d02daa49dcf2ull}},
    {"timings", {0x6e953c77b35ddcd3ull, 0x5f20daabcc795209ull, 0x641f948a27aac087ull, 0xf2a60e95ed5a8699ull}},
    {"chunks", {0xd32647b584efd103ull, 0x41557ff424c1825eull, 0x613d90ca0f559927ull, 0xda7b1a7ee2996185ull}},
    {"no-chunks", {0x83df377a5631850bull, 0x41557ff424c1825eull, 0x29dff78eebcb73a4ull, 0xf52a2d1b50a28927ull}},
    {"chunks-two", {0xff72dddcf2e5a99full, 0x2295e691021ff0e8ull, 0x2d0f7b91bf559c07ull, 0x65da41d53cc73fa9ull}},
    {"chunks-c12", {0x475a64d1a1b95c37ull, 0x8edf0c36423bc200ull, 0xfd39d72ebe1b3070ull, 0x14a4d30ee2704f4cull}},
    {"every", {0x4fcaba2bcf096173ull, 0x89ae6a9d324d0b37ull, 0xaa6eecb46457eb23ull, 0xe2bade87ef36ae6full}},
    {"mixed-timings", {0x888283872bcbea44ull, 0xf46d7ee2a2d407caull, 0x6460206b685f47acull, 0x5c1297c6e998c9b2ull}},
    {"one-leg", {0x56e24ea9ebf73e12ull, 0x8983455eb3e3ed0bull, 0x27b01b243a602bc3ull, 0x9e668bf04321ea89ull}},
    {"sweep-nt", {0xa3f879c560260b24ull, 0x36707e9217c2546full, 0xf430afcd1461221eull, 0xbf8e5062afa60931ull}},
    {"sweep-plain", {0xc4f30acd01a23a25ull, 0x36707e9217c2546full, 0xb87f51b1260a0362ull, 0x90ba4d0761c3a42full}},
};

static void wide_case(const std::string& name, const twr::BatchPlan& B, int n_cu) {
  twr::BatchPlan C = B;
  C.PlaceRecords(0x7e0000000000ull);
  Fnv placed;
  placed.i64((int64_t)hash_lists(C)), placed.i64((int64_t)hash_rest(C));
  const uint64_t hash[4] = {hash_lists(B), hash_rest(B), hash_all_plans(B, n_cu), placed.h};
  parent_record(kParentWide, name, hash);
}

static const int kCu = 256;

static void parent_case(const std::string& name, const twr::BatchPlan& B, bool uniform) {
  const uint64_t hl = hash_lists(B), hp = hash_plans(B, kCu, uniform);
  wide_case(name, B, kCu);
  const Parent* q = nullptr;
  for (const Parent& e : kParent)
    if (name == e.name) q = &e;
  CHECK(q != nullptr, "%s: no parent record", name.c_str());
  if (!q) return;
  CHECK(q->lists == hl, "%s: the work lists differ from the parent's (%016llx, parent %016llx)", name.c_str(), (unsigned long long)hl,
        (unsigned long long)q->lists);
  CHECK(q->plans == hp, "%s: the evaluation plans differ from the parent's (%016llx, parent %016llx)", name.c_str(),
        (unsigned long long)hp, (unsigned long long)q->plans);
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

// A small batch for kParentWide alone: what it reaches is asserted by the caller
static twr::BatchPlan small_case(const std::string& name, const std::vector<const twr::Structure*>& sp, const std::vector<int32_t>& sop, int n_cu,
                                 int64_t cache_bytes = (int64_t)256 << 20) {
  const twr::BatchPlan B = twr::PlanBatch(sp, sop, blob_at(sp.size()), n_cu, cache_bytes, twr::kForceChunk);
  wide_case(name, B, n_cu);
  const auto& L = B.lists;
  std::printf("small   %-14s families %d chunks %zu %zu %zu %zu, xc %d, nt %d, fused %d, uniform %d, %zu pdyn %zu ploc %zu prom, records %zu B\n",
              name.c_str(), B.node_families, L.fam[0].size(), L.fam[1].size(), L.fam[2].size(), L.fam[3].size(), B.dyn_map_chunks, (int)B.stream_nt,
              (int)B.score_fused, B.dyn_uniform.s, L.pdyn.size(), L.ploc.size(), L.prom.size(), B.records_bytes);
  return B;
}

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
  // The branches of PlanBatch the batches above leave out, on bipeds, the hopper and a K = 12 ANYmal (seconds under ASan).
  // The coarse grids here all stage more than 128 doubles in some slice (dyn_map_chunks == 4); K = 200 above stays below.
  const int kAll = 63;   // every set but TWR_SET_TOTAL_TIME and TWR_SET_BASE_ROM
  CHECK(k200.dyn_staged_max <= 128 && k40.dyn_staged_max > 128, "staged doubles: K200 %d, K40 %d", k200.dyn_staged_max, k40.dyn_staged_max);
  const twr::Structure biped = build(1, 0, 0, 2.0, kAll, 1.0, 24), biped_t = build(1, 0, 0, 2.0, kAll | 64, 1.0, 24);
  const twr::Structure biped_every = build(1, 0, 0, 2.0, 255, 1.1, 24), hopper = build(0, 0, 0, 2.0, kAll, 1.0, 24);
  const twr::Structure c12 = build(3, 0, 1, 2.0, kAll, 1.0, 12);
  const twr::Structure sw0 = build(1, 0, 1, 1.6, 27, 0.9, 24), sw1 = build(1, 0, 1, 1.8, 27, 0.9, 24), sw2 = build(1, 0, 2, 2.0, 27, 0.9, 24);
  const std::vector<int32_t> x32(32, 0);
  std::vector<int32_t> alt40(40);
  for (int i = 0; i < 40; ++i) alt40[i] = i % 2;
  auto chunks = [](const twr::BatchPlan& B) { return B.lists.fam[0].size() + B.lists.fam[1].size() + B.lists.fam[2].size() + B.lists.fam[3].size(); };
  {
    const twr::BatchPlan B = small_case("chunks", {&biped}, x32, 4);   // 32 problems >= 8 x 4 CUs
    CHECK(B.node_families == 4 && !B.lists.fam[0].empty() && !B.lists.fam[1].empty() && !B.lists.fam[2].empty() && !B.lists.fam[3].empty(),
          "chunks: no chunk lists");
    const twr::BatchPlan C = small_case("no-chunks", {&biped}, x32, 8);   // the same batch below the cut-over
    CHECK(C.node_families == 4 && chunks(C) == 0, "no-chunks: chunk lists below eight problems per CU");
    const twr::BatchPlan D = small_case("chunks-two", {&biped, &hopper}, alt40, 4);
    CHECK(chunks(D) > 0 && D.dyn_uniform.s == 0, "chunks-two");
    const twr::BatchPlan E = small_case("chunks-c12", {&c12}, x32, 4);
    CHECK(chunks(E) > 0 && E.dyn_map_chunks == 4, "chunks-c12: dyn_map_chunks %d", E.dyn_map_chunks);
  }
  {
    const twr::BatchPlan B = small_case("every", {&biped_every}, x32, 4);   // TWR_SET_BASE_ROM | TWR_SET_TOTAL_TIME: never chunked
    CHECK(B.node_families == 4 && chunks(B) == 0 && !B.lists.pdyn.empty() && !B.lists.prom.empty() && B.records_bytes > 0 && !B.score_fused, "every");
    const twr::BatchPlan C = small_case("mixed-timings", {&biped, &biped_t}, {0, 1, 0, 1, 1}, 256);
    CHECK(!C.lists.dyn.empty() && !C.lists.pdyn.empty() && !C.score_fused && C.lists.flat.empty() && C.lists.score_slot.empty() &&
              C.lists.score_first.empty() && C.score_slab == 0,
          "mixed-timings: fixed and optimised timings, no scoring lists");
    const twr::BatchPlan D = small_case("one-leg", {&hopper}, {0, 0, 0, 0, 0}, 256);
    CHECK(D.dyn_uniform.s > 0 && D.score_fused && D.lists.rom.size() % 5 == 0, "one-leg");
    const twr::BatchPlan E = small_case("sweep-nt", {&sw0, &sw1, &sw2}, {0, 1, 2}, 256, 1 << 10);   // a cache the output does not fit
    CHECK(E.stream_nt && E.node_families == 2, "sweep-nt: plain stores");
    const twr::BatchPlan F = small_case("sweep-plain", {&sw0, &sw1, &sw2}, {0, 1, 2}, 256);
    CHECK(!F.stream_nt, "sweep-plain: non-temporal stores");
  }
  std::printf("dyn_uniform_plan_driver: %d failures\n", fails);
  return fails ? 1 : 0;
}
