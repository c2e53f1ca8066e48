// What every host plan driver (tests/*_plan_driver.cc, tests/eval_matrix_driver.cc) needs: the failure counter, a structure
// from the public presets, byte comparison and bounds-checked views of a plan's tables, hand-made patterns, stand-in device
// addresses, and the FNV-1a hasher behind the recorded plans (kParent / OPS_FINGERPRINTS).  Stand-alone programs built by
// tests/host_build.py against the host planner; no HIP.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
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

// A structure of the presets: K time nodes on the dynamic / range-of-motion grids, swing durations scaled by `scale`
static inline twr::Structure build(int robot, int terrain, int combo, double T, int sets, double scale, int K,
                                   std::shared_ptr<const twr::TerrainGrid> grid = nullptr, double base_poly = 0.1) {
  twr::Structure S;
  twr::ModelPreset(robot, terrain, &S.model);
  twr::GaitCombo(S.model.n_ee, combo, T, scale, &S.schedule);
  twr_params& p = S.params;
  p.dt_dynamic = p.dt_rom = T / (K - 1.5);
  p.duration_base_poly = base_poly;
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

// A pattern made by hand (only what the solver plans read): row r with len[r] entries from column first[r] on, every
// `step`-th column, over n variables.
static inline twr::Structure pattern(int n, const std::vector<int>& first, const std::vector<int>& len, int step) {
  twr::Structure S{};
  S.n_vars = n;
  S.n_rows = (int)len.size();
  S.row_ptr.push_back(0);
  for (size_t r = 0; r < len.size(); ++r) {
    for (int j = 0; j < len[r]; ++j) S.col_idx.push_back(first[r] + j * step);
    S.row_ptr.push_back((int32_t)S.col_idx.size());
  }
  S.nnz = (int)S.col_idx.size();
  return S;
}

template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// a table of `count` T at byte offset off of `tables`, or nullptr (and a failure) when it does not lie inside
template <class T>
static const T* table(const char* name, const std::vector<char>& tables, uint64_t off, size_t count) {
  const bool ok = off % alignof(T) == 0 && off <= tables.size() && count * sizeof(T) <= tables.size() - off;
  CHECK(ok, "%s: table [%llu, +%zu x %zu) outside the %zu bytes", name, (unsigned long long)off, count, sizeof(T), tables.size());
  return ok ? reinterpret_cast<const T*>(tables.data() + off) : nullptr;
}

// stand-in device addresses of n structures' blobs, 1 MB apart
static inline std::vector<uint64_t> blob_at(size_t n) {
  std::vector<uint64_t> at;
  for (size_t i = 0; i < n; ++i) at.push_back(0x7f0000000000ull + 0x100000ull * i);
  return at;
}

// FNV-1a, byte by byte.  A vector goes in as its length, then its bytes: vec() with the length as an int (the BatchPlan
// records of dyn_uniform_plan_driver.cc), vec64() as 8 bytes (the PlanJacOps fingerprints of test_jac_normal_plan.py).  Both
// stay, since records taken with either are in the tree.
struct Fnv {
  uint64_t h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  }
  void i32(int v) { bytes(&v, sizeof(v)); }
  void i64(int64_t v) { bytes(&v, sizeof(v)); }
  template <class T>
  void vec(const std::vector<T>& v) {
    i32((int)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
  template <class T>
  void vec64(const std::vector<T>& v) {
    i64((int64_t)v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
};

// The K hashes recorded for one batch from the commit before the planner was cut into units: printed with
// -DTWR_RECORD_PARENT, compared otherwise.
template <size_t K>
struct ParentRecord {
  const char* name;
  uint64_t hash[K];
};
template <size_t N, size_t K>
static void parent_record(const ParentRecord<K> (&records)[N], const std::string& name, const uint64_t (&hash)[K]) {
#ifdef TWR_RECORD_PARENT
  (void)records;
  std::printf("    {\"%s\", {", name.c_str());
  for (size_t k = 0; k < K; ++k) std::printf("%s0x%016llxull", k ? ", " : "", (unsigned long long)hash[k]);
  std::printf("}},\n");
#else
  const ParentRecord<K>* q = nullptr;
  for (const ParentRecord<K>& e : records)
    if (name == e.name) q = &e;
  CHECK(q != nullptr, "%s: no parent record", name.c_str());
  for (size_t k = 0; q && k < K; ++k)
    CHECK(q->hash[k] == hash[k], "%s: hash %zu differs from the parent's (%016llx, parent %016llx)", name.c_str(), k, (unsigned long long)hash[k],
          (unsigned long long)q->hash[k]);
#endif
}
