// C ABI of libtowr_amd.so (see include/towr_amd.h), the Jacobian linear algebra: the products with J (twr_jac_ops), the damped
// least-squares solves (twr_jac_lsq) and the bounded LM driver (twr_jac_lm).  Host code: the handles, the argument checks and the
// order of calls; every launch is a function of jac_tu.hip (jac_launch.h).  Of a batch it uses twr_batch_eval and the layout alone.
#include <cmath>
#include <cstring>

#include "capi_internal.h"
#include "jac_launch.h"

struct twr_jac_ops {   // twr::PlanJacOps's tables and work lists on the device, and the slab of J^T w's partials
  int device = 0, n_problems = 0;
  std::vector<int64_t> x_off, g_off, j_off;
  DevPtr<void> tables;
  DevList<twr::JacMulWork> mul;
  DevList<twr::JacTWork> tmul;
  DevList<twr::JacFoldWork> fold;
  DevPtr<double> slab;
  int lds_x = 0, distinct_patterns = 0;
  int64_t resident = 0;
  // The one-pass product (twr_jac_ops_reserve_normal) and the Gram matrix (twr_jac_ops_reserve_gram): planned, uploaded and
  // allocated on first use, from the patterns the device tables hold (read back then).  For that the host keeps, per distinct
  // pattern, its sizes and where its col / row_ptr tables lie (twr::JacPatternPlaces of the plan the handle was made from), and
  // every problem's pattern.
  struct PatternSizes {
    int32_t n, m, nnz;
  };
  std::vector<PatternSizes> pattern_sizes;
  std::vector<twr::JacPatternPlace> pattern_places;
  std::vector<int32_t> pattern_of_problem;
  size_t table_bytes = 0;
  bool normal_ready = false;
  DevPtr<void> ntables;
  DevList<twr::JacNormalWork> nwork;
  DevList<twr::JacFoldWork> nfold;
  DevPtr<double> nslab;
  int n_lds_x = 0, n_tile = 0;
  // The Gram matrix (twr_jac_ops_reserve_gram): twr::PlanJacGram's tables and work lists, made from the same patterns
  bool gram_ready = false;
  std::vector<int64_t> gram_off;
  DevPtr<void> gtables;
  DevList<twr::JacGramWork> gform;
  DevList<twr::JacGramMulWork> gmul;
  DevList<twr::JacGramSolveWork> gsolve;
  int gram_max_n = 0;
};

struct twr_jac_lsq {   // twr::PlanJacLsq's work records and bound tables on the device, and the solver's workspace
  twr_jac_ops* ops = nullptr;   // borrowed
  int device = 0, n_problems = 0;
  DevPtr<void> bounds;
  DevList<twr::JacLsqWork> work;
  DevPtr<double> ws;
  twr::LsqBuffers buf{};
  int lds_x = 0;
  int64_t resident = 0;
  DevPtr<double> ws2;           // the scaled solve's vectors (twr_jac_lsq_reserve_scaled); resident counts them once they exist
  twr::LsqScaledBuffers buf2{};
  int64_t ws2_e = 0, ws2_cp = 0, ws2_doubles = 0;
  DevPtr<double> ws3;           // the one-pass solve's vectors (twr_jac_lsq_solve_onepass); resident counts them once they exist
  twr::LsqOnepassBuffers buf3{};
  int64_t ws3_s = 0, ws3_u = 0, ws3_doubles = 0;
};

struct twr_jac_lm {   // the bounded LM driver: twr::PlanJacLm's workspace, and what twr_jac_lm_start bound
  twr_batch* batch = nullptr;   // borrowed
  twr_jac_lsq* lsq = nullptr;   // borrowed (and through it its twr_jac_ops)
  int device = 0, n_problems = 0;
  twr_jac_lm_params params{};
  int solver = TWR_JAC_LM_CGLS;
  DevPtr<double> gram;          // the driver's own N (twr_jac_lm_set_solver with TWR_JAC_LM_GRAM)
  DevPtr<double> ws;
  twr::LmBuffers buf{};
  int64_t resident = 0;
  double *x = nullptr, *g = nullptr, *jac = nullptr;   // the caller's (twr_jac_lm_start)
  const double *xlo = nullptr, *xup = nullptr;
};

namespace {

// A handle's products with one J on one stream: what the entry points launch, and the J the solves are given
twr::JacProducts products(const twr_jac_ops* ops, const double* jac, void* hip_stream) {
  return {ops->mul.d.get(),   ops->mul.n,   ops->tmul.d.get(),  ops->tmul.n,  ops->fold.d.get(), ops->fold.n,
          ops->nwork.d.get(), ops->nwork.n, ops->nfold.d.get(), ops->nfold.n, ops->slab.get(),   ops->nslab.get(),
          ops->lds_x,         ops->n_lds_x, ops->n_tile,        jac,          static_cast<hipStream_t>(hip_stream)};
}

// The launches of an entry point, on the handle's device (DeviceScope), as the entry point's return code
template <class Launch> int on_device(int device, Launch launch) {
  DeviceScope on(device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  return launched(launch());
}

// What every solve does before it launches, in this order: the argument checks, the workspace or tables the handle makes on
// first need (reserve; the handle is not read before), the handle's device.
template <class Reserve, class Launch>
int checked_solve(twr_jac_lsq* lsq, bool any_null, int iters, double tol, std::initializer_list<const void*> buffers, Reserve reserve,
                  Launch launch) {
  if (any_null) return fail(TWR_ERR_INVALID, "null argument");
  if (iters < 0 || !(tol >= 0.0)) return fail(TWR_ERR_INVALID, "iters and tol must not be negative");
  if (misaligned(buffers)) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  const int rc = reserve();
  if (rc != TWR_OK) return rc;
  return on_device(lsq->device, launch);
}

// twr_jac_lsq_solve_scaled, twr_jac_lsq_solve_masked and the LM driver's CGLS step (its own vectors: the checks pass, ws2 exists)
int solve_scaled(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu, const double* d_scale,
                 int iters, double tol, double* d_d, double* d_info, void* hip_stream, bool masked) {
  return checked_solve(
      lsq, !lsq || !d_jac || !d_b || !d_mu || !d_scale || !d_d || !d_info, iters, tol, {d_jac, d_b, d_w, d_mu, d_scale, d_d, d_info},
      [&] { return twr_jac_lsq_reserve_scaled(lsq); },
      [&] {
        return twr::launch_lsq_solve_scaled(lsq->work.d.get(), lsq->work.n, lsq->lds_x, lsq->buf, lsq->buf2, d_b, d_w, d_mu, d_scale, iters, tol,
                                            d_d, d_info, products(lsq->ops, d_jac, hip_stream), masked);
      });
}

// A plan's tables on the device, for its Place (never an empty allocation).  *bytes: what was allocated.
DevPtr<void> upload_tables(const std::vector<char>& tables, int64_t* bytes) {
  *bytes = (int64_t)std::max<size_t>(16, tables.size());
  DevPtr<void> d = dev_alloc<void>((size_t)*bytes);
  if (!tables.empty()) TWR_HIP(hipMemcpy(d.get(), tables.data(), tables.size(), hipMemcpyHostToDevice));
  return d;
}

// A workspace the solver allocates on first need (ws2, ws3); resident counts it from then on
int reserve_workspace(twr_jac_lsq* lsq, DevPtr<double>& ws, int64_t doubles) {
  try {
    DeviceScope on(lsq->device);
    TWR_HIP(on.status);
    ws = dev_alloc<double>(std::max<size_t>(16, sizeof(double) * (size_t)doubles));
    lsq->resident += 8 * doubles;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

}  // namespace

extern "C" {

int twr_structure_transpose(const twr_structure* s, int32_t* col_ptr, int32_t* row_idx, int32_t* csr_pos) {
  if (!s) return fail(TWR_ERR_INVALID, "null structure");
  try {
    const twr::CscPattern t = twr::TransposePattern(s->s);
    if (col_ptr) std::memcpy(col_ptr, t.col_ptr.data(), t.col_ptr.size() * sizeof(int32_t));
    if (row_idx && !t.row_idx.empty()) std::memcpy(row_idx, t.row_idx.data(), t.row_idx.size() * sizeof(int32_t));
    if (csr_pos && !t.csr_pos.empty()) std::memcpy(csr_pos, t.csr_pos.data(), t.csr_pos.size() * sizeof(int32_t));
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_jac_ops_create(const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem, int n_problems, int device,
                       twr_jac_ops** out) {
  if (!structs || !struct_of_problem || !out || n_structs < 1 || n_problems < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  twr::JacOpsPlan plan;
  try {   // argument errors
    plan = twr::PlanJacOps(structure_ptrs(structs, n_structs), std::vector<int32_t>(struct_of_problem, struct_of_problem + n_problems));
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  std::unique_ptr<twr_jac_ops> h(new twr_jac_ops());
  try {   // device errors
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
      return fail(TWR_ERR_NO_DEVICE, "no HIP device visible: towr_amd has no CPU fallback");
    if (device < 0 || device >= n_dev) return fail(TWR_ERR_INVALID, "device ordinal out of range");
    DeviceScope on(device);
    TWR_HIP(on.status);
    h->device = device;
    h->n_problems = n_problems;
    h->x_off = plan.x_off;
    h->g_off = plan.g_off;
    h->j_off = plan.j_off;
    int64_t tb = 0;
    h->tables = upload_tables(plan.tables, &tb);
    h->table_bytes = plan.tables.size();
    h->pattern_places = twr::JacPatternPlaces(plan, std::vector<int32_t>(struct_of_problem, struct_of_problem + n_problems));
    for (const twr::JacPatternPlace& a : h->pattern_places) {   // (a structure no problem uses leaves its pattern without a place)
      if (a.first_struct < 0) h->pattern_sizes.push_back({0, 0, 0});
      else h->pattern_sizes.push_back({structs[a.first_struct]->s.n_vars, structs[a.first_struct]->s.n_rows, structs[a.first_struct]->s.nnz});
    }
    plan.Place(reinterpret_cast<uint64_t>(h->tables.get()));
    h->mul = upload_nonempty(plan.mul);
    h->tmul = upload_nonempty(plan.tmul);
    h->fold = upload_nonempty(plan.fold);
    h->slab = dev_alloc<double>(sizeof(double) * std::max<size_t>(1, (size_t)plan.slab));
    h->lds_x = plan.mul_lds_x;
    h->distinct_patterns = plan.distinct_patterns;
    h->pattern_of_problem.resize(n_problems);
    for (int p = 0; p < n_problems; ++p) h->pattern_of_problem[p] = plan.pattern_of_struct[struct_of_problem[p]];
    h->resident = tb + (int64_t)(plan.mul.size() * sizeof(twr::JacMulWork) + plan.tmul.size() * sizeof(twr::JacTWork) +
                                 plan.fold.size() * sizeof(twr::JacFoldWork)) +
                  8 * std::max<int64_t>(1, plan.slab);
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    twr_jac_ops_destroy(h.release());
    return fail(TWR_ERR_HIP, e.what());
  }
}

void twr_jac_ops_destroy(twr_jac_ops* ops) {
  if (!ops) return;
  DeviceScope on(ops->device);
  delete ops;
}

int twr_jac_ops_layout(const twr_jac_ops* ops, int64_t* x_off, int64_t* g_off, int64_t* jac_off) {
  if (!ops) return fail(TWR_ERR_INVALID, "null handle");
  const size_t bytes = (ops->n_problems + 1) * sizeof(int64_t);
  if (x_off) std::memcpy(x_off, ops->x_off.data(), bytes);
  if (g_off) std::memcpy(g_off, ops->g_off.data(), bytes);
  if (jac_off) std::memcpy(jac_off, ops->j_off.data(), bytes);
  return TWR_OK;
}

int twr_jac_ops_bytes(const twr_jac_ops* ops, int64_t* resident, int32_t* distinct_patterns) {
  if (!ops) return fail(TWR_ERR_INVALID, "null handle");
  if (resident) *resident = ops->resident;
  if (distinct_patterns) *distinct_patterns = ops->distinct_patterns;
  return TWR_OK;
}

int twr_jac_mul(twr_jac_ops* ops, const double* d_jac, const double* d_v, double* d_y, void* hip_stream) {
  if (!ops || !d_jac || !d_v || !d_y) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_jac, d_v, d_y})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(ops->device, [&] { return twr::launch_jac_mul(products(ops, d_jac, hip_stream), d_v, d_y); });
}

int twr_jac_tmul(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_z, void* hip_stream) {
  if (!ops || !d_jac || !d_w || !d_z) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_jac, d_w, d_z})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(ops->device, [&] { return twr::launch_jac_tmul(products(ops, d_jac, hip_stream), d_w, d_z); });
}

int twr_jac_col_sqnorms(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_out, void* hip_stream) {
  if (!ops || !d_jac || !d_out) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_jac, d_w, d_out})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(ops->device, [&] { return twr::launch_jac_colsq(products(ops, d_jac, hip_stream), d_w, d_out); });
}

namespace {
// The distinct patterns of a products handle as structures (n_vars, n_rows, nnz, row_ptr, col_idx alone), read back from the
// tables the device holds: what the plans made after twr_jac_ops_create start from.
int ops_patterns(twr_jac_ops* ops, std::vector<twr::Structure>* out) {
  std::vector<char> tables(ops->table_bytes);
  try {
    DeviceScope on(ops->device);
    TWR_HIP(on.status);
    if (!tables.empty()) TWR_HIP(hipMemcpy(tables.data(), ops->tables.get(), tables.size(), hipMemcpyDeviceToHost));
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
  std::vector<twr::Structure>& pats = *out;
  pats.assign(ops->pattern_sizes.size(), twr::Structure{});
  for (size_t q = 0; q < pats.size(); ++q) {
    const twr_jac_ops::PatternSizes& Z = ops->pattern_sizes[q];
    const twr::JacPatternPlace& A = ops->pattern_places[q];
    twr::Structure& S = pats[q];
    S.n_vars = Z.n, S.n_rows = Z.m, S.nnz = Z.nnz;
    S.row_ptr.assign(Z.m + 1, 0);
    S.col_idx.resize(Z.nnz);
    if (Z.m > 0) {
      if (A.row_ptr + sizeof(int32_t) * (Z.m + 1) > tables.size() || A.col + sizeof(uint16_t) * Z.nnz > tables.size())
        return fail(TWR_ERR_INVALID, "a pattern's tables lie outside the handle's");
      std::memcpy(S.row_ptr.data(), tables.data() + A.row_ptr, sizeof(int32_t) * (Z.m + 1));
      const uint16_t* col = reinterpret_cast<const uint16_t*>(tables.data() + A.col);
      std::copy(col, col + Z.nnz, S.col_idx.begin());
    }
  }
  return TWR_OK;
}
}  // namespace

int twr_jac_ops_reserve_normal(twr_jac_ops* ops) { return twr_jac_ops_reserve_normal_tile(ops, twr::kJacNormNnz); }

int twr_jac_ops_reserve_normal_tile(twr_jac_ops* ops, int tile_entries) {
  if (!ops) return fail(TWR_ERR_INVALID, "null handle");
  if (tile_entries < 1 || tile_entries > twr::kJacNormNnz) return fail(TWR_ERR_INVALID, "the tile is 1 .. 2048 entries");
  if (ops->normal_ready)
    return ops->n_tile == tile_entries ? TWR_OK : fail(TWR_ERR_INVALID, "the one-pass tables exist, made for another tile");
  twr::JacNormalPlan plan;
  std::vector<twr::Structure> pats;
  int rc = ops_patterns(ops, &pats);
  if (rc != TWR_OK) return rc;
  try {
    std::vector<const twr::Structure*> sp;
    for (const twr::Structure& S : pats) sp.push_back(&S);
    plan = twr::PlanJacNormal(sp, ops->pattern_places, ops->pattern_of_problem, tile_entries);
    if (plan.x_off != ops->x_off || plan.g_off != ops->g_off || plan.j_off != ops->j_off)
      throw std::runtime_error("the one-pass plan's layout is not the handle's");
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  try {
    DeviceScope on(ops->device);
    TWR_HIP(on.status);
    TWR_HIP(twr::prepare_jac_normal());
    int64_t tb = 0;
    DevPtr<void> tables = upload_tables(plan.tables, &tb);
    plan.Place(reinterpret_cast<uint64_t>(ops->tables.get()), reinterpret_cast<uint64_t>(tables.get()));
    DevList<twr::JacNormalWork> work = upload_nonempty(plan.work);
    DevList<twr::JacFoldWork> fold = upload_nonempty(plan.fold);
    DevPtr<double> slab = dev_alloc<double>(sizeof(double) * std::max<size_t>(1, (size_t)plan.slab));
    ops->ntables = std::move(tables);
    ops->nwork = std::move(work);
    ops->nfold = std::move(fold);
    ops->nslab = std::move(slab);
    ops->n_lds_x = plan.lds_x;
    ops->n_tile = plan.tile;
    ops->resident += tb + (int64_t)(plan.work.size() * sizeof(twr::JacNormalWork) + plan.fold.size() * sizeof(twr::JacFoldWork)) +
                     8 * std::max<int64_t>(1, plan.slab);
    ops->normal_ready = true;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_jac_normal_mul(twr_jac_ops* ops, const double* d_jac, const double* d_w, const double* d_v, double* d_y, double* d_u,
                       void* hip_stream) {
  if (!ops || !d_jac || !d_v || !d_u) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_jac, d_w, d_v, d_y, d_u})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  if (!ops->normal_ready) {   // (tables of any tile serve)
    const int rc = twr_jac_ops_reserve_normal(ops);
    if (rc != TWR_OK) return rc;
  }
  return on_device(ops->device, [&] { return twr::launch_jac_normal(products(ops, d_jac, hip_stream), d_w, d_v, d_y, d_u); });
}

int twr_jac_lsq_create(twr_jac_ops* ops, const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem,
                       int n_problems, twr_jac_lsq** out) {
  if (!ops || !structs || !struct_of_problem || !out || n_structs < 1 || n_problems < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  twr::JacLsqPlan plan;
  try {   // argument errors
    plan = twr::PlanJacLsq(structure_ptrs(structs, n_structs), std::vector<int32_t>(struct_of_problem, struct_of_problem + n_problems));
    if (n_problems != ops->n_problems || plan.x_off != ops->x_off || plan.g_off != ops->g_off)
      throw std::runtime_error("the structures are not the ones the products handle was created with");
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  std::unique_ptr<twr_jac_lsq> h(new twr_jac_lsq());
  try {   // device errors
    DeviceScope on(ops->device);
    TWR_HIP(on.status);
    h->ops = ops;
    h->device = ops->device;
    h->n_problems = n_problems;
    int64_t bb = 0;
    h->bounds = upload_tables(plan.bounds, &bb);
    plan.Place(reinterpret_cast<uint64_t>(h->bounds.get()));
    h->work = upload(plan.work);
    h->ws = dev_alloc<double>(sizeof(double) * (size_t)plan.ws_doubles);
    double* w = h->ws.get();
    h->buf = {w + plan.ws_p, w + plan.ws_z, w + plan.ws_q, w + plan.ws_r, w + plan.ws_t, w + plan.ws_rec};
    h->lds_x = plan.lds_x;
    h->resident = bb + (int64_t)(plan.work.size() * sizeof(twr::JacLsqWork)) + 8 * plan.ws_doubles;
    h->ws2_e = plan.ws2_e, h->ws2_cp = plan.ws2_cp, h->ws2_doubles = plan.ws2_doubles;
    h->ws3_s = plan.ws3_s, h->ws3_u = plan.ws3_u, h->ws3_doubles = plan.ws3_doubles;
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    twr_jac_lsq_destroy(h.release());
    return fail(TWR_ERR_HIP, e.what());
  }
}

void twr_jac_lsq_destroy(twr_jac_lsq* lsq) {
  if (!lsq) return;
  DeviceScope on(lsq->device);
  delete lsq;
}

int twr_jac_lsq_bytes(const twr_jac_lsq* lsq, int64_t* resident) {
  if (!lsq) return fail(TWR_ERR_INVALID, "null handle");
  if (resident) *resident = lsq->resident;
  return TWR_OK;
}

int twr_jac_dot(twr_jac_lsq* lsq, int space, const double* d_a, const double* d_b, double* d_out, void* hip_stream) {
  if (!lsq || !d_a || !d_b || !d_out) return fail(TWR_ERR_INVALID, "null argument");
  if (space != 0 && space != 1) return fail(TWR_ERR_INVALID, "space is 0 (the x layout) or 1 (the g layout)");
  if (misaligned({d_a, d_b, d_out})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(lsq->device, [&] {
    return twr::launch_lsq_dot(lsq->work.d.get(), lsq->work.n, space, d_a, d_b, d_out, static_cast<hipStream_t>(hip_stream));
  });
}

int twr_jac_violation(twr_jac_lsq* lsq, const double* d_g, const double* d_w, double* d_r, double* d_w_active, double* d_merit,
                      void* hip_stream) {
  if (!lsq || !d_g || !d_r) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_g, d_w, d_r, d_w_active, d_merit})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(lsq->device, [&] {
    return twr::launch_lsq_violation(lsq->work.d.get(), lsq->work.n, d_g, d_w, d_r, d_w_active, d_merit, static_cast<hipStream_t>(hip_stream));
  });
}

int twr_jac_lsq_solve(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu, int iters,
                      double tol, double* d_d, double* d_info, void* hip_stream) {
  return checked_solve(
      lsq, !lsq || !d_jac || !d_b || !d_mu || !d_d || !d_info, iters, tol, {d_jac, d_b, d_w, d_mu, d_d, d_info}, [] { return TWR_OK; },
      [&] {
        return twr::launch_lsq_solve(lsq->work.d.get(), lsq->work.n, lsq->lds_x, lsq->buf, d_b, d_w, d_mu, iters, tol, d_d, d_info,
                                     products(lsq->ops, d_jac, hip_stream));
      });
}

int twr_jac_lsq_reserve_scaled(twr_jac_lsq* lsq) {
  if (!lsq) return fail(TWR_ERR_INVALID, "null handle");
  if (lsq->ws2) return TWR_OK;
  const int rc = reserve_workspace(lsq, lsq->ws2, lsq->ws2_doubles);
  if (rc == TWR_OK) lsq->buf2 = {lsq->ws2.get() + lsq->ws2_e, lsq->ws2.get() + lsq->ws2_cp};
  return rc;
}

int twr_jac_col_scale(twr_jac_lsq* lsq, const double* d_colsq, double* d_colsq_max, double rel_floor, double* d_scale, void* hip_stream) {
  if (!lsq || !d_colsq || !d_scale) return fail(TWR_ERR_INVALID, "null argument");
  if (!(rel_floor > 0.0 && rel_floor <= 1.0)) return fail(TWR_ERR_INVALID, "rel_floor must be in (0, 1]");
  if (misaligned({d_colsq, d_colsq_max, d_scale})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(lsq->device, [&] {
    return twr::launch_lsq_col_scale(lsq->work.d.get(), lsq->work.n, d_colsq, d_colsq_max, rel_floor, d_scale, static_cast<hipStream_t>(hip_stream));
  });
}

int twr_jac_lsq_solve_scaled(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                             const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream) {
  return solve_scaled(lsq, d_jac, d_b, d_w, d_mu, d_scale, iters, tol, d_d, d_info, hip_stream, false);
}

int twr_jac_lsq_reserve_onepass(twr_jac_lsq* lsq, int scaled) {
  if (!lsq) return fail(TWR_ERR_INVALID, "null handle");
  int rc = lsq->ops->normal_ready ? TWR_OK : twr_jac_ops_reserve_normal(lsq->ops);   // (tables of any tile serve)
  if (rc == TWR_OK && scaled) rc = twr_jac_lsq_reserve_scaled(lsq);
  if (rc != TWR_OK || lsq->ws3) return rc;
  rc = reserve_workspace(lsq, lsq->ws3, lsq->ws3_doubles);
  if (rc == TWR_OK) lsq->buf3 = {lsq->ws3.get() + lsq->ws3_s, lsq->ws3.get() + lsq->ws3_u};
  return rc;
}

int twr_jac_lsq_solve_onepass(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                              const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream) {
  return checked_solve(
      lsq, !lsq || !d_jac || !d_b || !d_mu || !d_d || !d_info, iters, tol, {d_jac, d_b, d_w, d_mu, d_scale, d_d, d_info},
      [&] { return twr_jac_lsq_reserve_onepass(lsq, d_scale != nullptr); },   // (what exists is left as it is)
      [&] {
        return twr::launch_lsq_solve_onepass(lsq->work.d.get(), lsq->work.n, lsq->buf, lsq->buf2, lsq->buf3, d_b, d_w, d_mu, d_scale, iters, tol,
                                             d_d, d_info, products(lsq->ops, d_jac, hip_stream));
      });
}

int twr_jac_lsq_solve_masked(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                             const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream) {
  return solve_scaled(lsq, d_jac, d_b, d_w, d_mu, d_scale, iters, tol, d_d, d_info, hip_stream, true);
}

int twr_jac_free_set(twr_jac_lsq* lsq, const double* d_x, const double* d_xlo, const double* d_xup, const double* d_z,
                     const double* d_scale_in, double* d_scale_out, double* d_nfree, void* hip_stream) {
  if (!lsq || !d_x || !d_xlo || !d_xup || !d_z || !d_scale_out || !d_nfree) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_x, d_xlo, d_xup, d_z, d_scale_in, d_scale_out, d_nfree})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(lsq->device, [&] {
    return twr::launch_lm_free_set(lsq->work.d.get(), lsq->work.n, d_x, d_xlo, d_xup, d_z, d_scale_in, d_scale_out, d_nfree,
                                   static_cast<hipStream_t>(hip_stream));
  });
}

int twr_structure_gram_pattern(const twr_structure* s, int32_t* row_ptr, int32_t* col_idx, int64_t* nnz) {
  if (!s) return fail(TWR_ERR_INVALID, "null structure");
  try {
    std::vector<int32_t> rp, ci;
    twr::GramPattern(s->s, &rp, &ci);
    if (row_ptr) std::memcpy(row_ptr, rp.data(), rp.size() * sizeof(int32_t));
    if (col_idx && !ci.empty()) std::memcpy(col_idx, ci.data(), ci.size() * sizeof(int32_t));
    if (nnz) *nnz = (int64_t)ci.size();
    return TWR_OK;
  } catch (const twr::JacGramUnsupported& e) {
    return fail(TWR_ERR_UNSUPPORTED, e.what());
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_jac_ops_reserve_gram(twr_jac_ops* ops) {
  if (!ops) return fail(TWR_ERR_INVALID, "null handle");
  if (ops->gram_ready) return TWR_OK;
  twr::JacGramPlan plan;
  std::vector<twr::Structure> pats;
  const int rc = ops_patterns(ops, &pats);
  if (rc != TWR_OK) return rc;
  try {
    std::vector<const twr::Structure*> sp;
    for (const twr::Structure& S : pats) sp.push_back(&S);
    plan = twr::PlanJacGram(sp, ops->pattern_of_problem);
    if (plan.x_off != ops->x_off || plan.g_off != ops->g_off || plan.j_off != ops->j_off)
      throw std::runtime_error("the Gram plan's layout is not the handle's");
  } catch (const twr::JacGramUnsupported& e) {
    return fail(TWR_ERR_UNSUPPORTED, e.what());
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  try {
    DeviceScope on(ops->device);
    TWR_HIP(on.status);
    TWR_HIP(twr::prepare_gram_cg());
    int64_t tb = 0;
    DevPtr<void> tables = upload_tables(plan.tables, &tb);
    plan.Place(reinterpret_cast<uint64_t>(tables.get()));
    DevList<twr::JacGramWork> form = upload_nonempty(plan.form);
    DevList<twr::JacGramMulWork> mul = upload_nonempty(plan.mul);
    ops->gsolve = upload(plan.solve);
    ops->gtables = std::move(tables);
    ops->gform = std::move(form);
    ops->gmul = std::move(mul);
    ops->gram_off = plan.gram_off;
    ops->gram_max_n = plan.max_n;
    ops->resident += tb + (int64_t)(plan.form.size() * sizeof(twr::JacGramWork) + plan.mul.size() * sizeof(twr::JacGramMulWork) +
                                    plan.solve.size() * sizeof(twr::JacGramSolveWork));
    ops->gram_ready = true;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_jac_ops_gram_layout(const twr_jac_ops* ops, int64_t* gram_off) {
  if (!ops || !gram_off) return fail(TWR_ERR_INVALID, "null argument");
  if (!ops->gram_ready) return fail(TWR_ERR_INVALID, "twr_jac_ops_reserve_gram has not been called");
  std::memcpy(gram_off, ops->gram_off.data(), (ops->n_problems + 1) * sizeof(int64_t));
  return TWR_OK;
}

int twr_jac_gram(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_gram, void* hip_stream) {
  if (!ops || !d_jac || !d_gram) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_jac, d_w, d_gram})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  const int rc = twr_jac_ops_reserve_gram(ops);   // (nothing to do once the tables exist)
  if (rc != TWR_OK) return rc;
  return on_device(ops->device, [&] {
    return twr::launch_jac_gram(ops->gform.d.get(), ops->gform.n, d_jac, d_w, d_gram, static_cast<hipStream_t>(hip_stream));
  });
}

int twr_jac_gram_mul(twr_jac_ops* ops, const double* d_gram, const double* d_v, double* d_u, void* hip_stream) {
  if (!ops || !d_gram || !d_v || !d_u) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_gram, d_v, d_u})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  const int rc = twr_jac_ops_reserve_gram(ops);
  if (rc != TWR_OK) return rc;
  return on_device(ops->device, [&] {
    return twr::launch_jac_gram_mul(ops->gmul.d.get(), ops->gmul.n, d_gram, d_v, d_u, static_cast<hipStream_t>(hip_stream));
  });
}

int twr_jac_lsq_solve_gram(twr_jac_lsq* lsq, const double* d_gram, const double* d_z, const double* d_mu, const double* d_scale, int iters,
                           double tol, double* d_d, double* d_info, void* hip_stream) {
  return checked_solve(
      lsq, !lsq || !d_gram || !d_z || !d_mu || !d_d || !d_info, iters, tol, {d_gram, d_z, d_mu, d_scale, d_d, d_info},
      [&] { return twr_jac_ops_reserve_gram(lsq->ops); },
      [&] {
        const twr_jac_ops* ops = lsq->ops;
        return twr::launch_gram_cg(ops->gsolve.d.get(), ops->gsolve.n, ops->gram_max_n, d_gram, d_z, d_mu, d_scale, iters, tol, d_d, d_info,
                                   static_cast<hipStream_t>(hip_stream));
      });
}

int twr_jac_lm_params_default(twr_jac_lm_params* out) {
  if (!out) return fail(TWR_ERR_INVALID, "null output");
  out->cg_iters = 60;
  out->power_iters = 30;
  out->cg_tol = 1e-8;
  out->mu_down = 1.0 / 3.0;
  out->mu_up = 10.0;
  out->mu_min = 1e-16;
  out->mu_max = 1e16;
  out->rel_floor = 1e-12;
  out->tau = 1e-2;
  out->merit_done = 0.0;
  return TWR_OK;
}

int twr_jac_lm_create(twr_batch* batch, twr_jac_lsq* lsq, const twr_jac_lm_params* params, twr_jac_lm** out) {
  if (!batch || !lsq || !params || !out) return fail(TWR_ERR_INVALID, "null argument");
  const twr_jac_lm_params& q = *params;
  if (q.cg_iters < 0 || q.power_iters < 0 || !(q.cg_tol >= 0.0) || !(q.mu_down > 0.0 && q.mu_down <= 1.0) || !(q.mu_up >= 1.0) ||
      !(q.mu_min >= 0.0 && q.mu_min <= q.mu_max) || !std::isfinite(q.mu_up) || !std::isfinite(q.mu_max) ||
      !(q.rel_floor > 0.0 && q.rel_floor <= 1.0) || !(q.tau > 0.0) || !std::isfinite(q.tau) || q.merit_done != q.merit_done)
    return fail(TWR_ERR_INVALID, "bad LM parameters");
  const twr_jac_ops* ops = lsq->ops;
  if (batch->n_problems != ops->n_problems || batch->plan.x_off != ops->x_off || batch->plan.g_off != ops->g_off ||
      batch->plan.j_off != ops->j_off)
    return fail(TWR_ERR_INVALID, "the batch's layout is not the products handle's");
  if (batch->device != lsq->device) return fail(TWR_ERR_INVALID, "the batch and the solver live on different devices");
  const int n = batch->n_problems;
  twr::JacLmPlan plan;   // (from the layout: the plan reads the sizes alone)
  {
    std::vector<twr::Structure> sizes(n);
    std::vector<const twr::Structure*> sp(n);
    std::vector<int32_t> sop(n);
    for (int p = 0; p < n; ++p) {
      sizes[p].n_vars = (int)(ops->x_off[p + 1] - ops->x_off[p]);
      sizes[p].n_rows = (int)(ops->g_off[p + 1] - ops->g_off[p]);
      sp[p] = &sizes[p], sop[p] = p;
    }
    try {
      plan = twr::PlanJacLm(sp, sop);
    } catch (const std::exception& e) {
      return fail(TWR_ERR_INVALID, e.what());
    }
  }
  if (plan.x_off != ops->x_off || plan.g_off != ops->g_off) return fail(TWR_ERR_INVALID, "the driver's plan does not match the layout");
  const int rc = twr_jac_lsq_reserve_scaled(lsq);
  if (rc != TWR_OK) return rc;
  std::unique_ptr<twr_jac_lm> h(new twr_jac_lm());
  try {
    DeviceScope on(lsq->device);
    TWR_HIP(on.status);
    h->batch = batch, h->lsq = lsq, h->device = lsq->device, h->n_problems = n, h->params = q;
    h->ws = dev_zeros<double>(std::max<size_t>(2, (size_t)plan.ws_doubles));
    double* w = h->ws.get();
    h->buf = {w + plan.ws_xt, w + plan.ws_d,  w + plan.ws_z,  w + plan.ws_colsq, w + plan.ws_colmax,  w + plan.ws_c,
              w + plan.ws_cf, w + plan.ws_r,  w + plan.ws_b,  w + plan.ws_wa,    w + plan.ws_gt,      w + plan.ws_rt,
              w + plan.ws_rec, w + plan.ws_mu, w + plan.ws_merit_t, w + plan.ws_merit_lin, w + plan.ws_nfree, w + plan.ws_info};
    h->resident = 8 * std::max<int64_t>(2, plan.ws_doubles);
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    twr_jac_lm_destroy(h.release());
    return fail(TWR_ERR_HIP, e.what());
  }
}

void twr_jac_lm_destroy(twr_jac_lm* lm) {
  if (!lm) return;
  DeviceScope on(lm->device);
  delete lm;
}

int twr_jac_lm_bytes(const twr_jac_lm* lm, int64_t* resident) {
  if (!lm) return fail(TWR_ERR_INVALID, "null handle");
  if (resident) *resident = lm->resident;
  return TWR_OK;
}

static_assert(TWR_JAC_LM_REC == twr::kLmRec, "the record of twr_jac_lm_state");

int twr_jac_lm_set_solver(twr_jac_lm* lm, int solver) {
  if (!lm) return fail(TWR_ERR_INVALID, "null handle");
  if (solver != TWR_JAC_LM_CGLS && solver != TWR_JAC_LM_GRAM) return fail(TWR_ERR_INVALID, "solver is TWR_JAC_LM_CGLS or TWR_JAC_LM_GRAM");
  if (lm->x) return fail(TWR_ERR_INVALID, "the solver is chosen between twr_jac_lm_create and twr_jac_lm_start");
  if (solver == TWR_JAC_LM_GRAM && !lm->gram) {
    twr_jac_ops* ops = lm->lsq->ops;
    const int rc = twr_jac_ops_reserve_gram(ops);
    if (rc != TWR_OK) return rc;
    try {
      DeviceScope on(lm->device);
      TWR_HIP(on.status);
      const int64_t doubles = std::max<int64_t>(2, ops->gram_off.back());
      lm->gram = dev_zeros<double>((size_t)doubles);
      lm->resident += 8 * doubles;
    } catch (const std::exception& e) {
      return fail(TWR_ERR_HIP, e.what());
    }
  }
  lm->solver = solver;
  return TWR_OK;
}

namespace {
twr::LmParams lm_device_params(const twr_jac_lm_params& q) { return {q.mu_down, q.mu_up, q.mu_min, q.mu_max, q.tau, q.merit_done}; }

// eval(BOTH) at x, then what the linearisation is made of (twr::launch_lm_linearise)
int lm_linearise(twr_jac_lm* lm, int first, hipStream_t stream) {
  twr_jac_lsq* lsq = lm->lsq;
  const int rc = twr_batch_eval(lm->batch, lm->x, lm->g, lm->jac, TWR_EVAL_BOTH, stream);
  if (rc != TWR_OK) return rc;
  return launched(twr::launch_lm_linearise(lsq->work.d.get(), lm->n_problems, lm->x, lm->g, lm->xlo, lm->xup, lm->buf, lm->params.merit_done,
                                           lm->params.rel_floor, first, products(lsq->ops, lm->jac, stream)));
}
}  // namespace

// (twr_jac_lm_start and twr_jac_lm_step hold their DeviceScope themselves: between their launches they call entry points that
// return codes of their own)
int twr_jac_lm_start(twr_jac_lm* lm, double* d_x, const double* d_xlo, const double* d_xup, double* d_g, double* d_jac,
                     void* hip_stream) {
  if (!lm || !d_x || !d_xlo || !d_xup || !d_g || !d_jac) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_x, d_xlo, d_xup, d_g, d_jac})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  DeviceScope on(lm->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  lm->x = d_x, lm->xlo = d_xlo, lm->xup = d_xup, lm->g = d_g, lm->jac = d_jac;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  twr_jac_lsq* lsq = lm->lsq;
  const twr::JacLsqWork* work = lsq->work.d.get();
  const int n = lm->n_problems;
  const hipError_t e = twr::launch_lm_project(work, n, d_x, d_xlo, d_xup, lm->buf, lm->params.tau, stream);
  if (e != hipSuccess) return launched(e);
  const int rc = lm_linearise(lm, 1, stream);
  if (rc != TWR_OK) return rc;
  return launched(twr::launch_lm_power(work, n, lm->buf, lm_device_params(lm->params), lm->params.power_iters,
                                       products(lsq->ops, d_jac, stream)));
}

int twr_jac_lm_step(twr_jac_lm* lm, void* hip_stream) {
  if (!lm) return fail(TWR_ERR_INVALID, "null handle");
  if (!lm->x) return fail(TWR_ERR_INVALID, "twr_jac_lm_start has not been called");
  DeviceScope on(lm->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  twr_jac_lsq* lsq = lm->lsq;
  const twr_jac_ops* ops = lsq->ops;
  const twr::LmBuffers& B = lm->buf;
  const twr::JacLsqWork* work = lsq->work.d.get();
  const int n = lm->n_problems;
  int rc = lm_linearise(lm, 0, stream);
  if (rc != TWR_OK) return rc;
  if (lm->solver == TWR_JAC_LM_GRAM) {   // N = J^T W_a J once, then the whole masked solve on it in one launch (z is the linearisation's)
    hipError_t e = twr::launch_jac_gram(ops->gform.d.get(), ops->gform.n, lm->jac, B.wa, lm->gram.get(), stream);
    if (e == hipSuccess)
      e = twr::launch_gram_cg(ops->gsolve.d.get(), ops->gsolve.n, ops->gram_max_n, lm->gram.get(), B.z, B.mu, B.cf, lm->params.cg_iters,
                              lm->params.cg_tol, B.d, B.info, stream);
    rc = launched(e);
  } else {
    rc = solve_scaled(lsq, lm->jac, B.b, B.wa, B.mu, B.cf, lm->params.cg_iters, lm->params.cg_tol, B.d, B.info, stream, true);
  }
  if (rc != TWR_OK) return rc;
  const hipError_t e = twr::launch_lm_trial(work, n, lm->x, lm->xlo, lm->xup, B, stream);
  if (e != hipSuccess) return launched(e);
  rc = twr_batch_eval(lm->batch, B.xt, B.gt, nullptr, TWR_EVAL_VALUES, stream);
  if (rc != TWR_OK) return rc;
  return launched(twr::launch_lm_accept(work, n, lm->x, B, lm_device_params(lm->params), stream));
}

int twr_jac_lm_state(twr_jac_lm* lm, double* d_out, void* hip_stream) {
  if (!lm || !d_out) return fail(TWR_ERR_INVALID, "null argument");
  if (misaligned({d_out})) return fail(TWR_ERR_INVALID, "buffers must be 8-byte aligned");
  return on_device(lm->device, [&] {
    return hipMemcpyAsync(d_out, lm->buf.rec, sizeof(double) * twr::kLmRec * (size_t)lm->n_problems, hipMemcpyDeviceToDevice,
                          static_cast<hipStream_t>(hip_stream));
  });
}

}  // extern "C"
