// C ABI of libtowr_amd.so (see include/towr_amd.h), the batch runtime: structures, batches, their evaluation, sampling,
// planes and scoring; error reporting.  The Jacobian linear algebra (twr_jac_*) is capi_jac.cc, on the launchers of jac_tu.hip (jac_launch.h).
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <thread>
#include <utility>

#include "capi_internal.h"

namespace {
thread_local std::string g_err;
}
int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {
// sample_kernel's work list (twr_batch_sample, twr_batch_initial_guess): count(p) samples of problem p, 64 per item, its
// records from p * stride on.  The old list is freed once the new one is known.
template <class Count>
void build_sample_work(twr_batch& b, DevList<twr::SampleWork>& list, int64_t stride, Count count) {
  std::vector<twr::SampleWork> work;
  for (int p = 0; p < b.n_problems; ++p) {
    const int n = count(p);
    if (!b.plan.sample_ok[p]) throw std::runtime_error("too many polynomials per spline for trajectory sampling");
    for (int s0 = 0; s0 < n; s0 += 64)
      work.push_back({b.plan.blob_of_problem[p], b.plan.x_off[p], (int64_t)p * stride, s0, std::min(64, n - s0)});
  }
  list = DevList<twr::SampleWork>();
  list = upload(work);
}

// the work list of twr_batch_sample for (dt, stride), (re)built where the last call's was another (twr_batch_joints walks it too)
void sample_work_for(twr_batch& b, double dt, int64_t problem_stride) {
  if (b.swork.d && b.swork_dt == dt && b.swork_stride == problem_stride) return;
  build_sample_work(b, b.swork, problem_stride, [&](int p) {
    const int n = twr::SampleCount(b.plan.t_total[p], dt);
    if ((int64_t)n * (20 + 13 * b.n_ee) > problem_stride) throw std::runtime_error("problem_stride too small for the samples");
    return n;
  });
  b.swork_dt = dt;
  b.swork_stride = problem_stride;
}

void check_params(const twr_params& p) {   // throws: what twr_structure_create rejects before it builds anything
  if (p.polys_per_swing < 1 || p.polys_per_stance_force < 1) throw std::runtime_error("polynomials per phase must be >= 1");
  if (p.constraint_sets <= 0 || (p.constraint_sets & ~TWR_SETS_EVERY))
    throw std::runtime_error("constraint_sets must be a non-empty mask of TWR_SET_* bits");
  if ((p.constraint_sets & TWR_SET_BASE_ROM) && !std::isfinite(p.base_z_init))
    throw std::runtime_error("TWR_SET_BASE_ROM needs twr_params.base_z_init (the initial base height; "
                             "base_motion_constraint.cc:51-55 reads it from the spline)");
}

void copy_set(const twr::SetInfo& s, twr_set_info* out) {
  std::memset(out, 0, sizeof(*out));
  std::strncpy(out->name, s.name.c_str(), TWR_NAME_LEN - 1);
  out->offset = s.offset;
  out->size = s.size;
  out->nnz_offset = s.nnz_offset;
  out->nnz = s.nnz;
}

}  // namespace

extern "C" {

const char* twr_last_error(void) { return g_err.c_str(); }

int twr_model_preset(int robot, int terrain, twr_model* out) {
  if (!out) return fail(TWR_ERR_INVALID, "null output");
  try {
    twr::ModelPreset(robot, terrain, out);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_params_default(twr_params* out) {
  if (!out) return fail(TWR_ERR_INVALID, "null output");
  out->dt_dynamic = 0.1;  // parameters.cc:43-50
  out->dt_rom = 0.08;
  out->duration_base_poly = 0.1;
  out->polys_per_swing = 2;
  out->polys_per_stance_force = 3;
  out->constraint_sets = TWR_SETS_HOT_PATH;
  out->reserved_ = 0;
  out->dt_base_motion = out->duration_base_poly / 4.;  // parameters.cc:51
  out->base_z_init = std::nan("");  // must be set by callers that enable TWR_SET_BASE_ROM
  return TWR_OK;
}

int twr_gait_combo(int n_ee, int combo, double t_total, double swing_scale, twr_schedule* out) {
  if (!out) return fail(TWR_ERR_INVALID, "null output");
  try {
    if (!(t_total > 0) || !(swing_scale > 0)) throw std::runtime_error("t_total and swing_scale must be positive");
    twr::GaitCombo(n_ee, combo, t_total, swing_scale, out);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_terrain_grid_create(const double* heights, int rows, int cols, twr_terrain_grid** out) {
  if (!heights || !out || rows < 1 || cols < 1) return fail(TWR_ERR_INVALID, "bad grid");
  try {
    std::unique_ptr<twr_terrain_grid> h(new twr_terrain_grid());
    h->g = std::make_shared<twr::TerrainGrid>();
    h->g->heights.assign(heights, heights + (size_t)rows * cols);
    h->g->rows = rows;
    h->g->cols = cols;
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}
int twr_terrain_grid_map_create(const float* elevation, int size_x, int size_y, double resolution, double pos_x,
                                double pos_y, twr_terrain_grid** out) {
  if (!elevation || !out || size_x < 1 || size_y < 1 || !(resolution > 0) || !std::isfinite(pos_x) || !std::isfinite(pos_y))
    return fail(TWR_ERR_INVALID, "bad grid map");
  try {
    std::unique_ptr<twr_terrain_grid> h(new twr_terrain_grid());
    h->g = std::make_shared<twr::TerrainGrid>();
    h->g->grid_map = true;
    h->g->elevation.assign(elevation, elevation + (size_t)size_x * size_y);
    h->g->rows = size_x;
    h->g->cols = size_y;
    h->g->res = resolution;
    h->g->eps = resolution / 6.0;  // grid_height_map.h:25
    h->g->pos_x = pos_x;
    h->g->pos_y = pos_y;
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}
namespace {
// What the map-update calls check of a layer, its start index and the map centre: false with the reason in `why`.
bool layer_ok(const twr::TerrainGrid& t, const void* layer, const char* layer_name, int start_x, int start_y, double pos_x, double pos_y,
              std::string& why) {
  if (!layer) why = std::string(layer_name) + " is NULL";
  else if (reinterpret_cast<uintptr_t>(layer) & 3) why = std::string(layer_name) + " is not 4-byte aligned";
  else if (start_x < 0 || start_x >= t.rows) why = "start_x " + std::to_string(start_x) + " is outside [0, size_x = " + std::to_string(t.rows) + ")";
  else if (start_y < 0 || start_y >= t.cols) why = "start_y " + std::to_string(start_y) + " is outside [0, size_y = " + std::to_string(t.cols) + ")";
  else if (!std::isfinite(pos_x)) why = "pos_x is not finite";
  else if (!std::isfinite(pos_y)) why = "pos_y is not finite";
  else return true;
  return false;
}
}  // namespace

int twr_terrain_grid_map_update(twr_terrain_grid* g, const float* elevation, int start_x, int start_y, double pos_x, double pos_y) {
  if (!g || !g->g) return fail(TWR_ERR_INVALID, "g is NULL");
  twr::TerrainGrid& t = *g->g;
  if (!t.grid_map) return fail(TWR_ERR_INVALID, "g is not a grid_map layer (a CSV grid cannot be updated)");
  std::string why;
  if (!layer_ok(t, elevation, "elevation", start_x, start_y, pos_x, pos_y, why)) return fail(TWR_ERR_INVALID, why);
  try {
    // stored[i, j] = elevation[(i + start_x) mod size_x, (j + start_y) mod size_y], column by column as two runs; built aside
    // (`elevation` may be the handle's own data) and copied in, so that the address twr_terrain_grid_info gave out stays
    // valid: cells as they are, NaN included
    const size_t sx = (size_t)t.rows, sy = (size_t)t.cols, head = sx - (size_t)start_x;
    std::vector<float> next(sx * sy);
    for (size_t j = 0; j < sy; ++j) {
      const float* s = elevation + ((j + (size_t)start_y) % sy) * sx;
      float* d = next.data() + j * sx;
      std::memcpy(d, s + start_x, head * sizeof(float));
      std::memcpy(d + head, s, (size_t)start_x * sizeof(float));
    }
    std::memcpy(t.elevation.data(), next.data(), next.size() * sizeof(float));
    t.pos_x = pos_x;
    t.pos_y = pos_y;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}
void twr_terrain_grid_destroy(twr_terrain_grid* g) { delete g; }

int twr_structure_create(const twr_model* model, const twr_schedule* schedule, const twr_params* params,
                         twr_structure** out) {
  return twr_structure_create_with_grid(model, schedule, params, nullptr, out);
}

int twr_structure_create_with_grid(const twr_model* model, const twr_schedule* schedule, const twr_params* params,
                                   const twr_terrain_grid* grid, twr_structure** out) {
  if (!model || !schedule || !params || !out) return fail(TWR_ERR_INVALID, "null argument");
  try {
    std::unique_ptr<twr_structure> h(new twr_structure());
    if (grid) h->s.grid = grid->g;
    h->s.model = *model;
    h->s.schedule = *schedule;
    h->s.params = *params;
    check_params(*params);
    h->s.Build();
    *out = h.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

void twr_structure_destroy(twr_structure* s) { delete s; }

int twr_structure_create_many(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n,
                              int n_threads, twr_structure** out) {
  return twr_structure_create_many_with_grid(model, schedules, params, n, n_threads, nullptr, out);
}

int twr_structure_create_many_with_grid(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n,
                                        int n_threads, const twr_terrain_grid* grid, twr_structure** out) {
  if (!model || !schedules || !params || !out || n < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
  n_threads = std::max(1, std::min(n_threads, n));
  for (int i = 0; i < n; ++i) out[i] = nullptr;
  std::vector<std::string> errs(n_threads);
  std::atomic<int> next(0);
  auto worker = [&](int tid) {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      // the error string of the failing call lives in the worker's thread_local slot: carry it out
      if (twr_structure_create_with_grid(model, &schedules[i], &params[i], grid, &out[i]) != TWR_OK && errs[tid].empty())
        errs[tid] = "structure " + std::to_string(i) + ": " + twr_last_error();
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) {
    try {
      pool.emplace_back(worker, t);
    } catch (const std::exception&) {   // no more threads to be had: the ones that run share the work
      break;
    }
  }
  worker(0);
  for (auto& t : pool) t.join();
  for (const std::string& e : errs)
    if (!e.empty()) {
      for (int i = 0; i < n; ++i) {
        twr_structure_destroy(out[i]);
        out[i] = nullptr;
      }
      return fail(TWR_ERR_INVALID, e);
    }
  return TWR_OK;
}

// Bytes one callback of every candidate moves, 8 (n + m + nnz): the weight SURVEY 8e shards a sweep by.  Only the
// variable layout, the time tables and the CSR pattern are built (no device tables), on n_threads host threads.
int twr_candidate_bytes(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n, int n_threads,
                        int64_t* bytes) {
  if (!model || !schedules || !params || !bytes || n < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  if (n_threads <= 0) n_threads = (int)std::thread::hardware_concurrency();
  n_threads = std::max(1, std::min(n_threads, n));
  std::vector<std::string> errs(n_threads);
  std::atomic<int> next(0);
  auto worker = [&](int tid) {
    for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) {
      try {
        twr::Structure s;
        s.model = *model;
        s.schedule = schedules[i];
        s.params = params[i];
        check_params(params[i]);
        s.BuildSizes();
        bytes[i] = 8 * ((int64_t)s.n_vars + s.n_rows + s.nnz);
      } catch (const std::exception& e) {
        if (errs[tid].empty()) errs[tid] = "candidate " + std::to_string(i) + ": " + e.what();
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) {
    try {
      pool.emplace_back(worker, t);
    } catch (const std::exception&) {
      break;
    }
  }
  worker(0);
  for (auto& t : pool) t.join();
  for (const std::string& e : errs)
    if (!e.empty()) return fail(TWR_ERR_INVALID, e);
  return TWR_OK;
}

// Contiguous shards balanced by the prefix sum of the weights: rank r owns [bounds[r], bounds[r + 1]).  Never an empty
// shard; TWR_ERR_INVALID (on every rank alike: the arguments are the same everywhere) when there are fewer candidates
// than ranks.  The boundary is the prefix whose sum is closest to r / world of the total (ties: the earlier one).
int twr_shard_bounds(const double* weights, int n, int world, int32_t* bounds) {
  if (!weights || !bounds || n < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  if (world < 1 || world > n)
    return fail(TWR_ERR_INVALID, "cannot shard " + std::to_string(n) + " candidates over " + std::to_string(world) +
                                     " ranks: every rank needs at least one");
  std::vector<double> csum(n + 1, 0.0);
  for (int i = 0; i < n; ++i) {
    if (!(weights[i] >= 0.0)) return fail(TWR_ERR_INVALID, "negative or NaN weight");
    csum[i + 1] = csum[i] + weights[i];
  }
  const double total = csum[n];
  bounds[0] = 0;
  for (int r = 1; r < world; ++r) {
    const double target = total * r / world;
    int i = (int)(std::lower_bound(csum.begin(), csum.end(), target) - csum.begin());   // first prefix >= target
    if (i > 0 && std::fabs(csum[i - 1] - target) <= std::fabs(csum[std::min(i, n)] - target)) --i;
    bounds[r] = std::min(std::max(i, bounds[r - 1] + 1), n - (world - r));
  }
  bounds[world] = n;
  return TWR_OK;
}

int twr_terrain_grid_info(const twr_terrain_grid* g, int32_t* kind, int32_t* rows_or_size_x, int32_t* cols_or_size_y,
                          double* resolution, double* pos_x, double* pos_y, const void** data) {
  if (!g || !g->g) return fail(TWR_ERR_INVALID, "null grid");
  const twr::TerrainGrid& t = *g->g;
  if (kind) *kind = t.grid_map ? 1 : 0;
  if (rows_or_size_x) *rows_or_size_x = t.rows;
  if (cols_or_size_y) *cols_or_size_y = t.cols;
  if (resolution) *resolution = t.res;
  if (pos_x) *pos_x = t.pos_x;
  if (pos_y) *pos_y = t.pos_y;
  if (data) *data = t.grid_map ? static_cast<const void*>(t.elevation.data()) : static_cast<const void*>(t.heights.data());
  return TWR_OK;
}

int twr_structure_sizes(const twr_structure* s, twr_sizes* out) {
  if (!s || !out) return fail(TWR_ERR_INVALID, "null argument");
  out->n_vars = s->s.n_vars;
  out->n_rows = s->s.n_rows;
  out->nnz = s->s.nnz;
  out->n_var_sets = (int)s->s.var_sets.size();
  out->n_con_sets = (int)s->s.con_sets.size();
  out->k_dynamic = (int)s->s.grid_dyn.size();
  out->k_rom = (int)s->s.grid_rom.size();
  return TWR_OK;
}

int twr_structure_values_items(const twr_structure* s, int32_t* n_dynamic_items, int32_t* n_rom_items, int32_t* dynamic_takes_rom,
                               int32_t* items) {
  if (!s || !n_dynamic_items || !n_rom_items || !dynamic_takes_rom) return fail(TWR_ERR_INVALID, "null argument");
  const bool on = s->s.off_flat_polys != 0;
  *n_dynamic_items = on ? (int32_t)s->s.flat_items_dyn.size() : 0;
  *n_rom_items = on ? (int32_t)s->s.flat_items_rom.size() : 0;
  *dynamic_takes_rom = on && s->s.flat_with_rom ? 1 : 0;
  if (items && on) {
    int32_t* o = items;
    for (const auto* list : {&s->s.flat_items_dyn, &s->s.flat_items_rom})
      for (const auto& it : *list) {
        int widest = 0;
        for (int sp = 0; sp < 8; ++sp) widest = std::max(widest, (int)((it.count >> (8 * sp)) & 0xFFu));
        *o++ = it.k0;
        *o++ = it.cnt;
        *o++ = it.gather ? 0 : widest;
      }
  }
  return TWR_OK;
}

int twr_structure_var_set(const twr_structure* s, int i, twr_set_info* out) {
  if (!s || !out || i < 0 || i >= (int)s->s.var_sets.size()) return fail(TWR_ERR_INVALID, "bad variable set index");
  copy_set(s->s.var_sets[i], out);
  return TWR_OK;
}

int twr_structure_con_set(const twr_structure* s, int i, twr_set_info* out) {
  if (!s || !out || i < 0 || i >= (int)s->s.con_sets.size()) return fail(TWR_ERR_INVALID, "bad constraint set index");
  copy_set(s->s.con_sets[i], out);
  return TWR_OK;
}

const int32_t* twr_structure_row_ptr(const twr_structure* s) { return s ? s->s.row_ptr.data() : nullptr; }
const int32_t* twr_structure_col_idx(const twr_structure* s) { return s ? s->s.col_idx.data() : nullptr; }

int twr_structure_bounds(const twr_structure* s, double* lower, double* upper) {
  if (!s || !lower || !upper) return fail(TWR_ERR_INVALID, "null argument");
  std::memcpy(lower, s->s.lower.data(), s->s.lower.size() * sizeof(double));
  std::memcpy(upper, s->s.upper.data(), s->s.upper.size() * sizeof(double));
  return TWR_OK;
}

int twr_structure_initial_guess(const twr_structure* s, const double init_base_lin[3], const double init_base_ang[3],
                                const double final_base_lin[3], const double final_base_ang[3],
                                const double* init_ee_pos, double* x_out) {
  if (!s || !init_base_lin || !init_base_ang || !final_base_lin || !final_base_ang || !init_ee_pos || !x_out)
    return fail(TWR_ERR_INVALID, "null argument");
  try {
    s->s.InitialGuess(init_base_lin, init_base_ang, final_base_lin, final_base_ang, init_ee_pos, x_out);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_structure_variable_bounds(const twr_structure* s, const double init_base[12], const double final_base[12],
                                  const double* init_ee_pos, double* lower, double* upper) {
  if (!s || !init_base || !final_base || !init_ee_pos || !lower || !upper) return fail(TWR_ERR_INVALID, "null argument");
  try {
    s->s.VariableBounds(init_base, final_base, init_ee_pos, lower, upper);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_structure_start_host(const twr_structure* s, const double request[TWR_START_REC], double* x, double* lower, double* upper) {
  if (!s || !request) return fail(TWR_ERR_INVALID, "null argument");
  try {
    s->s.StartHost(request, x, lower, upper);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_batch_create(const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem,
                     int n_problems, int device, twr_batch** out) {
  if (!structs || !struct_of_problem || !out || n_structs < 1 || n_problems < 1)
    return fail(TWR_ERR_INVALID, "bad arguments");
  std::unique_ptr<twr_batch> b(new twr_batch());
  try {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0)
      return fail(TWR_ERR_NO_DEVICE, "no HIP device visible: towr_amd has no CPU fallback");
    if (device < 0 || device >= n_dev) return fail(TWR_ERR_INVALID, "device ordinal out of range");
    DeviceScope on(device);
    TWR_HIP(on.status);
    const std::vector<const twr::Structure*> sp = structure_ptrs(structs, n_structs);
    for (const twr::Structure* s : sp)
      if (s->n_ee != sp[0]->n_ee) throw std::runtime_error("all structures of a batch must share n_ee");
    b->device = device;
    b->n_problems = n_problems;
    b->n_ee = sp[0]->n_ee;
    for (const twr::Structure* s : sp) b->start_tables.push_back(s->start_table);   // (twr_batch_reserve_start)
    b->struct_of_problem.assign(struct_of_problem, struct_of_problem + n_problems);
    // the arena; every distinct gridded terrain is uploaded once and its address patched into the headers that use it
    const std::vector<size_t> blob_off = twr::BlobOffsets(sp);
    b->arena = dev_alloc<void>(blob_off[n_structs]);
    std::vector<char> host_arena(blob_off[n_structs], 0);
    std::vector<uint64_t> blob_at(n_structs);
    std::vector<const twr::TerrainGrid*> host_grids;
    std::vector<std::vector<uint64_t>> hdr_of_grid;   // per distinct `Grid` map: where its readers keep the map centre
    for (int i = 0; i < n_structs; ++i) {
      blob_at[i] = reinterpret_cast<uint64_t>(b->arena.get()) + blob_off[i];
      std::memcpy(host_arena.data() + blob_off[i], sp[i]->blob.data(), sp[i]->blob.size());
      const twr::TerrainGrid* tg = sp[i]->grid.get();
      if (!tg) continue;
      const size_t q = std::find(host_grids.begin(), host_grids.end(), tg) - host_grids.begin();
      if (q == host_grids.size()) {
        const void* src = tg->grid_map ? (const void*)tg->elevation.data() : (const void*)tg->heights.data();
        const size_t bytes = tg->grid_map ? tg->elevation.size() * sizeof(float) : tg->heights.size() * sizeof(double);
        b->grids.push_back(dev_alloc<void>(bytes));
        TWR_HIP(hipMemcpy(b->grids[q].get(), src, bytes, hipMemcpyHostToDevice));
        host_grids.push_back(tg);
        b->grid_of.push_back(sp[i]->grid);
        hdr_of_grid.emplace_back();
      }
      twr::DevStruct* H = reinterpret_cast<twr::DevStruct*>(host_arena.data() + blob_off[i]);
      H->grid_ptr = reinterpret_cast<uint64_t>(b->grids[q].get());
      if (tg->grid_map) {
        // the centre as the handle has it now (twr_terrain_grid_map_update may have moved it since the structure was built)
        H->grid_px = tg->pos_x;
        H->grid_py = tg->pos_y;
        hdr_of_grid[q].push_back(blob_off[i] + offsetof(twr::DevStruct, grid_px));
      }
    }
    static_assert(offsetof(twr::DevStruct, grid_py) == offsetof(twr::DevStruct, grid_px) + sizeof(double), "grid_py follows grid_px");
    {
      std::vector<uint64_t> all;
      b->grid_hdr_first.assign(1, 0);
      for (const std::vector<uint64_t>& h : hdr_of_grid) {
        all.insert(all.end(), h.begin(), h.end());
        b->grid_hdr_first.push_back((int32_t)all.size());
      }
      b->grid_hdr = upload_nonempty(all);
    }
    TWR_HIP(hipMemcpy(b->arena.get(), host_arena.data(), host_arena.size(), hipMemcpyHostToDevice));
    b->table_bytes = (int64_t)host_arena.size();
    hipDeviceProp_t prop;
    TWR_HIP(hipGetDeviceProperties(&prop, device));
    b->n_cu = prop.multiProcessorCount;
    // (a compute partition -- CPX -- shows up as a device with a fraction of the chip's CUs: its share of the cache follows)
    b->plan = twr::PlanBatch(sp, std::vector<int32_t>(struct_of_problem, struct_of_problem + n_problems), blob_at, b->n_cu,
                             twr::MemorySideCacheBytes(prop.gcnArchName, prop.l2CacheSize, 1), twr::kForceChunk);
#ifdef TWR_TUNING_KNOBS   // (include/towr_amd.h, "Tuning knobs")
    if (const char* e = getenv("TWR_STREAM_NT")) b->plan.stream_nt = atoi(e) != 0;
#endif
    const twr::BatchPlan::Lists& L = b->plan.lists;
    b->dyn = upload(L.dyn);
    b->rom = upload(L.rom);
    b->node = upload(L.node);
    b->node.n = n_problems;
    b->flat = upload_nonempty(L.flat);
    for (int f = 0; f < 4; ++f) b->fam[f] = upload_nonempty(L.fam[f]);
    b->goff = upload(b->plan.g_off);
    b->joff = upload(b->plan.j_off);
    b->dump = dev_zeros<double>(twr::kDynDump);
    b->best = dev_zeros<double>(2 * (size_t)twr::best_max_blocks() + 1);
    if (b->plan.score_fused) {
      b->score_blob = upload_nonempty(L.score_blob);
      b->score_first = upload(L.score_first);
      b->score_slot = upload(L.score_slot);
      b->score_slab = dev_alloc<double>(sizeof(double) * twr::kScorePartial * (size_t)b->plan.score_slab);
    }
    b->status = dev_zeros<int32_t>(n_problems);
    if (!L.ploc.empty()) {
      b->precs = dev_alloc<void>(b->plan.records_bytes);
      b->plan.PlaceRecords(reinterpret_cast<uint64_t>(b->precs.get()));
      b->ploc = upload(L.ploc);
    }
    b->prom = upload_nonempty(L.prom);
    b->pdyn = upload_nonempty(L.pdyn);
    b->plan.lists = twr::BatchPlan::Lists();   // (on the device now)
    TWR_HIP(twr::prepare_phase_kernels(b->plan.pdyn_img_cap, b->plan.prom_img_cap));
    *out = b.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    twr_batch_destroy(b.release());
    return fail(TWR_ERR_HIP, e.what());
  }
}

void twr_batch_destroy(twr_batch* b) {
  if (!b) return;
  DeviceScope on(b->device);   // (the handle's owners free its device memory, stream and events)
  delete b;
}

int twr_batch_num_problems(const twr_batch* b) { return b ? b->n_problems : 0; }

int twr_batch_streaming_stores(const twr_batch* b) { return b && b->plan.stream_nt ? 1 : 0; }

int twr_batch_dyn_uniform_kinds(const twr_batch* b) { return b ? b->plan.dyn_uniform.s : 0; }

int twr_batch_table_bytes(const twr_batch* b, int64_t* resident, int64_t* dyn_layout, int64_t* dyn_layout_distinct) {
  if (!b) return fail(TWR_ERR_INVALID, "null batch");
  if (resident) *resident = b->table_bytes;
  if (dyn_layout) *dyn_layout = b->plan.dyn_layout_bytes;
  if (dyn_layout_distinct) *dyn_layout_distinct = b->plan.dyn_layout_distinct_bytes;
  return TWR_OK;
}

int twr_batch_layout(const twr_batch* b, int64_t* x_off, int64_t* g_off, int64_t* jac_off) {
  if (!b) return fail(TWR_ERR_INVALID, "null batch");
  size_t bytes = (b->n_problems + 1) * sizeof(int64_t);
  if (x_off) std::memcpy(x_off, b->plan.x_off.data(), bytes);
  if (g_off) std::memcpy(g_off, b->plan.g_off.data(), bytes);
  if (jac_off) std::memcpy(jac_off, b->plan.j_off.data(), bytes);
  return TWR_OK;
}

namespace {
// The batch's copy of the map behind handle g: its index in twr_batch::grids, or -1 with the reason in `why`.
int held_grid_map(const twr_batch* b, const twr_terrain_grid* g, std::string& why) {
  if (!b) return why = "b is NULL", -1;
  if (!g || !g->g) return why = "g is NULL", -1;
  if (!g->g->grid_map) return why = "g is not a grid_map layer (a CSV grid cannot be updated)", -1;
  for (size_t q = 0; q < b->grid_of.size(); ++q)
    if (b->grid_of[q].get() == g->g.get()) return (int)q;
  return why = "g is not a map of this batch (no structure of the batch was created with it)", -1;
}
// The one launch of both update calls: layer `src` on the device (start index (start_x, start_y)) into the batch's map q
int update_held_map(twr_batch* b, int q, const float* d_src, int start_x, int start_y, double pos_x, double pos_y, hipStream_t stream) {
  const twr::TerrainGrid& t = *b->grid_of[q];
  const int first = b->grid_hdr_first[q], n_hdr = b->grid_hdr_first[q + 1] - first;
  return launched(twr::launch_grid_map_update(d_src, static_cast<float*>(b->grids[q].get()), t.rows, t.cols, start_x, start_y, pos_x, pos_y,
                                              b->arena.get(), n_hdr ? b->grid_hdr.d.get() + first : nullptr, n_hdr, stream));
}
}  // namespace

int twr_batch_grid_map_sync(twr_batch* b, const twr_terrain_grid* g, void* hip_stream) {
  std::string why;
  const int q = held_grid_map(b, g, why);
  if (q < 0) return fail(TWR_ERR_INVALID, why);
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const twr::TerrainGrid& t = *g->g;
    if (!b->grid_stage) {   // one staging buffer for every map of the batch
      size_t cells = 0;
      for (const auto& m : b->grid_of)
        if (m->grid_map) cells = std::max(cells, m->elevation.size());
      b->grid_stage = dev_alloc<float>(cells * sizeof(float));
    }
    // host layer -> staging (ordered behind what the stream holds; the map an evaluation in front of it reads is not touched),
    // staging -> the map and the headers: the same launch as twr_batch_grid_map_update_device, with start index (0,0)
    TWR_HIP(hipMemcpyAsync(b->grid_stage.get(), t.elevation.data(), t.elevation.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    return update_held_map(b, q, b->grid_stage.get(), 0, 0, t.pos_x, t.pos_y, stream);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_grid_map_update_device(twr_batch* b, const twr_terrain_grid* g, const float* d_elevation, int start_x, int start_y,
                                     double pos_x, double pos_y, void* hip_stream) {
  std::string why;
  const int q = held_grid_map(b, g, why);
  if (q < 0) return fail(TWR_ERR_INVALID, why);
  if (!layer_ok(*g->g, d_elevation, "d_elevation", start_x, start_y, pos_x, pos_y, why)) return fail(TWR_ERR_INVALID, why);
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  return update_held_map(b, q, d_elevation, start_x, start_y, pos_x, pos_y, static_cast<hipStream_t>(hip_stream));
}

namespace {
// Plans and uploads what twr_batch_start reads (once; under the caller's DeviceScope).  Throws.
void reserve_start(twr_batch& b) {
  if (b.start_work.d) return;
  std::vector<const std::vector<char>*> tables;
  for (const auto& t : b.start_tables) tables.push_back(t.get());
  twr::StartPlan plan = twr::PlanStart(tables, b.struct_of_problem, b.plan.x_off, b.plan.blob_of_problem);
  DevPtr<char> dev = dev_alloc<char>(plan.tables.size());
  TWR_HIP(hipMemcpy(dev.get(), plan.tables.data(), plan.tables.size(), hipMemcpyHostToDevice));
  plan.Place(reinterpret_cast<uint64_t>(dev.get()));
  DevList<twr::StartWork> work = upload(plan.work);
  b.start_dev = std::move(dev);
  b.start_work = std::move(work);
}
}  // namespace

int twr_batch_reserve_start(twr_batch* b) {
  if (!b) return fail(TWR_ERR_INVALID, "b is NULL");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    reserve_start(*b);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_start(twr_batch* b, const double* d_request, int64_t request_stride, double* d_x, double* d_xlo, double* d_xup,
                    void* hip_stream) {
  if (!b) return fail(TWR_ERR_INVALID, "b is NULL");
  if (!d_request) return fail(TWR_ERR_INVALID, "d_request is NULL");
  if (!d_x && !d_xlo && !d_xup) return fail(TWR_ERR_INVALID, "d_x, d_xlo and d_xup are all NULL");
  if (request_stride != 0 && request_stride < TWR_START_REC)
    return fail(TWR_ERR_INVALID, "request_stride must be 0 (one record for all problems) or >= TWR_START_REC");
  if (misaligned({d_request})) return fail(TWR_ERR_INVALID, "d_request is not 8-byte aligned");
  if (misaligned({d_x})) return fail(TWR_ERR_INVALID, "d_x is not 8-byte aligned");
  if (misaligned({d_xlo})) return fail(TWR_ERR_INVALID, "d_xlo is not 8-byte aligned");
  if (misaligned({d_xup})) return fail(TWR_ERR_INVALID, "d_xup is not 8-byte aligned");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    reserve_start(*b);   // (a no-op after twr_batch_reserve_start; otherwise the first call allocates and uploads)
    return launched(twr::launch_start(b->start_work.d.get(), b->start_work.n, d_request, request_stride, d_x, d_xlo, d_xup,
                                      static_cast<hipStream_t>(hip_stream)));
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

// Tuning knobs of the launches (include/towr_amd.h): a TUNING=1 build reads them on every evaluation; the default build reads
// nothing and keeps the defaults of twr::LaunchTuning.
static twr::LaunchTuning tuning_knobs() {
  twr::LaunchTuning t;
#ifdef TWR_TUNING_KNOBS
  const auto knob = [](const char* name, int& v) {
    const char* e = getenv(name);
    if (e && atoi(e) > 0) v = atoi(e);
  };
  knob("TWR_DYN_BPC", t.dyn_bpc);
  knob("TWR_ROM_BPC", t.rom_bpc);
  knob("TWR_NODE_BPC", t.node_bpc);
  knob("TWR_PDYN_BPC", t.pdyn_bpc);
  knob("TWR_PROM_BPC", t.prom_bpc);
  knob("TWR_FUSED_MAX_ROM", t.fused_max_rom);
  knob("TWR_FUSED_SPLIT", t.fused_split);
  knob("TWR_FUSED_GROM", t.fused_grom);
  knob("TWR_FUSED_GDYN", t.fused_gdyn);
#endif
  return t;
}

// The shape of a call on this batch (batch_plan.h MakeEvalShape): what twr_batch_eval, the scoring entry points and
// twr_batch_eval_plan all plan from.
static twr::EvalShape eval_shape(const twr_batch* b, int flags, bool events) {
  twr::EvalCounts c;
  c.dyn = b->dyn.n, c.rom = b->rom.n, c.node = b->node.n, c.flat = b->flat.n, c.pdyn = b->pdyn.n, c.ploc = b->ploc.n, c.prom = b->prom.n;
  for (int f = 0; f < 4; ++f) c.fam[f] = b->fam[f].n;
  return twr::MakeEvalShape(b->plan, c, b->n_cu, flags, events, tuning_knobs());
}

int twr_batch_eval_plan(const twr_batch* b, int request, int flags, int events, twr_launch_step* steps, int max_steps, int* n_steps) {
  if (!b || !n_steps || (max_steps > 0 && !steps)) return fail(TWR_ERR_INVALID, "null argument");
  if (request != TWR_PLAN_EVAL && request != TWR_PLAN_SCORES && request != TWR_PLAN_SCORE_BEST) return fail(TWR_ERR_INVALID, "unknown request");
  if (request == TWR_PLAN_EVAL && (flags & TWR_EVAL_BOTH) == 0) return fail(TWR_ERR_INVALID, "flags select nothing");
  const int f = request == TWR_PLAN_EVAL ? flags & TWR_EVAL_BOTH : twr::kEvalScores | (request == TWR_PLAN_SCORE_BEST ? twr::kEvalBest : 0);
  const twr::EvalPlan plan = twr::PlanEval(eval_shape(b, f, events != 0));
  int n = 0;
  for (int i = 0; i < plan.n; ++i) {
    const twr::LaunchStep& p = plan.step[i];
    if (p.kernel == twr::Launch::kEvent) continue;
    if (n < max_steps) {
      twr_launch_step& o = steps[n];
      std::memset(&o, 0, sizeof(o));
      std::strncpy(o.kernel, twr::KernelName(p), sizeof(o.kernel) - 1);
      std::strncpy(o.instantiation, twr::InstantiationName(p).c_str(), sizeof(o.instantiation) - 1);
      const bool has_store = p.kernel == twr::Launch::kDyn || p.kernel == twr::Launch::kRom || p.kernel == twr::Launch::kFused ||
                             p.kernel == twr::Launch::kDynPhase || p.kernel == twr::Launch::kRomPhase || p.kernel == twr::Launch::kChunk;
      if (has_store) std::strncpy(o.store, twr::StoreName(p.store), sizeof(o.store) - 1);
      o.nit = p.nit;
      o.xc = p.xc;
      o.grid = p.grid;
      o.block = p.block;
      o.lds_bytes = p.lds;
      o.uniform_kinds = p.uni.s;
    }
    ++n;
  }
  *n_steps = n;
  return TWR_OK;
}

int twr_batch_eval(twr_batch* b, const double* d_x, double* d_g, double* d_jac, int flags, void* hip_stream) {
  if (!b || !d_x) return fail(TWR_ERR_INVALID, "null argument");
  if ((flags & TWR_EVAL_BOTH) == 0) return fail(TWR_ERR_INVALID, "flags select nothing");
  if (((flags & TWR_EVAL_VALUES) && !d_g) || ((flags & TWR_EVAL_JACOBIAN) && !d_jac))
    return fail(TWR_ERR_INVALID, "missing output buffer");
  // One process may drive several devices: the launch needs the batch's device current.  The calling thread's current
  // device is restored afterwards and its error state is left alone (the launch's own status is what is returned).
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipEvent_t* ev = nullptr;
  if (b->prof_count < b->prof_capacity) ev = b->prof_events.ev.data() + 4 * b->prof_count++;
  hipStream_t stream = static_cast<hipStream_t>(hip_stream);
  const twr::EvalShape s = eval_shape(b, flags & TWR_EVAL_BOTH, ev != nullptr);
  const twr::EvalBuffers buf{b->dyn.d.get(), b->rom.d.get(), b->node.d.get(), b->flat.d.get(),
                             {b->fam[0].d.get(), b->fam[1].d.get(), b->fam[2].d.get(), b->fam[3].d.get()},
                             b->pdyn.d.get(), b->ploc.d.get(), b->prom.d.get(), d_x, d_g, d_jac, b->dump.get()};
  hipError_t e = twr::launch_eval(s, buf, stream, ev);
  if (e != hipSuccess) return launched(e);
  if (flags & TWR_EVAL_CHECK) {
    e = twr::launch_check(b->n_problems, b->goff.d.get(), b->joff.d.get(), d_g, d_jac, b->status.get(), flags & TWR_EVAL_BOTH, stream);
    if (e != hipSuccess) return fail(TWR_ERR_HIP, std::string("check kernel launch: ") + hipGetErrorString(e));
  }
  return TWR_OK;
}

int twr_batch_status(twr_batch* b, int32_t* h_status, void* hip_stream) {
  if (!b || !h_status) return fail(TWR_ERR_INVALID, "null argument");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    TWR_HIP(hipMemcpyAsync(h_status, b->status.get(), sizeof(int32_t) * (size_t)b->n_problems, hipMemcpyDeviceToHost, stream));
    TWR_HIP(hipStreamSynchronize(stream));
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_profile_begin(twr_batch* b, int max_evals) {
  if (!b || max_evals < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    b->prof_events.clear();
    b->prof_events.ev.assign(4 * (size_t)max_evals, nullptr);
    for (auto& e : b->prof_events.ev) TWR_HIP(hipEventCreate(&e));
    b->prof_capacity = max_evals;
    b->prof_count = 0;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_profile_end(twr_batch* b, double avg_ms[3], int* n_evals) {
  if (!b || !avg_ms) return fail(TWR_ERR_INVALID, "null argument");
  try {
    DeviceScope on(b->device);   // (events belong to the batch's device, like in _begin)
    TWR_HIP(on.status);
    const int n = b->prof_count;
    avg_ms[0] = avg_ms[1] = avg_ms[2] = 0.0;
    if (n > 0) {
      TWR_HIP(hipEventSynchronize(b->prof_events.ev[4 * (size_t)n - 1]));
      for (int i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
          float ms = 0.f;
          TWR_HIP(hipEventElapsedTime(&ms, b->prof_events.ev[4 * (size_t)i + k], b->prof_events.ev[4 * (size_t)i + k + 1]));
          avg_ms[k] += ms / n;
        }
    }
    if (n_evals) *n_evals = n;
    b->prof_capacity = 0;
    b->prof_count = 0;
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_eval_host(twr_batch* b, const double* h_x, double* h_g, double* h_jac, int flags) {
  if (!b || !h_x) return fail(TWR_ERR_INVALID, "null argument");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    const size_t nx = b->plan.x_off.back(), ng = b->plan.g_off.back(), nj = b->plan.j_off.back();
    // device staging buffers, each on first need (the zero-copy branch below needs none of them: a single-problem adapter
    // batch that only ever hands over its own page-locked buffers allocates nothing in HBM here)
    auto need_x = [&]() {
      if (!b->d_x) b->d_x = dev_alloc<double>(nx * sizeof(double));
    };
    auto need_out = [&]() {
      if (!b->d_g) b->d_g = dev_alloc<double>(ng * sizeof(double));
      if (!b->d_j) b->d_j = dev_alloc<double>(nj * sizeof(double));
    };
    if (!b->host_stream) {
      hipStream_t s = nullptr;
      TWR_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      b->host_stream.reset(s);
    }
    hipStream_t hs = b->host_stream.get();
    // one stream-ordered chain on the batch's own stream and a single synchronisation (with page-locked buffers the copies are DMA)
#ifdef TWR_TUNING_KNOBS   // (include/towr_amd.h, "Tuning knobs")
    static const bool zero_copy = [] { const char* e = getenv("TWR_HOST_ZERO_COPY"); return !e || atoi(e) != 0; }();
    static const bool zero_copy_x = [] { const char* e = getenv("TWR_HOST_ZERO_COPY_X"); return !e || atoi(e) != 0; }();
#else
    const bool zero_copy = true, zero_copy_x = true;
#endif
    const bool zc = zero_copy && b->p_g && h_g == b->p_g.get() && h_jac == b->p_j.get() && nj * sizeof(double) <= (size_t)(32u << 20);
    const double* dx = nullptr;
    if (zc && zero_copy_x && h_x == b->p_x.get()) {   // x too: the kernels gather it straight from the page-locked buffer
      TWR_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(const_cast<double**>(&dx)), b->p_x.get(), 0));
    } else {
      need_x();
      dx = b->d_x.get();
      TWR_HIP(hipMemcpyAsync(b->d_x.get(), h_x, nx * sizeof(double), hipMemcpyHostToDevice, hs));
    }
    if (zc) {
      // The batch's own page-locked buffers, small batch (the single-problem callback of the ifopt adapter): the
      // kernels store g and the Jacobian values straight into host memory over PCIe -- coalesced 16-byte stores,
      // each value written once -- instead of HBM plus two device-to-host copies.
      double *dg = nullptr, *dj = nullptr;
      TWR_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dg), b->p_g.get(), 0));
      TWR_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dj), b->p_j.get(), 0));
      int rc0 = twr_batch_eval(b, dx, dg, dj, flags, hs);
      if (rc0 != TWR_OK) return rc0;
      TWR_HIP(hipStreamSynchronize(hs));
      return TWR_OK;
    }
    need_out();
    int rc = twr_batch_eval(b, dx, b->d_g.get(), b->d_j.get(), flags, hs);
    if (rc != TWR_OK) return rc;
    if ((flags & TWR_EVAL_VALUES) && h_g)
      TWR_HIP(hipMemcpyAsync(h_g, b->d_g.get(), ng * sizeof(double), hipMemcpyDeviceToHost, hs));
    if ((flags & TWR_EVAL_JACOBIAN) && h_jac)
      TWR_HIP(hipMemcpyAsync(h_jac, b->d_j.get(), nj * sizeof(double), hipMemcpyDeviceToHost, hs));
    TWR_HIP(hipStreamSynchronize(hs));
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_structure_sample_count(const twr_structure* s, double dt, int32_t* n_samples) {
  if (!s || !n_samples) return fail(TWR_ERR_INVALID, "null argument");
  try {
    *n_samples = s->s.SampleCount(dt);
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
}

int twr_batch_sample(twr_batch* b, const double* d_x, double dt, double* d_out, int64_t problem_stride, void* hip_stream) {
  if (!b || !d_x || !d_out) return fail(TWR_ERR_INVALID, "null argument");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    sample_work_for(*b, dt, problem_stride);
    hipError_t e = twr::launch_sample(b->swork.d.get(), b->swork.n, d_x, d_out, dt, nullptr, static_cast<hipStream_t>(hip_stream));
    return launched(e);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_initial_guess(twr_batch* b, const double* d_x, const double* d_times, int32_t n_times, double* d_out,
                            int64_t problem_stride, void* hip_stream) {
  if (!b || !d_x || !d_times || !d_out || n_times < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  if ((int64_t)n_times * 49 > problem_stride) return fail(TWR_ERR_INVALID, "problem_stride too small for the records");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    if (!b->gwork.d || b->gwork_times != n_times || b->gwork_stride != problem_stride) {
      build_sample_work(*b, b->gwork, problem_stride, [&](int) { return (int)n_times; });
      b->gwork_times = n_times;
      b->gwork_stride = problem_stride;
    }
    hipError_t e = twr::launch_sample(b->gwork.d.get(), b->gwork.n, d_x, d_out, 0.0, d_times, static_cast<hipStream_t>(hip_stream));
    return launched(e);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_planes_create(const double* regions, const double* boundary_xy, const int32_t* boundary_start, int32_t n_regions,
                      int device, twr_planes** out) {
  if (!out || n_regions < 0 || (n_regions > 0 && (!regions || !boundary_start))) return fail(TWR_ERR_INVALID, "bad arguments");
  std::unique_ptr<twr_planes> pl;
  try {   // argument errors
    pl = std::make_unique<twr_planes>();
    pl->device = device;
    pl->start.assign(1, 0);
    for (int r = 0; r < n_regions; ++r) {
      if (boundary_start[r + 1] < boundary_start[r] || boundary_start[0] != 0) throw std::runtime_error("boundary_start must ascend from 0");
      // (boost::geometry::distance throws on an empty geometry; a region without boundary points cannot be the nearest)
      if (boundary_start[r + 1] == boundary_start[r]) throw std::runtime_error("planar region " + std::to_string(r) + " has no boundary points");
      pl->start.push_back(boundary_start[r + 1]);
    }
    const int n_pts = pl->start.back();
    if (n_pts > 0 && !boundary_xy) throw std::runtime_error("boundary_xy is null");
    pl->world_xy.resize(2 * (size_t)n_pts);
    for (int r = 0; r < n_regions; ++r) {   // PlanarRegionsToPolygons: tf::Matrix3x3(q) * (x, y, 0) + position
      const double* P = regions + 7 * r;
      const double x = P[3], y = P[4], z = P[5], w = P[6];
      const double d = x * x + y * y + z * z + w * w;
      if (!(d > 0)) throw std::runtime_error("zero orientation quaternion");
      const double s2 = 2.0 / d, xs = x * s2, ys = y * s2, zs = z * s2, wz = w * zs, xx = x * xs, xy = x * ys, yy = y * ys, zz = z * zs;
      const double R00 = 1.0 - (yy + zz), R01 = xy - wz, R10 = xy + wz, R11 = 1.0 - (xx + zz);
      for (int i = pl->start[r]; i < pl->start[r + 1]; ++i) {
        const double lx = boundary_xy[2 * i], ly = boundary_xy[2 * i + 1];
        pl->world_xy[2 * i] = (R00 * lx + R01 * ly + 0.0) + P[0];
        pl->world_xy[2 * i + 1] = (R10 * lx + R11 * ly + 0.0) + P[1];
      }
    }
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  try {   // device errors
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) return fail(TWR_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n_dev) return fail(TWR_ERR_INVALID, "device ordinal out of range");
    DeviceScope on(device);
    TWR_HIP(on.status);
    const int n_pts = pl->start.back();
    pl->d_xy = dev_alloc<double>(std::max<size_t>(16, pl->world_xy.size() * sizeof(double)));
    pl->d_start = dev_alloc<int32_t>(pl->start.size() * sizeof(int32_t));
    if (n_pts > 0) TWR_HIP(hipMemcpy(pl->d_xy.get(), pl->world_xy.data(), pl->world_xy.size() * sizeof(double), hipMemcpyHostToDevice));
    TWR_HIP(hipMemcpy(pl->d_start.get(), pl->start.data(), pl->start.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    *out = pl.release();
    return TWR_OK;
  } catch (const std::exception& e) {
    twr_planes_destroy(pl.release());
    return fail(TWR_ERR_HIP, e.what());
  }
}

void twr_planes_destroy(twr_planes* planes) {
  if (!planes) return;
  DeviceScope on(planes->device);
  delete planes;
}

int twr_planes_world_xy(const twr_planes* planes, double* world_xy) {
  if (!planes || !world_xy) return fail(TWR_ERR_INVALID, "null argument");
  std::memcpy(world_xy, planes->world_xy.data(), planes->world_xy.size() * sizeof(double));
  return TWR_OK;
}

int twr_batch_contact_planes(twr_batch* b, const twr_planes* planes, const double* d_plan, const int32_t* d_counts,
                             int32_t max_steps, int32_t* d_plane_index, void* hip_stream) {
  if (!b || !planes || !d_plan || !d_counts || !d_plane_index || max_steps < 1) return fail(TWR_ERR_INVALID, "bad arguments");
  if (planes->device != b->device) return fail(TWR_ERR_INVALID, "planes and batch live on different devices");
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipError_t e = twr::launch_planes(d_plan, d_counts, planes->d_xy.get(), planes->d_start.get(), (int)planes->start.size() - 1, b->n_problems,
                                    max_steps, b->n_ee, d_plane_index, static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_batch_score(twr_batch* b, const double* d_g, double* d_scores, void* hip_stream) {
  if (!b || !d_g || !d_scores) return fail(TWR_ERR_INVALID, "null argument");
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipError_t e = twr::launch_score(b->node.d.get(), b->n_problems, d_g, d_scores, static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_batch_score_best(twr_batch* b, const double* d_g, double* d_scores, uint32_t families, int64_t index_offset, double* d_best,
                         void* hip_stream) {
  if (!b || !d_g || !d_scores || !d_best) return fail(TWR_ERR_INVALID, "null argument");
  if (!(families & 0xffu) || (families & ~0xffu)) return fail(TWR_ERR_INVALID, "families must be a non-empty mask of the eight TWR_SET_* bits");
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  // two launches behind one call: the scores, then the arg-min over this batch's rows.  (One launch -- the scoring kernel's
  // last workgroup taking the decision behind a block counter -- was built and measured: 1024 atomics on one address cost
  // more than the launch they save, 73 vs 63 us per planner step of 1024 candidates)
  unsigned* counter = reinterpret_cast<unsigned*>(b->best.get() + 2 * (size_t)twr::best_max_blocks());
  hipError_t e = twr::launch_score(b->node.d.get(), b->n_problems, d_g, d_scores, static_cast<hipStream_t>(hip_stream));
  if (e == hipSuccess)
    e = twr::launch_best(d_scores, b->n_problems, families, b->best.get(), counter, d_best, (double)index_offset, static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_batch_scores_without_g(const twr_batch* b) { return b && b->plan.score_fused ? 1 : 0; }

namespace {
// twr_batch_eval_scores / twr_batch_eval_score_best: the launches PlanEval plans for a scoring request (kEvalScores)
int eval_scores(twr_batch* b, const double* d_x, double* d_g, double* d_scores, bool best, uint32_t families, int64_t index_offset,
                double* d_best, void* hip_stream) {
  if (!b || !d_x || !d_scores || (best && !d_best)) return fail(TWR_ERR_INVALID, "null argument");
  if (best && (!(families & 0xffu) || (families & ~0xffu))) return fail(TWR_ERR_INVALID, "families must be a non-empty mask of the eight TWR_SET_* bits");
  if (!b->plan.score_fused && !d_g)
    return fail(TWR_ERR_INVALID, "this batch scores through g (twr_batch_scores_without_g == 0): d_g is required");
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  const twr::BatchPlan& P = b->plan;
  const twr::EvalShape s = eval_shape(b, twr::kEvalScores | (best ? twr::kEvalBest : 0), false);
  twr::EvalBuffers buf{b->dyn.d.get(), b->rom.d.get(), b->node.d.get(), b->flat.d.get(),
                       {b->fam[0].d.get(), b->fam[1].d.get(), b->fam[2].d.get(), b->fam[3].d.get()},
                       b->pdyn.d.get(), b->ploc.d.get(), b->prom.d.get(), d_x, P.score_fused ? nullptr : d_g, nullptr, b->dump.get()};
  buf.score_blob = b->score_blob.d.get();
  buf.score_first = b->score_first.d.get();
  buf.score_slot = b->score_slot.d.get();
  buf.slab = b->score_slab.get();
  buf.scores = d_scores;
  buf.families = families;
  buf.index_offset = (double)index_offset;
  buf.best_partial = b->best.get();
  buf.best_counter = reinterpret_cast<unsigned*>(b->best.get() + 2 * (size_t)twr::best_max_blocks());
  buf.best = d_best;
  hipError_t e = twr::launch_eval(s, buf, static_cast<hipStream_t>(hip_stream), nullptr);
  return launched(e);
}
}  // namespace

int twr_batch_eval_scores(twr_batch* b, const double* d_x, double* d_g, double* d_scores, void* hip_stream) {
  return eval_scores(b, d_x, d_g, d_scores, false, 0, 0, nullptr, hip_stream);
}

int twr_batch_eval_score_best(twr_batch* b, const double* d_x, double* d_g, double* d_scores, uint32_t families, int64_t index_offset,
                              double* d_best, void* hip_stream) {
  return eval_scores(b, d_x, d_g, d_scores, true, families, index_offset, d_best, hip_stream);
}

int twr_batch_best(twr_batch* b, const double* d_scores, int32_t n_candidates, uint32_t families, double* d_best, void* hip_stream) {
  if (!b || !d_scores || !d_best) return fail(TWR_ERR_INVALID, "null argument");
  if (n_candidates < 1) return fail(TWR_ERR_INVALID, "twr_batch_best needs at least one candidate");
  if (!(families & 0xffu) || (families & ~0xffu)) return fail(TWR_ERR_INVALID, "families must be a non-empty mask of the eight TWR_SET_* bits");
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  unsigned* counter = reinterpret_cast<unsigned*>(b->best.get() + 2 * (size_t)twr::best_max_blocks());
  hipError_t e = twr::launch_best(d_scores, n_candidates, families, b->best.get(), counter, d_best, 0.0, static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_structure_contact_steps_max(const twr_structure* s, int32_t* max_steps) {
  if (!s || !max_steps) return fail(TWR_ERR_INVALID, "null argument");
  int n = 1;   // the first sample, then at most one footstep state per phase change of any foot
  for (int e = 0; e < s->s.n_ee; ++e) n += s->s.schedule.n_phases[e] - 1;
  *max_steps = n;
  return TWR_OK;
}

int twr_batch_contact_plan(twr_batch* b, const double* d_x, double dt, double time_horizon, double* d_out, int32_t max_steps,
                           int32_t* d_counts, void* hip_stream) {
  if (!b || !d_x || !d_out || !d_counts || max_steps < 1 || !(dt > 0)) return fail(TWR_ERR_INVALID, "bad arguments");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    int n_max = 0;
    for (int p = 0; p < b->n_problems; ++p) {
      if (!b->plan.sample_ok[p]) throw std::runtime_error("too many polynomials per spline for trajectory sampling");
      n_max = std::max(n_max, twr::SampleCount(b->plan.t_total[p], dt));
    }
    hipError_t e = twr::launch_contact_plan(b->node.d.get(), b->n_problems, d_x, d_out, d_counts, dt, time_horizon, n_max, max_steps,
                                            static_cast<hipStream_t>(hip_stream));
    return launched(e);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_leg_kinematics_preset(int robot, twr_leg_kinematics* out) {
  if (!out) return fail(TWR_ERR_INVALID, "null output");
  if (robot < TWR_ROBOT_MONOPED || robot > TWR_ROBOT_GO1) return fail(TWR_ERR_INVALID, "unknown robot id");
  if (!twr::LegKinematicsPreset(robot, out)) return fail(TWR_ERR_UNSUPPORTED, "the reference has inverse kinematics for Go1 only");
  return TWR_OK;
}

namespace {
// What the three joint calls check before any device is touched; *n_max: the largest sample count of a problem.  Strides are
// checked against every problem's own count (a stride of -1: that buffer is not part of the call).
int check_joint_call(const twr_batch* b, const twr_leg_kinematics* kin, std::initializer_list<const void*> buffers, double dt,
                     int64_t traj_stride, int64_t joint_stride, int* n_max) {
  if (!kin) return fail(TWR_ERR_INVALID, "null kin");
  try {   // (the descriptor first: it can be judged without a batch)
    twr::CheckLegKinematics(*kin);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  if (!b) return fail(TWR_ERR_INVALID, "null batch");
  for (const void* p : buffers)
    if (!p) return fail(TWR_ERR_INVALID, "null device buffer");
  if (misaligned(buffers)) return fail(TWR_ERR_INVALID, "device buffers must be 8-byte aligned");
  if (!std::isfinite(dt) || !(dt > 0)) return fail(TWR_ERR_INVALID, "dt must be finite and > 0");
  try {
    if (kin->n_ee != b->n_ee) throw std::runtime_error("twr_leg_kinematics: n_ee differs from the batch's");
    *n_max = 0;
    for (int p = 0; p < b->n_problems; ++p) {
      if (!b->plan.sample_ok[p]) throw std::runtime_error("too many polynomials per spline for trajectory sampling");
      const int n = twr::SampleCount(b->plan.t_total[p], dt);
      if (traj_stride >= 0 && (int64_t)n * (20 + 13 * b->n_ee) > traj_stride) throw std::runtime_error("traj_stride too small for the samples");
      if (joint_stride >= 0 && (int64_t)n * TWR_JOINT_REC(b->n_ee) > joint_stride) throw std::runtime_error("joint_stride too small for the samples");
      *n_max = std::max(*n_max, n);
    }
  } catch (const std::exception& e) {
    return fail(TWR_ERR_INVALID, e.what());
  }
  return TWR_OK;
}
}  // namespace

int twr_batch_joints(twr_batch* b, const twr_leg_kinematics* kin, const double* d_traj, int64_t traj_stride, double dt, double* d_joints,
                     int64_t joint_stride, void* hip_stream) {
  int n_max = 0;
  if (traj_stride < 0 || joint_stride < 0) return fail(TWR_ERR_INVALID, "negative stride");
  const int rc = check_joint_call(b, kin, {d_traj, d_joints}, dt, traj_stride, joint_stride, &n_max);
  if (rc != TWR_OK) return rc;
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    sample_work_for(*b, dt, traj_stride);
    hipError_t e = twr::launch_joints(b->swork.d.get(), b->swork.n, d_traj, traj_stride, d_joints, joint_stride, b->n_ee, *kin,
                                      static_cast<hipStream_t>(hip_stream));
    return launched(e);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_joint_scores(twr_batch* b, const twr_leg_kinematics* kin, const double* d_joints, int64_t joint_stride, double dt,
                           double* d_jscores, void* hip_stream) {
  int n_max = 0;
  if (joint_stride < 0) return fail(TWR_ERR_INVALID, "negative stride");
  const int rc = check_joint_call(b, kin, {d_joints, d_jscores}, dt, -1, joint_stride, &n_max);
  if (rc != TWR_OK) return rc;
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipError_t e = twr::launch_joint_scores(b->node.d.get(), b->n_problems, d_joints, joint_stride, dt, n_max, d_jscores, *kin,
                                          static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_batch_eval_joint_scores(twr_batch* b, const twr_leg_kinematics* kin, const double* d_x, double dt, double* d_jscores,
                                void* hip_stream) {
  int n_max = 0;
  const int rc = check_joint_call(b, kin, {d_x, d_jscores}, dt, -1, -1, &n_max);
  if (rc != TWR_OK) return rc;
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipError_t e = twr::launch_eval_joint_scores(b->node.d.get(), b->n_problems, d_x, dt, n_max, d_jscores, *kin,
                                               static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

namespace {
// What the two check calls check before any device is touched (strides as check_joint_call); *n_max: the largest sample count.
int check_checks_call(const twr_batch* b, std::initializer_list<const void*> buffers, double dt, int64_t traj_stride, int64_t check_stride,
                      int* n_max) {
  if (!b) return fail(TWR_ERR_INVALID, "null batch");
  for (const void* p : buffers)
    if (!p) return fail(TWR_ERR_INVALID, "null device buffer");
  if (misaligned(buffers)) return fail(TWR_ERR_INVALID, "device buffers must be 8-byte aligned");
  if (!std::isfinite(dt) || !(dt > 0)) return fail(TWR_ERR_INVALID, "dt must be finite and > 0");
  *n_max = 0;
  for (int p = 0; p < b->n_problems; ++p) {
    if (!b->plan.sample_ok[p]) return fail(TWR_ERR_INVALID, "too many polynomials per spline for trajectory sampling");
    const int n = twr::SampleCount(b->plan.t_total[p], dt);
    if (traj_stride >= 0 && (int64_t)n * (20 + 13 * b->n_ee) > traj_stride) return fail(TWR_ERR_INVALID, "traj_stride too small for the samples");
    if ((int64_t)n * TWR_CHECK_REC(b->n_ee) > check_stride) return fail(TWR_ERR_INVALID, "check_stride too small for the samples");
    *n_max = std::max(*n_max, n);
  }
  return TWR_OK;
}
}  // namespace

int twr_batch_checks(twr_batch* b, const twr_model* model, const double* d_traj, int64_t traj_stride, double dt, double* d_checks,
                     int64_t check_stride, void* hip_stream) {
  int n_max = 0;
  if (!model) return fail(TWR_ERR_INVALID, "null model");
  if (model->n_ee < 1 || model->n_ee > TWR_MAX_EE) return fail(TWR_ERR_INVALID, "twr_model: n_ee must be 1..4");
  for (int e = 0; e < model->n_ee; ++e)
    for (int d = 0; d < 3; ++d)
      if (!std::isfinite(model->nominal_stance[e][d])) return fail(TWR_ERR_INVALID, "twr_model: nominal_stance must be finite");
  for (int d = 0; d < 3; ++d)
    if (!std::isfinite(model->max_dev[d]) || !(model->max_dev[d] >= 0)) return fail(TWR_ERR_INVALID, "twr_model: max_dev must be finite and >= 0");
  if (!std::isfinite(model->force_limit)) return fail(TWR_ERR_INVALID, "twr_model: force_limit must be finite");
  if (traj_stride < 0 || check_stride < 0) return fail(TWR_ERR_INVALID, "negative stride");
  const int rc = check_checks_call(b, {d_traj, d_checks}, dt, traj_stride, check_stride, &n_max);
  if (rc != TWR_OK) return rc;
  if (model->n_ee != b->n_ee) return fail(TWR_ERR_INVALID, "twr_model: n_ee differs from the batch's");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    sample_work_for(*b, dt, traj_stride);
    hipError_t e = twr::launch_checks(b->swork.d.get(), b->swork.n, d_traj, traj_stride, d_checks, check_stride, *model,
                                      static_cast<hipStream_t>(hip_stream));
    return launched(e);
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

int twr_batch_check_scores(twr_batch* b, const double* d_checks, int64_t check_stride, double dt, double* d_cscores, void* hip_stream) {
  int n_max = 0;
  if (check_stride < 0) return fail(TWR_ERR_INVALID, "negative stride");
  const int rc = check_checks_call(b, {d_checks, d_cscores}, dt, -1, check_stride, &n_max);
  if (rc != TWR_OK) return rc;
  DeviceScope on(b->device);
  if (on.status != hipSuccess) return fail(TWR_ERR_HIP, "hipSetDevice failed");
  hipError_t e = twr::launch_check_scores(b->node.d.get(), b->n_problems, d_checks, check_stride, dt, n_max, d_cscores,
                                          static_cast<hipStream_t>(hip_stream));
  return launched(e);
}

int twr_batch_host_buffers(twr_batch* b, double** h_x, double** h_g, double** h_jac) {
  if (!b) return fail(TWR_ERR_INVALID, "null batch");
  try {
    DeviceScope on(b->device);
    TWR_HIP(on.status);
    auto pinned = [](int64_t count) {
      void* p = nullptr;
      TWR_HIP(hipHostMalloc(&p, count * sizeof(double), hipHostMallocDefault));
      return PinnedPtr<double>(static_cast<double*>(p));
    };
    if (!b->p_x) {
      b->p_x = pinned(b->plan.x_off.back());
      b->p_g = pinned(b->plan.g_off.back());
      b->p_j = pinned(b->plan.j_off.back());
    }
    if (h_x) *h_x = b->p_x.get();
    if (h_g) *h_g = b->p_g.get();
    if (h_jac) *h_jac = b->p_j.get();
    return TWR_OK;
  } catch (const std::exception& e) {
    return fail(TWR_ERR_HIP, e.what());
  }
}

}  // extern "C"
