// What the two units of the C ABI share (capi.cc: the batch runtime; capi_jac.cc: the Jacobian linear algebra): the handles
// both read, the owners of device memory, and the helpers every entry point is written with.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "jac_plan.h"
#include "launch.h"

struct twr_structure {
  twr::Structure s;
};
struct twr_terrain_grid {
  std::shared_ptr<twr::TerrainGrid> g;
};

// Makes `device` current for a scope and restores the calling thread's device afterwards: no entry point of the library
// leaves its caller on another device (one process may drive several GPUs).  The caller's error state is not touched.
struct DeviceScope {
  int prev = -1;
  bool switched = false;
  hipError_t status = hipSuccess;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != device) {
      status = hipSetDevice(device);
      switched = status == hipSuccess;
    }
  }
  ~DeviceScope() {
    if (switched && prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// Owners of what a handle holds on its device.  They release it where they are destroyed, so whoever destroys a handle
// holds a DeviceScope of its device (twr_batch_destroy, twr_planes_destroy).
struct HipFree {
  void operator()(void* p) const { (void)hipFree(p); }
};
struct HipHostFree {
  void operator()(void* p) const { (void)hipHostFree(p); }
};
struct HipStreamDestroy {
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
template <class T> using DevPtr = std::unique_ptr<T, HipFree>;
template <class T> using PinnedPtr = std::unique_ptr<T, HipHostFree>;
using StreamPtr = std::unique_ptr<std::remove_pointer_t<hipStream_t>, HipStreamDestroy>;
template <class T> struct DevList {   // a work list in device memory
  DevPtr<T> d;
  int n = 0;
};
struct Events {   // hipEvent_t[] (launch_eval records into consecutive ones)
  std::vector<hipEvent_t> ev;
  Events() = default;
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  ~Events() { clear(); }
  void clear() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
  }
};

struct twr_planes {
  int device = 0;
  std::vector<int32_t> start;      // polygon r = points [start[r], start[r+1])
  std::vector<double> world_xy;    // PlanarRegionsToPolygons output
  DevPtr<double> d_xy;
  DevPtr<int32_t> d_start;
};

struct twr_batch {
  int device = 0;
  int n_problems = 0, n_ee = 0, n_cu = 0;
  twr::BatchPlan plan;                       // offsets, what twr_batch_sample needs, policy (its work lists are on the device, below)
  DevPtr<void> arena;                        // ONE allocation for the tables of all structures (a sweep has a thousand
                                             // of them: one mapping with large pages instead of a thousand small ones,
                                             // one upload instead of a thousand)
  int64_t table_bytes = 0;                   // arena bytes
  std::vector<DevPtr<void>> grids;           // device copies of the distinct gridded terrains
  // twr_batch_grid_map_sync / _update_device: the handle behind grids[q] (kept alive: it is how a caller names the map), and
  // for a `Grid` map the headers that read it -- entries [grid_hdr_first[q], grid_hdr_first[q + 1]) of grid_hdr, each the
  // byte offset of a DevStruct::grid_px in the arena.  Built once by twr_batch_create; a CSV grid has no entries.
  std::vector<std::shared_ptr<const twr::TerrainGrid>> grid_of;
  std::vector<int32_t> grid_hdr_first;
  DevList<uint64_t> grid_hdr;
  DevPtr<float> grid_stage;                  // twr_batch_grid_map_sync: where the host layer lands (first call; the largest map)
  DevList<twr::DynWork> dyn;
  DevList<twr::RomWork> rom;
  DevList<twr::NodeWork> node;               // (+ the end entry, not counted)
  DevList<twr::FlatWork> flat;               // values-only evaluation of dynamic / rangeofmotion-* (empty: not for this batch)
  DevList<twr::FamWork> fam[4];              // chunk lists of node_chunk_kernel (large batches only)
  // optimised-timings problems have their own work lists
  DevList<twr::PDynWork> pdyn;
  DevList<twr::LocWork> ploc;
  DevList<twr::RomPhaseWork> prom;
  DevPtr<void> precs;                        // scratch: x-dependent DynLoc / RomRec records of the optimised-timings problems
  DevList<int64_t> goff, joff;               // device copies of g_off / j_off (TWR_EVAL_CHECK)
  DevPtr<int32_t> status;                    // per-problem non-finite flags of the last checked evaluation
  DevPtr<double> dump;                       // where dyn_kernel's first (empty) copy-out of every workgroup goes
  DevPtr<double> best;                       // twr_batch_best: per-block results (2 doubles each) + the block counter behind them
  DevList<uint64_t> score_blob;              // twr_batch_eval_scores without g (plan.score_fused): BatchPlan::Lists score_*
  DevList<int32_t> score_first, score_slot;
  DevPtr<double> score_slab;                 // the scoring launch's partial records (kScorePartial doubles each)
  DevList<twr::SampleWork> swork;            // work list of the last twr_batch_sample call (cached per dt / stride)
  double swork_dt = 0.0;
  int64_t swork_stride = -1;
  DevList<twr::SampleWork> gwork;            // work list of the last twr_batch_initial_guess call (cached per count / stride)
  int gwork_times = -1;
  int64_t gwork_stride = -1;
  // twr_batch_start: the start tables of the batch's structures as the structures hold them (shared, not copied) and the
  // structure of every problem, kept by twr_batch_create; twr_batch_reserve_start plans from them (twr::PlanStart) and uploads
  // the distinct tables and the work list into device memory of their own
  std::vector<std::shared_ptr<const std::vector<char>>> start_tables;
  std::vector<int32_t> struct_of_problem;
  DevPtr<char> start_dev;
  DevList<twr::StartWork> start_work;
  // lazily sized scratch for twr_batch_eval_host
  DevPtr<double> d_x, d_g, d_j;
  PinnedPtr<double> p_x, p_g, p_j;           // page-locked host buffers (twr_batch_host_buffers)
  // twr_batch_eval_host runs on a stream of the batch's own (non-blocking: it neither waits for nor holds up work the host
  // application has on the NULL stream or on other blocking streams); created on first use
  StreamPtr host_stream;
  // optional per-kernel timing (twr_batch_profile_begin/end): 4 events per recorded eval
  Events prof_events;
  int prof_capacity = 0, prof_count = 0;
};

// Records the message twr_last_error returns (per thread) and hands `code` back.  Defined in capi.cc.
__attribute__((visibility("hidden"))) int fail(int code, const std::string& msg);

#define TWR_HIP(call)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

namespace {   // (each unit has its own copy: nothing here is a symbol of the library)

template <class T> DevPtr<T> dev_alloc(size_t bytes) {
  void* p = nullptr;
  TWR_HIP(hipMalloc(&p, bytes));
  return DevPtr<T>(static_cast<T*>(p));
}
template <class T> DevPtr<T> dev_zeros(size_t count) {
  DevPtr<T> d = dev_alloc<T>(count * sizeof(T));
  TWR_HIP(hipMemset(d.get(), 0, count * sizeof(T)));
  return d;
}
template <class T> DevList<T> upload(const std::vector<T>& v) {
  DevList<T> l{dev_alloc<T>(v.size() * sizeof(T)), (int)v.size()};
  TWR_HIP(hipMemcpy(l.d.get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return l;
}
template <class T> DevList<T> upload_nonempty(const std::vector<T>& v) {   // an empty list: no allocation, no copy
  return v.empty() ? DevList<T>() : upload(v);
}

// The structures behind an array of handles (throws on a NULL one)
inline std::vector<const twr::Structure*> structure_ptrs(const twr_structure* const* structs, int n_structs) {
  std::vector<const twr::Structure*> sp(n_structs);
  for (int i = 0; i < n_structs; ++i) {
    if (!structs[i]) throw std::runtime_error("null structure");
    sp[i] = &structs[i]->s;
  }
  return sp;
}

inline bool misaligned(std::initializer_list<const void*> ptrs) {   // NULL (an optional buffer left out) counts as aligned
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  return (bits & 7) != 0;
}
inline int launched(hipError_t e) {   // the return code of an entry point whose launches gave `e`
  if (e != hipSuccess) return fail(TWR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return TWR_OK;
}

}  // namespace
