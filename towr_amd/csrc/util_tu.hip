// Third translation unit of the kernels, plain flags: the utility kernels -- trajectory sampling, scoring from g, the planner's arg-min,
// contact plan, nearest plane, joint-space trajectories and their scores, the trajectory checks and their scores, TWR_EVAL_CHECK, the grid_map layer update, the start of a request (x0 and variable bounds) -- each followed by its launch_* function (launch.h); none is used by an evaluation kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "launch.h"

#include "kernels/common.h"
#include "kernels/host_launch.h"
#include "kernels/spline_math.h"
#include "kernels/phase_durations.h"
#include "kernels/checks.h"
#include "kernels/grid_map_update.h"
#include "kernels/joints.h"
#include "kernels/planes.h"
#include "kernels/sample.h"
#include "kernels/start.h"

namespace twr {

// ---------------------------------------------------------------- trajectory sampling (the device functions: kernels/sample.h)
// With `times` set the kernel is fpowr::ExtractInitialGuess (fpowr/include/fpowr/initial_guess_extractor.h:17-34)
// instead: sample s of every problem is taken at times[s] and the record is [ t | state: base-lin p, base-ang p (Euler
// angles), base-lin v, base-ang v (Euler rates) | controls (36): ee-motion acceleration of ee i at 3 i, twelve zeros
// ("joint torques"), ee-force of ee i at 24 + 3 i ] = 49 doubles.
__global__ __launch_bounds__(64) void sample_kernel(const SampleWork* __restrict__ work, const double* __restrict__ x,
                                                    double* __restrict__ out, double dt, const double* __restrict__ times) {
  __shared__ double s_bd[2 * kMaxPhasePolys], s_ph[kMaxEE][TWR_MAX_PHASES_DEV], s_md[kMaxEE][kMaxPhasePolys],
      s_fd[kMaxEE][kMaxPhasePolys];
  const SampleWork sw = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(sw.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const SampleTables* ST = tbl<SampleTables>(blob, H->o_sample);
  const double* xp = x + sw.x_off;
  const int lane = threadIdx.x, n_ee = H->n_ee;
  for (int q = lane; q < ST->n_base; q += 64) s_bd[q] = tbl<double>(blob, ST->o_bdur)[q];
  for (int e = 0; e < n_ee; ++e) {
    if (H->timings) {  // PhaseDurations::SetVariables + ConvertPhaseToPolyDurations (phase_durations.cc:77-103)
      const PhaseTables* PT = tbl<PhaseTables>(blob, H->o_phase);
      phase_poly_durations_wave(PT, blob, xp, e, s_ph[e], s_md[e], lane);
      const PhasePoly* fp = tbl<PhasePoly>(blob, PT->o_fpoly[e]);
      for (int q = lane; q < PT->n_fpoly[e]; q += 64) s_fd[e][q] = s_ph[e][fp[q].phase] / fp[q].n_in_phase;
    } else {
      for (int q = lane; q < ST->n_phases[e]; q += 64) s_ph[e][q] = tbl<double>(blob, ST->o_phdur[e])[q];
      for (int q = lane; q < ST->n_mpoly[e]; q += 64) s_md[e][q] = tbl<double>(blob, ST->o_mdur[e])[q];
      for (int q = lane; q < ST->n_fpoly[e]; q += 64) s_fd[e][q] = tbl<double>(blob, ST->o_fdur[e])[q];
    }
  }
  __syncthreads();
  if (lane >= sw.cnt) return;
  const int s_idx = sw.s0 + lane;
  double t = 0.0;
  if (times) t = times[s_idx];
  else for (int i = 0; i < s_idx; ++i) t += dt;   // the reference's accumulated sample time
  const int rec = times ? 49 : 20 + 13 * n_ee;
  double* o = out + sw.out_off + (int64_t)s_idx * rec;
  o[0] = t;
  BaseSample B;
  sample_base(xp, ST, s_bd, t, B);
  const double (&e3)[3] = B.e3, (&ed)[3] = B.ed;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    o[1 + d] = B.p[d];
    o[4 + d] = B.v[d];
    o[7 + d] = B.a[d];
  }
  if (times) {   // ExtractInitialGuess record
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const double lv = o[4 + d];
      o[4 + d] = e3[d];
      o[7 + d] = lv;
      o[10 + d] = ed[d];
    }
    for (int q = 13; q < 49; ++q) o[q] = 0.0;
    for (int e = 0; e < n_ee; ++e) {
      double tlm, tlf, p[3], v[3], a[3];
      const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
      const int qf = locate_segment(s_fd[e], ST->n_fpoly[e], t, tlf);
      sample_spline(xp, tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm], tlm, s_md[e][qm], p, v, a);
#pragma unroll
      for (int d = 0; d < 3; ++d) o[13 + 3 * e + d] = a[d];
      sample_spline(xp, tbl<PolyDesc>(blob, ST->o_fdesc[e])[qf], tlf, s_fd[e][qf], p, v, a);
#pragma unroll
      for (int d = 0; d < 3; ++d) o[37 + 3 * e + d] = p[d];
    }
    return;
  }
  BaseAngular A;
  sample_angular(B, A);
  o[10] = A.q[3]; o[11] = A.q[0]; o[12] = A.q[1]; o[13] = A.q[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o[14 + i] = A.omega[i];
    o[17 + i] = A.omega_dot[i];
  }
  for (int e = 0; e < n_ee; ++e) {
    double* oe = o + 20 + 13 * e;
    double tlp, tlm, tlf;
    const int phase = locate_segment(s_ph[e], ST->n_phases[e], t, tlp);   // PhaseDurations::IsContactPhase
    oe[0] = ((phase & 1) == 0) == (ST->contact0[e] != 0) ? 1.0 : 0.0;
    const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
    const int qf = locate_segment(s_fd[e], ST->n_fpoly[e], t, tlf);
    const PolyDesc pm = tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm];
    const PolyDesc pf = tbl<PolyDesc>(blob, ST->o_fdesc[e])[qf];
    double p[3], v[3], a[3];
    sample_spline(xp, pm, tlm, s_md[e][qm], p, v, a);
#pragma unroll
    for (int d = 0; d < 3; ++d) { oe[1 + d] = p[d]; oe[4 + d] = v[d]; oe[7 + d] = a[d]; }
    sample_spline(xp, pf, tlf, s_fd[e][qf], p, v, a);
#pragma unroll
    for (int d = 0; d < 3; ++d) oe[10 + d] = p[d];
  }
}
hipError_t launch_sample(const SampleWork* work, int n_work, const double* x, double* out, double dt, const double* times,
                         hipStream_t stream) {
  if (n_work <= 0) return hipSuccess;
  return twr_launch(sample_kernel, dim3(n_work), dim3(64), 0, stream, work, x, out, dt, times);
}

// ---------------------------------------------------------------- candidate scoring
// twr_batch_score: per problem and constraint family the inf- and 1-norm of the bound violation
// max(lower - g, g - upper, 0) over the family's rows (bounds of ConstraintSet::GetBounds, twr_structure_bounds).
// A sweep then returns 16 doubles per candidate instead of its Jacobian.
// (round 5: 256 threads per problem, row r = 256 k + thread, sixteen rows per thread; family slot and bounds of a row come
// from its 16-bit meta word and the structure's short table of distinct (lower, upper) pairs, device_tables.h ScoreTables.)
// Two dependent round trips: (1) the work item and its successor (row count = difference of their g offsets; the list
// carries an end entry), (2) the rows of g, the meta words of the rows AND the head of the score record (2 KB requested on spec:
// the pair table) -> LDS -- the record sits at a fixed offset of the blob (kScoreOff), no field of the header is needed.  The slot of a thread's rows never falls, so it keeps one
// running (max, sum) pair and hands it to its LDS cell when the slot moves on.  Round 4's kernel fetched a cold candidate's
// fields one s_load at a time and 16 bytes of bounds per row: 25 us for 128 candidates, 43 us for 1024.
__device__ __forceinline__ void best_of(double& v, int& i, double ov, int oi) {
  if (ov < v || (ov == v && oi < i)) {
    v = ov;
    i = oi;
  }
}
__global__ __launch_bounds__(256) void score_kernel(const NodeWork* __restrict__ work, const double* __restrict__ g,
                                                    double* __restrict__ scores) {
  constexpr int kHeadDwords = kScoreHeadBytes / 4, kTabDwords = (int)(sizeof(ScoreTables) / 4);
  static_assert(kHeadDwords == 512 && kTabDwords + 4 * kScoreMaxPairs <= kHeadDwords, "the whole record within its head: two loads per thread");
  __shared__ __attribute__((aligned(16))) int32_t s_tab[kHeadDwords];   // the record as in the blob
  __shared__ double red[256 * 16 + 16 * 16];   // cell (2 slot + {max, sum}, thread), then the partial results of the fold
  const int tid = threadIdx.x;
  const NodeWork w = work[blockIdx.x];
  const int n_rows = (int)(work[blockIdx.x + 1].g_off - w.g_off);
  if (n_rows <= 0) {   // (uniform) a structure whose constraint sets have no rows: nothing is violated, nothing is read
    if (tid < 16) scores[16 * (size_t)blockIdx.x + tid] = 0.0;
    return;
  }
  const double* gp = g + w.g_off;
  const char* blob = reinterpret_cast<const char*>(w.blob);
#pragma unroll
  for (int c = 0; c < 16; ++c) red[c * 256 + tid] = 0.0;   // (a cell is written at most once more; own cells only: no barrier)
  int cur = 0;
  double cm = 0.0, cs = 0.0;
  for (int base = 0; base < n_rows; base += 16 * 256) {   // (one trip for structures of up to 4096 rows)
    double v[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = gp[min(base + 256 * k + tid, n_rows - 1)];
    const int32_t* Tw = reinterpret_cast<const int32_t*>(tbl<ScoreTables>(blob, kScoreOff));   // (fixed offset: no header field)
    const uint16_t* meta = reinterpret_cast<const uint16_t*>(blob + kScoreOff + kScoreHeadBytes);
    uint32_t m[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m[k] = meta[min(base + 256 * k + tid, n_rows - 1)];
    if (base == 0) {
      const int32_t a = Tw[tid], c = Tw[tid + 256];
      s_tab[tid] = a;
      s_tab[tid + 256] = c;
      __syncthreads();
    }
    const double* s_pairs = reinterpret_cast<const double*>(s_tab + kTabDwords);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (base + 256 * k < n_rows) {   // uniform
        const bool live = base + 256 * k + tid < n_rows;
        const int slot = (int)(m[k] >> 12), q = (int)(m[k] & 0xFFFu);
        const double lo = s_pairs[2 * q], up = s_pairs[2 * q + 1], val = v[k];
        // NaN-propagating: a non-finite constraint value makes the family's scores NaN instead of hiding in a max()
        double viol = fmax(fmax(lo - val, val - up), 0.0);
        if (val != val) viol = val;
        if (live && slot != cur) {   // the slot moved on: hand over the running pair (rare: a few times per thread)
          red[(2 * cur) * 256 + tid] = cm;
          red[(2 * cur + 1) * 256 + tid] = cs;
          cm = cs = 0.0;
          cur = slot;
        }
        if (live) {
          cm = nan_max(cm, viol);
          cs += viol;
        }
      }
    }
  }
  red[(2 * cur) * 256 + tid] = cm;
  red[(2 * cur + 1) * 256 + tid] = cs;
  // 256 threads x 16 cells -> 16 values, transposed: thread 16 c + j folds column j of threads c, c + 16, ..., then sixteen
  // threads fold the sixteen partial results of their column and store it at its FAMILY's place
  __syncthreads();
  {
    const int j = tid & 15, c = tid >> 4;   // column j (even: an inf-norm, odd: a 1-norm)
    double acc = red[j * 256 + c];
#pragma unroll
    for (int i = 1; i < 16; ++i) {
      const double o = red[j * 256 + c + 16 * i];
      acc = (j & 1) ? acc + o : nan_max(acc, o);
    }
    red[256 * 16 + c * 16 + j] = acc;
  }
  __syncthreads();
  if (tid < 16) {
    const int slot = reinterpret_cast<const int8_t*>(s_tab + 2)[tid >> 1];   // ScoreTables::slot_of_family[family tid / 2]
    double acc = 0.0;
    if (slot >= 0) {
      const int j = 2 * slot + (tid & 1);
      acc = red[256 * 16 + j];
      for (int c = 1; c < 16; ++c) {
        const double o = red[256 * 16 + c * 16 + j];
        acc = (tid & 1) ? acc + o : nan_max(acc, o);
      }
    }
    scores[16 * (size_t)blockIdx.x + tid] = acc;
  }
}
hipError_t launch_score(const NodeWork* work, int n_problems, const double* g, double* scores, hipStream_t stream) {
  return twr_launch(score_kernel, dim3(n_problems), dim3(256), 0, stream, work, g, scores);
}

// twr_batch_best: the planner's decision on the device -- arg-min over a score table of the summed inf-norm violations of
// the chosen constraint families (the table may be longer than this batch: after an all-gather it holds the candidates of
// every rank).  Same rule as towr_amd.dist.best_candidate: families summed in ascending order, NaN loses, first index wins
// a tie.  One launch: every block reduces its stride of candidates, the last block to finish reduces the blocks' results
// (threadfence + counter, reset for the next call) and writes best[0] = index, best[1] = its total.
__global__ __launch_bounds__(256) void best_kernel(const double* __restrict__ scores, int n, unsigned families, double* __restrict__ partial,
                                                   unsigned* __restrict__ counter, double* __restrict__ best, double index_offset) {
  __shared__ double s_v[4];
  __shared__ int s_i[4];
  __shared__ bool s_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double bv = __builtin_inf();
  int bi = 0x7fffffff;
  for (int c = blockIdx.x * 256 + tid; c < n; c += gridDim.x * 256) {
    const double* row = scores + 16 * (size_t)c;
    double t = 0.0;
    bool first = true;
#pragma unroll
    for (int f = 0; f < 8; ++f)
      if (families >> f & 1u) {
        t = first ? row[2 * f] : t + row[2 * f];
        first = false;
      }
    if (t != t) t = __builtin_inf();
    best_of(bv, bi, t, c);
  }
  auto block_reduce = [&]() {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best_of(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
    if (lane == 0) {
      s_v[wave] = bv;
      s_i[wave] = bi;
    }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < 4; ++w) best_of(bv, bi, s_v[w], s_i[w]);
  };
  block_reduce();
  if (tid == 0) {
    partial[2 * blockIdx.x] = bv;
    partial[2 * blockIdx.x + 1] = (double)bi;
    __threadfence();
    s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  bv = __builtin_inf();
  bi = 0x7fffffff;
  for (int k = tid; k < (int)gridDim.x; k += 256)
    best_of(bv, bi, __builtin_nontemporal_load(partial + 2 * k), (int)__builtin_nontemporal_load(partial + 2 * k + 1));
  __syncthreads();
  block_reduce();
  if (tid == 0) {
    best[0] = index_offset + (double)(bi == 0x7fffffff ? 0 : bi);
    best[1] = bv;
    *counter = 0u;
  }
}
int best_max_blocks() { return 256; }
hipError_t launch_best(const double* scores, int n, unsigned families, double* partial, unsigned* counter, double* best, double index_offset,
                       hipStream_t stream) {
  int blocks = (n + 1023) / 1024;   // >= four candidates per thread before another block pays
  blocks = blocks < 1 ? 1 : (blocks > best_max_blocks() ? best_max_blocks() : blocks);
  return twr_launch(best_kernel, dim3(blocks), dim3(256), 0, stream, scores, n, families, partial, counter, best, index_offset);
}

// ---------------------------------------------------------------- contact plan
// fpowr::ExtractFootstepPlan (fpowr/include/fpowr/footstep_plan_extractor.h:69-133) minus the nearest-plane lookup
// (boost::geometry over ROS messages, left to the caller): the solution is sampled every dt like GetTrajectory
// (t accumulated), a footstep state is the first sample and every sample whose contact flags differ from the
// previous sample's (HasEndEffectorContactChanged, :55-67); its duration is the time to the next footstep state, the
// last one lasts until time_horizon (:121-128).  One wave per problem, lane = sample, 64 samples per round, footstep
// states compacted with a ballot.  Record: [ t | duration | contact per ee | ee-motion position (3) per ee ].
__global__ __launch_bounds__(64) void contact_plan_kernel(const NodeWork* __restrict__ work, const double* __restrict__ x,
                                                          double* __restrict__ out, int32_t* __restrict__ counts, double dt,
                                                          double time_horizon, int n_samples_max, int max_steps) {
  __shared__ double s_ph[kMaxEE][TWR_MAX_PHASES_DEV], s_md[kMaxEE][kMaxPhasePolys];
  const NodeWork w = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(w.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const SampleTables* ST = tbl<SampleTables>(blob, H->o_sample);
  const double* xp = x + w.x_off;
  const int lane = threadIdx.x, n_ee = H->n_ee;
  for (int e = 0; e < n_ee; ++e) {
    if (H->timings) {  // PhaseDurations::SetVariables + ConvertPhaseToPolyDurations (phase_durations.cc:77-103)
      phase_poly_durations_wave(tbl<PhaseTables>(blob, H->o_phase), blob, xp, e, s_ph[e], s_md[e], lane);
    } else {
      for (int q = lane; q < ST->n_phases[e]; q += 64) s_ph[e][q] = tbl<double>(blob, ST->o_phdur[e])[q];
      for (int q = lane; q < ST->n_mpoly[e]; q += 64) s_md[e][q] = tbl<double>(blob, ST->o_mdur[e])[q];
    }
  }
  __syncthreads();
  // GetTrajectory: while (t <= T + 1e-5) { ...; t += dt; }
  const double T = ST->t_total;
  const int rec = 2 + 4 * n_ee;
  double* o = out + (size_t)blockIdx.x * (size_t)max_steps * rec;
  int n_steps = 0;          // wave-uniform
  double t_carry = 0.0;     // t of the last footstep state of the previous round (wave-uniform)
  for (int s0 = 0; s0 < n_samples_max; s0 += 64) {
    const int s_idx = s0 + lane;
    double t = 0.0, tq = 0.0;   // this sample's and the previous sample's accumulated time (t += dt, like the reference)
    for (int i = 0; i < s_idx; ++i) {
      tq = t;
      t += dt;
    }
    const bool live = t <= T + 1e-5;
    unsigned mask = 0, mask_prev = 0;
    for (int e = 0; e < n_ee; ++e) {  // PhaseDurations::IsContactPhase (phase_durations.cc:118-124)
      double tl;
      const int ph = locate_segment(s_ph[e], ST->n_phases[e], t, tl);
      mask |= ((((ph & 1) == 0) == (ST->contact0[e] != 0)) ? 1u : 0u) << e;
      const int pq = locate_segment(s_ph[e], ST->n_phases[e], tq, tl);
      mask_prev |= ((((pq & 1) == 0) == (ST->contact0[e] != 0)) ? 1u : 0u) << e;
    }
    const bool step = live && (s_idx == 0 || mask != mask_prev);
    const uint64_t ball = __ballot(step);
    if (ball == 0) {
      if (!__any(live)) break;
      continue;
    }
    const uint64_t below = ball & ((1ull << lane) - 1ull);
    const uint64_t above = lane == 63 ? 0ull : (ball >> (lane + 1));
    const int my = n_steps + __popcll(below);
    // time of the footstep state before this one: the closest step lane below, or the previous round's last
    const double t_below = __shfl(t, below ? 63 - __clzll(below) : lane);
    const double t_prev = below ? t_below : t_carry;
    if (step && my < max_steps) {
      double* r = o + (size_t)my * rec;
      r[0] = t;
      if (!above) r[1] = time_horizon - t;   // last footstep state so far (:125-127); a later round may close it
      for (int e = 0; e < n_ee; ++e) {
        r[2 + e] = (mask >> e) & 1u ? 1.0 : 0.0;
        double tlm;
        const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
        const PolyDesc pm = tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm];
        double p[3], v[3], a[3];
        sample_spline(xp, pm, tlm, s_md[e][qm], p, v, a);
#pragma unroll
        for (int d = 0; d < 3; ++d) r[2 + n_ee + 3 * e + d] = p[d];
      }
    }
    // duration of the state before (:121-123) -- also when THIS state no longer fits the output (my == max_steps): the
    // last record that was kept still gets its duration
    if (step && my > 0 && my - 1 < max_steps) o[(size_t)(my - 1) * rec + 1] = t - t_prev;
    t_carry = __shfl(t, 63 - __clzll(ball));
    n_steps += __popcll(ball);
  }
  if (lane == 0) counts[blockIdx.x] = n_steps;
}
hipError_t launch_contact_plan(const NodeWork* work, int n_problems, const double* x, double* out, int32_t* counts, double dt,
                               double time_horizon, int n_samples_max, int max_steps, hipStream_t stream) {
  return twr_launch(contact_plan_kernel, dim3(n_problems), dim3(64), 0, stream, work, x, out, counts, dt, time_horizon,
                    n_samples_max, max_steps);
}

// ---------------------------------------------------------------- nearest plane of a footstep
// plane_kernel: one thread per (problem, footstep state, end-effector) of a contact plan; the lookup is nearest_plane of
// kernels/planes.h.
__global__ __launch_bounds__(256) void plane_kernel(const double* __restrict__ plan, const int32_t* __restrict__ counts,
                                                    const double* __restrict__ poly_xy, const int32_t* __restrict__ poly_start,
                                                    int n_polys, int n_problems, int max_steps, int n_ee,
                                                    int32_t* __restrict__ plane_index) {
  const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (int64_t)n_problems * max_steps * n_ee) return;
  const int e = (int)(id % n_ee), s = (int)((id / n_ee) % max_steps), p = (int)(id / ((int64_t)n_ee * max_steps));
  const double* rec = plan + ((int64_t)p * max_steps + s) * (2 + 4 * n_ee);
  int nearest = -1;
  if (s < counts[p] && rec[2 + e] != 0.0) {
    const double px = rec[2 + n_ee + 3 * e], py = rec[2 + n_ee + 3 * e + 1];
    nearest = nearest_plane(poly_xy, poly_start, n_polys, px, py);
  }
  plane_index[id] = nearest;
}
hipError_t launch_planes(const double* plan, const int32_t* counts, const double* poly_xy, const int32_t* poly_start, int n_polys,
                         int n_problems, int max_steps, int n_ee, int32_t* plane_index, hipStream_t stream) {
  const int64_t n = (int64_t)n_problems * max_steps * n_ee;
  if (n <= 0) return hipSuccess;
  return twr_launch(plane_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, plan, counts, poly_xy, poly_start, n_polys,
                    n_problems, max_steps, n_ee, plane_index);
}

// ---------------------------------------------------------------- joint-space trajectories (kernels/joints.h)
// twr_batch_joints: records of sample_kernel -> joint records, lane = sample over the same work list (the problem is the
// item's record offset over the trajectory stride).  Only the records are read: no table, no x.
__global__ __launch_bounds__(64) void joints_kernel(const SampleWork* __restrict__ work, const double* __restrict__ traj,
                                                    int64_t traj_stride, double* __restrict__ out, int64_t joint_stride, int n_ee,
                                                    twr_leg_kinematics K) {
  const SampleWork sw = work[blockIdx.x];
  const int lane = threadIdx.x;
  if (lane >= sw.cnt) return;
  const int s_idx = sw.s0 + lane;
  const int64_t p = sw.out_off / traj_stride;
  const double* r = traj + sw.out_off + (int64_t)s_idx * (20 + 13 * n_ee);
  double* o = out + p * joint_stride + (int64_t)s_idx * TWR_JOINT_REC(n_ee);
  o[0] = r[0];
  double R[3][3];
  base_frame_rotation(r[10], r[11], r[12], r[13], R);
  const double pb[3] = {r[1], r[2], r[3]};
  for (int e = 0; e < n_ee; ++e) {
    const double pe[3] = {r[21 + 13 * e], r[22 + 13 * e], r[23 + 13 * e]};
    double foot[3];
    base_frame(R, pb, pe, foot);
    LegIk k;
    leg_ik_of_foot(foot, e, K, k);
    put_leg(o + 1 + kJointLeg * e, k, K);
  }
}
hipError_t launch_joints(const SampleWork* work, int n_work, const double* traj, int64_t traj_stride, double* out, int64_t joint_stride,
                         int n_ee, const twr_leg_kinematics& kin, hipStream_t stream) {
  if (n_work <= 0) return hipSuccess;
  return twr_launch(joints_kernel, dim3(n_work), dim3(64), 0, stream, work, traj, traj_stride, out, joint_stride, n_ee, kin);
}

// twr_batch_joint_scores: one wave per problem folds its joint records, 64 samples per round (JointFold).  The sample count is
// GetTrajectory's: while (t <= T + 1e-5) with t accumulated.
__global__ __launch_bounds__(64) void joint_scores_kernel(const NodeWork* __restrict__ work, const double* __restrict__ joints,
                                                          int64_t joint_stride, double dt, int n_samples_max,
                                                          double* __restrict__ scores, twr_leg_kinematics K) {
  const char* blob = reinterpret_cast<const char*>(work[blockIdx.x].blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const double T = tbl<SampleTables>(blob, H->o_sample)->t_total;
  const int lane = threadIdx.x, n_ee = H->n_ee, rec = TWR_JOINT_REC(n_ee);
  const double* jp = joints + (int64_t)blockIdx.x * joint_stride;
  JointFold F;
  F.init();
  for (int s0 = 0; s0 < n_samples_max; s0 += 64) {
    const int s_idx = s0 + lane;
    double t = 0.0;
    for (int i = 0; i < s_idx; ++i) t += dt;
    const bool live = t <= T + 1e-5;
    if (!__any(live)) break;
    double q[kMaxEE][3] = {};
    double ov[kMaxEE] = {};
    int fl[kMaxEE] = {};
#pragma unroll
    for (int e = 0; e < kMaxEE; ++e)
      if (live && e < n_ee) {
        const double* l = jp + (int64_t)s_idx * rec + 1 + kJointLeg * e;
        q[e][0] = l[0]; q[e][1] = l[1]; q[e][2] = l[2];
        fl[e] = (int)l[3];
        ov[e] = l[4];
      }
    F.round(lane, s_idx, live, n_ee, q, fl, ov, dt, K);
  }
  F.finish(lane, scores + TWR_JOINT_SCORE_REC * (size_t)blockIdx.x);
}
hipError_t launch_joint_scores(const NodeWork* work, int n_problems, const double* joints, int64_t joint_stride, double dt,
                               int n_samples_max, double* scores, const twr_leg_kinematics& kin, hipStream_t stream) {
  return twr_launch(joint_scores_kernel, dim3(n_problems), dim3(64), 0, stream, work, joints, joint_stride, dt, n_samples_max, scores, kin);
}

// twr_batch_eval_joint_scores: x -> the same eight doubles without a trajectory.  One wave per problem like
// contact_plan_kernel: durations to LDS, then per round the lane's sample as sample_kernel takes it (sample_base, sample_angular,
// sample_spline with every result kept alive: the same bits), the frame change and the leg IK as joints_kernel, the fold as
// joint_scores_kernel.
__global__ __launch_bounds__(64) void eval_joint_scores_kernel(const NodeWork* __restrict__ work, const double* __restrict__ x, double dt,
                                                               int n_samples_max, double* __restrict__ scores, twr_leg_kinematics K) {
  __shared__ double s_bd[2 * kMaxPhasePolys], s_ph[kMaxEE][TWR_MAX_PHASES_DEV], s_md[kMaxEE][kMaxPhasePolys];
  const NodeWork w = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(w.blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const SampleTables* ST = tbl<SampleTables>(blob, H->o_sample);
  const double* xp = x + w.x_off;
  const int lane = threadIdx.x, n_ee = H->n_ee;
  for (int q = lane; q < ST->n_base; q += 64) s_bd[q] = tbl<double>(blob, ST->o_bdur)[q];
  for (int e = 0; e < n_ee; ++e) {
    if (H->timings) {
      phase_poly_durations_wave(tbl<PhaseTables>(blob, H->o_phase), blob, xp, e, s_ph[e], s_md[e], lane);
    } else {
      for (int q = lane; q < ST->n_mpoly[e]; q += 64) s_md[e][q] = tbl<double>(blob, ST->o_mdur[e])[q];
    }
  }
  __syncthreads();
  const double T = ST->t_total;
  JointFold F;
  F.init();
  for (int s0 = 0; s0 < n_samples_max; s0 += 64) {
    const int s_idx = s0 + lane;
    double t = 0.0;
    for (int i = 0; i < s_idx; ++i) t += dt;
    const bool live = t <= T + 1e-5;
    if (!__any(live)) break;
    double q[kMaxEE][3] = {};
    double ov[kMaxEE] = {};
    int fl[kMaxEE] = {};
    if (live) {
      BaseSample B;
      BaseAngular A;
      sample_base(xp, ST, s_bd, t, B);
      sample_angular(B, A);
#pragma unroll
      for (int d = 0; d < 3; ++d) {   // (what sample_kernel stores and this kernel has no use for)
        keep_alive(B.v[d]);
        keep_alive(B.a[d]);
        keep_alive(A.omega[d]);
        keep_alive(A.omega_dot[d]);
      }
      const double (&pb)[3] = B.p;
      double R[3][3];
      base_frame_rotation(A.q[3], A.q[0], A.q[1], A.q[2], R);
      for (int e = 0; e < n_ee; ++e) {
        double tlm, pe[3], v[3], a[3], foot[3];
        const int qm = locate_segment(s_md[e], ST->n_mpoly[e], t, tlm);
        sample_spline(xp, tbl<PolyDesc>(blob, ST->o_mdesc[e])[qm], tlm, s_md[e][qm], pe, v, a);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          keep_alive(v[d]);
          keep_alive(a[d]);
        }
        base_frame(R, pb, pe, foot);
        LegIk k;
        leg_ik_of_foot(foot, e, K, k);
        const double over = over_reach(k.r, K);
#pragma unroll
        for (int j = 0; j < kMaxEE; ++j)   // (a rolled loop over the legs, its results selected into registers)
          if (j == e) {
            q[j][0] = k.q[0]; q[j][1] = k.q[1]; q[j][2] = k.q[2];
            fl[j] = k.flags;
            ov[j] = over;
          }
      }
    }
    F.round(lane, s_idx, live, n_ee, q, fl, ov, dt, K);
  }
  F.finish(lane, scores + TWR_JOINT_SCORE_REC * (size_t)blockIdx.x);
}
hipError_t launch_eval_joint_scores(const NodeWork* work, int n_problems, const double* x, double dt, int n_samples_max, double* scores,
                                    const twr_leg_kinematics& kin, hipStream_t stream) {
  return twr_launch(eval_joint_scores_kernel, dim3(n_problems), dim3(64), 0, stream, work, x, dt, n_samples_max, scores, kin);
}

// ---------------------------------------------------------------- trajectory checks (kernels/checks.h)
// twr_batch_checks: records of sample_kernel -> check records over the same work list, one wave per item, lane = sample.
// An item's records are contiguous (64 x 576 B at four feet) but a lane's own record is 576 B from its neighbour's.  STAGED: the wave
// copies the item into LDS with coalesced loads (lane l takes doubles l, l + 64, ...), each record at an odd number of doubles from
// the next (a lane's ds_read_b64 then lands on its own bank pair), does the per-lane math from there, puts its check record into
// the same image and copies the item's check records out the same way.  One workgroup holds 64 x 73 doubles = 37,376 B at four
// feet: four waves per CU by LDS.  !STAGED: every lane reads its record from and writes its check record to global memory,
// occupancy by registers alone.  Both run check_record, so they give the same bits (tests/test_checks.py runs on either build: one,
// two and four feet against the numpy restatement; no robot of the presets has three).  Measured: the direct reads are the
// faster form on both sweeps, 0.126 against 0.216 ms and 0.019 against 0.029 ms -- at one wave per SIMD the staged wave waits for
// its own loads, its barrier and its stores in turn with nothing else to run -- so they are the default;
// make DIAG=-DTWR_CHECKS_STAGED builds the other.
#ifdef TWR_CHECKS_STAGED
constexpr bool kChecksStaged = true;
#else
constexpr bool kChecksStaged = false;
#endif
// the wave's copy between `n` contiguous doubles at g and records of kRec doubles, kPad apart, in the image: double k of the
// item is double k % kRec of record k / kRec.  A lane walks k = lane, lane + 64, ... with a running (row, col) instead of a
// division per element; check_image_walk proves at compile time, for the record sizes in use, that the walk is that map.
struct CheckImageWalk {
  int row, col;
  template <int kRec>
  __host__ __device__ constexpr void start(int lane) {
    row = lane / kRec;
    col = lane % kRec;
  }
  template <int kRec>
  __host__ __device__ constexpr void step() {
    col += 64;
    while (col >= kRec) {
      col -= kRec;
      ++row;
    }
  }
};
template <int kRec>
constexpr bool check_image_walk() {
  for (int lane = 0; lane < 64; ++lane) {
    CheckImageWalk w{0, 0};
    w.start<kRec>(lane);
    for (int k = lane; k < 64 * kRec; k += 64) {
      if (w.row != k / kRec || w.col != k % kRec) return false;
      w.step<kRec>();
    }
  }
  return true;
}
template <int kRec, int kPad, bool kIn>
TWR_DEV void check_image_copy(double* __restrict__ img, double* __restrict__ g, int n, int lane) {
  static_assert(kRec > 0 && kPad >= kRec && check_image_walk<kRec>(), "the running (row, col) of every lane is (k / kRec, k % kRec)");
  CheckImageWalk w{0, 0};
  w.start<kRec>(lane);
#pragma unroll 8
  for (int k = lane; k < n; k += 64) {
    if (kIn) img[w.row * kPad + w.col] = g[k];
    else g[k] = img[w.row * kPad + w.col];
    w.step<kRec>();
  }
}
template <int N_EE, bool STAGED>
__global__ __launch_bounds__(64) void checks_kernel(const SampleWork* __restrict__ work, const double* __restrict__ traj,
                                                    int64_t traj_stride, double* __restrict__ out, int64_t check_stride, CheckModel M) {
  constexpr int kRec = 20 + 13 * N_EE, kRecPad = kRec | 1, kOut = TWR_CHECK_REC(N_EE), kOutPad = kOut | 1;
  static_assert(kOutPad <= kRecPad, "the check records fit the image of the sample records");
  const SampleWork sw = work[blockIdx.x];
  const DevStruct* H = reinterpret_cast<const DevStruct*>(sw.blob);
  const int lane = threadIdx.x;
  const int64_t p = sw.out_off / traj_stride;
  const double* src = traj + sw.out_off + (int64_t)sw.s0 * kRec;      // the item's cnt records, and where its check records go
  double* dst = out + p * check_stride + (int64_t)sw.s0 * kOut;
  double o[kOut];
  if constexpr (STAGED) {
    __shared__ double img[64 * kRecPad];
    check_image_copy<kRec, kRecPad, true>(img, const_cast<double*>(src), sw.cnt * kRec, lane);
    __syncthreads();
    if (lane < sw.cnt) check_record<N_EE>(static_cast<const double*>(img + lane * kRecPad), H, M, o);
    __syncthreads();
    if (lane < sw.cnt) {
#pragma unroll
      for (int j = 0; j < kOut; ++j) img[lane * kOutPad + j] = o[j];
    }
    __syncthreads();
    check_image_copy<kOut, kOutPad, false>(img, dst, sw.cnt * kOut, lane);
  } else {
    if (lane >= sw.cnt) return;
    check_record<N_EE>(src + (int64_t)lane * kRec, H, M, o);
#pragma unroll
    for (int j = 0; j < kOut; ++j) dst[(int64_t)lane * kOut + j] = o[j];
  }
}
hipError_t launch_checks(const SampleWork* work, int n_work, const double* traj, int64_t traj_stride, double* out, int64_t check_stride,
                         const twr_model& model, hipStream_t stream) {
  if (n_work <= 0) return hipSuccess;
  CheckModel M;
  for (int e = 0; e < kMaxEE; ++e)
    for (int d = 0; d < 3; ++d) M.nominal[e][d] = e < model.n_ee ? model.nominal_stance[e][d] : 0.0;
  for (int d = 0; d < 3; ++d) M.max_dev[d] = model.max_dev[d];
  switch (model.n_ee) {
    case 1: return twr_launch(checks_kernel<1, kChecksStaged>, dim3(n_work), dim3(64), 0, stream, work, traj, traj_stride, out, check_stride, M);
    case 2: return twr_launch(checks_kernel<2, kChecksStaged>, dim3(n_work), dim3(64), 0, stream, work, traj, traj_stride, out, check_stride, M);
    case 3: return twr_launch(checks_kernel<3, kChecksStaged>, dim3(n_work), dim3(64), 0, stream, work, traj, traj_stride, out, check_stride, M);
    case 4: return twr_launch(checks_kernel<4, kChecksStaged>, dim3(n_work), dim3(64), 0, stream, work, traj, traj_stride, out, check_stride, M);
  }
  return hipErrorInvalidValue;
}

// twr_batch_check_scores: one wave per problem folds its check records, 64 samples per round (CheckFold); the sample count is
// GetTrajectory's, as in joint_scores_kernel.
__global__ __launch_bounds__(64) void check_scores_kernel(const NodeWork* __restrict__ work, const double* __restrict__ checks,
                                                          int64_t check_stride, double dt, int n_samples_max, double* __restrict__ scores) {
  const char* blob = reinterpret_cast<const char*>(work[blockIdx.x].blob);
  const DevStruct* H = reinterpret_cast<const DevStruct*>(blob);
  const double T = tbl<SampleTables>(blob, H->o_sample)->t_total;
  const int lane = threadIdx.x, n_ee = H->n_ee, rec = TWR_CHECK_REC(n_ee);
  const double* cp = checks + (int64_t)blockIdx.x * check_stride;
  CheckFold F;
  F.init();
  for (int s0 = 0; s0 < n_samples_max; s0 += 64) {
    const int s_idx = s0 + lane;
    double t = 0.0;
    for (int i = 0; i < s_idx; ++i) t += dt;
    const bool live = t <= T + 1e-5;
    if (!__any(live)) break;
    if (live) F.take(cp + (int64_t)s_idx * rec, n_ee);
  }
  F.finish(lane, scores + TWR_CHECK_SCORE_REC * (size_t)blockIdx.x);
}
hipError_t launch_check_scores(const NodeWork* work, int n_problems, const double* checks, int64_t check_stride, double dt,
                               int n_samples_max, double* scores, hipStream_t stream) {
  return twr_launch(check_scores_kernel, dim3(n_problems), dim3(64), 0, stream, work, checks, check_stride, dt, n_samples_max, scores);
}

// ---------------------------------------------------------------- TWR_EVAL_CHECK
// Per-problem non-finite flags (failure detection): a separate pass over the outputs of one
// evaluation, off the hot path (it re-reads g and jac once).  status[p] |= 1 if a constraint value of problem p is
// NaN/Inf, |= 2 if a Jacobian value is.  Sixteen workgroups per problem, each scanning a contiguous share.
constexpr int kCheckParts = 16;
TWR_DEV bool non_finite(double v) { return (__double2hiint(v) & 0x7ff00000) == 0x7ff00000; }
__global__ __launch_bounds__(256) void check_kernel(const int64_t* __restrict__ g_off, const int64_t* __restrict__ j_off,
                                                    const double* __restrict__ g, const double* __restrict__ jac,
                                                    int32_t* __restrict__ status, int flags) {
  const int p = blockIdx.x / kCheckParts, part = blockIdx.x % kCheckParts;
  int bad = 0;
  if (flags & 1) {
    const int64_t a = g_off[p], n = g_off[p + 1] - a;
    const int64_t lo = a + n * part / kCheckParts, hi = a + n * (part + 1) / kCheckParts;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) bad |= non_finite(g[i]) ? 1 : 0;
  }
  if (flags & 2) {
    const int64_t a = j_off[p], n = j_off[p + 1] - a;
    const int64_t lo = a + n * part / kCheckParts, hi = a + n * (part + 1) / kCheckParts;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) bad |= non_finite(jac[i]) ? 2 : 0;
  }
  if (bad) atomicOr(&status[p], bad);
}
hipError_t launch_check(int n_problems, const int64_t* g_off, const int64_t* j_off, const double* g, const double* jac,
                        int32_t* status, int flags, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n_problems, stream);
  if (e != hipSuccess) return e;
  return twr_launch(check_kernel, dim3(n_problems * kCheckParts), dim3(256), 0, stream, g_off, j_off, g, jac, status, flags);
}

// ---------------------------------------------------------------- a new grid_map layer (kernels/grid_map_update.h)
// One launch: wave w of the grid copies columns w, w + waves, ... of the layer (un-rolling the circular buffer), and thread t
// of the grid writes the new map centre into headers t, t + threads, ... of the map's list.  Every index comes from the sizes,
// the start index and that list; src is only read.
__global__ __launch_bounds__(256) void grid_map_update_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst, int size_x,
                                                              int size_y, int start_x, int start_y, double pos_x, double pos_y,
                                                              char* __restrict__ arena, const uint64_t* __restrict__ hdr_off, int n_hdr) {
  const int lane = threadIdx.x & 63, wave = blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = gridDim.x * 4;
  for (int j = wave; j < size_y; j += n_waves) grid_map_unroll_column(src, dst, size_x, size_y, start_x, start_y, j, lane);
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n_hdr; k += gridDim.x * 256) grid_map_put_centre(arena, hdr_off, k, pos_x, pos_y);
}
hipError_t launch_grid_map_update(const float* src, float* dst, int size_x, int size_y, int start_x, int start_y, double pos_x,
                                  double pos_y, void* arena, const uint64_t* hdr_off, int n_hdr, hipStream_t stream) {
  if (size_x < 1 || size_y < 1 || start_x < 0 || start_x >= size_x || start_y < 0 || start_y >= size_y || n_hdr < 0)
    return hipErrorInvalidValue;   // (the C ABI has checked all of it: nothing out of range reaches the device)
  const int want = std::max((size_y + 3) / 4, (n_hdr + 255) / 256);   // a wave per column, a thread per header
  const int blocks = std::min(std::max(want, 1), 1024);
  return twr_launch(grid_map_update_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint32_t*>(src),
                    reinterpret_cast<uint32_t*>(dst), size_x, size_y, start_x, start_y, pos_x, pos_y, static_cast<char*>(arena), hdr_off,
                    n_hdr);
}

// ---------------------------------------------------------------- x0 and variable bounds of a request (kernels/start.h)
// One workgroup per work item.  stride: doubles between two problems' request records (0: one record for all).
__global__ __launch_bounds__(kStartItem) void start_kernel(const StartWork* __restrict__ work, const double* __restrict__ request,
                                                           int64_t stride, double* __restrict__ x, double* __restrict__ lower,
                                                           double* __restrict__ upper) {
  __shared__ double s_rq[kStartRequest];
  __shared__ StartEnd s_end[kStartSplines];
  const StartWork w = work[blockIdx.x];
  const char* table = reinterpret_cast<const char*>(w.table);
  const StartHeader* H = reinterpret_cast<const StartHeader*>(table);
  const DevStruct* S = reinterpret_cast<const DevStruct*>(w.blob);
  const int t = threadIdx.x;
  if (t < kStartRequest) s_rq[t] = request[(int64_t)w.problem * stride + t];
  __syncthreads();
  if (x) {   // (the bounds need no endpoints)
    if (t < H->n_ee) start_foot_ends(H, S, s_rq, t, s_end);
    else if (t == 64) start_base_ends(H, S, s_rq, s_end);
    __syncthreads();
  }
  if (t < w.cnt)
    start_put(H, table, s_end, H->nm1, s_rq, w.v0 + t, x ? x + w.x_off : nullptr, lower ? lower + w.x_off : nullptr,
              upper ? upper + w.x_off : nullptr);
}
hipError_t launch_start(const StartWork* work, int n_work, const double* request, int64_t stride, double* x, double* lower, double* upper,
                        hipStream_t stream) {
  if (n_work < 1 || !work || !request || (!x && !lower && !upper) || stride < 0) return hipErrorInvalidValue;
  return twr_launch(start_kernel, dim3(n_work), dim3(kStartItem), 0, stream, work, request, stride, x, lower, upper);
}

}  // namespace twr
