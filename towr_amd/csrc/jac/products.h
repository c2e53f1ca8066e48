// Products with a batch's Jacobian values, per problem p (twr_jac_mul / twr_jac_tmul, include/towr_amd.h):
//   jac_mul_kernel:                    y[g_off[p] + r] = sum_k J_p[r][k] v[x_off[p] + k]
//   jac_tmul_kernel + jac_fold_kernel: z[x_off[p] + k] = sum_r J_p[r][k] w[g_off[p] + r]
//   jac_colsq_kernel + jac_fold_kernel: c[x_off[p] + k] = sum_r w[g_off[p] + r] J_p[r][k]^2   (twr_jac_col_sqnorms)
//   jac_normal_kernel + jac_fold_kernel: u = J_p^T (w o (J_p v)) and y = J_p v from one pass over J_p   (twr_jac_normal_mul;
//                                        twr::PlanJacNormal)
// The work split, the tables and the order of every sum are planned on the host (twr::PlanJacOps, jac_plan.h).  No atomics:
// every output is written by exactly one lane, which sums its terms in an order fixed by the pattern alone, so a problem's
// outputs have the same bits wherever it sits in whatever batch.  Every index comes from the plan's tables; J, v and w are
// only multiplied and added, so a NaN or Inf in one problem's inputs reaches that problem's outputs and no other's.
// Included by jac_tu.hip alone, which holds the launchers (jac_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include <tuple>

#include "../jac_plan.h"

namespace twr {

template <typename T>
__device__ inline const T* jac_table(uint64_t addr) {
  return reinterpret_cast<const T*>(addr);
}

// Stages the values jac[k0 .. k1) of one problem: op(i, value) for i = k - k0.  Aligned pairs inside the range are read with
// 16-byte loads, four per lane in flight; an end of the range that cuts a pair is read alone (never a neighbour's value).
template <class Op>
__device__ inline void jac_stream(const double* __restrict__ jac, int64_t k0, int64_t k1, Op op) {
  if (k0 >= k1) return;
  const int64_t head = (reinterpret_cast<uintptr_t>(jac + k0) & 15) ? 1 : 0;
  const int64_t s = k0 + head, npair = (k1 - s) / 2;
  if (head && threadIdx.x == 0) op(0, jac[k0]);
  if (s + 2 * npair < k1 && threadIdx.x == kJacThreads - 1) op((int)(k1 - 1 - k0), jac[k1 - 1]);
  const double2* p = reinterpret_cast<const double2*>(jac + s);
  const int base = (int)(s - k0);
  constexpr int U = 4;
  for (int64_t q0 = threadIdx.x; q0 < npair; q0 += U * kJacThreads) {
    double2 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t q = q0 + u * kJacThreads;
      if (q < npair) v[u] = p[q];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t q = q0 + u * kJacThreads;
      if (q < npair) {
        op(base + 2 * (int)q, v[u].x);
        op(base + 2 * (int)q + 1, v[u].y);
      }
    }
  }
}

// y = J v over the rows [r0, r1) of one problem: lane t owns row r0 + t and adds its products in column order, tile by tile.
template <bool kStaged>
__device__ inline void jac_mul_block(const JacMulWork& w, const double* __restrict__ jac, const double* __restrict__ v,
                                     double* __restrict__ y, double* prod, double* vs) {
  const uint16_t* col = jac_table<uint16_t>(w.col);
  const int32_t* rp = jac_table<int32_t>(w.row_ptr);
  const double* vp = v + w.x_off;
  if (kStaged) {
    for (int i = threadIdx.x; i < w.n; i += kJacThreads) vs[i] = vp[i];
    __syncthreads();
  }
  const int r = w.r0 + (int)threadIdx.x;
  const bool mine = r < w.r1;
  const int rs = mine ? rp[r] : 0, re = mine ? rp[r + 1] : 0;
  const int b0 = rp[w.r0], b1 = rp[w.r1];
  const double* J = jac + w.j_off;
  double acc = 0.0;
  for (int t0 = b0; t0 < b1; t0 += kJacMulNnz) {
    const int t1 = min(b1, t0 + kJacMulNnz);
    jac_stream(J, t0, t1, [&](int i, double a) { prod[i] = a * (kStaged ? vs[col[t0 + i]] : vp[col[t0 + i]]); });
    __syncthreads();
    const int a = max(rs, t0), b = min(re, t1);
    for (int k = a; k < b; ++k) acc += prod[k - t0];
    __syncthreads();
  }
  if (mine) y[w.g_off + r] = acc;
}

__global__ __launch_bounds__(kJacThreads) void jac_mul_kernel(const JacMulWork* __restrict__ work, const double* __restrict__ jac,
                                                              const double* __restrict__ v, double* __restrict__ y, int lds_x) {
  extern __shared__ double jac_lds[];   // kJacMulNnz products, then the problem's v (lds_x doubles)
  const JacMulWork w = work[blockIdx.x];
  if (w.n <= lds_x) jac_mul_block<true>(w, jac, v, y, jac_lds, jac_lds + kJacMulNnz);
  else jac_mul_block<false>(w, jac, v, y, jac_lds, nullptr);
}

// One partial of z = J^T w per column of the entries [k0, k1) of one problem: the values times their row's w in LDS, then lane
// j adds the products of the block's j-th column in row order.  kSquare: the values are squared as they are staged and wv may be
// NULL (unit weights): one partial of the weighted squared column norms (twr_jac_col_sqnorms).
template <bool kSquare>
__device__ inline void jac_tmul_block(const JacTWork& t, const double* __restrict__ jac, const double* __restrict__ wv,
                                      double* __restrict__ slab, double* vals, double* ws) {
  if (kSquare && !wv) {
    for (int i = threadIdx.x; i < t.span; i += kJacThreads) ws[i] = 1.0;
  } else {
    const double* wp = wv + t.g_off + t.r_first;
    for (int i = threadIdx.x; i < t.span; i += kJacThreads) ws[i] = wp[i];
  }
  jac_stream(jac + t.j_off, t.k0, t.k1, [&](int i, double a) { vals[i] = kSquare ? a * a : a; });
  __syncthreads();
  const int32_t* rp = jac_table<int32_t>(t.row_ptr);
  for (int i = threadIdx.x; i < t.span; i += kJacThreads) {
    const int r = t.r_first + i, a = max(rp[r], t.k0), b = min(rp[r + 1], t.k1);
    for (int k = a; k < b; ++k) vals[k - t.k0] *= ws[i];
  }
  __syncthreads();
  if ((int)threadIdx.x < t.ncols) {
    const uint16_t* map = jac_table<uint16_t>(t.map);
    const uint16_t* pos = map + t.ncols + 1;
    const int a = map[threadIdx.x], b = map[threadIdx.x + 1];
    double acc = 0.0;
    for (int i = a; i < b; ++i) acc += vals[pos[i]];
    slab[t.slab + threadIdx.x] = acc;
  }
}

__global__ __launch_bounds__(kJacThreads) void jac_tmul_kernel(const JacTWork* __restrict__ work, const double* __restrict__ jac,
                                                               const double* __restrict__ wv, double* __restrict__ slab) {
  __shared__ double vals[kJacTNnz];
  __shared__ double ws[kJacTSpan];
  jac_tmul_block<false>(work[blockIdx.x], jac, wv, slab, vals, ws);
}

__global__ __launch_bounds__(kJacThreads) void jac_colsq_kernel(const JacTWork* __restrict__ work, const double* __restrict__ jac,
                                                                const double* __restrict__ wv, double* __restrict__ slab) {
  __shared__ double vals[kJacTNnz];
  __shared__ double ws[kJacTSpan];
  jac_tmul_block<true>(work[blockIdx.x], jac, wv, slab, vals, ws);
}

// z[c] = the partials of column c in block order; 0 for a column without entries.
__global__ __launch_bounds__(kJacFoldCols) void jac_fold_kernel(const JacFoldWork* __restrict__ work, const double* __restrict__ slab,
                                                                double* __restrict__ z) {
  const JacFoldWork f = work[blockIdx.x];
  const int c = f.c0 + (int)threadIdx.x;
  if (c >= f.c1) return;
  const int32_t* ptr = jac_table<int32_t>(f.ptr);
  const int32_t* slot = jac_table<int32_t>(f.slot);
  double acc = 0.0;
  for (int i = ptr[c]; i < ptr[c + 1]; ++i) acc += slab[f.slab + slot[i]];
  z[f.x_off + c] = acc;
}

// One pass over the rows [r0, r1) of one problem for u = J^T (w o (J v)) (twr_jac_normal_mul; twr::PlanJacNormal): the block's
// values are read once, kept raw in `vals` and multiplied by v[col] in `prod`.  Lane t owns row r0 + t: it adds the row's products
// in column order (y_r), forms t_r = w_r y_r and multiplies the row's raw values by it (its own entries: no barrier in between).
// The column lanes then loop over the block's columns, each adding its column's products in row order into one partial.
template <bool kStaged>
__device__ inline void jac_normal_block(const JacNormalWork& w, const double* __restrict__ jac, const double* __restrict__ wv,
                                        const double* __restrict__ v, double* __restrict__ y, double* __restrict__ slab, int tile,
                                        double* prod, double* vals, double* vs) {
  const uint16_t* col = jac_table<uint16_t>(w.col);
  const int32_t* rp = jac_table<int32_t>(w.row_ptr);
  const double* vp = v + w.x_off;
  if (kStaged) {
    for (int i = threadIdx.x; i < w.n; i += kJacThreads) vs[i] = vp[i];
    __syncthreads();
  }
  const double* J = jac + w.j_off;
  const int b0 = rp[w.r0], b1 = rp[w.r1];
  if (w.is_long) {   // one row of more than a tile: lane 0 adds the tiles' products in column order, then a partial per entry
    double acc = 0.0;
    for (int t0 = b0; t0 < b1; t0 += tile) {
      const int t1 = min(b1, t0 + tile);
      jac_stream(J, t0, t1, [&](int i, double a) { prod[i] = a * (kStaged ? vs[col[t0 + i]] : vp[col[t0 + i]]); });
      __syncthreads();
      if (threadIdx.x == 0)
        for (int k = 0; k < t1 - t0; ++k) acc += prod[k];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      if (y) y[w.g_off + w.r0] = acc;
      vals[0] = wv ? wv[w.g_off + w.r0] * acc : acc;
    }
    __syncthreads();
    const double t = vals[0];
    double* out = slab + w.slab;
    jac_stream(J, b0, b1, [&](int i, double a) { out[i] = a * t; });
    return;
  }
  jac_stream(J, b0, b1, [&](int i, double a) {
    vals[i] = a;
    prod[i] = a * (kStaged ? vs[col[b0 + i]] : vp[col[b0 + i]]);
  });
  __syncthreads();
  const int r = w.r0 + (int)threadIdx.x;
  if (r < w.r1) {
    const int a = rp[r] - b0, b = rp[r + 1] - b0;
    double acc = 0.0;
    for (int k = a; k < b; ++k) acc += prod[k];
    if (y) y[w.g_off + r] = acc;
    const double t = wv ? wv[w.g_off + r] * acc : acc;
    for (int k = a; k < b; ++k) vals[k] *= t;
  }
  __syncthreads();
  const uint16_t* map = jac_table<uint16_t>(w.map);
  const uint16_t* pos = map + w.ncols + 1;
  for (int j = threadIdx.x; j < w.ncols; j += kJacThreads) {
    const int a = map[j], b = map[j + 1];
    double acc = 0.0;
    for (int i = a; i < b; ++i) acc += vals[pos[i]];
    slab[w.slab + j] = acc;
  }
}

__global__ __launch_bounds__(kJacThreads) void jac_normal_kernel(const JacNormalWork* __restrict__ work, const double* __restrict__ jac,
                                                                 const double* __restrict__ wv, const double* __restrict__ v,
                                                                 double* __restrict__ y, double* __restrict__ slab, int lds_x,
                                                                 int tile) {
  extern __shared__ double jac_lds[];   // `tile` products, `tile` raw values (the plan's tile), then the problem's v (lds_x doubles)
  const JacNormalWork w = work[blockIdx.x];
  if (w.n <= lds_x) jac_normal_block<true>(w, jac, wv, v, y, slab, tile, jac_lds, jac_lds + tile, jac_lds + 2 * tile);
  else jac_normal_block<false>(w, jac, wv, v, y, slab, tile, jac_lds, jac_lds + tile, nullptr);
}

// hipLaunchKernel returns the launch's status instead of leaving it in the thread's sticky error slot
template <typename... P, typename... A>
inline hipError_t jac_launch(void (*kern)(P...), int grid, int block, size_t lds, hipStream_t stream, A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
  std::tuple<P...> vals{static_cast<P>(args)...};
  return std::apply(
      [&](auto&... a) {
        void* ptrs[] = {static_cast<void*>(&a)...};
        return hipLaunchKernel(reinterpret_cast<const void*>(kern), dim3(grid), dim3(block), ptrs, lds, stream);
      },
      vals);
}

}  // namespace twr
