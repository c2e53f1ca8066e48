// The Gram matrix N_p = J_p^T W_p J_p of every problem of a batch, formed once per linearisation and kept, and what runs on it
// (twr_jac_gram, twr_jac_gram_mul, twr_jac_lsq_solve_gram, include/towr_amd.h).  Tables and work lists are planned on the host
// (twr::PlanJacGram, jac_plan.h); every index comes from them, never from J, w, v or N.
//   jac_gram_kernel:      one lane per stored entry (i, j), i >= j, of the lower triangle, in the planner's order (entries sorted
//                         by the length of their lists, so the lanes of a wave do comparable work; a wave's table words lie
//                         interleaved, term t of lane l at t * 64 + l, and are read in full lines).  The lane gathers J_ri and
//                         J_rj, adds (w_r J_ri) J_rj to its sum in ascending r and stores the sum to (i, j) and to (j, i).
//   jac_gram_mul_kernel:  u = N v.  kGramRowLanes lanes share a row: lane l adds the products l, l + 16, ... in column order, then
//                         a butterfly over the 16 lanes (both partners of a step add the same two numbers).
//   gram_cg_kernel:       the whole solve (C N C + mu I) e = c o z, d = c o e of one problem in one workgroup: e, s, p, c, c o p and
//                         N (c o p) in LDS, the rows of N streamed once per iteration by the row product above, the two dots of an
//                         iteration by lsq_sum (lsq.h).  A problem that has stopped leaves the loop and its workgroup ends.
// No atomics; the order of every sum is a function of the pattern alone.  The row product and the CG multiply, then add (no fused
// multiply-add: `fp contract(off)` in their bodies), every sum in the order stated here, so that the numpy restatement
// (scripts/gram_cpu.py gram_cg_device) takes the same roundings in the same order and stops at the same iteration.
// Included by jac_tu.hip alone, which holds the launchers (jac_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "lsq.h"
#include "products.h"
#include "../jac_plan.h"

namespace twr {

static_assert(kGramThreads == kLsqThreads, "gram_cg_kernel sums with lsq_sum");
static_assert(kGramSlice == 64, "a slice is a wave");

__global__ __launch_bounds__(kGramThreads) void jac_gram_kernel(const JacGramWork* __restrict__ work, const double* __restrict__ jac,
                                                                const double* __restrict__ w, double* __restrict__ gram) {
  const JacGramWork W = work[blockIdx.x];
  const int e = W.e0 + (int)threadIdx.x;
  if (e >= W.e1) return;
  const int cnt = jac_table<int32_t>(W.cnt)[e];
  const uint64_t* word = jac_table<uint64_t>(W.words) + jac_table<int32_t>(W.slice_ptr)[e / kGramSlice] + e % kGramSlice;
  const double* J = jac + W.j_off;
  const double* wp = w ? w + W.g_off : nullptr;
  double acc = 0.0;
  for (int t = 0; t < cnt; ++t) {
    const uint64_t x = word[(int64_t)t * kGramSlice];
    const double a = J[(x >> 24) & 0xffffffu], b = J[x & 0xffffffu];
    acc = fma(wp ? wp[x >> 48] * a : a, b, acc);
  }
  double* N = gram + W.gram_off;
  const int pos = jac_table<int32_t>(W.pos)[e], mirror = jac_table<int32_t>(W.mirror)[e];
  N[pos] = acc;
  if (mirror != pos) N[mirror] = acc;
}

// The sum over row [k0, k1) of N of val[k] * v[col[k]], the same bits in all kGramRowLanes lanes of the row's group
template <class V>
__device__ inline double gram_row_dot(const double* __restrict__ val, const uint16_t* __restrict__ col, int k0, int k1, V v) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int k = k0 + (int)(threadIdx.x % kGramRowLanes); k < k1; k += kGramRowLanes) acc = acc + val[k] * v[col[k]];
#pragma unroll
  for (int s = kGramRowLanes / 2; s >= 1; s >>= 1) acc += __shfl_xor(acc, s, 64);
  return acc;
}

__global__ __launch_bounds__(kGramThreads) void jac_gram_mul_kernel(const JacGramMulWork* __restrict__ work, const double* __restrict__ gram,
                                                                    const double* __restrict__ v, double* __restrict__ u) {
  const JacGramMulWork W = work[blockIdx.x];
  const int32_t* rp = jac_table<int32_t>(W.row_ptr);
  const uint16_t* col = jac_table<uint16_t>(W.col);
  const double* N = gram + W.gram_off;
  const double* vp = v + W.x_off;
  // (every group of a wave takes the same number of turns: the butterfly never meets a lane that has left)
  for (int r = W.r0 + (int)threadIdx.x / kGramRowLanes; r < W.r0 + kGramThreads; r += kGramThreads / kGramRowLanes) {
    const bool mine = r < W.r1;
    const double sum = gram_row_dot(N, col, mine ? rp[r] : 0, mine ? rp[r + 1] : 0, vp);
    if (mine && threadIdx.x % kGramRowLanes == 0) u[W.x_off + r] = sum;
  }
}

// lds: six vectors of max_n doubles, then kGramRed doubles for lsq_sum
__global__ __launch_bounds__(kGramThreads) void gram_cg_kernel(const JacGramSolveWork* __restrict__ work, const double* __restrict__ gram,
                                                               const double* __restrict__ z, const double* __restrict__ mu,
                                                               const double* __restrict__ scale, int iters, double tol2,
                                                               double* __restrict__ d, double* __restrict__ info, int max_n) {
#pragma clang fp contract(off)
  extern __shared__ double gram_lds[];
  const JacGramSolveWork W = work[blockIdx.x];
  const int n = W.n, tid = (int)threadIdx.x;
  double* e = gram_lds;
  double* s = e + max_n;
  double* p = s + max_n;
  double* c = p + max_n;
  double* cp = c + max_n;
  double* t = cp + max_n;
  double* red = t + max_n;
  const int32_t* rp = jac_table<int32_t>(W.row_ptr);
  const uint16_t* col = jac_table<uint16_t>(W.col);
  const double* N = gram + W.gram_off;
  const double* zp = z + W.x_off;
  double* dp = d + W.x_off;
  double* o = info + 4 * (int64_t)blockIdx.x;
  const double m_u = mu[blockIdx.x];
  // s = c o z over the free variables (an exact +0 where c_k == 0, whatever z_k holds), gamma0, the checks of mu and c
  double acc[2] = {0.0, 0.0};   // s^T s, the bad c_k
  for (int i = tid; i < n; i += kGramThreads) {
    const double ck = scale ? scale[W.x_off + i] : 1.0;
    if (!(ck >= 0.0) || !lsq_finite(ck)) acc[1] += 1.0;
    const double sk = ck == 0.0 ? 0.0 : ck * zp[i];
    c[i] = ck, s[i] = sk, p[i] = sk, e[i] = 0.0;
    cp[i] = ck == 0.0 ? 0.0 : ck * sk;
    acc[0] = acc[0] + sk * sk;
    dp[i] = 0.0;
  }
  lsq_sum(acc, red);   // (its barriers also publish the vectors)
  const double g0 = acc[0];
  double gamma = g0, state = kLsqRunning;
  if (!(m_u >= 0.0) || !lsq_finite(m_u) || !lsq_finite(g0) || acc[1] != 0.0) state = 2.0;
  else if (g0 <= tol2 * g0) state = 0.0;   // |s0| = 0 (z = 0, no rows), or tol >= 1
  int k = 0;
  while (state == kLsqRunning && k < iters) {
    // t = N (c o p), a row per group of lanes; every lane of a wave takes the same number of turns
    for (int r0 = 0; r0 < n; r0 += kGramThreads / kGramRowLanes) {
      const int r = r0 + tid / kGramRowLanes;
      const bool mine = r < n;
      const double sum = gram_row_dot(N, col, mine ? rp[r] : 0, mine ? rp[r + 1] : 0, cp);
      if (mine && tid % kGramRowLanes == 0) t[r] = sum;
    }
    __syncthreads();
    double dots[2] = {0.0, 0.0};   // p^T u with u = c o t, p^T p
    for (int i = tid; i < n; i += kGramThreads) {
      const double uk = c[i] == 0.0 ? 0.0 : c[i] * t[i];
      t[i] = uk;   // (the lane's own elements from here on)
      dots[0] = dots[0] + p[i] * uk;
      dots[1] = dots[1] + p[i] * p[i];
    }
    lsq_sum(dots, red);
    const double delta = dots[0] + m_u * dots[1];
    if (!(delta > 0.0) || !lsq_finite(delta)) {   // NaN, Inf, or no curvature along p: alpha would not be a number
      state = 2.0;
      break;
    }
    const double alpha = gamma / delta;
    double gs[1] = {0.0};
    for (int i = tid; i < n; i += kGramThreads) {
      e[i] = e[i] + alpha * p[i];
      const double sn = s[i] - alpha * (m_u * p[i] + t[i]);
      s[i] = sn;
      gs[0] = gs[0] + sn * sn;
    }
    lsq_sum(gs, red);
    const double gn = gs[0];
    ++k;
    double beta = 0.0;
    if (!lsq_finite(gn)) state = 2.0;
    else if (gn <= tol2 * g0) state = 0.0;
    else beta = gn / gamma;
    gamma = gn;
    if (state != kLsqRunning) break;
    for (int i = tid; i < n; i += kGramThreads) {
      const double pn = s[i] + beta * p[i];
      p[i] = pn;
      cp[i] = c[i] == 0.0 ? 0.0 : c[i] * pn;
    }
    __syncthreads();   // c o p is read by every group
  }
  if (k > 0)
    for (int i = tid; i < n; i += kGramThreads) dp[i] = c[i] == 0.0 ? 0.0 : c[i] * e[i];
  if (tid == 0) {
    lsq_info(o, (double)k, gamma, g0, state);
  }
}

}  // namespace twr
