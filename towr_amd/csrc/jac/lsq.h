// The damped weighted least-squares step with a batch's Jacobian values, per problem p (twr_jac_lsq_solve, include/towr_amd.h):
//   d_p = argmin_d  sum_r w_r (J_p d - b_p)_r^2 + mu_p |d|^2      <=>   (J_p^T W_p J_p + mu_p I) d_p = J_p^T W_p b_p
// by CGLS on top of the two products of products.h (used as they are), and what feeds it: the bound-violation residual
// (twr_jac_violation) and per-problem dot products (twr_jac_dot).  One workgroup of kLsqThreads lanes per problem in every kernel
// here; the work records, the workspace and the bound tables are planned on the host (twr::PlanJacLsq, jac_plan.h).
//   lsq_start_kernel:  d = 0, r = b, t = w o r                                   (then z = J^T t by the product kernels)
//   lsq_dir_kernel:    s = z - mu d, gamma' = s^T s; first: gamma0 = gamma', p = s; later: beta = gamma' / gamma, convergence
//                      test, p = s + beta p; writes the problem's info                (then q = J p)
//   lsq_step_kernel:   delta = q^T (w o q) + mu p^T p, alpha = gamma / delta, d += alpha p, r -= alpha q, t = w o r
// The Marquardt-scaled step (twr_jac_col_scale, twr_jac_lsq_solve_scaled): (J^T W J + mu C^-2) d = J^T W b, C = diag(c), is the
// same iteration on J C in e = d / c.  The three kernels above are thin wrappers of bodies templated on SCALED; their _scaled
// siblings read c, keep e and c o p (for J to read) in a second workspace and write d = c o e; the products are used as they are.
//   lsq_col_scale_kernel:  c_k = 1 / sqrt(max(a_k, rel_floor max_k a_k)) from the squared column norms (or their running maximum)
// The one-pass solve (twr_jac_lsq_solve_onepass) recurs s instead and needs one vector kernel per iteration (lsq_onepass_kernel).
// Every scalar (alpha, beta, gamma, mu, the state) stays on the device: the launch sequence depends on `iters` alone.  A problem
// that has stopped (converged, or bad input) is skipped by its workgroup in every later kernel: its d, r, p no longer change.
// No atomics: every sum is taken by lsq_sum in an order fixed by the vector's length (jac_plan.h), so a problem's outputs have
// the same bits wherever it sits in whatever batch.  Every index comes from the work record, never from the data.
// Included by jac_tu.hip alone, which holds the launchers (jac_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "products.h"
#include "../jac_plan.h"

namespace twr {

// The pair (a[i], a[i + 1]) of a vector of `len` doubles, i even: one 16-byte load where the vector starts on a 16-byte boundary
// (al; offsets in the batch layout are only 8-byte aligned in general), else two 8-byte loads.  The element behind the end reads
// as 0 and is never used in a sum or stored.
__device__ inline bool lsq_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__device__ inline double2 lsq_ld(const double* __restrict__ a, int i, int len, bool al) {
  if (i + 1 < len) {
    if (al) return *reinterpret_cast<const double2*>(a + i);
    return make_double2(a[i], a[i + 1]);
  }
  return make_double2(a[i], 0.0);
}
__device__ inline void lsq_st(double* __restrict__ a, int i, int len, bool al, double2 v) {
  if (i + 1 < len) {
    if (al) *reinterpret_cast<double2*>(a + i) = v;
    else a[i] = v.x, a[i + 1] = v.y;
  } else {
    a[i] = v.x;
  }
}

// A lane's sum over its pairs: acc += a.x b.x, then a.y b.y where the pair is whole, in this order; weighted: a (w b)
__device__ inline void lsq_add(double& acc, double2 a, double2 b, int i, int len) {
  acc += a.x * b.x;
  if (i + 1 < len) acc += a.y * b.y;
}
__device__ inline void lsq_add(double& acc, double2 a, double2 w, double2 b, int i, int len) {
  acc += a.x * (w.x * b.x);
  if (i + 1 < len) acc += a.y * (w.y * b.y);
}

// Sums of K values over the workgroup, the same bits in every lane: a butterfly over the wave (both partners of a step add the
// same two numbers), lane 0 of every wave to LDS, then the waves' partials in wave order.  red: K * (kLsqThreads / 64) doubles.
template <int K>
__device__ inline void lsq_sum(double (&v)[K], double* red) {
  constexpr int kWaves = kLsqThreads / 64;
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v[k] += __shfl_xor(v[k], s, 64);
  const int wave = threadIdx.x / 64;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double acc = red[k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) acc += red[w * K + k];
    v[k] = acc;
  }
  __syncthreads();   // red may be written again
}

// out[p] = sum_i a_i b_i over the x layout (space 0) or the g layout
__global__ __launch_bounds__(kLsqThreads) void lsq_dot_kernel(const JacLsqWork* __restrict__ work, int space,
                                                              const double* __restrict__ a, const double* __restrict__ b,
                                                              double* __restrict__ out) {
  __shared__ double red[kLsqThreads / 64];
  const JacLsqWork W = work[blockIdx.x];
  const int len = space == 0 ? W.n : W.m;
  const int64_t off = space == 0 ? W.x_off : W.g_off;
  const double* ap = a + off;
  const double* bp = b + off;
  const bool aa = lsq_aligned(ap), ab = lsq_aligned(bp);
  double acc[1] = {0.0};
  for (int i = 2 * (int)threadIdx.x; i < len; i += 2 * kLsqThreads) {
    const double2 x = lsq_ld(ap, i, len, aa), y = lsq_ld(bp, i, len, ab);
    lsq_add(acc[0], x, y, i, len);
  }
  lsq_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc[0];
}

// r = g - min(max(g, lower), upper), a NaN g staying NaN; w_active = w [r != 0]; merit = 1/2 sum_i w_i r_i^2 (w NULL: 1)
__device__ inline double lsq_viol(double g, double lo, double hi) {
  double c = g < lo ? lo : g;
  c = c > hi ? hi : c;
  return g - c;
}
__global__ __launch_bounds__(kLsqThreads) void lsq_violation_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ g,
                                                                    const double* __restrict__ w, double* __restrict__ r,
                                                                    double* __restrict__ w_active, double* __restrict__ merit) {
  __shared__ double red[kLsqThreads / 64];
  const JacLsqWork W = work[blockIdx.x];
  const int m = W.m;
  const double* gp = g + W.g_off;
  const double* wp = w ? w + W.g_off : nullptr;
  double* rp = r + W.g_off;
  double* ap = w_active ? w_active + W.g_off : nullptr;
  const double* lo = jac_table<double>(W.lower);
  const double* hi = jac_table<double>(W.upper);
  const bool ag = lsq_aligned(gp), aw = lsq_aligned(wp), ar = lsq_aligned(rp), aa = lsq_aligned(ap), al = lsq_aligned(lo),
             ah = lsq_aligned(hi);
  double acc[1] = {0.0};
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 gv = lsq_ld(gp, i, m, ag), l = lsq_ld(lo, i, m, al), h = lsq_ld(hi, i, m, ah);
    const double2 wv = wp ? lsq_ld(wp, i, m, aw) : make_double2(1.0, 1.0);
    const double2 rv = make_double2(lsq_viol(gv.x, l.x, h.x), lsq_viol(gv.y, l.y, h.y));
    lsq_st(rp, i, m, ar, rv);
    if (ap) lsq_st(ap, i, m, aa, make_double2(wv.x * (rv.x != 0.0 ? 1.0 : 0.0), wv.y * (rv.y != 0.0 ? 1.0 : 0.0)));
    acc[0] += wv.x * (rv.x * rv.x);   // (written out: through lsq_add the kernel's code differs)
    if (i + 1 < m) acc[0] += wv.y * (rv.y * rv.y);
  }
  if (!merit) return;
  lsq_sum(acc, red);
  if (threadIdx.x == 0) merit[blockIdx.x] = 0.5 * acc[0];
}

// d = 0, r = b, t = w o r (w NULL: t = r), and the problem's state: running.  SCALED: e = 0 as well.
template <bool SCALED>
__device__ inline void lsq_start_body(const JacLsqWork* __restrict__ work, double* __restrict__ rec, const double* __restrict__ b,
                                      const double* __restrict__ w, double* __restrict__ d, double* __restrict__ e,
                                      double* __restrict__ r, double* __restrict__ t) {
  const JacLsqWork W = work[blockIdx.x];
  double* dp = d + W.x_off;
  const bool ad = lsq_aligned(dp);
  for (int i = 2 * (int)threadIdx.x; i < W.n; i += 2 * kLsqThreads) lsq_st(dp, i, W.n, ad, make_double2(0.0, 0.0));
  if constexpr (SCALED) {
    double* ep = e + W.x_off;
    const bool ae = lsq_aligned(ep);
    for (int i = 2 * (int)threadIdx.x; i < W.n; i += 2 * kLsqThreads) lsq_st(ep, i, W.n, ae, make_double2(0.0, 0.0));
  }
  const double* bp = b + W.g_off;
  const double* wp = w ? w + W.g_off : nullptr;
  double* rp = r + W.g_off;
  double* tp = t + W.g_off;
  const bool ab = lsq_aligned(bp), aw = lsq_aligned(wp), ar = lsq_aligned(rp), at = lsq_aligned(tp);
  for (int i = 2 * (int)threadIdx.x; i < W.m; i += 2 * kLsqThreads) {
    const double2 bv = lsq_ld(bp, i, W.m, ab);
    const double2 wv = wp ? lsq_ld(wp, i, W.m, aw) : make_double2(1.0, 1.0);
    lsq_st(rp, i, W.m, ar, bv);
    lsq_st(tp, i, W.m, at, wp ? make_double2(wv.x * bv.x, wv.y * bv.y) : bv);
  }
  if (threadIdx.x == 0) rec[(int64_t)kLsqRec * blockIdx.x + kLsqState] = kLsqRunning;
}
__global__ __launch_bounds__(kLsqThreads) void lsq_start_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                const double* __restrict__ b, const double* __restrict__ w,
                                                                double* __restrict__ d, double* __restrict__ r, double* __restrict__ t) {
  lsq_start_body<false>(work, rec, b, w, d, nullptr, r, t);
}
__global__ __launch_bounds__(kLsqThreads) void lsq_start_scaled_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                       const double* __restrict__ b, const double* __restrict__ w,
                                                                       double* __restrict__ d, double* __restrict__ e,
                                                                       double* __restrict__ r, double* __restrict__ t) {
  lsq_start_body<true>(work, rec, b, w, d, e, r, t);
}

__device__ inline bool lsq_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and Inf

// A problem's info record: iterations, |s| / |s0|, |s0|, status (still running when the last launch has gone by: the iteration cap)
__device__ inline void lsq_info(double* o, double iters, double gn, double g0, double state) {
  o[0] = iters;
  o[1] = g0 == 0.0 ? 0.0 : sqrt(gn / g0);
  o[2] = sqrt(g0);
  o[3] = state == kLsqRunning ? 1.0 : state;
}

// After q = J p.  A problem that is running: delta, alpha, the three updates and the next J^T's input.  SCALED (q = J (c o p)):
// the update is e += alpha p, and d = c o e is written beside it.
template <bool SCALED>
__device__ inline void lsq_step_body(const JacLsqWork* __restrict__ work, double* __restrict__ rec, const double* __restrict__ mu,
                                     const double* __restrict__ q, const double* __restrict__ w, const double* __restrict__ p,
                                     const double* __restrict__ c, double* __restrict__ e, double* __restrict__ d,
                                     double* __restrict__ r, double* __restrict__ t, double* red) {
  double* rc = rec + (int64_t)kLsqRec * blockIdx.x;
  if (rc[kLsqState] != kLsqRunning) return;   // the whole workgroup: every lane reads the same word, written by an earlier launch
  const double gamma = rc[kLsqGamma], m_u = mu[blockIdx.x];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n, m = W.m;
  const double* qp = q + W.g_off;
  const double* wp = w ? w + W.g_off : nullptr;
  const double* pp = p + W.x_off;
  double* dp = d + W.x_off;
  double* rp = r + W.g_off;
  double* tp = t + W.g_off;
  const bool aq = lsq_aligned(qp), aw = lsq_aligned(wp), ap = lsq_aligned(pp), ad = lsq_aligned(dp), ar = lsq_aligned(rp),
             at = lsq_aligned(tp);
  double acc[2] = {0.0, 0.0};   // q^T (w o q), p^T p
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 qv = lsq_ld(qp, i, m, aq);
    const double2 wv = wp ? lsq_ld(wp, i, m, aw) : make_double2(1.0, 1.0);
    lsq_add(acc[0], qv, wv, qv, i, m);
  }
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 pv = lsq_ld(pp, i, n, ap);
    lsq_add(acc[1], pv, pv, i, n);
  }
  lsq_sum(acc, red);
  const double delta = acc[0] + m_u * acc[1];
  if (!(delta > 0.0) || !lsq_finite(delta)) {   // NaN, Inf, or no curvature along p: alpha would not be a number
    if (threadIdx.x == 0) rc[kLsqState] = 2.0;
    return;
  }
  const double alpha = gamma / delta;
  if constexpr (SCALED) {
    const double* cp = c + W.x_off;
    double* ep = e + W.x_off;
    const bool ac = lsq_aligned(cp), ae = lsq_aligned(ep);
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 pv = lsq_ld(pp, i, n, ap), ev = lsq_ld(ep, i, n, ae), cv = lsq_ld(cp, i, n, ac);
      const double2 en = make_double2(fma(alpha, pv.x, ev.x), fma(alpha, pv.y, ev.y));
      lsq_st(ep, i, n, ae, en);
      lsq_st(dp, i, n, ad, make_double2(cv.x * en.x, cv.y * en.y));
    }
  } else {
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 pv = lsq_ld(pp, i, n, ap), dv = lsq_ld(dp, i, n, ad);
      lsq_st(dp, i, n, ad, make_double2(fma(alpha, pv.x, dv.x), fma(alpha, pv.y, dv.y)));
    }
  }
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 qv = lsq_ld(qp, i, m, aq), rv = lsq_ld(rp, i, m, ar);
    const double2 rn = make_double2(fma(-alpha, qv.x, rv.x), fma(-alpha, qv.y, rv.y));
    lsq_st(rp, i, m, ar, rn);
    if (wp) {
      const double2 wv = lsq_ld(wp, i, m, aw);
      lsq_st(tp, i, m, at, make_double2(wv.x * rn.x, wv.y * rn.y));
    } else {
      lsq_st(tp, i, m, at, rn);
    }
  }
  if (threadIdx.x == 0) rc[kLsqIters] += 1.0;
}
__global__ __launch_bounds__(kLsqThreads) void lsq_step_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                               const double* __restrict__ mu, const double* __restrict__ q,
                                                               const double* __restrict__ w, const double* __restrict__ p,
                                                               double* __restrict__ d, double* __restrict__ r, double* __restrict__ t) {
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_step_body<false>(work, rec, mu, q, w, p, nullptr, nullptr, d, r, t, red);
}
__global__ __launch_bounds__(kLsqThreads) void lsq_step_scaled_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                      const double* __restrict__ mu, const double* __restrict__ q,
                                                                      const double* __restrict__ w, const double* __restrict__ p,
                                                                      const double* __restrict__ c, double* __restrict__ e,
                                                                      double* __restrict__ d, double* __restrict__ r,
                                                                      double* __restrict__ t) {
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_step_body<true>(work, rec, mu, q, w, p, c, e, d, r, t, red);
}

// After z = J^T t.  s = z - mu d (kept in LDS when n <= lds_x, else formed again from memory by the same expression), gamma',
// and the new direction.  first: the start of a solve (d = 0, so s = z), which also checks mu and sets gamma0.
// SCALED: `d` is e, s = c o z - mu e, and c o p is written to `cp` for J to read; first also counts the c_k that are not
// positive finite numbers (bad input: status 2).  MASKED (twr_jac_lsq_solve_masked; with SCALED): a c_k that is exactly 0 is legal
// and takes variable k out of the solve: its s is an exact +0 whatever z holds, so p, e and d = c o e stay +0 and |s| is taken over
// the free variables; only a negative, NaN or Inf c_k is bad.  The other instantiations are the code they were.
template <bool SCALED, bool MASKED = false>
__device__ inline void lsq_dir_body(const JacLsqWork* __restrict__ work, double* __restrict__ rec, const double* __restrict__ mu,
                                    const double* __restrict__ z, const double* __restrict__ d, const double* __restrict__ c,
                                    double* __restrict__ p, double* __restrict__ cp, double* __restrict__ info, double tol2, int first,
                                    int lds_x, double* lsq_s, double* red) {
  double* rc = rec + (int64_t)kLsqRec * blockIdx.x;
  if (!first && rc[kLsqState] != kLsqRunning) {   // stopped: only the status is written again (the step kernel may have set it)
    if (threadIdx.x == 0) info[4 * (int64_t)blockIdx.x + 3] = rc[kLsqState];
    return;
  }
  const double m_u = mu[blockIdx.x], gamma = rc[kLsqGamma], gamma0 = rc[kLsqGamma0], iters = rc[kLsqIters];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  const double* zp = z + W.x_off;
  const double* dp = d + W.x_off;
  double* pp = p + W.x_off;
  const bool az = lsq_aligned(zp), ad = lsq_aligned(dp), ap = lsq_aligned(pp), staged = n <= lds_x;
  const double* cs = SCALED ? c + W.x_off : nullptr;
  double* cpp = SCALED ? cp + W.x_off : nullptr;
  const bool ac = lsq_aligned(cs), acp = lsq_aligned(cpp);
  const auto s_at = [&](int i) {
    double2 zv = lsq_ld(zp, i, n, az);
    if constexpr (SCALED) {
      const double2 cv = lsq_ld(cs, i, n, ac);
      zv = make_double2(cv.x * zv.x, cv.y * zv.y);
      if constexpr (MASKED) zv = make_double2(cv.x == 0.0 ? 0.0 : zv.x, cv.y == 0.0 ? 0.0 : zv.y);
    }
    if (first) return zv;
    const double2 dv = lsq_ld(dp, i, n, ad);
    return make_double2(fma(-m_u, dv.x, zv.x), fma(-m_u, dv.y, zv.y));
  };
  double acc[SCALED ? 2 : 1] = {};   // s^T s; SCALED: and the bad c_k
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 sv = s_at(i);
    if constexpr (SCALED)
      if (first) {
        const double2 cv = lsq_ld(cs, i, n, ac);
        if constexpr (MASKED) {
          if (!(cv.x >= 0.0) || !lsq_finite(cv.x)) acc[1] += 1.0;
          if (i + 1 < n && (!(cv.y >= 0.0) || !lsq_finite(cv.y))) acc[1] += 1.0;
        } else {
          if (!(cv.x > 0.0) || !lsq_finite(cv.x)) acc[1] += 1.0;
          if (i + 1 < n && (!(cv.y > 0.0) || !lsq_finite(cv.y))) acc[1] += 1.0;
        }
      }
    if (staged) {   // the lane reads back what it wrote: no barrier
      lsq_s[i] = sv.x;
      if (i + 1 < n) lsq_s[i + 1] = sv.y;
    }
    lsq_add(acc[0], sv, sv, i, n);
  }
  lsq_sum(acc, red);
  const double gn = acc[0];
  double state = kLsqRunning, beta = 0.0, g0 = gamma0;
  if (first) {
    g0 = gn;
    bool bad = !(m_u >= 0.0) || !lsq_finite(m_u) || !lsq_finite(gn);
    if constexpr (SCALED) bad = bad || acc[1] != 0.0;
    if (bad) state = 2.0;
    else if (gn <= tol2 * gn) state = 0.0;   // |s0| = 0 (b = 0, no rows), or tol >= 1
  } else {
    if (!lsq_finite(gn)) state = 2.0;
    else if (gn <= tol2 * g0) state = 0.0;
    else beta = gn / gamma;
  }
  if (state == kLsqRunning)
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 sv = staged ? make_double2(lsq_s[i], i + 1 < n ? lsq_s[i + 1] : 0.0) : s_at(i);
      double2 pn = sv;
      if (!first) {
        const double2 pv = lsq_ld(pp, i, n, ap);
        pn = make_double2(fma(beta, pv.x, sv.x), fma(beta, pv.y, sv.y));
      }
      lsq_st(pp, i, n, ap, pn);
      if constexpr (SCALED) {
        const double2 cv = lsq_ld(cs, i, n, ac);
        lsq_st(cpp, i, n, acp, make_double2(cv.x * pn.x, cv.y * pn.y));
      }
    }
  if (threadIdx.x == 0) {
    rc[kLsqGamma] = gn;
    rc[kLsqState] = state;
    if (first) rc[kLsqGamma0] = g0, rc[kLsqIters] = 0.0;
    lsq_info(info + 4 * (int64_t)blockIdx.x, first ? 0.0 : iters, gn, g0, state);
  }
}
__global__ __launch_bounds__(kLsqThreads) void lsq_dir_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                              const double* __restrict__ mu, const double* __restrict__ z,
                                                              const double* __restrict__ d, double* __restrict__ p,
                                                              double* __restrict__ info, double tol2, int first, int lds_x) {
  extern __shared__ double lsq_s[];   // lds_x doubles
  __shared__ double red[kLsqThreads / 64];
  lsq_dir_body<false>(work, rec, mu, z, d, nullptr, p, nullptr, info, tol2, first, lds_x, lsq_s, red);
}
__global__ __launch_bounds__(kLsqThreads) void lsq_dir_scaled_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                     const double* __restrict__ mu, const double* __restrict__ z,
                                                                     const double* __restrict__ e, const double* __restrict__ c,
                                                                     double* __restrict__ p, double* __restrict__ cp,
                                                                     double* __restrict__ info, double tol2, int first, int lds_x) {
  extern __shared__ double lsq_s[];   // lds_x doubles
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_dir_body<true>(work, rec, mu, z, e, c, p, cp, info, tol2, first, lds_x, lsq_s, red);
}
__global__ __launch_bounds__(kLsqThreads) void lsq_dir_masked_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                     const double* __restrict__ mu, const double* __restrict__ z,
                                                                     const double* __restrict__ e, const double* __restrict__ c,
                                                                     double* __restrict__ p, double* __restrict__ cp,
                                                                     double* __restrict__ info, double tol2, int first, int lds_x) {
  extern __shared__ double lsq_s[];   // lds_x doubles
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_dir_body<true, true>(work, rec, mu, z, e, c, p, cp, info, tol2, first, lds_x, lsq_s, red);
}

// The one-pass solve (twr_jac_lsq_solve_onepass): the gradient s is recurred, s -= alpha (u + mu p) with u = J^T (w o (J p)) from
// the one-pass product, so the vector work of an iteration needs no product in its middle and is this one kernel.
//   first (after z = J^T (w o b)): s = z, gamma0 = gamma = s^T s, the checks of mu (and c), p = s.
//   later (after (q, u) = normal(p)): delta, alpha, d += alpha p, r -= alpha q, s -= alpha (u + mu p), gamma' = s^T s, the
//   convergence test, beta, p = s + beta p; writes the problem's info.
// SCALED: the iteration on J C in e = d / c: s0 = c o z, the product read c o p (written to `cp`), u is multiplied by c,
// e += alpha p and d = c o e.  With c = 1 every one of these is exact: the bits of the unscaled kernel.
// A lane reads back from memory only what it wrote itself (the same index pairs): no barrier for s.
template <bool SCALED>
__device__ inline void lsq_onepass_body(const JacLsqWork* __restrict__ work, double* __restrict__ rec, const double* __restrict__ mu,
                                        const double* __restrict__ z, const double* __restrict__ q, const double* __restrict__ u,
                                        const double* __restrict__ w, const double* __restrict__ c, double* __restrict__ p,
                                        double* __restrict__ cp, double* __restrict__ s, double* __restrict__ e, double* __restrict__ d,
                                        double* __restrict__ r, double* __restrict__ info, double tol2, int first, double* red) {
  double* rc = rec + (int64_t)kLsqRec * blockIdx.x;
  double* o = info + 4 * (int64_t)blockIdx.x;
  if (!first && rc[kLsqState] != kLsqRunning) {   // stopped: only the status is written again
    if (threadIdx.x == 0) o[3] = rc[kLsqState];
    return;
  }
  const double m_u = mu[blockIdx.x];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n, m = W.m;
  double* pp = p + W.x_off;
  double* sp = s + W.x_off;
  const double* cs = SCALED ? c + W.x_off : nullptr;
  double* cpp = SCALED ? cp + W.x_off : nullptr;
  const bool ap = lsq_aligned(pp), as = lsq_aligned(sp), ac = lsq_aligned(cs), acp = lsq_aligned(cpp);
  const auto put_p = [&](int i, double2 pn) {
    lsq_st(pp, i, n, ap, pn);
    if constexpr (SCALED) {
      const double2 cv = lsq_ld(cs, i, n, ac);
      lsq_st(cpp, i, n, acp, make_double2(cv.x * pn.x, cv.y * pn.y));
    }
  };
  if (first) {
    const double* zp = z + W.x_off;
    const bool az = lsq_aligned(zp);
    double acc[SCALED ? 2 : 1] = {};   // s^T s; SCALED: and the bad c_k
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      double2 sv = lsq_ld(zp, i, n, az);
      if constexpr (SCALED) {
        const double2 cv = lsq_ld(cs, i, n, ac);
        sv = make_double2(cv.x * sv.x, cv.y * sv.y);
        if (!(cv.x > 0.0) || !lsq_finite(cv.x)) acc[1] += 1.0;
        if (i + 1 < n && (!(cv.y > 0.0) || !lsq_finite(cv.y))) acc[1] += 1.0;
      }
      lsq_st(sp, i, n, as, sv);
      lsq_add(acc[0], sv, sv, i, n);
    }
    lsq_sum(acc, red);
    const double gn = acc[0];
    double state = kLsqRunning;
    bool bad = !(m_u >= 0.0) || !lsq_finite(m_u) || !lsq_finite(gn);
    if constexpr (SCALED) bad = bad || acc[1] != 0.0;
    if (bad) state = 2.0;
    else if (gn <= tol2 * gn) state = 0.0;   // |s0| = 0 (b = 0, no rows), or tol >= 1
    if (state == kLsqRunning)
      for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) put_p(i, lsq_ld(sp, i, n, as));
    if (threadIdx.x == 0) {
      rc[kLsqGamma] = gn, rc[kLsqGamma0] = gn, rc[kLsqIters] = 0.0, rc[kLsqState] = state;
      lsq_info(o, 0.0, gn, gn, state);
    }
    return;
  }
  const double gamma = rc[kLsqGamma], g0 = rc[kLsqGamma0], iters = rc[kLsqIters];
  const double* qp = q + W.g_off;
  const double* wp = w ? w + W.g_off : nullptr;
  const double* up = u + W.x_off;
  double* dp = d + W.x_off;
  double* rp = r + W.g_off;
  const bool aq = lsq_aligned(qp), aw = lsq_aligned(wp), au = lsq_aligned(up), ad = lsq_aligned(dp), ar = lsq_aligned(rp);
  double acc[2] = {0.0, 0.0};   // q^T (w o q), p^T p
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 qv = lsq_ld(qp, i, m, aq);
    const double2 wv = wp ? lsq_ld(wp, i, m, aw) : make_double2(1.0, 1.0);
    lsq_add(acc[0], qv, wv, qv, i, m);
  }
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 pv = lsq_ld(pp, i, n, ap);
    lsq_add(acc[1], pv, pv, i, n);
  }
  lsq_sum(acc, red);
  const double delta = acc[0] + m_u * acc[1];
  if (!(delta > 0.0) || !lsq_finite(delta)) {   // NaN, Inf, or no curvature along p: alpha would not be a number
    if (threadIdx.x == 0) rc[kLsqState] = 2.0, o[3] = 2.0;
    return;
  }
  const double alpha = gamma / delta;
  double* ep = SCALED ? e + W.x_off : nullptr;
  const bool ae = lsq_aligned(ep);
  double gs[1] = {0.0};   // s^T s of the new s
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 pv = lsq_ld(pp, i, n, ap), sv = lsq_ld(sp, i, n, as);
    double2 uv = lsq_ld(up, i, n, au);
    if constexpr (SCALED) {
      const double2 cv = lsq_ld(cs, i, n, ac), ev = lsq_ld(ep, i, n, ae);
      uv = make_double2(cv.x * uv.x, cv.y * uv.y);
      const double2 en = make_double2(fma(alpha, pv.x, ev.x), fma(alpha, pv.y, ev.y));
      lsq_st(ep, i, n, ae, en);
      lsq_st(dp, i, n, ad, make_double2(cv.x * en.x, cv.y * en.y));
    } else {
      const double2 dv = lsq_ld(dp, i, n, ad);
      lsq_st(dp, i, n, ad, make_double2(fma(alpha, pv.x, dv.x), fma(alpha, pv.y, dv.y)));
    }
    const double2 sn = make_double2(fma(-alpha, fma(m_u, pv.x, uv.x), sv.x), fma(-alpha, fma(m_u, pv.y, uv.y), sv.y));
    lsq_st(sp, i, n, as, sn);
    lsq_add(gs[0], sn, sn, i, n);
  }
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 qv = lsq_ld(qp, i, m, aq), rv = lsq_ld(rp, i, m, ar);
    lsq_st(rp, i, m, ar, make_double2(fma(-alpha, qv.x, rv.x), fma(-alpha, qv.y, rv.y)));
  }
  lsq_sum(gs, red);
  const double gn = gs[0];
  double state = kLsqRunning, beta = 0.0;
  if (!lsq_finite(gn)) state = 2.0;
  else if (gn <= tol2 * g0) state = 0.0;
  else beta = gn / gamma;
  if (state == kLsqRunning)
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 sv = lsq_ld(sp, i, n, as), pv = lsq_ld(pp, i, n, ap);
      put_p(i, make_double2(fma(beta, pv.x, sv.x), fma(beta, pv.y, sv.y)));
    }
  if (threadIdx.x == 0) {
    rc[kLsqGamma] = gn;
    rc[kLsqState] = state;
    rc[kLsqIters] = iters + 1.0;
    lsq_info(o, iters + 1.0, gn, g0, state);
  }
}
__global__ __launch_bounds__(kLsqThreads) void lsq_onepass_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                  const double* __restrict__ mu, const double* __restrict__ z,
                                                                  const double* __restrict__ q, const double* __restrict__ u,
                                                                  const double* __restrict__ w, double* __restrict__ p,
                                                                  double* __restrict__ s, double* __restrict__ d, double* __restrict__ r,
                                                                  double* __restrict__ info, double tol2, int first) {
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_onepass_body<false>(work, rec, mu, z, q, u, w, nullptr, p, nullptr, s, nullptr, d, r, info, tol2, first, red);
}
__global__ __launch_bounds__(kLsqThreads) void lsq_onepass_scaled_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                         const double* __restrict__ mu, const double* __restrict__ z,
                                                                         const double* __restrict__ q, const double* __restrict__ u,
                                                                         const double* __restrict__ w, const double* __restrict__ c,
                                                                         double* __restrict__ p, double* __restrict__ cp,
                                                                         double* __restrict__ s, double* __restrict__ e,
                                                                         double* __restrict__ d, double* __restrict__ r,
                                                                         double* __restrict__ info, double tol2, int first) {
  __shared__ double red[2 * (kLsqThreads / 64)];
  lsq_onepass_body<true>(work, rec, mu, z, q, u, w, c, p, cp, s, e, d, r, info, tol2, first, red);
}

// c_k = 1 / sqrt(max(a_k, rel_floor top)), top = max_k a_k, a = colsq or the running maximum colsq_max = max(colsq_max, colsq)
// (in / out, may be NULL); c = 1 for a problem with top == 0.  A NaN a_k gives a NaN c_k and takes no part in top.
__device__ inline double lsq_scale_a(double m, double a) { return a != a ? a : (m < a ? a : m); }   // max that keeps either NaN
__global__ __launch_bounds__(kLsqThreads) void lsq_col_scale_kernel(const JacLsqWork* __restrict__ work,
                                                                    const double* __restrict__ colsq, double* __restrict__ colsq_max,
                                                                    double rel_floor, double* __restrict__ scale) {
  __shared__ double red[kLsqThreads / 64];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  const double* ap = colsq + W.x_off;
  double* mp = colsq_max ? colsq_max + W.x_off : nullptr;
  double* sp = scale + W.x_off;
  const bool aa = lsq_aligned(ap), am = lsq_aligned(mp), as = lsq_aligned(sp);
  const auto a_at = [&](int i) {
    const double2 a = lsq_ld(ap, i, n, aa);
    if (!mp) return a;
    const double2 m = lsq_ld(mp, i, n, am);
    return make_double2(lsq_scale_a(m.x, a.x), lsq_scale_a(m.y, a.y));
  };
  double top = 0.0;
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 a = a_at(i);
    top = fmax(top, a.x);   // fmax drops a NaN
    if (i + 1 < n) top = fmax(top, a.y);
  }
  for (int s = 32; s >= 1; s >>= 1) top = fmax(top, __shfl_xor(top, s, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x / 64] = top;
  __syncthreads();
  top = red[0];
  for (int w = 1; w < kLsqThreads / 64; ++w) top = fmax(top, red[w]);
  const double f = rel_floor * top;
  const auto c_of = [&](double a) { return a != a ? a : (top == 0.0 ? 1.0 : 1.0 / sqrt(a < f ? f : a)); };
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {   // the pairs this lane read above
    const double2 a = a_at(i);
    if (mp) lsq_st(mp, i, n, am, a);
    lsq_st(sp, i, n, as, make_double2(c_of(a.x), c_of(a.y)));
  }
}

}  // namespace twr
