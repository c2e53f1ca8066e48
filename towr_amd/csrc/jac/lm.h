// The bound-constrained Levenberg-Marquardt driver (twr_jac_lm_*, twr_jac_free_set; include/towr_amd.h): the vector kernels between
// the evaluation, the products and the masked solve of lsq.h.  Projected active-set LM: a variable that sits on a bound the
// step would push it through (every variable with lo == up among them) gets an exact 0 in the column scale and so stays out of the
// solve, the trial point is projected onto the box, and accept / reject and mu are decided per problem here.
//   lm_project_kernel:   x = min(max(x, lo), up), the checks of x and the bounds, the start of the problem's record, colmax = 0 and
//                        the start vector of the power iteration
//   lm_rhs_kernel:       b = -r, wb = w o b; the merit of the linearisation decides done / bad
//   lm_free_set_kernel:  cf_k = blocked_k ? +0 : c_k, and the free count
//   lm_weight_kernel:    y = w o y                                         (the power iteration, between J and J^T)
//   lm_normalise_kernel: u = cf o u, lambda = v^T u / v^T v, v = u / |u|, cv = cf o v; the last one sets mu0
//   lm_trial_kernel:     xt = min(max(x + d, lo), up) (a problem that is not running: xt = x)
//   lm_accept_kernel:    ok = merit_t < merit, x = xt where ok, mu, the counters
// One workgroup of kLsqThreads lanes per problem in every kernel, the sums by lsq_sum over the index pairs of lsq.h: an order
// fixed by the vector's length, so x after any number of steps has the same bits wherever the problem sits.  No atomics.  Every
// index comes from the work record, never from the data.  The workspace is planned on the host (twr::PlanJacLm, jac_plan.h).
// Included by jac_tu.hip alone, which holds the launchers (jac_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "lsq.h"
#include "../jac_launch.h"   // LmParams, a kernel argument

namespace twr {

constexpr double kLmHuge = 1e20;   // ifopt's NoBound: an |x_k| beyond it is not a number to the NLP

__device__ inline double lm_clamp(double v, double lo, double hi) {   // a NaN v stays NaN
  double c = v < lo ? lo : v;
  return c > hi ? hi : c;
}
__device__ inline double lm_mu_clamp(double mu, const LmParams& P) { return lm_clamp(mu, P.mu_min, P.mu_max); }

// The k-th entry of the power iteration's start vector: a fixed pattern in [0.5, 1.5), a function of k alone
__device__ inline double lm_v0(int k) {
  uint32_t h = (uint32_t)k * 2654435761u + 0x9e3779b9u;
  h ^= h >> 15, h *= 0x85ebca6bu, h ^= h >> 13;
  return 0.5 + (double)(h >> 8) * (1.0 / 16777216.0);
}

__global__ __launch_bounds__(kLsqThreads) void lm_project_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ x,
                                                                 const double* __restrict__ lo, const double* __restrict__ up,
                                                                 double* __restrict__ colmax, double* __restrict__ v,
                                                                 double* __restrict__ rec, double* __restrict__ mu, double tau) {
  __shared__ double red[kLsqThreads / 64];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  double* xp = x + W.x_off;
  const double* lp = lo + W.x_off;
  const double* hp = up + W.x_off;
  double* mp = colmax + W.x_off;
  double* vp = v + W.x_off;
  const bool ax = lsq_aligned(xp), al = lsq_aligned(lp), ah = lsq_aligned(hp), am = lsq_aligned(mp), av = lsq_aligned(vp);
  const auto bad_at = [](double xv, double l, double h) { return !(fabs(xv) <= kLmHuge) || !(l <= h); };   // NaN: bad
  double acc[1] = {0.0};
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 xv = lsq_ld(xp, i, n, ax), l = lsq_ld(lp, i, n, al), h = lsq_ld(hp, i, n, ah);
    if (bad_at(xv.x, l.x, h.x)) acc[0] += 1.0;
    if (i + 1 < n && bad_at(xv.y, l.y, h.y)) acc[0] += 1.0;
    lsq_st(mp, i, n, am, make_double2(0.0, 0.0));
    lsq_st(vp, i, n, av, make_double2(lm_v0(i), lm_v0(i + 1)));
  }
  lsq_sum(acc, red);
  const bool bad = acc[0] != 0.0;
  if (!bad)
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {   // the pairs this lane read above
      const double2 xv = lsq_ld(xp, i, n, ax), l = lsq_ld(lp, i, n, al), h = lsq_ld(hp, i, n, ah);
      lsq_st(xp, i, n, ax, make_double2(lm_clamp(xv.x, l.x, h.x), lm_clamp(xv.y, l.y, h.y)));
    }
  if (threadIdx.x == 0) {
    double* rc = rec + (int64_t)kLmRec * blockIdx.x;
    rc[kLmMerit0] = 0.0, rc[kLmMerit] = 0.0, rc[kLmMu] = tau, rc[kLmSteps] = 0.0, rc[kLmAccepted] = 0.0, rc[kLmFree] = 0.0;
    rc[kLmCgIters] = 0.0, rc[kLmState] = bad ? kLmBad : kLmRunning;
    mu[blockIdx.x] = tau;
  }
}

// After the violation at x.  first: the record's merit is this one; later it is the accepted trials' (lm_accept_kernel).
__global__ __launch_bounds__(kLsqThreads) void lm_rhs_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ r,
                                                             const double* __restrict__ wa, const double* __restrict__ merit_lin,
                                                             double* __restrict__ b, double* __restrict__ wb,
                                                             double* __restrict__ rec, double merit_done, int first) {
  const JacLsqWork W = work[blockIdx.x];
  const int m = W.m;
  const double* rp = r + W.g_off;
  const double* wp = wa + W.g_off;
  double* bp = b + W.g_off;
  double* tp = wb + W.g_off;
  const bool ar = lsq_aligned(rp), aw = lsq_aligned(wp), ab = lsq_aligned(bp), at = lsq_aligned(tp);
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 rv = lsq_ld(rp, i, m, ar), wv = lsq_ld(wp, i, m, aw);
    const double2 bv = make_double2(-rv.x, -rv.y);
    lsq_st(bp, i, m, ab, bv);
    lsq_st(tp, i, m, at, make_double2(wv.x * bv.x, wv.y * bv.y));
  }
  if (threadIdx.x == 0) {
    double* rc = rec + (int64_t)kLmRec * blockIdx.x;
    const double ml = merit_lin[blockIdx.x];
    if (first) rc[kLmMerit0] = ml, rc[kLmMerit] = ml;
    if (rc[kLmState] == kLmRunning) {
      if (!lsq_finite(ml)) rc[kLmState] = kLmBad;
      else if (ml <= merit_done) rc[kLmState] = kLmDone;
    }
  }
}

// c_out_k = blocked_k ? +0 : c_in_k (c_in NULL: 1); blocked_k = (x_k <= lo_k && z_k <= 0) || (x_k >= up_k && z_k >= 0)
__global__ __launch_bounds__(kLsqThreads) void lm_free_set_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ x,
                                                                  const double* __restrict__ lo, const double* __restrict__ up,
                                                                  const double* __restrict__ z, const double* c_in, double* c_out,
                                                                  double* __restrict__ nfree) {
  __shared__ double red[kLsqThreads / 64];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  const double* xp = x + W.x_off;
  const double* lp = lo + W.x_off;
  const double* hp = up + W.x_off;
  const double* zp = z + W.x_off;
  const double* ip = c_in ? c_in + W.x_off : nullptr;
  double* op = c_out + W.x_off;
  const bool ax = lsq_aligned(xp), al = lsq_aligned(lp), ah = lsq_aligned(hp), az = lsq_aligned(zp), ai = lsq_aligned(ip),
             ao = lsq_aligned(op);
  const auto blocked = [](double xv, double l, double h, double zv) { return (xv <= l && zv <= 0.0) || (xv >= h && zv >= 0.0); };
  double acc[1] = {0.0};
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 xv = lsq_ld(xp, i, n, ax), l = lsq_ld(lp, i, n, al), h = lsq_ld(hp, i, n, ah), zv = lsq_ld(zp, i, n, az);
    const double2 cv = ip ? lsq_ld(ip, i, n, ai) : make_double2(1.0, 1.0);
    const bool b0 = blocked(xv.x, l.x, h.x, zv.x), b1 = blocked(xv.y, l.y, h.y, zv.y);
    lsq_st(op, i, n, ao, make_double2(b0 ? 0.0 : cv.x, b1 ? 0.0 : cv.y));
    if (!b0) acc[0] += 1.0;
    if (i + 1 < n && !b1) acc[0] += 1.0;
  }
  lsq_sum(acc, red);
  if (threadIdx.x == 0) nfree[blockIdx.x] = acc[0];
}

__global__ __launch_bounds__(kLsqThreads) void lm_weight_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ wa,
                                                                double* __restrict__ y) {
  const JacLsqWork W = work[blockIdx.x];
  const int m = W.m;
  const double* wp = wa + W.g_off;
  double* yp = y + W.g_off;
  const bool aw = lsq_aligned(wp), ay = lsq_aligned(yp);
  for (int i = 2 * (int)threadIdx.x; i < m; i += 2 * kLsqThreads) {
    const double2 wv = lsq_ld(wp, i, m, aw), yv = lsq_ld(yp, i, m, ay);
    lsq_st(yp, i, m, ay, make_double2(wv.x * yv.x, wv.y * yv.y));
  }
}

// The power iteration on C_f J^T W J C_f.  mode 0: cv = cf o v (its start).  mode 1, after u = J^T(w o (J cv)): u = cf o u,
// lambda = v^T u / max(v^T v, 1e-300), v = u / max(|u|, 1e-300), cv = cf o v.  last: mu = clamp(tau lambda) (mode 0: clamp(tau),
// the driver without power iterations).
__global__ __launch_bounds__(kLsqThreads) void lm_normalise_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ cf,
                                                                   double* __restrict__ v, const double* __restrict__ u,
                                                                   double* __restrict__ cv, double* __restrict__ rec,
                                                                   double* __restrict__ mu, LmParams P, int mode, int last) {
  __shared__ double red[3 * (kLsqThreads / 64)];
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  const double* cp = cf + W.x_off;
  double* vp = v + W.x_off;
  const double* up = u + W.x_off;
  double* op = cv + W.x_off;
  const bool ac = lsq_aligned(cp), av = lsq_aligned(vp), au = lsq_aligned(up), ao = lsq_aligned(op);
  double lam = 1.0;
  if (mode == 0) {
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 c = lsq_ld(cp, i, n, ac), vv = lsq_ld(vp, i, n, av);
      lsq_st(op, i, n, ao, make_double2(c.x * vv.x, c.y * vv.y));
    }
  } else {
    double acc[3] = {0.0, 0.0, 0.0};   // v^T v, v^T u, u^T u with u = cf o u
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
      const double2 c = lsq_ld(cp, i, n, ac), vv = lsq_ld(vp, i, n, av), uv = lsq_ld(up, i, n, au);
      const double2 s = make_double2(c.x * uv.x, c.y * uv.y);
      acc[0] += vv.x * vv.x, acc[1] += vv.x * s.x, acc[2] += s.x * s.x;
      if (i + 1 < n) acc[0] += vv.y * vv.y, acc[1] += vv.y * s.y, acc[2] += s.y * s.y;
    }
    lsq_sum(acc, red);
    lam = acc[1] / (acc[0] < 1e-300 ? 1e-300 : acc[0]);
    const double nrm = sqrt(acc[2]), inv = 1.0 / (nrm < 1e-300 ? 1e-300 : nrm);
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {   // the pairs this lane read above
      const double2 c = lsq_ld(cp, i, n, ac), uv = lsq_ld(up, i, n, au);
      const double2 vn = make_double2(c.x * uv.x * inv, c.y * uv.y * inv);
      lsq_st(vp, i, n, av, vn);
      lsq_st(op, i, n, ao, make_double2(c.x * vn.x, c.y * vn.y));
    }
  }
  if (last && threadIdx.x == 0) {
    const double m0 = lm_mu_clamp(P.tau * lam, P);
    mu[blockIdx.x] = m0;
    rec[(int64_t)kLmRec * blockIdx.x + kLmMu] = m0;
  }
}

__global__ __launch_bounds__(kLsqThreads) void lm_trial_kernel(const JacLsqWork* __restrict__ work, const double* __restrict__ rec,
                                                               const double* __restrict__ x, const double* __restrict__ d,
                                                               const double* __restrict__ lo, const double* __restrict__ up,
                                                               double* __restrict__ xt) {
  const JacLsqWork W = work[blockIdx.x];
  const int n = W.n;
  const bool running = rec[(int64_t)kLmRec * blockIdx.x + kLmState] == kLmRunning;   // written by an earlier launch
  const double* xp = x + W.x_off;
  const double* dp = d + W.x_off;
  const double* lp = lo + W.x_off;
  const double* hp = up + W.x_off;
  double* tp = xt + W.x_off;
  const bool ax = lsq_aligned(xp), ad = lsq_aligned(dp), al = lsq_aligned(lp), ah = lsq_aligned(hp), at = lsq_aligned(tp);
  for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) {
    const double2 xv = lsq_ld(xp, i, n, ax);
    if (!running) {
      lsq_st(tp, i, n, at, xv);
      continue;
    }
    const double2 dv = lsq_ld(dp, i, n, ad), l = lsq_ld(lp, i, n, al), h = lsq_ld(hp, i, n, ah);
    lsq_st(tp, i, n, at, make_double2(lm_clamp(xv.x + dv.x, l.x, h.x), lm_clamp(xv.y + dv.y, l.y, h.y)));
  }
}

__global__ __launch_bounds__(kLsqThreads) void lm_accept_kernel(const JacLsqWork* __restrict__ work, double* __restrict__ rec,
                                                                double* __restrict__ mu, const double* __restrict__ merit_t,
                                                                const double* __restrict__ info, const double* __restrict__ nfree,
                                                                double* __restrict__ x, const double* __restrict__ xt, LmParams P) {
  double* rc = rec + (int64_t)kLmRec * blockIdx.x;
  const double state = rc[kLmState], merit = rc[kLmMerit], mt = merit_t[blockIdx.x], m_u = mu[blockIdx.x];
  const double status = info[4 * (int64_t)blockIdx.x + 3], cg = info[4 * (int64_t)blockIdx.x];
  __syncthreads();   // every lane has read the record before lane 0 writes it
  if (state != kLmRunning) return;
  if (status == 2.0) {   // the solve met bad input: x stays as it is
    if (threadIdx.x == 0) rc[kLmState] = kLmBad;
    return;
  }
  const bool ok = mt < merit;   // a NaN rejects
  if (ok) {
    const JacLsqWork W = work[blockIdx.x];
    const int n = W.n;
    double* xp = x + W.x_off;
    const double* tp = xt + W.x_off;
    const bool ax = lsq_aligned(xp), at = lsq_aligned(tp);
    for (int i = 2 * (int)threadIdx.x; i < n; i += 2 * kLsqThreads) lsq_st(xp, i, n, ax, lsq_ld(tp, i, n, at));
  }
  if (threadIdx.x == 0) {
    const double mn = lm_mu_clamp(m_u * (ok ? P.mu_down : P.mu_up), P);
    mu[blockIdx.x] = mn;
    rc[kLmMu] = mn;
    rc[kLmSteps] += 1.0;
    if (ok) rc[kLmAccepted] += 1.0, rc[kLmMerit] = mt;
    rc[kLmFree] = nfree[blockIdx.x];
    rc[kLmCgIters] = cg;
  }
}

}  // namespace twr
