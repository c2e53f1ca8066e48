// Fourth translation unit of the kernels, plain flags: the Jacobian linear algebra -- the products with J, the damped least-squares
// solves, the Gram matrix and the bounded LM driver's vector kernels (jac/*.h, of which this is the only includer: they define
// kernels) -- and their launch_* functions (jac_launch.h).  One stream per call; a launcher stops at its first error.
#include <hip/hip_runtime.h>

#include "jac_launch.h"

#include "jac/gram.h"
#include "jac/lm.h"
#include "jac/lsq.h"
#include "jac/products.h"

namespace twr {

// ---------------------------------------------------------------- products
// one workgroup per work item (nothing to launch for a batch without rows)
hipError_t launch_jac_mul(const JacProducts& J, const double* v, double* y) {
  if (J.n_mul == 0) return hipSuccess;
  const size_t lds = sizeof(double) * ((size_t)kJacMulNnz + J.lds_x);
  return jac_launch(jac_mul_kernel, J.n_mul, kJacThreads, lds, J.stream, J.mul, J.jac, v, y, J.lds_x);
}

// the partials of J^T w's work list, then the fold (which also writes the zeros of columns without entries)
static hipError_t tmul_and_fold(decltype(&jac_tmul_kernel) partials, const JacProducts& J, const double* w, double* z) {
  hipError_t e = hipSuccess;
  if (J.n_tmul > 0) e = jac_launch(partials, J.n_tmul, kJacThreads, 0, J.stream, J.tmul, J.jac, w, J.slab);
  if (e == hipSuccess && J.n_fold > 0) e = jac_launch(jac_fold_kernel, J.n_fold, kJacFoldCols, 0, J.stream, J.fold, J.slab, z);
  return e;
}
hipError_t launch_jac_tmul(const JacProducts& J, const double* w, double* z) { return tmul_and_fold(jac_tmul_kernel, J, w, z); }
hipError_t launch_jac_colsq(const JacProducts& J, const double* w, double* out) { return tmul_and_fold(jac_colsq_kernel, J, w, out); }

// the one pass, then the fold over its own slab.  With v staged the kernel's LDS passes 64 KB: prepare_jac_normal raises the limit
hipError_t prepare_jac_normal() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(jac_normal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
hipError_t launch_jac_normal(const JacProducts& J, const double* w, const double* v, double* y, double* u) {
  const size_t lds = sizeof(double) * (2 * (size_t)J.n_tile + J.n_lds_x);
  hipError_t e = hipSuccess;
  if (J.n_normal > 0)
    e = jac_launch(jac_normal_kernel, J.n_normal, kJacThreads, lds, J.stream, J.normal, J.jac, w, v, y, J.nslab, J.n_lds_x, J.n_tile);
  if (e == hipSuccess && J.n_nfold > 0) e = jac_launch(jac_fold_kernel, J.n_nfold, kJacFoldCols, 0, J.stream, J.nfold, J.nslab, u);
  return e;
}

// ---------------------------------------------------------------- least squares
hipError_t launch_lsq_dot(const JacLsqWork* work, int n, int space, const double* a, const double* b, double* out, hipStream_t stream) {
  return jac_launch(lsq_dot_kernel, n, kLsqThreads, 0, stream, work, space, a, b, out);
}
hipError_t launch_lsq_violation(const JacLsqWork* work, int n, const double* g, const double* w, double* r, double* w_active, double* merit,
                                hipStream_t stream) {
  return jac_launch(lsq_violation_kernel, n, kLsqThreads, 0, stream, work, g, w, r, w_active, merit);
}
hipError_t launch_lsq_col_scale(const JacLsqWork* work, int n, const double* colsq, double* colsq_max, double rel_floor, double* scale,
                                hipStream_t stream) {
  return jac_launch(lsq_col_scale_kernel, n, kLsqThreads, 0, stream, work, colsq, colsq_max, rel_floor, scale);
}

// CGLS.  c NULL: the plain solve.  Else the same sequence on J C in e = d / c (sc): the product kernels as they are, the vector
// kernels' SCALED instantiations, J reading c o p; masked: the direction kernel's MASKED instantiation, while the start and step
// kernels serve as they are, since p_k = +0 keeps e_k and d_k = c_k e_k at +0.
static hipError_t lsq_cgls(const JacLsqWork* work, int n, int lds_x, const LsqBuffers& ws, const LsqScaledBuffers& sc, const double* b,
                           const double* w, const double* mu, const double* c, int iters, double tol, double* d, double* info,
                           const JacProducts& J, bool masked) {
  const hipStream_t stream = J.stream;
  const size_t lds = sizeof(double) * (size_t)lds_x;
  const double tol2 = tol * tol;
  const auto dir = [&](int first) {
    if (!c) return jac_launch(lsq_dir_kernel, n, kLsqThreads, lds, stream, work, ws.rec, mu, ws.z, d, ws.p, info, tol2, first, lds_x);
    return jac_launch(masked ? lsq_dir_masked_kernel : lsq_dir_scaled_kernel, n, kLsqThreads, lds, stream, work, ws.rec, mu, ws.z, sc.e, c,
                      ws.p, sc.cp, info, tol2, first, lds_x);
  };
  hipError_t e = c ? jac_launch(lsq_start_scaled_kernel, n, kLsqThreads, 0, stream, work, ws.rec, b, w, d, sc.e, ws.r, ws.t)
                   : jac_launch(lsq_start_kernel, n, kLsqThreads, 0, stream, work, ws.rec, b, w, d, ws.r, ws.t);
  if (e == hipSuccess) e = launch_jac_tmul(J, ws.t, ws.z);
  if (e == hipSuccess) e = dir(1);
  for (int k = 0; k < iters && e == hipSuccess; ++k) {
    e = launch_jac_mul(J, c ? sc.cp : ws.p, ws.q);
    if (e == hipSuccess)
      e = c ? jac_launch(lsq_step_scaled_kernel, n, kLsqThreads, 0, stream, work, ws.rec, mu, ws.q, w, ws.p, c, sc.e, d, ws.r, ws.t)
            : jac_launch(lsq_step_kernel, n, kLsqThreads, 0, stream, work, ws.rec, mu, ws.q, w, ws.p, d, ws.r, ws.t);
    if (e == hipSuccess) e = launch_jac_tmul(J, ws.t, ws.z);
    if (e == hipSuccess) e = dir(0);
  }
  return e;
}
hipError_t launch_lsq_solve(const JacLsqWork* work, int n, int lds_x, const LsqBuffers& ws, const double* b, const double* w, const double* mu,
                            int iters, double tol, double* d, double* info, const JacProducts& J) {
  return lsq_cgls(work, n, lds_x, ws, LsqScaledBuffers{}, b, w, mu, nullptr, iters, tol, d, info, J, false);
}
hipError_t launch_lsq_solve_scaled(const JacLsqWork* work, int n, int lds_x, const LsqBuffers& ws, const LsqScaledBuffers& sc, const double* b,
                                   const double* w, const double* mu, const double* c, int iters, double tol, double* d, double* info,
                                   const JacProducts& J, bool masked) {
  return lsq_cgls(work, n, lds_x, ws, sc, b, w, mu, c, iters, tol, d, info, J, masked);
}

hipError_t launch_lsq_solve_onepass(const JacLsqWork* work, int n, const LsqBuffers& ws, const LsqScaledBuffers& sc, const LsqOnepassBuffers& op,
                                    const double* b, const double* w, const double* mu, const double* c, int iters, double tol, double* d,
                                    double* info, const JacProducts& J) {
  const hipStream_t stream = J.stream;
  const double tol2 = tol * tol;
  const auto vec = [&](int first) {
    if (c)
      return jac_launch(lsq_onepass_scaled_kernel, n, kLsqThreads, 0, stream, work, ws.rec, mu, ws.z, ws.q, op.u, w, c, ws.p, sc.cp, op.s,
                        sc.e, d, ws.r, info, tol2, first);
    return jac_launch(lsq_onepass_kernel, n, kLsqThreads, 0, stream, work, ws.rec, mu, ws.z, ws.q, op.u, w, ws.p, op.s, d, ws.r, info,
                      tol2, first);
  };
  hipError_t e = c ? jac_launch(lsq_start_scaled_kernel, n, kLsqThreads, 0, stream, work, ws.rec, b, w, d, sc.e, ws.r, ws.t)
                   : jac_launch(lsq_start_kernel, n, kLsqThreads, 0, stream, work, ws.rec, b, w, d, ws.r, ws.t);
  if (e == hipSuccess) e = launch_jac_tmul(J, ws.t, ws.z);
  if (e == hipSuccess) e = vec(1);
  for (int k = 0; k < iters && e == hipSuccess; ++k) {
    e = launch_jac_normal(J, w, c ? sc.cp : ws.p, ws.q, op.u);
    if (e == hipSuccess) e = vec(0);
  }
  return e;
}

// ---------------------------------------------------------------- the Gram matrix
hipError_t launch_jac_gram(const JacGramWork* work, int n_work, const double* jac, const double* w, double* gram, hipStream_t stream) {
  if (n_work == 0) return hipSuccess;
  return jac_launch(jac_gram_kernel, n_work, kGramThreads, 0, stream, work, jac, w, gram);
}
hipError_t launch_jac_gram_mul(const JacGramMulWork* work, int n_work, const double* gram, const double* v, double* u, hipStream_t stream) {
  if (n_work == 0) return hipSuccess;
  return jac_launch(jac_gram_mul_kernel, n_work, kGramThreads, 0, stream, work, gram, v, u);
}
// the solve's LDS may pass 64 KB: prepare_gram_cg raises the kernel's limit
hipError_t prepare_gram_cg() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(gram_cg_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kGramLdsBytes);
}
hipError_t launch_gram_cg(const JacGramSolveWork* work, int n_problems, int max_n, const double* gram, const double* z, const double* mu,
                          const double* scale, int iters, double tol, double* d, double* info, hipStream_t stream) {
  const size_t lds = sizeof(double) * ((size_t)kGramSolveVectors * max_n + kGramRed);
  return jac_launch(gram_cg_kernel, n_problems, kGramThreads, lds, stream, work, gram, z, mu, scale, iters, tol * tol, d, info, max_n);
}

// ---------------------------------------------------------------- the bounded LM driver
hipError_t launch_lm_free_set(const JacLsqWork* work, int n, const double* x, const double* lo, const double* up, const double* z,
                              const double* c_in, double* c_out, double* nfree, hipStream_t stream) {
  return jac_launch(lm_free_set_kernel, n, kLsqThreads, 0, stream, work, x, lo, up, z, c_in, c_out, nfree);
}
hipError_t launch_lm_project(const JacLsqWork* work, int n, double* x, const double* lo, const double* up, const LmBuffers& B, double tau,
                             hipStream_t stream) {
  return jac_launch(lm_project_kernel, n, kLsqThreads, 0, stream, work, x, lo, up, B.colmax, B.d, B.rec, B.mu, tau);
}
hipError_t launch_lm_linearise(const JacLsqWork* work, int n, const double* x, const double* g, const double* lo, const double* up,
                               const LmBuffers& B, double merit_done, double rel_floor, int first, const JacProducts& J) {
  const hipStream_t stream = J.stream;
  hipError_t e = launch_lsq_violation(work, n, g, nullptr, B.r, B.wa, B.merit_lin, stream);
  if (e == hipSuccess)   // (w o b goes to rt, which is free until the trial point's violation)
    e = jac_launch(lm_rhs_kernel, n, kLsqThreads, 0, stream, work, B.r, B.wa, B.merit_lin, B.b, B.rt, B.rec, merit_done, first);
  if (e == hipSuccess) e = launch_jac_colsq(J, B.wa, B.colsq);
  if (e == hipSuccess) e = launch_lsq_col_scale(work, n, B.colsq, B.colmax, rel_floor, B.c, stream);
  if (e == hipSuccess) e = launch_jac_tmul(J, B.rt, B.z);
  if (e == hipSuccess) e = launch_lm_free_set(work, n, x, lo, up, B.z, B.c, B.cf, B.nfree, stream);
  return e;
}
hipError_t launch_lm_power(const JacLsqWork* work, int n, const LmBuffers& B, const LmParams& P, int iters, const JacProducts& J) {
  const hipStream_t stream = J.stream;
  hipError_t e = jac_launch(lm_normalise_kernel, n, kLsqThreads, 0, stream, work, B.cf, B.d, B.z, B.xt, B.rec, B.mu, P, 0, iters == 0);
  for (int k = 0; k < iters && e == hipSuccess; ++k) {
    e = launch_jac_mul(J, B.xt, B.gt);
    if (e == hipSuccess) e = jac_launch(lm_weight_kernel, n, kLsqThreads, 0, stream, work, B.wa, B.gt);
    if (e == hipSuccess) e = launch_jac_tmul(J, B.gt, B.z);
    if (e == hipSuccess)
      e = jac_launch(lm_normalise_kernel, n, kLsqThreads, 0, stream, work, B.cf, B.d, B.z, B.xt, B.rec, B.mu, P, 1, k == iters - 1);
  }
  return e;
}
hipError_t launch_lm_trial(const JacLsqWork* work, int n, const double* x, const double* lo, const double* up, const LmBuffers& B,
                           hipStream_t stream) {
  return jac_launch(lm_trial_kernel, n, kLsqThreads, 0, stream, work, B.rec, x, B.d, lo, up, B.xt);
}
hipError_t launch_lm_accept(const JacLsqWork* work, int n, double* x, const LmBuffers& B, const LmParams& P, hipStream_t stream) {
  hipError_t e = launch_lsq_violation(work, n, B.gt, nullptr, B.rt, nullptr, B.merit_t, stream);
  if (e == hipSuccess) e = jac_launch(lm_accept_kernel, n, kLsqThreads, 0, stream, work, B.rec, B.mu, B.merit_t, B.info, B.nfree, x, B.xt, P);
  return e;
}

}  // namespace twr
