// Host launchers of the Jacobian solver kernels (jac_tu.hip, the only includer of jac/*.h), called by the C ABI (capi_jac.cc): the
// counterpart of launch.h.  Plain structs and declarations; every launcher returns its first launch's error.
#pragma once
#include <hip/hip_runtime.h>

#include "jac_plan.h"

namespace twr {

// A products handle's work lists and slabs with one J on one stream: what the product launchers and the solves are given
struct JacProducts {
  const JacMulWork* mul;         // y = J v
  int n_mul;
  const JacTWork* tmul;          // z = J^T w and the column norms: the partials into slab, then fold
  int n_tmul;
  const JacFoldWork* fold;
  int n_fold;
  const JacNormalWork* normal;   // the one-pass product (once reserved): the partials into nslab, then nfold
  int n_normal;
  const JacFoldWork* nfold;
  int n_nfold;
  double *slab, *nslab;
  int lds_x, n_lds_x, n_tile;
  const double* jac;
  hipStream_t stream;
};
struct LsqBuffers {   // the handle's workspace (JacLsqPlan's segments)
  double *p, *z, *q, *r, *t, *rec;
};
struct LsqScaledBuffers {   // the second allocation (twr_jac_lsq_reserve_scaled): e = d / c, and c o p for J to read
  double *e, *cp;
};
struct LsqOnepassBuffers {   // the third allocation (twr_jac_lsq_solve_onepass): the recurred s, and u = J^T (w o (J p))
  double *s, *u;
};
struct LmBuffers {   // the handle's workspace (JacLmPlan's segments)
  double *xt, *d, *z, *colsq, *colmax, *c, *cf, *r, *b, *wa, *gt, *rt, *rec, *mu, *merit_t, *merit_lin, *nfree, *info;
};
struct LmParams {   // twr_jac_lm_params, what the kernels read
  double mu_down, mu_up, mu_min, mu_max, tau, merit_done;
};

// The products (jac/products.h).  y = J v; z = J^T w; out[k] = sum_r w_r J[r][k]^2 (w NULL: unit weights); u = J^T (w o (J v)) and
// y = J v from one pass (y NULL: not written; w NULL: unit weights).  prepare_jac_normal: once, on the handle's device, outside any
// capture (the one-pass kernel's LDS may pass 64 KB).
hipError_t launch_jac_mul(const JacProducts& J, const double* v, double* y);
hipError_t launch_jac_tmul(const JacProducts& J, const double* w, double* z);
hipError_t launch_jac_colsq(const JacProducts& J, const double* w, double* out);
hipError_t launch_jac_normal(const JacProducts& J, const double* w, const double* v, double* y, double* u);
hipError_t prepare_jac_normal();

// The least-squares step (jac/lsq.h); the vector kernels go to J.stream, where the products go
hipError_t launch_lsq_dot(const JacLsqWork* work, int n, int space, const double* a, const double* b, double* out, hipStream_t stream);
hipError_t launch_lsq_violation(const JacLsqWork* work, int n, const double* g, const double* w, double* r, double* w_active, double* merit,
                                hipStream_t stream);
hipError_t launch_lsq_col_scale(const JacLsqWork* work, int n, const double* colsq, double* colsq_max, double rel_floor, double* scale,
                                hipStream_t stream);
// The whole solve: 3 launches to start, 5 per iteration (J p, step, J^T t and its fold, direction), none of them conditional.
hipError_t launch_lsq_solve(const JacLsqWork* work, int n, int lds_x, const LsqBuffers& ws, const double* b, const double* w, const double* mu,
                            int iters, double tol, double* d, double* info, const JacProducts& J);
// The same sequence on J C in e = d / c.  masked: a c_k that is exactly 0 takes variable k out of the solve (twr_jac_lsq_solve_masked)
hipError_t launch_lsq_solve_scaled(const JacLsqWork* work, int n, int lds_x, const LsqBuffers& ws, const LsqScaledBuffers& sc, const double* b,
                                   const double* w, const double* mu, const double* c, int iters, double tol, double* d, double* info,
                                   const JacProducts& J, bool masked);
// The one-pass solve: 4 launches to start (start, J^T t and its fold, first), 3 per iteration (the one-pass product, its fold,
// the vector kernel), none of them conditional.  c NULL: the unscaled step; else sc holds e and c o p.
hipError_t launch_lsq_solve_onepass(const JacLsqWork* work, int n, const LsqBuffers& ws, const LsqScaledBuffers& sc, const LsqOnepassBuffers& op,
                                    const double* b, const double* w, const double* mu, const double* c, int iters, double tol, double* d,
                                    double* info, const JacProducts& J);

// The Gram matrix (jac/gram.h).  prepare_gram_cg: as prepare_jac_normal, for the solve's LDS.
hipError_t launch_jac_gram(const JacGramWork* work, int n_work, const double* jac, const double* w, double* gram, hipStream_t stream);
hipError_t launch_jac_gram_mul(const JacGramMulWork* work, int n_work, const double* gram, const double* v, double* u, hipStream_t stream);
hipError_t launch_gram_cg(const JacGramSolveWork* work, int n_problems, int max_n, const double* gram, const double* z, const double* mu,
                          const double* scale, int iters, double tol, double* d, double* info, hipStream_t stream);
hipError_t prepare_gram_cg();

// The bounded LM driver (jac/lm.h), in the order twr_jac_lm_start and twr_jac_lm_step call them; between them the C ABI evaluates
// the batch.  B: the driver's workspace; x, lo, up: the caller's.
hipError_t launch_lm_free_set(const JacLsqWork* work, int n, const double* x, const double* lo, const double* up, const double* z,
                              const double* c_in, double* c_out, double* nfree, hipStream_t stream);
// x onto the box, the checks, the start of the records (mu = tau) and of the power iteration's vector
hipError_t launch_lm_project(const JacLsqWork* work, int n, double* x, const double* lo, const double* up, const LmBuffers& B, double tau,
                             hipStream_t stream);
// After eval(BOTH) at x: violation, b = -r, the column norms and the scale with the running maximum, z = J^T(w o b), the free set
hipError_t launch_lm_linearise(const JacLsqWork* work, int n, const double* x, const double* g, const double* lo, const double* up,
                               const LmBuffers& B, double merit_done, double rel_floor, int first, const JacProducts& J);
// mu0 = clamp(tau lambda_max(C_f J^T W_a J C_f)) by `iters` power iterations; borrows d (v), xt (cf o v), z (u) and gt (y)
hipError_t launch_lm_power(const JacLsqWork* work, int n, const LmBuffers& B, const LmParams& P, int iters, const JacProducts& J);
// xt = x + d on the box
hipError_t launch_lm_trial(const JacLsqWork* work, int n, const double* x, const double* lo, const double* up, const LmBuffers& B,
                           hipStream_t stream);
// After eval(VALUES) at xt into gt: its violation and merit, then accept / reject, mu and the counters
hipError_t launch_lm_accept(const JacLsqWork* work, int n, double* x, const LmBuffers& B, const LmParams& P, hipStream_t stream);

}  // namespace twr
