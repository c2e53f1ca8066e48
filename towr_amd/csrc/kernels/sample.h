// Sampling a solution at a time (twr_batch_sample, twr_batch_eval_joint_scores): the device functions under sample_kernel and
// contact_plan_kernel of util_tu.hip, includable on their own (tests/attitude_probe.hip runs sample_angular per point).
#pragma once
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "joints.h"
#include "spline_math.h"

namespace twr {
// ---------------------------------------------------------------- trajectory sampling
// fpowr::GetTrajectory (fpowr/include/fpowr/footstep_plan_extractor.h:19-53) for a batch of solutions: lane =
// sample.  Durations (constants of the structure, or recomputed from x with optimised timings) go to LDS once
// per workgroup; every lane accumulates its sample time like the reference (t += dt), locates the active
// polynomial of every spline and evaluates position / velocity / acceleration in Hermite basis form.
TWR_DEV void sample_spline(const double* __restrict__ xp, const PolyDesc& pd, double tl, double T, double p[3], double v[3],
                           double a[3]) {
  double X[12], nv[4][3], wp[4], wv[4], wa[4];
  gather12c(xp, pd.xbase, pd.cand, X);
  node_values(slots_of(pd.cand), meta_shared(pd.meta), X, nv);
  hermite_all(tl, 1.0 / T, wp, wv, wa);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    p[d] = wp[0] * nv[0][d] + wp[1] * nv[1][d] + wp[2] * nv[2][d] + wp[3] * nv[3][d];
    v[d] = wv[0] * nv[0][d] + wv[1] * nv[1][d] + wv[2] * nv[2][d] + wv[3] * nv[3][d];
    a[d] = wa[0] * nv[0][d] + wa[1] * nv[1][d] + wa[2] * nv[2][d] + wa[3] * nv[3][d];
  }
}
// The base of a sample at time t, shared by sample_kernel and eval_joint_scores_kernel (which must form the very same doubles:
// the compiler's choice of fused operations depends on what else uses a product, so that kernel keeps every result alive).
struct BaseSample {
  double p[3], v[3], a[3];       // base-lin
  double e3[3], ed[3], edd[3];   // base-ang: Euler angles, rates, accelerations
};
struct BaseAngular {
  double q[4];                   // x y z w
  double omega[3], omega_dot[3];
};
// base-lin / base-ang (NodesVariablesAll: [p0 v0 p1 v1] x 3 of polynomial q at 6 q)
TWR_DEV void sample_base(const double* __restrict__ xp, const SampleTables* ST, const double* s_bd, double t, BaseSample& B) {
  double tl;
  const int qb = locate_segment(s_bd, ST->n_base, t, tl);
  double wp[4], wv[4], wa[4];
  hermite_all(tl, 1.0 / s_bd[qb], wp, wv, wa);
  const double* xl = xp + ST->off_lin + 6 * qb;
  const double* xa = xp + ST->off_ang + 6 * qb;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    B.p[d] = wp[0] * xl[d] + wp[1] * xl[3 + d] + wp[2] * xl[6 + d] + wp[3] * xl[9 + d];
    B.v[d] = wv[0] * xl[d] + wv[1] * xl[3 + d] + wv[2] * xl[6 + d] + wv[3] * xl[9 + d];
    B.a[d] = wa[0] * xl[d] + wa[1] * xl[3 + d] + wa[2] * xl[6 + d] + wa[3] * xl[9 + d];
    B.e3[d] = wp[0] * xa[d] + wp[1] * xa[3 + d] + wp[2] * xa[6 + d] + wp[3] * xa[9 + d];
    B.ed[d] = wv[0] * xa[d] + wv[1] * xa[3 + d] + wv[2] * xa[6 + d] + wv[3] * xa[9 + d];
    B.edd[d] = wa[0] * xa[d] + wa[1] * xa[3 + d] + wa[2] * xa[6 + d] + wa[3] * xa[9 + d];
  }
}
TWR_DEV void sample_angular(const BaseSample& B, BaseAngular& A) {
  Rot ro;
  rotation(B.e3, ro);
  quat_of_rotation(ro.R, A.q);
  {  // omega = M edot, omega_dot = Mdot edot + M eddot (euler_converter.cc:58-83,133-166)
    const double sy = ro.sy, cy = ro.cy, sz = ro.sz, cz = ro.cz;
    const double xd = B.ed[0], yd = B.ed[1], zd = B.ed[2];
    const double Mx[3] = {cy * cz, cy * sz, -sy}, My[3] = {-sz, cz, 0.0};
    const double Mdx[3] = {-cz * sy * yd - cy * sz * zd, cy * cz * zd - sy * sz * yd, -cy * yd};
    const double Mdy[3] = {-cz * zd, -sz * zd, 0.0};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      A.omega[i] = Mx[i] * xd + My[i] * yd + (i == 2 ? zd : 0.0);
      A.omega_dot[i] = Mdx[i] * xd + Mdy[i] * yd + Mx[i] * B.edd[0] + My[i] * B.edd[1] + (i == 2 ? B.edd[2] : 0.0);
    }
  }
}
// keeps a value computed where nothing stores it
TWR_DEV void keep_alive(double v) { asm volatile("" ::"v"(v)); }
}  // namespace twr
