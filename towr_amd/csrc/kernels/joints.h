// Leg inverse kinematics of a sampled trajectory (twr_batch_joints, twr_batch_joint_scores, twr_batch_eval_joint_scores): the
// reference's Go1legInverseKinematics::GetJointAngles + EnforceLimits (src/go1/go1leg_inverse_kinematics.cc:16-115) and
// InverseKinematicsGo1::GetAllJointAngles (src/go1/inverse_kinematics_go1.cc:8-47) on a twr_leg_kinematics descriptor, the
// frame change in front of them, and the per-problem fold of the results.  The kernels are in util_tu.hip.
#pragma once
#include <stdint.h>

#include "../../../include/towr_amd.h"
#include "../device_tables.h"
#include "common.h"
#include "spline_math.h"

namespace twr {
constexpr int kJointLeg = 5;   // doubles per leg of a joint record: q_HAA q_HFE q_KFE flags over-reach
static_assert(TWR_JOINT_REC(4) == 1 + kJointLeg * 4, "joint record layout");
enum : int { kIkBeta = 1, kIkGamma = 2, kIkHaa = 4, kIkHfe = 8, kIkKfe = 16, kIkNan = 32 };

// Eigen::Quaterniond(R) (euler_converter.cc:51-56; Eigen 3.3 Quaternion.h, quaternionbase_assign_impl); q = x y z w
// The trace is summed as (m00 + m11) + m22, like the oracle's and the Eigen subset's statement of it (DESIGN 5 "Base attitude").
// No contraction: the reference converts the ROUNDED entries of R.  Inlined behind rotation(), whose entries are products, the
// sums and differences below were otherwise fused with those products, so that q was not a function of R (tests/attitude_probe.hip
// found q one ulp off the conversion of the very R the same thread had stored) and depended on what else used the products.
TWR_DEV void quat_of_rotation(const double (&m)[3][3], double q[4]) {
#pragma clang fp contract(off)
  double tr = m[0][0] + m[1][1] + m[2][2];
  if (tr > 0) {
    tr = sqrt(tr + 1.0);
    q[3] = 0.5 * tr;
    tr = 0.5 / tr;
    q[0] = (m[2][1] - m[1][2]) * tr;
    q[1] = (m[0][2] - m[2][0]) * tr;
    q[2] = (m[1][0] - m[0][1]) * tr;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > (i == 0 ? m[0][0] : m[1][1])) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    auto M = [&](int r, int c) { return sel3(r, sel3(c, m[0][0], m[0][1], m[0][2]), sel3(c, m[1][0], m[1][1], m[1][2]),
                                             sel3(c, m[2][0], m[2][1], m[2][2])); };
    tr = sqrt(M(i, i) - M(j, j) - M(k, k) + 1.0);
    const double qi = 0.5 * tr;
    tr = 0.5 / tr;
    const double qw = (M(k, j) - M(j, k)) * tr, qj = (M(j, i) + M(i, j)) * tr, qk = (M(k, i) + M(i, k)) * tr;
    q[3] = qw;
    q[0] = i == 0 ? qi : (j == 0 ? qj : qk);
    q[1] = i == 1 ? qi : (j == 1 ? qj : qk);
    q[2] = i == 2 ? qi : (j == 2 ? qj : qk);
  }
}

// Feet in the base frame: R(q)^T (p_ee - p_base), R(q) = Eigen's toRotationMatrix of the NORMALISED quaternion (w x y z as in
// a sample record).  base_frame_rotation once per sample, base_frame once per foot.
// (no contraction in either: the fused kernel and the kernel that reads records must round alike whatever surrounds the call)
TWR_DEV void base_frame_rotation(double w, double x, double y, double z, double R[3][3]) {
#pragma clang fp contract(off)
  double n = sqrt(x * x + y * y + z * z + w * w);
  // A quaternion that cannot be normalised is NaN, not a rotation: |q| = 0 and a NaN component give NaN by themselves (0 / 0),
  // but a norm of Inf (an Inf component, or squares that overflow from 1e155 on) would divide every finite component to 0 and
  // R to the identity.
  if (!(n < __builtin_inf())) n = n - n;
  w /= n; x /= n; y /= n; z /= n;
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz;         R[0][2] = txz + twy;
  R[1][0] = txy + twz;         R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy;         R[2][1] = tyz + twx;         R[2][2] = 1.0 - (txx + tyy);
}
TWR_DEV void base_frame(const double R[3][3], const double p_base[3], const double p_ee[3], double out[3]) {
#pragma clang fp contract(off)
  const double d[3] = {p_ee[0] - p_base[0], p_ee[1] - p_base[1], p_ee[2] - p_base[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = R[0][i] * d[0] + R[1][i] * d[1] + R[2][i] * d[2];
}

struct LegIk {
  double q[3];                  // HAA, HFE, KFE after EnforceLimits
  double cos_beta, cos_gamma;   // the law-of-cosines arguments before the clamp
  double r;                     // HFE-to-foot distance
  int flags;                    // kIk*
};
// std::max(lo, std::min(hi, v)) of the reference's clamp: a NaN v becomes hi
TWR_DEV double ik_clamp(double v, double lo, double hi) {
  const double m = v < hi ? v : hi;
  return lo < m ? m : lo;
}
// GetJointAngles on a foot in the hip frame, operation for operation and without contraction: the 3x3 product with its 0 and 1
// entries (0 * Inf is the reference's NaN), the sums left to right, the signed zeros of atan2.
TWR_DEV void leg_ik(const double p[3], int bend, const twr_leg_kinematics& K, LegIk& o) {
#pragma clang fp contract(off)
  double q_haa = -atan2(p[1], -p[2]);
  const double c = cos(q_haa), s = sin(q_haa);
  double xr[3];
  xr[0] = 1.0 * p[0] + 0.0 * p[1] + 0.0 * p[2];
  xr[1] = 0.0 * p[0] + c * p[1] + (-s) * p[2];
  xr[2] = 0.0 * p[0] + s * p[1] + c * p[2];
#pragma unroll
  for (int d = 0; d < 3; ++d) xr[d] += K.hfe_to_haa[d];
  const double sq = xr[0] * xr[0] + xr[2] * xr[2];
  const double lu = K.length_thigh, ll = K.length_shank;
  const double alpha = (bend == 0 ? atan2(-xr[2], xr[0]) : atan2(-xr[2], -xr[0])) - 0.5 * 3.14159265358979323846;
  const double r = sqrt(sq);
  const double cb = (lu * lu + sq - ll * ll) / (2. * lu * r);
  double q_hfe = alpha + acos(ik_clamp(cb, -1.0, 1.0));
  const double cg = (ll * ll + lu * lu - sq) / (2. * ll * lu);
  double q_kfe = acos(ik_clamp(cg, -1.0, 1.0)) - 3.14159265358979323846;
  int flags = (!(-1.0 <= cb && cb <= 1.0) ? kIkBeta : 0) | (!(-1.0 <= cg && cg <= 1.0) ? kIkGamma : 0);
  auto enforce = [&](double& v, int j, int bit) {   // EnforceLimits: a NaN stays
    if (v > K.q_max[j]) { v = K.q_max[j]; flags |= bit; }
    if (v < K.q_min[j]) { v = K.q_min[j]; flags |= bit; }
  };
  enforce(q_haa, 0, kIkHaa);
  enforce(q_hfe, 1, kIkHfe);
  enforce(q_kfe, 2, kIkKfe);
  if (q_haa != q_haa || q_hfe != q_hfe || q_kfe != q_kfe) flags |= kIkNan;
  o.q[0] = q_haa; o.q[1] = q_hfe; o.q[2] = q_kfe;
  o.cos_beta = cb; o.cos_gamma = cg; o.r = r; o.flags = flags;
}
// GetAllJointAngles for leg e: mirrored onto the front-left leg, minus its hip offset
TWR_DEV void leg_ik_of_foot(const double foot_B[3], int e, const twr_leg_kinematics& K, LegIk& o) {
#pragma clang fp contract(off)
  double h[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) h[d] = foot_B[d] * K.mirror[e][d] - K.base_to_hip[d];
  leg_ik(h, K.knee_bend[e], K, o);
}
// how far the foot lies outside the annulus the two links reach, in metres (a NaN r gives NaN)
TWR_DEV double over_reach(double r, const twr_leg_kinematics& K) {
  const double lu = K.length_thigh, ll = K.length_shank;
  if (r != r) return r;
  return fmax(fmax(r - (lu + ll), fabs(lu - ll) - r), 0.0);
}
// one leg of a joint record
TWR_DEV void put_leg(double* __restrict__ o, const LegIk& k, const twr_leg_kinematics& K) {
  o[0] = k.q[0]; o[1] = k.q[1]; o[2] = k.q[2];
  o[3] = (double)k.flags;
  o[4] = over_reach(k.r, K);
}

// ---------------------------------------------------------------- the per-problem fold (one wave per problem)
// Every lane folds its own samples round after round, then one xor tree over the 64 lanes: maxima, minima and counts only,
// so the result does not depend on where the problem sits, and no atomics.
TWR_DEV double nan_min(double a, double b) { return (a != a || b != b) ? (a != a ? a : b) : fmin(a, b); }
struct JointFold {
  double prev[kMaxEE][3];   // the angles of the previous round's lane 63 (wave-uniform)
  int n, unreachable, limited, nans, first;
  double over, vel, margin;
  TWR_DEV void init() {
    n = unreachable = limited = nans = 0;
    first = 0x7fffffff;
    over = vel = 0.0;
    margin = 1e20;
#pragma unroll
    for (int e = 0; e < kMaxEE; ++e) prev[e][0] = prev[e][1] = prev[e][2] = 0.0;
  }
  // one round: lane's sample s_idx (live or not) with its legs' angles q, flags fl (as in the record) and over-reach ov
  TWR_DEV void round(int lane, int s_idx, bool live, int n_ee, const double q[kMaxEE][3], const int fl[kMaxEE], const double ov[kMaxEE],
                     double dt, const twr_leg_kinematics& K) {
    bool unreach = false;
#pragma unroll
    for (int e = 0; e < kMaxEE; ++e) {   // (unrolled: the per-leg arrays stay in registers)
      if (e >= n_ee) continue;
      double qp[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double below = __shfl(q[e][j], (lane + 63) & 63);
        qp[j] = lane == 0 ? prev[e][j] : below;
        prev[e][j] = __shfl(q[e][j], 63);
      }
      if (!live) continue;
      if (fl[e] & (kIkBeta | kIkGamma)) { ++unreachable; unreach = true; }
      if (fl[e] & (kIkHaa | kIkHfe | kIkKfe)) ++limited;
      if (fl[e] & kIkNan) ++nans;
      over = nan_max(over, ov[e]);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        if (s_idx > 0) vel = nan_max(vel, fabs(q[e][j] - qp[j]) / dt);
        if (fl[e] == 0) margin = nan_min(margin, fmin(q[e][j] - K.q_min[j], K.q_max[j] - q[e][j]));
      }
    }
    if (live) ++n;
    if (live && unreach && s_idx < first) first = s_idx;
  }
  TWR_DEV void finish(int lane, double* __restrict__ out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      n += __shfl_xor(n, o);
      unreachable += __shfl_xor(unreachable, o);
      limited += __shfl_xor(limited, o);
      nans += __shfl_xor(nans, o);
      first = min(first, __shfl_xor(first, o));
      over = nan_max(over, __shfl_xor(over, o));
      vel = nan_max(vel, __shfl_xor(vel, o));
      margin = nan_min(margin, __shfl_xor(margin, o));
    }
    if (lane == 0) {
      out[0] = (double)n;
      out[1] = (double)unreachable;
      out[2] = (double)limited;
      out[3] = over;
      out[4] = vel;
      out[5] = margin;
      out[6] = (double)nans;
      out[7] = first == 0x7fffffff ? -1.0 : (double)first;
    }
  }
};
}  // namespace twr
