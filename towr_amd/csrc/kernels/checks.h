// Checks of a sampled trajectory between the constraint nodes (twr_batch_checks, twr_batch_check_scores): the rigid-body equation,
// terrain clearance, the friction pyramid and the range-of-motion box at every sample record of twr_batch_sample, and the
// per-problem fold of the results.  The kernels are in util_tu.hip.
//
// Check record of a sample:  [ t | residual: angular (3), linear (3) | per ee: contact clearance f_n cone rom ]; t and the contact
// flags are the sample record's own doubles.
// A check record is a function of the sample record, the problem's DevStruct (mass, gravity, inertia, friction, terrain) and the
// four fields of twr_model named below, and of nothing else.  Every function here is compiled without contraction, every sum is
// written in the order it is evaluated in, so a restatement in plainly rounded doubles (tests/check_points.py) gives the same
// bits -- the rule of joints.h, for the reason given there.  The orders:
//   R            base_frame_rotation (joints.h) of the record's quaternion w x y z
//   B            the symmetric body inertia of DevStruct::Ib: rows (Ib0 Ib1 Ib2), (Ib1 Ib3 Ib4), (Ib2 Ib4 Ib5)
//   A = R B      A[i][j] = R[i][0] B[0][j] + R[i][1] B[1][j] + R[i][2] B[2][j]
//   W = A R^T    W[i][j] = A[i][0] R[j][0] + A[i][1] R[j][1] + A[i][2] R[j][2]                 (I_w = R I_b R^T, row by row)
//   W v          (W v)[i] = W[i][0] v[0] + W[i][1] v[1] + W[i][2] v[2]                          for v = omega_dot and v = omega
//   a x b        (a[1] b[2] - a[2] b[1],  a[2] b[0] - a[0] b[2],  a[0] b[1] - a[1] b[0])
//   tau, fsum    start at 0; for e = 0 .. n_ee - 1 in turn: tau += f_e x (p_base - p_e), fsum += f_e   (component by component)
//   angular      (W omega_dot + omega x (W omega)) - tau
//   linear       m a - fsum on x and y, (m a - fsum) + m g on z
//   basis        v_n = (-hx, -hy, 1), v_t1 = (1, 0, hx), v_t2 = (0, 1, hy) at (p_e.x, p_e.y), each divided by
//                sqrt(v[0] v[0] + v[1] v[1] + v[2] v[2]) -- the normalised basis force_core forms (height_map.cc:93-139)
//   f . u        f[0] u[0] + f[1] u[1] + f[2] u[2]
//   cone         mu f_n - max(|f . t1|, |f . t2|), NaN if either is
//   rom          max over d = 0, 1, 2 in turn of |foot_B[d] - nominal_stance[e][d]| - max_dev[d], NaN if one of them is;
//                foot_B = base_frame (joints.h)
#pragma once
#include <stdint.h>

#include "../../../include/towr_amd.h"
#include "../device_tables.h"
#include "common.h"
#include "joints.h"
#include "terrain.h"

namespace twr {
constexpr int kCheckHead = 7;   // doubles in front of the legs of a check record: t, the six residuals
constexpr int kCheckLeg = 5;    // doubles per leg: contact clearance f_n cone rom
static_assert(TWR_CHECK_REC(4) == kCheckHead + kCheckLeg * 4, "check record layout");

// what the kernels read of a twr_model (passed by value)
struct CheckModel {
  double nominal[kMaxEE][3], max_dev[3];
};

// the body of a sample record -> t and the dynamics residual without the forces' part; R and the base position stay for the legs
struct CheckBody {
  double R[3][3], pb[3];
  double ang[3], lin[3];   // W omega_dot + omega x (W omega), m a: before tau and fsum
};
TWR_DEV void check_body(const double* __restrict__ r, const DevStruct* __restrict__ H, CheckBody& o) {
#pragma clang fp contract(off)
  base_frame_rotation(r[10], r[11], r[12], r[13], o.R);
  const double (&R)[3][3] = o.R;
  const double B[3][3] = {{H->Ib[0], H->Ib[1], H->Ib[2]}, {H->Ib[1], H->Ib[3], H->Ib[4]}, {H->Ib[2], H->Ib[4], H->Ib[5]}};
  double A[3][3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = R[i][0] * B[0][j] + R[i][1] * B[1][j] + R[i][2] * B[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) W[i][j] = A[i][0] * R[j][0] + A[i][1] * R[j][1] + A[i][2] * R[j][2];
  const double om[3] = {r[14], r[15], r[16]}, od[3] = {r[17], r[18], r[19]};
  double wd[3], wo[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    wd[i] = W[i][0] * od[0] + W[i][1] * od[1] + W[i][2] * od[2];
    wo[i] = W[i][0] * om[0] + W[i][1] * om[1] + W[i][2] * om[2];
  }
  o.ang[0] = wd[0] + (om[1] * wo[2] - om[2] * wo[1]);
  o.ang[1] = wd[1] + (om[2] * wo[0] - om[0] * wo[2]);
  o.ang[2] = wd[2] + (om[0] * wo[1] - om[1] * wo[0]);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    o.pb[d] = r[1 + d];
    o.lin[d] = H->mass * r[7 + d];
  }
}

// one leg of a sample record (l: its 13 doubles) -> its five doubles of the check record at o; tau and fsum take its force
TWR_DEV void check_leg(const double* __restrict__ l, int e, const DevStruct* __restrict__ H, const CheckModel& M, const CheckBody& b, double tau[3], double fsum[3],
                       double* __restrict__ o) {
#pragma clang fp contract(off)
  const double pe[3] = {l[1], l[2], l[3]}, f[3] = {l[10], l[11], l[12]};
  const double d[3] = {b.pb[0] - pe[0], b.pb[1] - pe[1], b.pb[2] - pe[2]};
  tau[0] += f[1] * d[2] - f[2] * d[1];
  tau[1] += f[2] * d[0] - f[0] * d[2];
  tau[2] += f[0] * d[1] - f[1] * d[0];
#pragma unroll
  for (int i = 0; i < 3; ++i) fsum[i] += f[i];
  const Terr t = terrain_eval(H, H->terrain_id, H->flat_height, pe[0], pe[1]);
  const double vb[3][3] = {{-t.hx, -t.hy, 1.0}, {1.0, 0.0, t.hx}, {0.0, 1.0, t.hy}};
  double dot[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double nr = sqrt(vb[k][0] * vb[k][0] + vb[k][1] * vb[k][1] + vb[k][2] * vb[k][2]);
    const double u[3] = {vb[k][0] / nr, vb[k][1] / nr, vb[k][2] / nr};
    dot[k] = f[0] * u[0] + f[1] * u[1] + f[2] * u[2];
  }
  double foot[3];
  base_frame(b.R, b.pb, pe, foot);
  double rom = fabs(foot[0] - M.nominal[e][0]) - M.max_dev[0];
#pragma unroll
  for (int k = 1; k < 3; ++k) rom = nan_max(rom, fabs(foot[k] - M.nominal[e][k]) - M.max_dev[k]);
  o[0] = l[0];
  o[1] = pe[2] - t.h;
  o[2] = dot[0];
  o[3] = H->mu * dot[0] - nan_max(fabs(dot[1]), fabs(dot[2]));
  o[4] = rom;
}

// the head of the check record once every leg has added its force
TWR_DEV void check_residual(double t, const DevStruct* __restrict__ H, const CheckBody& b, const double tau[3], const double fsum[3],
                            double* __restrict__ o) {
#pragma clang fp contract(off)
  o[0] = t;
#pragma unroll
  for (int d = 0; d < 3; ++d) o[1 + d] = b.ang[d] - tau[d];
  o[4] = b.lin[0] - fsum[0];
  o[5] = b.lin[1] - fsum[1];
  o[6] = (b.lin[2] - fsum[2]) + H->mass * H->gravity;
}

// a whole record: N_EE legs from r (global memory or the LDS image of the item) to o
template <int N_EE>
TWR_DEV void check_record(const double* __restrict__ r, const DevStruct* __restrict__ H, const CheckModel& M, double* __restrict__ o) {
  CheckBody b;
  check_body(r, H, b);
  double tau[3] = {0.0, 0.0, 0.0}, fsum[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int e = 0; e < N_EE; ++e) check_leg(r + 20 + 13 * e, e, H, M, b, tau, fsum, o + kCheckHead + kCheckLeg * e);
  check_residual(r[0], H, b, tau, fsum, o);
}

// ---------------------------------------------------------------- the per-problem fold (one wave per problem, as JointFold)
struct CheckFold {
  int n;
  double lin, ang, swing_clear, stance_clear, fn, cone, rom;
  TWR_DEV void init() {
    n = 0;
    lin = ang = stance_clear = 0.0;
    swing_clear = fn = cone = 1e20;
    rom = -__builtin_inf();
  }
  // the lane's record of this round (rec: a live sample's check record)
  TWR_DEV void take(const double* __restrict__ rec, int n_ee) {
    ++n;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      ang = nan_max(ang, fabs(rec[1 + d]));
      lin = nan_max(lin, fabs(rec[4 + d]));
    }
    for (int e = 0; e < n_ee; ++e) {
      const double* l = rec + kCheckHead + kCheckLeg * e;
      if (l[0] != 0.0) {
        stance_clear = nan_max(stance_clear, fabs(l[1]));
        fn = nan_min(fn, l[2]);
        cone = nan_min(cone, l[3]);
      } else {
        swing_clear = nan_min(swing_clear, l[1]);
      }
      rom = nan_max(rom, l[4]);
    }
  }
  TWR_DEV void finish(int lane, double* __restrict__ out) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      n += __shfl_xor(n, o);
      lin = nan_max(lin, __shfl_xor(lin, o));
      ang = nan_max(ang, __shfl_xor(ang, o));
      swing_clear = nan_min(swing_clear, __shfl_xor(swing_clear, o));
      stance_clear = nan_max(stance_clear, __shfl_xor(stance_clear, o));
      fn = nan_min(fn, __shfl_xor(fn, o));
      cone = nan_min(cone, __shfl_xor(cone, o));
      rom = nan_max(rom, __shfl_xor(rom, o));
    }
    if (lane == 0) {
      out[0] = (double)n;
      out[1] = lin;
      out[2] = ang;
      out[3] = swing_clear;
      out[4] = stance_clear;
      out[5] = fn;
      out[6] = cone;
      out[7] = rom;
    }
  }
};
}  // namespace twr
