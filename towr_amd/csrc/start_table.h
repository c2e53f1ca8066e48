// The start table of a structure and its decode: where every entry of x0, x_l and x_u of a planning request comes from.
// One header for the host (Structure::StartHost, structure.cc) and the device (kernels/start.h): the functions below are the
// ONLY statement of the arithmetic of Structure::InitialGuess / VariableBounds besides those two functions themselves, and
// restate it operation for operation, so that both executors give the bits of the reference's
// NlpFormulation::Make*Variables + NodesVariables::SetByLinearInterpolation / AddStartBound / AddFinalBound
// (nlp_formulation.cc:95-181, nodes_variables.cc:52-62,152-181).
//
// A request record is kStartRequest doubles (include/towr_amd.h TWR_START_REC):
//   [0, 12)  initial base  {lin p, lin v, ang p, ang v}
//   [12, 24) final base    (the same order)
//   [24, 36) initial foot positions, 3 per end-effector
// A start table is StartHeader | double dur[n_dur] | StartRec rec[n_vars], built by Structure::BuildStartTable.
#pragma once
#include <stdint.h>

#include "device_tables.h"

#if defined(__HIPCC__)
#define TWR_START_HD __host__ __device__ inline
#else
#define TWR_START_HD inline
#endif
// no fused multiply-add anywhere in the decode (kernels/terrain.h says what one costs): a[d] + n / (N - 1) * dp[d] and the
// rotated stance are separately rounded operations in the reference
#if defined(__clang__)
#define TWR_START_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define TWR_START_NO_CONTRACT
#endif

namespace twr {

constexpr int kStartRequest = 36;              // doubles of a request record
constexpr int kStartSplines = 2 + 2 * kMaxEE;  // base-lin, base-ang, ee-motion e at 2 + e, ee-force e at 2 + kMaxEE + e
constexpr int kStartItem = 256;                // variables of one work item (= threads of a workgroup of start_kernel)
enum : uint8_t { kStartZero = 0, kStartNode = 1, kStartDuration = 2 };        // StartRec::value
enum : uint8_t { kStartNoBound = 0, kStartFixed = 1, kStartDurationBox = 2 }; // StartRec::bound

struct StartRec {    // one optimisation variable
  uint16_t node;     // kStartNode: the LATER of the nodes that share the variable; kStartDuration: index into dur[]
  uint8_t spline;    // kStartNode: the spline, see kStartSplines
  uint8_t comp;      // kStartNode: 3 * derivative + dimension
  uint8_t value;     // kStartZero / kStartNode / kStartDuration
  uint8_t bound;     // kStartNoBound / kStartFixed / kStartDurationBox
  uint8_t slot;      // kStartFixed: both bounds are entry `slot` of the request record
  uint8_t pad;
};
static_assert(sizeof(StartRec) == 8, "StartRec layout");

struct StartHeader {   // what the formulas need beyond DevStruct
  int32_t n_vars, n_ee;
  int32_t nm1[kStartSplines];   // n_nodes - 1 of every spline (0: no such spline)
  int32_t n_dur;
  uint32_t o_dur, o_rec;        // byte offsets inside the table
  uint32_t pad;
  double T, mass, gravity;
  double stance[kMaxEE][3];     // KinematicModel::GetNominalStanceInBase
};
static_assert(sizeof(StartHeader) % 8 == 0, "StartHeader layout");

struct StartWork {   // cnt <= kStartItem consecutive variables of one problem (batch_plan.h PlanStart)
  uint64_t table;    // the structure's start table (StartHeader)
  uint64_t blob;     // the structure's DevStruct: terrain constants and the live map
  int64_t x_off;     // the problem's x
  int32_t v0, cnt;   // variables [v0, v0 + cnt) of the problem
  int32_t problem;   // whose request record
  int32_t pad;
};
static_assert(sizeof(StartWork) == 40, "StartWork layout");

struct StartEnd {   // the endpoints of one spline's linear interpolation: start, difference, difference / T
  double a[3], dp[3], vel[3];
};

// NodesVariables::SetByLinearInterpolation (nodes_variables.cc:126-150): what depends on the endpoints alone
TWR_START_HD void start_end(const double a[3], const double b[3], double T, StartEnd& o) {
  TWR_START_NO_CONTRACT
  for (int d = 0; d < 3; ++d) {
    o.a[d] = a[d];
    o.dp[d] = b[d] - a[d];
    o.vel[d] = o.dp[d] / T;
  }
}
// base-lin's final position: the goal's x / y on the terrain (nlp_formulation.cc:105-108); h = terrain height at the goal
TWR_START_HD void start_final_base(const double lin1[3], double h, const double stance0[3], double fl[3]) {
  TWR_START_NO_CONTRACT
  fl[0] = lin1[0];
  fl[1] = lin1[1];
  fl[2] = h - stance0[2];
}
// x / y (and the z the terrain then replaces) of a final foothold: final_base.lin + GetRotationMatrixBaseToWorld((0, 0, yaw)) *
// nominal stance (nlp_formulation.cc:141-148), the expression of Structure::InitialGuess term for term with cos(0.0) = 1 and
// sin(0.0) = 0 written out -- the products with that zero stay (their signs reach the sums).  sz / cz: sin / cos of the yaw.
TWR_START_HD void start_foothold(const double lin1[3], double sz, double cz, const double nb[3], double fe[3]) {
  TWR_START_NO_CONTRACT
  const double c0 = 1.0, s0 = 0.0;
  const double R[3][3] = {{c0 * cz, cz * s0 * s0 - c0 * sz, s0 * sz + c0 * cz * s0},
                          {c0 * sz, c0 * cz + s0 * s0 * sz, c0 * s0 * sz - cz * s0},
                          {-s0, c0 * s0, c0 * c0}};
  for (int i = 0; i < 3; ++i) fe[i] = lin1[i] + (R[i][0] * nb[0] + R[i][1] * nb[1] + R[i][2] * nb[2]);
}
// the constant force of MakeForceVariables (nlp_formulation.cc:158-181)
TWR_START_HD void start_force(double mass, double gravity, int n_ee, double f[3]) {
  TWR_START_NO_CONTRACT
  f[0] = 0.0;
  f[1] = 0.0;
  f[2] = mass * gravity / n_ee;
}

// (record, per-spline endpoints) -> x
TWR_START_HD double start_value(const StartRec r, const StartEnd* ends, const int32_t* nm1, const double* dur) {
  TWR_START_NO_CONTRACT
  if (r.value == kStartNode) {
    const StartEnd& e = ends[r.spline];
    const int d = r.comp % 3;
    if (r.comp >= 3) return e.vel[d];
    return e.a[d] + (int)r.node / static_cast<double>(nm1[r.spline]) * e.dp[d];
  }
  if (r.value == kStartDuration) return dur[r.node];   // PhaseDurations::GetValues (phase_durations.cc:66-75)
  return 0.0;
}
// (record, request) -> lower, upper
TWR_START_HD void start_bounds(const StartRec r, const double* request, double& lower, double& upper) {
  if (r.bound == kStartFixed) {
    lower = upper = request[r.slot];
  } else if (r.bound == kStartDurationBox) {   // Parameters::bound_phase_duration_ (parameters.cc:52)
    lower = 0.2;
    upper = 1.0;
  } else {                                     // ifopt::NoBound
    lower = -1e20;
    upper = 1e20;
  }
}

}  // namespace twr
