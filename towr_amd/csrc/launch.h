// Host launchers of the kernels (launch_eval, prepare_phase_kernels: kernels.hip; the utility kernels': util_tu.hip), called by the C ABI (capi.cc; capi_jac.cc reaches them through twr_batch_eval; the solver kernels' launchers are jac_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "batch_plan.h"
#include "eval_plan.h"

namespace twr {

struct EvalBuffers {   // device memory of one evaluation: the batch's work lists and the caller's x / g / jac
  const DynWork* dyn;
  const RomWork* rom;
  const NodeWork* node;
  const FlatWork* flat;
  const FamWork* fam[4];
  const PDynWork* pdyn;
  const LocWork* ploc;
  const RomPhaseWork* prom;
  const double* x;
  double* g;
  double* jac;
  double* dump;   // kDynDump doubles
  // candidate scoring (EvalShape::flags kEvalScores / kEvalBest): the batch's scoring lists and slab, the caller's score table,
  // and twr_batch_best's arguments and scratch
  const uint64_t* score_blob;
  const int32_t* score_first;
  const int32_t* score_slot;
  double* slab;
  double* scores;
  unsigned families;
  double index_offset;
  double* best_partial;
  unsigned* best_counter;
  double* best;
};
// Issues the launches PlanEval plans for `shape` (ev: four events when shape.events); returns the first error.
hipError_t launch_eval(const EvalShape& shape, const EvalBuffers& buf, hipStream_t stream, hipEvent_t* ev);
hipError_t prepare_phase_kernels(int pdyn_img_cap, int prom_img_cap);
hipError_t launch_check(int n_problems, const int64_t* g_off, const int64_t* j_off, const double* g, const double* jac,
                        int32_t* status, int flags, hipStream_t stream);
hipError_t launch_score(const NodeWork* work, int n_problems, const double* g, double* scores, hipStream_t stream);
int best_max_blocks();
hipError_t launch_best(const double* scores, int n, unsigned families, double* partial, unsigned* counter, double* best, double index_offset,
                       hipStream_t stream);
hipError_t launch_contact_plan(const NodeWork* work, int n_problems, const double* x, double* out, int32_t* counts, double dt,
                               double time_horizon, int n_samples_max, int max_steps, hipStream_t stream);
hipError_t launch_planes(const double* plan, const int32_t* counts, const double* poly_xy, const int32_t* poly_start, int n_polys,
                         int n_problems, int max_steps, int n_ee, int32_t* plane_index, hipStream_t stream);
hipError_t launch_sample(const SampleWork* work, int n_work, const double* x, double* out, double dt, const double* times,
                         hipStream_t stream);
// Joint-space trajectories (kernels/joints.h): sample records -> joint records over sample_kernel's work list; joint records
// -> eight scores per problem; x -> the same scores without a trajectory.  n_samples_max: the largest sample count of a problem.
hipError_t launch_joints(const SampleWork* work, int n_work, const double* traj, int64_t traj_stride, double* out, int64_t joint_stride,
                         int n_ee, const twr_leg_kinematics& kin, hipStream_t stream);
hipError_t launch_joint_scores(const NodeWork* work, int n_problems, const double* joints, int64_t joint_stride, double dt,
                               int n_samples_max, double* scores, const twr_leg_kinematics& kin, hipStream_t stream);
hipError_t launch_eval_joint_scores(const NodeWork* work, int n_problems, const double* x, double dt, int n_samples_max, double* scores,
                                    const twr_leg_kinematics& kin, hipStream_t stream);
// Trajectory checks (kernels/checks.h): sample records -> check records over sample_kernel's work list (model: n_ee, nominal_stance
// and max_dev are read; n_ee in 1..4); check records -> eight scores per problem.
hipError_t launch_checks(const SampleWork* work, int n_work, const double* traj, int64_t traj_stride, double* out, int64_t check_stride,
                         const twr_model& model, hipStream_t stream);
hipError_t launch_check_scores(const NodeWork* work, int n_problems, const double* checks, int64_t check_stride, double dt,
                               int n_samples_max, double* scores, hipStream_t stream);
// dst (a batch's copy of a `Grid` layer, start index (0,0)) from src (the same sizes, start index (start_x, start_y)), and the map
// centre into the n_hdr headers whose DevStruct::grid_px lies hdr_off[k] bytes into arena (kernels/grid_map_update.h).  One launch.
hipError_t launch_grid_map_update(const float* src, float* dst, int size_x, int size_y, int start_x, int start_y, double pos_x,
                                  double pos_y, void* arena, const uint64_t* hdr_off, int n_hdr, hipStream_t stream);
// x0 / x_l / x_u of the batch from request records on the device (kernels/start.h): work list of PlanStart, `stride` doubles
// between two problems' records (0: one record for all); x / lower / upper in the layout of x_off, each may be null (not all).
hipError_t launch_start(const StartWork* work, int n_work, const double* request, int64_t stride, double* x, double* lower, double* upper,
                        hipStream_t stream);

}  // namespace twr
