"""towr_amd -- MI355X-native evaluation of towr's NLP constraint/Jacobian callback.

Thin ctypes layer over libtowr_amd.so (C ABI in include/towr_amd.h).  There is no CPU
fallback: every evaluation runs the HIP kernels; importing on a box without the built
library raises, evaluating without a GPU raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TWR_AMD_LIB") or os.path.join(_HERE, "libtowr_amd.so")   # (override: diagnostic builds)

MAX_EE, MAX_PHASES, NAME_LEN = 4, 32, 40
ROBOTS = {"monoped": 0, "biped": 1, "hyq": 2, "anymal": 3, "go1": 4}
TERRAINS = {"flat": 0, "block": 1, "stairs": 2, "gap": 3, "slope": 4, "chimney": 5, "chimney_lr": 6, "csv": 7,
            "grid_map": 8}
EVAL_VALUES, EVAL_JACOBIAN, EVAL_BOTH, EVAL_CHECK = 1, 2, 3, 4
SET_TERRAIN, SET_DYNAMIC, SET_BASE_ACC, SET_ROM, SET_FORCE, SET_SWING, SET_TOTAL_TIME = 1, 2, 4, 8, 16, 32, 64
SET_BASE_ROM = 128
SETS_HOT_PATH, SETS_TOWR_DEFAULT, SETS_ALL, SETS_EVERY = 27, 63, 127, 255  # TWR_SETS_* of include/towr_amd.h
FAMILIES = ("terrain", "dynamic", "splineacc", "rangeofmotion", "force", "swing", "totalduration", "baseMotion")  # twr_batch_score
SUPPORTS_OPTIMISED_TIMINGS = True  # TWR_SET_TOTAL_TIME has a device path


class Model(C.Structure):
    _fields_ = [("n_ee", C.c_int32), ("terrain_id", C.c_int32), ("mass", C.c_double), ("inertia", C.c_double * 6),
                ("nominal_stance", (C.c_double * 3) * MAX_EE), ("max_dev", C.c_double * 3), ("gravity", C.c_double),
                ("friction", C.c_double), ("force_limit", C.c_double), ("flat_height", C.c_double)]


class Schedule(C.Structure):
    _fields_ = [("n_ee", C.c_int32), ("n_phases", C.c_int32 * MAX_EE), ("in_contact_at_start", C.c_int32 * MAX_EE),
                ("phase_durations", (C.c_double * MAX_PHASES) * MAX_EE)]

    def durations(self):
        return [list(self.phase_durations[e][:self.n_phases[e]]) for e in range(self.n_ee)]

    def contact(self):
        return [int(self.in_contact_at_start[e]) for e in range(self.n_ee)]


class Params(C.Structure):
    _fields_ = [("dt_dynamic", C.c_double), ("dt_rom", C.c_double), ("duration_base_poly", C.c_double),
                ("polys_per_swing", C.c_int32), ("polys_per_stance_force", C.c_int32),
                ("constraint_sets", C.c_int32), ("reserved_", C.c_int32),
                ("dt_base_motion", C.c_double), ("base_z_init", C.c_double)]


class Sizes(C.Structure):
    _fields_ = [("n_vars", C.c_int32), ("n_rows", C.c_int32), ("nnz", C.c_int32), ("n_var_sets", C.c_int32),
                ("n_con_sets", C.c_int32), ("k_dynamic", C.c_int32), ("k_rom", C.c_int32)]


class SetInfo(C.Structure):
    _fields_ = [("name", C.c_char * NAME_LEN), ("offset", C.c_int32), ("size", C.c_int32),
                ("nnz_offset", C.c_int32), ("nnz", C.c_int32)]


class LaunchStep(C.Structure):
    """twr_launch_step: one launch of a planned call (Batch.eval_plan)."""
    _fields_ = [("kernel", C.c_char * 32), ("instantiation", C.c_char * 48), ("store", C.c_char * 8), ("nit", C.c_int32),
                ("xc", C.c_int32), ("grid", C.c_int32), ("block", C.c_int32), ("lds_bytes", C.c_int32), ("uniform_kinds", C.c_int32)]


class LegKinematics(C.Structure):
    """twr_leg_kinematics: one leg chain and how the legs map onto the front-left one (leg_kinematics_preset)."""
    _fields_ = [("n_ee", C.c_int32), ("knee_bend", C.c_int32 * 4), ("mirror", (C.c_double * 3) * 4), ("base_to_hip", C.c_double * 3),
                ("hfe_to_haa", C.c_double * 3), ("length_thigh", C.c_double), ("length_shank", C.c_double),
                ("q_min", C.c_double * 3), ("q_max", C.c_double * 3)]


JOINT_SCORE_REC = 8   # TWR_JOINT_SCORE_REC
IK_FLAGS = dict(beta_clamped=1, gamma_clamped=2, haa_limit=4, hfe_limit=8, kfe_limit=16, nan=32)


def joint_rec(n_ee):
    """TWR_JOINT_REC(n_ee): doubles per joint record, [t | per leg: q_HAA q_HFE q_KFE flags over_reach]"""
    return 1 + 5 * n_ee


CHECK_SCORE_REC = 8   # TWR_CHECK_SCORE_REC


def check_rec(n_ee):
    """TWR_CHECK_REC(n_ee): doubles per check record, [t | residual: angular 3, linear 3 | per ee: contact clearance f_n cone rom]"""
    return 7 + 5 * n_ee


class JacLmParams(C.Structure):
    """twr_jac_lm_params"""
    _fields_ = [("cg_iters", C.c_int32), ("power_iters", C.c_int32), ("cg_tol", C.c_double), ("mu_down", C.c_double),
                ("mu_up", C.c_double), ("mu_min", C.c_double), ("mu_max", C.c_double), ("rel_floor", C.c_double),
                ("tau", C.c_double), ("merit_done", C.c_double)]


_lib = None
_dp = C.POINTER(C.c_double)


def build():
    """Compile libtowr_amd.so for gfx950 with hipcc (in-tree)."""
    subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc")])


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so.7; if
    libtowr_amd.so pulled in /opt/rocm's copy first, a later `import torch` would bring up a second
    runtime and see no GPU.  So when torch is installed, its runtime is loaded first (without
    importing torch) and libtowr_amd.so binds to it through the shared SONAME."""
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libtowr_amd.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "or `make -C towr_amd/csrc`")
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.twr_last_error.restype = C.c_char_p
        L.twr_model_preset.argtypes = [C.c_int, C.c_int, C.POINTER(Model)]
        L.twr_params_default.argtypes = [C.POINTER(Params)]
        L.twr_gait_combo.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(Schedule)]
        L.twr_structure_create.argtypes = [C.POINTER(Model), C.POINTER(Schedule), C.POINTER(Params),
                                           C.POINTER(C.c_void_p)]
        L.twr_structure_destroy.argtypes = [C.c_void_p]
        L.twr_terrain_grid_create.argtypes = [_dp, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.twr_terrain_grid_map_create.argtypes = [C.POINTER(C.c_float), C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                  C.POINTER(C.c_void_p)]
        L.twr_terrain_grid_destroy.argtypes = [C.c_void_p]
        L.twr_terrain_grid_map_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double]
        L.twr_batch_grid_map_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_batch_grid_map_update_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double,
                                                       C.c_void_p]
        L.twr_structure_create_with_grid.argtypes = [C.POINTER(Model), C.POINTER(Schedule), C.POINTER(Params), C.c_void_p,
                                                     C.POINTER(C.c_void_p)]
        L.twr_structure_destroy.restype = None
        L.twr_structure_create_many.argtypes = [C.POINTER(Model), C.POINTER(Schedule), C.POINTER(Params), C.c_int, C.c_int,
                                                C.POINTER(C.c_void_p)]
        L.twr_structure_create_many_with_grid.argtypes = [C.POINTER(Model), C.POINTER(Schedule), C.POINTER(Params), C.c_int,
                                                          C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
        L.twr_candidate_bytes.argtypes = [C.POINTER(Model), C.POINTER(Schedule), C.POINTER(Params), C.c_int, C.c_int,
                                          C.POINTER(C.c_int64)]
        L.twr_shard_bounds.argtypes = [_dp, C.c_int, C.c_int, C.POINTER(C.c_int32)]
        L.twr_terrain_grid_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            _dp, _dp, _dp, C.POINTER(C.c_void_p)]
        L.twr_structure_sizes.argtypes = [C.c_void_p, C.POINTER(Sizes)]
        L.twr_structure_var_set.argtypes = [C.c_void_p, C.c_int, C.POINTER(SetInfo)]
        L.twr_structure_con_set.argtypes = [C.c_void_p, C.c_int, C.POINTER(SetInfo)]
        L.twr_structure_row_ptr.argtypes = [C.c_void_p]
        L.twr_structure_row_ptr.restype = C.POINTER(C.c_int32)
        L.twr_structure_col_idx.argtypes = [C.c_void_p]
        L.twr_structure_col_idx.restype = C.POINTER(C.c_int32)
        L.twr_structure_bounds.argtypes = [C.c_void_p, _dp, _dp]
        L.twr_structure_initial_guess.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]
        L.twr_structure_variable_bounds.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp]
        L.twr_structure_start_host.argtypes = [C.c_void_p, _dp, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_batch_reserve_start.argtypes = [C.c_void_p]
        L.twr_batch_start.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_batch_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                       C.POINTER(C.c_void_p)]
        L.twr_batch_destroy.argtypes = [C.c_void_p]
        L.twr_batch_destroy.restype = None
        L.twr_batch_num_problems.argtypes = [C.c_void_p]
        L.twr_batch_table_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.twr_batch_streaming_stores.argtypes = [C.c_void_p]
        L.twr_batch_dyn_uniform_kinds.argtypes = [C.c_void_p]
        L.twr_batch_eval_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(LaunchStep), C.c_int, C.POINTER(C.c_int)]
        L.twr_batch_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.twr_batch_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.twr_batch_status.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]
        L.twr_batch_eval_host.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
        L.twr_structure_sample_count.argtypes = [C.c_void_p, C.c_double, C.POINTER(C.c_int32)]
        L.twr_batch_sample.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]
        L.twr_batch_initial_guess.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.twr_batch_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_batch_best.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.twr_batch_score_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p]
        L.twr_batch_scores_without_g.argtypes = [C.c_void_p]
        L.twr_batch_eval_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_batch_eval_score_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p,
                                                C.c_void_p]
        L.twr_structure_contact_steps_max.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.twr_structure_values_items.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]
        L.twr_planes_create.argtypes = [_dp, _dp, C.POINTER(C.c_int32), C.c_int32, C.c_int, C.POINTER(C.c_void_p)]
        L.twr_planes_destroy.argtypes = [C.c_void_p]
        L.twr_planes_destroy.restype = None
        L.twr_planes_world_xy.argtypes = [C.c_void_p, _dp]
        L.twr_batch_contact_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.twr_batch_contact_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p]
        L.twr_batch_host_buffers.argtypes = [C.c_void_p, C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_dp)]
        L.twr_batch_profile_begin.argtypes = [C.c_void_p, C.c_int]
        L.twr_batch_profile_end.argtypes = [C.c_void_p, _dp, C.POINTER(C.c_int)]
        L.twr_structure_transpose.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_ops_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                         C.POINTER(C.c_void_p)]
        L.twr_jac_ops_destroy.argtypes = [C.c_void_p]
        L.twr_jac_ops_destroy.restype = None
        L.twr_jac_ops_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.twr_jac_ops_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.twr_jac_mul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_tmul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                         C.POINTER(C.c_void_p)]
        L.twr_jac_lsq_destroy.argtypes = [C.c_void_p]
        L.twr_jac_lsq_destroy.restype = None
        L.twr_jac_lsq_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.twr_jac_dot.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_violation.argtypes = [C.c_void_p] + [C.c_void_p] * 5 + [C.c_void_p]
        L.twr_jac_lsq_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.twr_jac_col_sqnorms.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_reserve_scaled.argtypes = [C.c_void_p]
        L.twr_jac_col_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_solve_scaled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_ops_reserve_normal.argtypes = [C.c_void_p]
        L.twr_jac_ops_reserve_normal_tile.argtypes = [C.c_void_p, C.c_int]
        L.twr_jac_normal_mul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_reserve_onepass.argtypes = [C.c_void_p, C.c_int]
        L.twr_jac_lsq_solve_onepass.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_solve_masked.argtypes = L.twr_jac_lsq_solve_scaled.argtypes
        L.twr_jac_free_set.argtypes = [C.c_void_p] * 9
        L.twr_jac_lm_params_default.argtypes = [C.POINTER(JacLmParams)]
        L.twr_jac_lm_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(JacLmParams), C.POINTER(C.c_void_p)]
        L.twr_jac_lm_destroy.argtypes = [C.c_void_p]
        L.twr_jac_lm_destroy.restype = None
        L.twr_jac_lm_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.twr_jac_lm_start.argtypes = [C.c_void_p] * 7
        L.twr_jac_lm_step.argtypes = [C.c_void_p, C.c_void_p]
        L.twr_jac_lm_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_structure_gram_pattern.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
        L.twr_jac_ops_reserve_gram.argtypes = [C.c_void_p]
        L.twr_jac_ops_gram_layout.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
        L.twr_jac_gram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_gram_mul.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lsq_solve_gram.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double,
                                             C.c_void_p, C.c_void_p, C.c_void_p]
        L.twr_jac_lm_set_solver.argtypes = [C.c_void_p, C.c_int]
        L.twr_leg_kinematics_preset.argtypes = [C.c_int, C.POINTER(LegKinematics)]
        L.twr_batch_joints.argtypes = [C.c_void_p, C.POINTER(LegKinematics), C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int64,
                                       C.c_void_p]
        L.twr_batch_joint_scores.argtypes = [C.c_void_p, C.POINTER(LegKinematics), C.c_void_p, C.c_int64, C.c_double, C.c_void_p,
                                             C.c_void_p]
        L.twr_batch_eval_joint_scores.argtypes = [C.c_void_p, C.POINTER(LegKinematics), C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        L.twr_batch_checks.argtypes = [C.c_void_p, C.POINTER(Model), C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]
        L.twr_batch_check_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


class TowrError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise TowrError("towr_amd error %d: %s" % (rc, lib().twr_last_error().decode()))


def _d(a):
    return a.ctypes.data_as(_dp)


def model_preset(robot, terrain):
    """RobotModel(robot) + HeightMap::MakeTerrain(terrain) as the POD model blob."""
    m = Model()
    r = ROBOTS[robot] if isinstance(robot, str) else robot
    t = TERRAINS[terrain] if isinstance(terrain, str) else terrain
    _check(lib().twr_model_preset(r, t, C.byref(m)))
    return m


def leg_kinematics_preset(robot):
    """twr_leg_kinematics_preset: the reference's Go1 leg inverse-kinematics constants (any other robot raises: the reference
    has no IK for them; fill a LegKinematics yourself)."""
    k = LegKinematics()
    _check(lib().twr_leg_kinematics_preset(ROBOTS[robot] if isinstance(robot, str) else robot, C.byref(k)))
    return k


def params_default(**kw):
    p = Params()
    _check(lib().twr_params_default(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def gait_combo(n_ee, combo, t_total, swing_scale=1.0):
    s = Schedule()
    _check(lib().twr_gait_combo(n_ee, combo, float(t_total), float(swing_scale), C.byref(s)))
    return s


def schedule(phase_durations, contact_at_start):
    s = Schedule()
    s.n_ee = len(phase_durations)
    for e, pd in enumerate(phase_durations):
        s.n_phases[e] = len(pd)
        s.in_contact_at_start[e] = int(contact_at_start[e])
        for i, d in enumerate(pd):
            s.phase_durations[e][i] = float(d)
    return s


START_REC = 36  # TWR_START_REC


def start_request(init_base, final_base, ee_pos0):
    """The request record of twr_structure_start_host / twr_batch_start: START_REC doubles [init_base (12: lin p, lin v, ang p,
    ang v) | final_base (12) | initial foot positions (3 per end-effector, zero padded to four feet)]."""
    a = np.asarray(init_base, dtype=np.float64).reshape(-1)
    b = np.asarray(final_base, dtype=np.float64).reshape(-1)
    ee = np.asarray(ee_pos0, dtype=np.float64).reshape(-1)
    if a.size != 12 or b.size != 12 or ee.size % 3 or ee.size > 12:
        raise TowrError("start_request: init_base and final_base are 12 doubles, ee_pos0 at most four feet of 3")
    rec = np.zeros(START_REC)
    rec[0:12], rec[12:24], rec[24:24 + ee.size] = a, b, ee
    return rec


class TerrainGrid:
    """Gridded terrain of HeightMapFromCSV: heights[y_cell, x_cell] (0.17 m cells)."""

    def __init__(self, heights):
        a = np.ascontiguousarray(heights, dtype=np.float64)
        assert a.ndim == 2
        self._h = C.c_void_p()
        _check(lib().twr_terrain_grid_create(_d(a), a.shape[0], a.shape[1], C.byref(self._h)))
        self.heights = a

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_terrain_grid_destroy(self._h)
            self._h = None


class GridMap(TerrainGrid):
    """The "elevation" layer of a ROS grid_map for the `Grid` terrain (TWR_TERRAIN_GRID_MAP):
    elevation[i, j] float32 with i along -x and j along -y (grid_map's index convention, start index (0,0)),
    cell size `resolution`, map centre `position`."""

    def __init__(self, elevation, resolution, position=(0.0, 0.0)):
        a = np.asfortranarray(elevation, dtype=np.float32)   # grid_map's Eigen::MatrixXf is column-major
        assert a.ndim == 2
        self._h = C.c_void_p()
        _check(lib().twr_terrain_grid_map_create(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[0], a.shape[1],
                                                 float(resolution), float(position[0]), float(position[1]),
                                                 C.byref(self._h)))
        self.elevation, self.resolution, self.position = a, float(resolution), (float(position[0]), float(position[1]))
        self.heights = None

    def update(self, elevation, position, start_index=(0, 0)):
        """twr_terrain_grid_map_update: a new map of the same size and resolution in this handle.  `elevation` is the layer as
        grid_map keeps it, a circular buffer with `start_index` (GridMap::getStartIndex(); (0, 0) for a map that was never
        moved).  Afterwards `elevation` is the handle's copy, with start index (0, 0) -- np.roll(elevation, (-start_x, -start_y),
        axis=(0, 1)) -- and `position` the new centre; every Structure built on this GridMap uses them in initial_guess and
        variable_bounds.  A Batch that holds the map keeps its device copy until Batch.sync_grid_map.  Not safe against a
        concurrent host call on a Structure of this map."""
        a = np.asfortranarray(elevation, dtype=np.float32)
        if a.shape != self.elevation.shape:
            raise TowrError("GridMap.update: the layer is %r, the map %r (another size is a new GridMap)" % (a.shape, self.elevation.shape))
        _check(lib().twr_terrain_grid_map_update(self._h, a.ctypes.data, int(start_index[0]), int(start_index[1]),
                                                 float(position[0]), float(position[1])))
        px, py, data = C.c_double(), C.c_double(), C.c_void_p()
        _check(lib().twr_terrain_grid_info(self._h, None, None, None, None, C.byref(px), C.byref(py), C.byref(data)))
        stored = np.ctypeslib.as_array(C.cast(data, C.POINTER(C.c_float)), shape=(a.size,))
        self.elevation = np.array(stored.reshape(a.shape, order="F"), dtype=np.float32, order="F")
        self.position = (px.value, py.value)


class Planes:
    """The planar regions of a terrain message as world polygons on a device (fpowr PlanarRegionsToPolygons /
    NearestPlaneLookup): regions (n, 7) [position xyz | orientation xyzw], boundaries = one (k, 2) array of local
    outer-boundary points per region."""

    def __init__(self, regions, boundaries, device=0):
        regions = np.ascontiguousarray(regions, dtype=np.float64).reshape(-1, 7)
        assert len(regions) == len(boundaries)
        pts = [np.asarray(b, dtype=np.float64).reshape(-1, 2) for b in boundaries]
        self.start = np.concatenate([[0], np.cumsum([len(b) for b in pts])]).astype(np.int32)
        xy = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2)))
        self._h = C.c_void_p()
        _check(lib().twr_planes_create(_d(regions), _d(xy), self.start.ctypes.data_as(C.POINTER(C.c_int32)), len(regions),
                                       int(device), C.byref(self._h)))
        self.world_xy = np.zeros_like(xy)
        if len(xy):
            _check(lib().twr_planes_world_xy(self._h, _d(self.world_xy)))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_planes_destroy(self._h)
            self._h = None


class Structure:
    """x-independent part of one candidate (index maps, time tables, CSR pattern).  The set tables and the CSR
    pattern are fetched from the library on first use (a sweep builds a thousand of these)."""

    def __init__(self, model, sched, params=None, grid=None, _handle=None):
        params = params or params_default()
        self._h = C.c_void_p()
        self.model, self.schedule, self.params, self.grid = model, sched, params, grid
        if _handle is not None:
            self._h = _handle
        elif grid is not None:
            _check(lib().twr_structure_create_with_grid(C.byref(model), C.byref(sched), C.byref(params), grid._h,
                                                        C.byref(self._h)))
        else:
            _check(lib().twr_structure_create(C.byref(model), C.byref(sched), C.byref(params), C.byref(self._h)))
        sz = Sizes()
        _check(lib().twr_structure_sizes(self._h, C.byref(sz)))
        self._sz = sz
        self.n, self.m, self.nnz = sz.n_vars, sz.n_rows, sz.nnz
        self.k_dynamic, self.k_rom = sz.k_dynamic, sz.k_rom
        self.n_ee = model.n_ee
        self._lazy = {}

    @classmethod
    def create_many(cls, model, scheds, params_list, threads=0, grid=None):
        """twr_structure_create_many[_with_grid]: the candidates of a sweep, built on `threads` host threads (0 = all);
        with a gridded terrain they all share `grid`."""
        n = len(scheds)
        assert n == len(params_list) and n > 0
        sa = (Schedule * n)(*scheds)
        pa = (Params * n)(*params_list)
        hs = (C.c_void_p * n)()
        _check(lib().twr_structure_create_many_with_grid(C.byref(model), sa, pa, n, int(threads),
                                                         grid._h if grid is not None else None, hs))
        return [cls(model, scheds[i], params_list[i], grid=grid, _handle=C.c_void_p(hs[i])) for i in range(n)]

    def _sets(self, fn, n):
        out = []
        for i in range(n):
            si = SetInfo()
            _check(fn(self._h, i, C.byref(si)))
            out.append(dict(name=si.name.decode(), offset=si.offset, size=si.size, nnz_offset=si.nnz_offset,
                            nnz=si.nnz))
        return out

    def _get(self, key, make):
        if key not in self._lazy:
            self._lazy[key] = make()
        return self._lazy[key]

    @property
    def var_sets(self):
        return self._get("var_sets", lambda: self._sets(lib().twr_structure_var_set, self._sz.n_var_sets))

    @property
    def con_sets(self):
        return self._get("con_sets", lambda: self._sets(lib().twr_structure_con_set, self._sz.n_con_sets))

    @property
    def row_ptr(self):
        return self._get("row_ptr", lambda: np.ctypeslib.as_array(lib().twr_structure_row_ptr(self._h),
                                                                  shape=(self.m + 1,)).copy())

    @property
    def col_idx(self):
        return self._get("col_idx", lambda: np.ctypeslib.as_array(lib().twr_structure_col_idx(self._h),
                                                                  shape=(self.nnz,)).copy())

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:  # (module globals are gone at interpreter exit)
            lib().twr_structure_destroy(self._h)
            self._h = None

    @property
    def algorithmic_bytes(self):
        """read x once, write g once, write the Jacobian values once."""
        return 8 * (self.n + self.m + self.nnz)

    def bounds(self):
        lo, up = np.zeros(self.m), np.zeros(self.m)
        _check(lib().twr_structure_bounds(self._h, _d(lo), _d(up)))
        return lo, up

    def initial_guess(self, base_lin0, base_ang0, base_lin1, base_ang1, ee_pos0):
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (base_lin0, base_ang0, base_lin1, base_ang1)]
        ee = np.ascontiguousarray(ee_pos0, dtype=np.float64).reshape(-1)
        assert ee.size == 3 * self.n_ee
        x = np.zeros(self.n)
        _check(lib().twr_structure_initial_guess(self._h, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(ee), _d(x)))
        return x

    def contact_steps_max(self):
        """Upper bound of the footstep states twr_batch_contact_plan can produce for this structure."""
        n = C.c_int32()
        _check(lib().twr_structure_contact_steps_max(self._h, C.byref(n)))
        return n.value

    def values_items(self):
        """The work items of the values-only path (twr_structure_values_items): {"dynamic": [(k0, cnt, widest window)],
        "rom": [...], "dynamic_takes_rom": bool}; empty lists for a structure that keeps the Jacobian kernels' cut."""
        nd, nr, both = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().twr_structure_values_items(self._h, C.byref(nd), C.byref(nr), C.byref(both), None))
        items = np.zeros((nd.value + nr.value, 3), dtype=np.int32)
        _check(lib().twr_structure_values_items(self._h, C.byref(nd), C.byref(nr), C.byref(both), items.ctypes.data))
        rows = [tuple(int(v) for v in r) for r in items]
        return {"dynamic": rows[:nd.value], "rom": rows[nd.value:], "dynamic_takes_rom": bool(both.value)}

    def transpose(self):
        """twr_structure_transpose: the CSC view of the CSR pattern as numpy (col_ptr[n + 1], row_idx[nnz], csr_pos[nnz]); rows
        ascend within a column, and the CSC values of CSR values v are v[csr_pos]."""
        cp = np.zeros(self.n + 1, dtype=np.int32)
        ri = np.zeros(self.nnz, dtype=np.int32)
        cs = np.zeros(self.nnz, dtype=np.int32)
        _check(lib().twr_structure_transpose(self._h, cp.ctypes.data, ri.ctypes.data, cs.ctypes.data))
        return cp, ri, cs

    def gram_pattern(self):
        """twr_structure_gram_pattern: the pattern of N = J^T J as full symmetric CSR (row_ptr[n + 1], col_idx[nnz N], columns
        ascending); structural, so an explicit zero of J counts."""
        nnz = C.c_int64(0)
        _check(lib().twr_structure_gram_pattern(self._h, None, None, C.byref(nnz)))
        rp = np.zeros(self.n + 1, dtype=np.int32)
        ci = np.zeros(nnz.value, dtype=np.int32)
        _check(lib().twr_structure_gram_pattern(self._h, rp.ctypes.data, ci.ctypes.data, None))
        return rp, ci

    def sample_count(self, dt=0.01):
        """Records fpowr::GetTrajectory produces for this structure at step dt."""
        n = C.c_int32()
        _check(lib().twr_structure_sample_count(self._h, float(dt), C.byref(n)))
        return n.value

    def variable_bounds(self, init_base, final_base, ee_pos0):
        """x_l, x_u of the reference's variable sets; base states = 12 doubles {lin p, lin v, ang p, ang v}."""
        a = np.ascontiguousarray(init_base, dtype=np.float64).reshape(-1)
        b = np.ascontiguousarray(final_base, dtype=np.float64).reshape(-1)
        ee = np.ascontiguousarray(ee_pos0, dtype=np.float64).reshape(-1)
        assert a.size == 12 and b.size == 12 and ee.size == 3 * self.n_ee
        lo, up = np.zeros(self.n), np.zeros(self.n)
        _check(lib().twr_structure_variable_bounds(self._h, _d(a), _d(b), _d(ee), _d(lo), _d(up)))
        return lo, up

    def start_host(self, request):
        """twr_structure_start_host: (x0, x_l, x_u) of one request record (start_request) from the structure's start table --
        the bits of initial_guess and variable_bounds; the host executor of Batch.start_device."""
        rq = np.ascontiguousarray(request, dtype=np.float64).reshape(-1)
        assert rq.size == START_REC
        x, lo, up = np.zeros(self.n), np.zeros(self.n), np.zeros(self.n)
        _check(lib().twr_structure_start_host(self._h, _d(rq), x.ctypes.data, lo.ctypes.data, up.ctypes.data))
        return x, lo, up


class Batch:
    """Device tables of a batch of candidates; problem p uses structures[struct_of_problem[p]]."""

    def __init__(self, structures, struct_of_problem=None, device=0):
        if struct_of_problem is None:
            struct_of_problem = list(range(len(structures)))
        self.structures = list(structures)
        self.struct_of_problem = np.ascontiguousarray(struct_of_problem, dtype=np.int32)
        hs = (C.c_void_p * len(structures))(*[s._h for s in structures])
        self._h = C.c_void_p()
        _check(lib().twr_batch_create(hs, len(structures), self.struct_of_problem.ctypes.data_as(C.POINTER(C.c_int32)),
                                      len(self.struct_of_problem), device, C.byref(self._h)))
        self.device = device
        self.n_problems = len(self.struct_of_problem)
        xo = np.zeros(self.n_problems + 1, dtype=np.int64)
        go, jo = xo.copy(), xo.copy()
        p64 = C.POINTER(C.c_int64)
        _check(lib().twr_batch_layout(self._h, xo.ctypes.data_as(p64), go.ctypes.data_as(p64), jo.ctypes.data_as(p64)))
        self.x_off, self.g_off, self.jac_off = xo, go, jo
        self.algorithmic_bytes = int(8 * (xo[-1] + go[-1] + jo[-1]))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_batch_destroy(self._h)
            self._h = None

    def eval_device(self, d_x, d_g, d_jac, flags=EVAL_BOTH, stream=0):
        """Asynchronous launch on raw device pointers (ints), e.g. torch tensors' data_ptr()."""
        _check(lib().twr_batch_eval(self._h, C.c_void_p(d_x), C.c_void_p(d_g), C.c_void_p(d_jac), flags,
                                    C.c_void_p(stream)))

    def sync_grid_map(self, gm, stream=None):
        """twr_batch_grid_map_sync: the batch's device copy of GridMap `gm` (one its structures were built on) brought to gm's
        current content and centre (GridMap.update), in place; stream-ordered on `stream` (a raw stream, None: the default
        stream), not capturable.  At most one update or evaluation of the batch in flight."""
        _check(lib().twr_batch_grid_map_sync(self._h, gm._h, C.c_void_p(stream or 0)))

    def update_grid_map_device(self, gm, d_elevation, start_index, position, stream=None):
        """twr_batch_grid_map_update_device: the same from a float32 layer on the batch's device -- a torch tensor in grid_map's
        column-major storage order (1-D of size_x * size_y, or 2-D [size_x, size_y] with stride (1, size_x), e.g.
        torch.empty(size_y, size_x).t()), or a raw device pointer -- with its start index and the new centre.  One kernel
        launch, asynchronous on `stream`, capturable; the layer is only read.  gm itself (the host handle) is NOT updated."""
        sx, sy = gm.elevation.shape
        if hasattr(d_elevation, "data_ptr"):
            t = d_elevation
            flat = t.dim() == 1 and t.is_contiguous()
            column_major = t.dim() == 2 and tuple(t.shape) == (sx, sy) and t.t().is_contiguous()
            if str(t.dtype) != "torch.float32" or t.numel() != sx * sy or not (flat or column_major):
                raise TowrError("update_grid_map_device: d_elevation must hold %d x %d float32 cells in column-major order" % (sx, sy))
            d_elevation = t.data_ptr()
        _check(lib().twr_batch_grid_map_update_device(self._h, gm._h, C.c_void_p(int(d_elevation)), int(start_index[0]),
                                                      int(start_index[1]), float(position[0]), float(position[1]),
                                                      C.c_void_p(stream or 0)))

    def reserve_start(self):
        """twr_batch_reserve_start: plans start_device and uploads its tables; afterwards start_device allocates nothing and
        can be captured in a graph."""
        _check(lib().twr_batch_reserve_start(self._h))

    def start_device(self, d_request, request_stride, d_x, d_xlo, d_xup, stream=0):
        """twr_batch_start: x0 / x_l / x_u of every problem (layout x_off; raw device pointers, 0 leaves one out) from request
        records on the device (start_request; problem p reads d_request + p * request_stride doubles, stride 0: one record
        for all).  One launch, asynchronous on `stream`; the terrain is the map the batch holds now."""
        _check(lib().twr_batch_start(self._h, C.c_void_p(int(d_request)), int(request_stride), C.c_void_p(int(d_x)),
                                     C.c_void_p(int(d_xlo)), C.c_void_p(int(d_xup)), C.c_void_p(stream or 0)))

    def table_bytes(self):
        """Device bytes of the batch's tables: resident, layout tables of the dynamic set as built, and what is left of them
        after byte-identical tables of different structures were merged (twr_batch_table_bytes)."""
        r, a, d = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _check(lib().twr_batch_table_bytes(self._h, C.byref(r), C.byref(a), C.byref(d)))
        return dict(resident=r.value, dyn_layout=a.value, dyn_layout_distinct=d.value)

    def streaming_stores(self):
        """True when the batch streams its Jacobian values out with non-temporal stores (twr_batch_streaming_stores)."""
        return bool(lib().twr_batch_streaming_stores(self._h))

    def dyn_uniform_kinds(self):
        """Slices per problem of the "dynamic" set when every problem references one structure with fixed timings (the
        batch may then run dyn_uniform_kernel), else 0 (twr_batch_dyn_uniform_kinds)."""
        return int(lib().twr_batch_dyn_uniform_kinds(self._h))

    def eval_plan(self, flags=EVAL_BOTH, events=False, request="eval"):
        """The launches a call on this batch would issue, in order, without issuing them (twr_batch_eval_plan): a list of dicts
        {kernel, instantiation, store, nit, xc, grid, block, lds_bytes, uniform_kinds}, kernels and instantiations by name
        ("eval_fused_kernel", "eval_fused_kernel<34,xc2,GJ>").  request: "eval" (eval_device with `flags`; events=True: as
        between profile_begin and profile_end), "scores" (eval_scores_device) or "score_best" (eval_score_best_device)."""
        req = {"eval": 0, "scores": 1, "score_best": 2}[request]
        steps = (LaunchStep * 16)()
        n = C.c_int(0)
        _check(lib().twr_batch_eval_plan(self._h, req, int(flags), int(bool(events)), steps, len(steps), C.byref(n)))
        assert n.value <= len(steps)
        return [dict(kernel=s.kernel.decode(), instantiation=s.instantiation.decode(), store=s.store.decode(), nit=s.nit, xc=s.xc,
                     grid=s.grid, block=s.block, lds_bytes=s.lds_bytes, uniform_kinds=s.uniform_kinds) for s in steps[:n.value]]

    def status(self, stream=0):
        """Per-problem non-finite flags of the last eval_device(..., flags | EVAL_CHECK): bit 0 g, bit 1 jac."""
        st = np.zeros(self.n_problems, dtype=np.int32)
        _check(lib().twr_batch_status(self._h, st.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(stream)))
        return st

    def profile_begin(self, max_evals):
        """Record HIP events around each kernel of the next `max_evals` eval_device calls."""
        _check(lib().twr_batch_profile_begin(self._h, int(max_evals)))

    def profile_end(self):
        """Average duration [ms] of the dynamic / range-of-motion / node kernels, and the eval count."""
        ms = np.zeros(3)
        n = C.c_int(0)
        _check(lib().twr_batch_profile_end(self._h, _d(ms), C.byref(n)))
        return dict(dynamic=float(ms[0]), rangeofmotion=float(ms[1]), nodes=float(ms[2])), n.value

    def kernel_bytes(self):
        """Algorithmic bytes per launch of each kernel: it reads x once and writes its own rows of g
        and its own Jacobian values once (SURVEY 8d applied per kernel; x is counted for each kernel,
        so the three figures sum to algorithmic_bytes + 2*8*n per problem)."""
        out = dict(dynamic=0, rangeofmotion=0, nodes=0)
        for si in self.struct_of_problem:
            S = self.structures[si]
            for cs in S.con_sets:
                k = "dynamic" if cs["name"] == "dynamic" else ("rangeofmotion" if cs["name"].startswith("rangeofmotion")
                                                               else "nodes")
                out[k] += 8 * (cs["size"] + cs["nnz"])
            for k in out:
                out[k] += 8 * S.n
        return out

    def sample_device(self, d_x, dt, d_out, problem_stride, stream=0):
        """twr_batch_sample: d_out[p * problem_stride + sample * (20 + 13 n_ee) + field] (device pointers)."""
        _check(lib().twr_batch_sample(self._h, C.c_void_p(d_x), float(dt), C.c_void_p(d_out), int(problem_stride),
                                      C.c_void_p(stream)))

    def initial_guess_device(self, d_x, d_times, n_times, d_out, problem_stride, stream=0):
        """twr_batch_initial_guess (fpowr ExtractInitialGuess): d_out[p * problem_stride + 49 s + field], sample s at
        d_times[s]; record [t | state 12 | controls 36] (device pointers)."""
        _check(lib().twr_batch_initial_guess(self._h, C.c_void_p(d_x), C.c_void_p(d_times), int(n_times), C.c_void_p(d_out),
                                             int(problem_stride), C.c_void_p(stream)))

    def score_device(self, d_g, d_scores, stream=0):
        """twr_batch_score: d_scores[16 p + 2 f + {0: inf-norm, 1: 1-norm}] of the bound violation per family f."""
        _check(lib().twr_batch_score(self._h, C.c_void_p(d_g), C.c_void_p(d_scores), C.c_void_p(stream)))

    def score_best_device(self, d_g, d_scores, d_best, families=(0, 1, 3, 4), index_offset=0, stream=0):
        """twr_batch_score_best: score_device + best_device over this batch's candidates behind one call; d_best[0] is
        index_offset + the winner's index in the batch."""
        mask = 0
        for f in families:
            mask |= 1 << int(f)
        _check(lib().twr_batch_score_best(self._h, C.c_void_p(d_g), C.c_void_p(d_scores), mask, int(index_offset), C.c_void_p(d_best),
                                          C.c_void_p(stream)))

    @property
    def scores_without_g(self):
        """True when eval_scores_device / eval_score_best_device write no g (twr_batch_scores_without_g): every problem takes
        the values-only path.  Otherwise they need d_g and are eval_device(EVAL_VALUES) + score_device."""
        return bool(lib().twr_batch_scores_without_g(self._h))

    def eval_scores_device(self, d_x, d_scores, d_g=0, stream=0):
        """twr_batch_eval_scores: the score table of score_device straight from x (device pointers); d_g may be 0 when
        scores_without_g, and is left untouched then."""
        _check(lib().twr_batch_eval_scores(self._h, C.c_void_p(d_x), C.c_void_p(d_g), C.c_void_p(d_scores), C.c_void_p(stream)))

    def eval_score_best_device(self, d_x, d_scores, d_best, families=(0, 1, 3, 4), index_offset=0, d_g=0, stream=0):
        """twr_batch_eval_score_best: eval_scores_device + this batch's decision as score_best_device (d_best = [index_offset +
        index, total])."""
        mask = 0
        for f in families:
            mask |= 1 << int(f)
        _check(lib().twr_batch_eval_score_best(self._h, C.c_void_p(d_x), C.c_void_p(d_g), C.c_void_p(d_scores), mask, int(index_offset),
                                               C.c_void_p(d_best), C.c_void_p(stream)))

    def best_device(self, d_scores, n_candidates, d_best, families=(0, 1, 3, 4), stream=0):
        """twr_batch_best: device arg-min of the summed inf-norm violations of `families` (indices into FAMILIES) over a
        score table of n_candidates rows (this batch's, or the all-gathered one); d_best = 2 doubles [index, total]."""
        mask = 0
        for f in families:
            mask |= 1 << int(f)
        _check(lib().twr_batch_best(self._h, C.c_void_p(d_scores), int(n_candidates), mask, C.c_void_p(d_best), C.c_void_p(stream)))

    def contact_plan_device(self, d_x, dt, time_horizon, d_out, max_steps, d_counts, stream=0):
        """twr_batch_contact_plan (fpowr ExtractFootstepPlan without the plane lookup)."""
        _check(lib().twr_batch_contact_plan(self._h, C.c_void_p(d_x), float(dt), float(time_horizon), C.c_void_p(d_out),
                                            int(max_steps), C.c_void_p(d_counts), C.c_void_p(stream)))

    def contact_planes_device(self, planes, d_plan, d_counts, max_steps, d_plane_index, stream=0):
        """twr_batch_contact_planes: nearest planar region of every foot in contact of every footstep state of
        contact_plan_device(); d_plane_index int32[n_problems, max_steps, n_ee], -1 = in the air / no such state."""
        _check(lib().twr_batch_contact_planes(self._h, planes._h, C.c_void_p(d_plan), C.c_void_p(d_counts), int(max_steps),
                                              C.c_void_p(d_plane_index), C.c_void_p(stream)))

    def joints_device(self, kin, d_traj, traj_stride, dt, d_joints, joint_stride, stream=0):
        """twr_batch_joints: the records of sample_device (same dt and stride) -> joint records
        d_joints[p * joint_stride + sample * joint_rec(n_ee) + field] (device pointers)."""
        _check(lib().twr_batch_joints(self._h, C.byref(kin), C.c_void_p(d_traj), int(traj_stride), float(dt), C.c_void_p(d_joints),
                                      int(joint_stride), C.c_void_p(stream)))

    def joint_scores_device(self, kin, d_joints, joint_stride, dt, d_jscores, stream=0):
        """twr_batch_joint_scores: joint records -> d_jscores[JOINT_SCORE_REC * p + slot]: samples, unreachable leg-samples,
        limit-enforced leg-samples, max over-reach [m], max |dq| / dt, min margin to a limit, NaN leg-samples, first
        unreachable sample (-1: none)."""
        _check(lib().twr_batch_joint_scores(self._h, C.byref(kin), C.c_void_p(d_joints), int(joint_stride), float(dt),
                                            C.c_void_p(d_jscores), C.c_void_p(stream)))

    def eval_joint_scores_device(self, kin, d_x, dt, d_jscores, stream=0):
        """twr_batch_eval_joint_scores: the scores of joint_scores_device straight from x, bit for bit, without a trajectory."""
        _check(lib().twr_batch_eval_joint_scores(self._h, C.byref(kin), C.c_void_p(d_x), float(dt), C.c_void_p(d_jscores),
                                                 C.c_void_p(stream)))

    def checks_device(self, model, d_traj, traj_stride, dt, d_checks, check_stride, stream=0):
        """twr_batch_checks: the records of sample_device (same dt and stride) -> check records
        d_checks[p * check_stride + sample * check_rec(n_ee) + field] (device pointers); `model`: the Model whose nominal stance
        and maximum deviation bound the range of motion."""
        _check(lib().twr_batch_checks(self._h, C.byref(model), C.c_void_p(d_traj), int(traj_stride), float(dt), C.c_void_p(d_checks),
                                      int(check_stride), C.c_void_p(stream)))

    def check_scores_device(self, d_checks, check_stride, dt, d_cscores, stream=0):
        """twr_batch_check_scores: check records -> d_cscores[CHECK_SCORE_REC * p + slot]: samples, max |linear residual|, max
        |angular residual|, min swing clearance, max |stance clearance|, min f_n in contact, min cone in contact, max rom."""
        _check(lib().twr_batch_check_scores(self._h, C.c_void_p(d_checks), int(check_stride), float(dt), C.c_void_p(d_cscores),
                                            C.c_void_p(stream)))

    def host_buffers(self):
        """Page-locked x / g / jac arrays owned by the batch (numpy views); eval_host_pinned() uses them."""
        px, pg, pj = _dp(), _dp(), _dp()
        _check(lib().twr_batch_host_buffers(self._h, C.byref(px), C.byref(pg), C.byref(pj)))
        as_np = lambda p, n: np.ctypeslib.as_array(p, shape=(int(n),))
        return as_np(px, self.x_off[-1]), as_np(pg, self.g_off[-1]), as_np(pj, self.jac_off[-1])

    def eval_host_pinned(self, flags=EVAL_BOTH):
        """Evaluate from / into the page-locked buffers of host_buffers() (fill x there first)."""
        px, pg, pj = _dp(), _dp(), _dp()
        _check(lib().twr_batch_host_buffers(self._h, C.byref(px), C.byref(pg), C.byref(pj)))
        _check(lib().twr_batch_eval_host(self._h, px, pg, pj, flags))

    def eval_host(self, x, flags=EVAL_BOTH):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.x_off[-1]
        g = np.zeros(self.g_off[-1])
        j = np.zeros(self.jac_off[-1])
        _check(lib().twr_batch_eval_host(self._h, _d(x), _d(g), _d(j), flags))
        return g, j


class JacOps:
    """Products with the Jacobian values of Batch(structures, struct_of_problem) on the device (twr_jac_ops_*), in that batch's
    x / g / jac layout: mul_device y = J v (v in the x layout, y in the g layout), tmul_device z = J^T w (w in the g layout,
    z in the x layout)."""

    def __init__(self, structures, struct_of_problem=None, device=0):
        if struct_of_problem is None:
            struct_of_problem = list(range(len(structures)))
        self.structures = list(structures)
        self.struct_of_problem = np.ascontiguousarray(struct_of_problem, dtype=np.int32)
        hs = (C.c_void_p * len(structures))(*[s._h for s in structures])
        self._h = C.c_void_p()
        _check(lib().twr_jac_ops_create(hs, len(structures), self.struct_of_problem.ctypes.data_as(C.POINTER(C.c_int32)),
                                        len(self.struct_of_problem), device, C.byref(self._h)))
        self.device = device
        self.n_problems = len(self.struct_of_problem)

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_jac_ops_destroy(self._h)
            self._h = None

    def layout(self):
        """(x_off, g_off, jac_off), each n_problems + 1 prefix sums: twr_batch_layout of the same arguments."""
        xo = np.zeros(self.n_problems + 1, dtype=np.int64)
        go, jo = xo.copy(), xo.copy()
        p64 = C.POINTER(C.c_int64)
        _check(lib().twr_jac_ops_layout(self._h, xo.ctypes.data_as(p64), go.ctypes.data_as(p64), jo.ctypes.data_as(p64)))
        return xo, go, jo

    def bytes(self):
        """twr_jac_ops_bytes: device bytes the handle holds, and the distinct patterns its tables hold once each."""
        r, d = C.c_int64(0), C.c_int32(0)
        _check(lib().twr_jac_ops_bytes(self._h, C.byref(r), C.byref(d)))
        return dict(resident=r.value, distinct_patterns=d.value)

    def mul_device(self, d_jac, d_v, d_y, stream=0):
        """twr_jac_mul on raw device pointers (ints); asynchronous on `stream`."""
        _check(lib().twr_jac_mul(self._h, C.c_void_p(d_jac), C.c_void_p(d_v), C.c_void_p(d_y), C.c_void_p(stream)))

    def tmul_device(self, d_jac, d_w, d_z, stream=0):
        """twr_jac_tmul on raw device pointers (ints); asynchronous on `stream`."""
        _check(lib().twr_jac_tmul(self._h, C.c_void_p(d_jac), C.c_void_p(d_w), C.c_void_p(d_z), C.c_void_p(stream)))

    def col_sqnorms_device(self, d_jac, d_out, d_w=0, stream=0):
        """twr_jac_col_sqnorms on raw device pointers (ints; d_w 0 = unit weights): d_out[k] = sum_r w_r J[r][k]^2 in the x
        layout; asynchronous on `stream`."""
        _check(lib().twr_jac_col_sqnorms(self._h, C.c_void_p(d_jac), C.c_void_p(d_w), C.c_void_p(d_out), C.c_void_p(stream)))

    def reserve_normal(self, tile_entries=None):
        """twr_jac_ops_reserve_normal: plan, upload and allocate the one-pass product's tables and slab now (before a hipGraph
        capture); bytes() counts them from then on.  tile_entries (1 .. 2048): twr_jac_ops_reserve_normal_tile, a smaller LDS
        tile for tuning and tests."""
        if tile_entries is None:
            _check(lib().twr_jac_ops_reserve_normal(self._h))
        else:
            _check(lib().twr_jac_ops_reserve_normal_tile(self._h, int(tile_entries)))

    def normal_mul_device(self, d_jac, d_v, d_u, d_w=0, d_y=0, stream=0):
        """twr_jac_normal_mul on raw device pointers (ints; d_w 0 = unit weights, d_y 0 = leave out): u = J^T (w o (J v)) in the
        x layout and y = J v in the g layout from one pass over J; asynchronous on `stream`."""
        _check(lib().twr_jac_normal_mul(self._h, C.c_void_p(d_jac), C.c_void_p(d_w), C.c_void_p(d_v), C.c_void_p(d_y), C.c_void_p(d_u),
                                        C.c_void_p(stream)))

    def reserve_gram(self):
        """twr_jac_ops_reserve_gram: plan and upload the Gram matrix's tables and work lists now (before a hipGraph capture);
        bytes() counts them from then on.  TowrError -5 (unsupported) for a structure beyond the limits of the tables."""
        _check(lib().twr_jac_ops_reserve_gram(self._h))

    def gram_layout(self):
        """twr_jac_ops_gram_layout: gram_off, n_problems + 1 prefix sums (doubles) into the caller's value buffer of N."""
        go = np.zeros(self.n_problems + 1, dtype=np.int64)
        _check(lib().twr_jac_ops_gram_layout(self._h, go.ctypes.data_as(C.POINTER(C.c_int64))))
        return go

    def gram_device(self, d_jac, d_gram, d_w=0, stream=0):
        """twr_jac_gram on raw device pointers (ints; d_w 0 = unit weights): N = J^T W J of every problem, full symmetric CSR
        values at gram_layout(); asynchronous on `stream`."""
        _check(lib().twr_jac_gram(self._h, C.c_void_p(d_jac), C.c_void_p(d_w), C.c_void_p(d_gram), C.c_void_p(stream)))

    def gram_mul_device(self, d_gram, d_v, d_u, stream=0):
        """twr_jac_gram_mul on raw device pointers (ints): u = N v in the x layout; asynchronous on `stream`."""
        _check(lib().twr_jac_gram_mul(self._h, C.c_void_p(d_gram), C.c_void_p(d_v), C.c_void_p(d_u), C.c_void_p(stream)))


class JacLsq:
    """The damped weighted least-squares step with the Jacobian values of a batch on the device (twr_jac_lsq_*), on top of the
    products of `jac_ops` (borrowed: it is kept alive here) and in its x / g / jac layout: per problem
    (J^T W J + mu I) d = J^T W b by CGLS, the bound-violation residual that feeds it, and per-problem dot products; with
    Marquardt's scaling (col_scale_device from JacOps.col_sqnorms_device, then solve_scaled_device) mu C^-2 in place of mu I."""

    X, G = 0, 1   # the `space` of dot_device

    def __init__(self, jac_ops):
        self.ops = jac_ops
        hs = (C.c_void_p * len(jac_ops.structures))(*[s._h for s in jac_ops.structures])
        self._h = C.c_void_p()
        _check(lib().twr_jac_lsq_create(jac_ops._h, hs, len(jac_ops.structures),
                                        jac_ops.struct_of_problem.ctypes.data_as(C.POINTER(C.c_int32)), jac_ops.n_problems,
                                        C.byref(self._h)))
        self.device = jac_ops.device
        self.n_problems = jac_ops.n_problems

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_jac_lsq_destroy(self._h)
            self._h = None

    def bytes(self):
        """twr_jac_lsq_bytes: device bytes the handle holds (bound tables, work records, workspace)."""
        r = C.c_int64(0)
        _check(lib().twr_jac_lsq_bytes(self._h, C.byref(r)))
        return dict(resident=r.value)

    def dot_device(self, space, d_a, d_b, d_out, stream=0):
        """twr_jac_dot on raw device pointers (ints): d_out[p] = a_p . b_p over the x layout (space 0) or the g layout (1)."""
        _check(lib().twr_jac_dot(self._h, space, C.c_void_p(d_a), C.c_void_p(d_b), C.c_void_p(d_out), C.c_void_p(stream)))

    def violation_device(self, d_g, d_r, d_w=0, d_w_active=0, d_merit=0, stream=0):
        """twr_jac_violation on raw device pointers (ints, 0 = leave out): r = g - clip(g, lower, upper), w_active = w [r != 0],
        merit[p] = 1/2 sum w r^2."""
        _check(lib().twr_jac_violation(self._h, C.c_void_p(d_g), C.c_void_p(d_w), C.c_void_p(d_r), C.c_void_p(d_w_active),
                                       C.c_void_p(d_merit), C.c_void_p(stream)))

    def solve_device(self, d_jac, d_b, d_mu, d_d, d_info, iters, tol, d_w=0, stream=0):
        """twr_jac_lsq_solve on raw device pointers (ints; d_w 0 = unit weights); asynchronous on `stream`.  d_info: 4 doubles
        per problem (iterations, |s| / |s0|, |s0|, status)."""
        _check(lib().twr_jac_lsq_solve(self._h, C.c_void_p(d_jac), C.c_void_p(d_b), C.c_void_p(d_w), C.c_void_p(d_mu), int(iters),
                                       float(tol), C.c_void_p(d_d), C.c_void_p(d_info), C.c_void_p(stream)))

    def reserve_scaled(self):
        """twr_jac_lsq_reserve_scaled: allocate the scaled solve's two extra vectors now (before a hipGraph capture)."""
        _check(lib().twr_jac_lsq_reserve_scaled(self._h))

    def col_scale_device(self, d_colsq, d_scale, rel_floor, d_colsq_max=0, stream=0):
        """twr_jac_col_scale on raw device pointers (ints): c = 1 / sqrt(max(a, rel_floor max(a))) per problem, a = colsq or the
        running maximum d_colsq_max (in / out, 0 = leave out)."""
        _check(lib().twr_jac_col_scale(self._h, C.c_void_p(d_colsq), C.c_void_p(d_colsq_max), float(rel_floor), C.c_void_p(d_scale),
                                       C.c_void_p(stream)))

    def solve_scaled_device(self, d_jac, d_b, d_mu, d_scale, d_d, d_info, iters, tol, d_w=0, stream=0):
        """twr_jac_lsq_solve_scaled on raw device pointers (ints; d_w 0 = unit weights): (J^T W J + mu C^-2) d = J^T W b with
        C = diag(d_scale); d_info as solve_device, in the scaled variables."""
        _check(lib().twr_jac_lsq_solve_scaled(self._h, C.c_void_p(d_jac), C.c_void_p(d_b), C.c_void_p(d_w), C.c_void_p(d_mu),
                                              C.c_void_p(d_scale), int(iters), float(tol), C.c_void_p(d_d), C.c_void_p(d_info),
                                              C.c_void_p(stream)))

    def reserve_onepass(self, scaled=False):
        """twr_jac_lsq_reserve_onepass: everything solve_onepass_device allocates on first use (the one-pass product of the
        borrowed JacOps, two vectors here, with `scaled` the scaled solve's), now (before a hipGraph capture)."""
        _check(lib().twr_jac_lsq_reserve_onepass(self._h, int(bool(scaled))))

    def solve_onepass_device(self, d_jac, d_b, d_mu, d_d, d_info, iters, tol, d_w=0, d_scale=0, stream=0):
        """twr_jac_lsq_solve_onepass on raw device pointers (ints; d_w 0 = unit weights, d_scale 0 = the unscaled step): the step
        of solve_device / solve_scaled_device with J read once per iteration; d_info as solve_device."""
        _check(lib().twr_jac_lsq_solve_onepass(self._h, C.c_void_p(d_jac), C.c_void_p(d_b), C.c_void_p(d_w), C.c_void_p(d_mu),
                                               C.c_void_p(d_scale), int(iters), float(tol), C.c_void_p(d_d), C.c_void_p(d_info),
                                               C.c_void_p(stream)))

    def solve_masked_device(self, d_jac, d_b, d_mu, d_scale, d_d, d_info, iters, tol, d_w=0, stream=0):
        """twr_jac_lsq_solve_masked on raw device pointers (ints; d_w 0 = unit weights): solve_scaled_device where a scale of
        exactly 0 takes its variable out of the solve (d_k = +0); with no zero in d_scale, the bits of solve_scaled_device."""
        _check(lib().twr_jac_lsq_solve_masked(self._h, C.c_void_p(d_jac), C.c_void_p(d_b), C.c_void_p(d_w), C.c_void_p(d_mu),
                                              C.c_void_p(d_scale), int(iters), float(tol), C.c_void_p(d_d), C.c_void_p(d_info),
                                              C.c_void_p(stream)))

    def free_set_device(self, d_x, d_xlo, d_xup, d_z, d_scale_out, d_nfree, d_scale_in=0, stream=0):
        """twr_jac_free_set on raw device pointers (ints): scale_out = 0 for every variable on a bound that z = J^T(w o b) pushes
        outwards (every fixed variable on its value), else scale_in (0 = ones); d_nfree[p] = the free count (doubles)."""
        _check(lib().twr_jac_free_set(self._h, C.c_void_p(d_x), C.c_void_p(d_xlo), C.c_void_p(d_xup), C.c_void_p(d_z),
                                      C.c_void_p(d_scale_in), C.c_void_p(d_scale_out), C.c_void_p(d_nfree), C.c_void_p(stream)))

    def solve_gram_device(self, d_gram, d_z, d_mu, d_d, d_info, iters, tol, d_scale=0, stream=0):
        """twr_jac_lsq_solve_gram on raw device pointers (ints; d_scale 0 = ones, an exact 0 in it takes its variable out):
        (C N C + mu I) e = c o z, d = c o e by CG on the Gram matrix of JacOps.gram_device, z = J^T (w o b) from
        JacOps.tmul_device; the whole solve is one launch.  d_info as solve_device."""
        _check(lib().twr_jac_lsq_solve_gram(self._h, C.c_void_p(d_gram), C.c_void_p(d_z), C.c_void_p(d_mu), C.c_void_p(d_scale),
                                            int(iters), float(tol), C.c_void_p(d_d), C.c_void_p(d_info), C.c_void_p(stream)))


class JacLm:
    """The bound-constrained Levenberg-Marquardt driver on the device (twr_jac_lm_*): projected active-set LM on a Batch and a
    JacLsq of the same layout (both borrowed: they are kept alive here).  Parameters as keywords (twr_jac_lm_params: cg_iters,
    cg_tol, power_iters, mu_down, mu_up, mu_min, mu_max, rel_floor, tau, merit_done)."""

    REC = 8   # TWR_JAC_LM_REC: doubles per problem of state_device
    FIELDS = ("merit_start", "merit", "mu", "steps", "accepted", "free", "cg_iters", "state")
    RUNNING, DONE, BAD = 0, 1, 2
    SOLVERS = {"cgls": 0, "gram": 1}   # TWR_JAC_LM_CGLS, TWR_JAC_LM_GRAM

    def __init__(self, batch, jac_lsq, solver="cgls", **params):
        if solver not in self.SOLVERS:
            raise TypeError("unknown LM solver %r" % (solver,))
        self.batch, self.lsq, self.solver = batch, jac_lsq, solver
        self.params = JacLmParams()
        _check(lib().twr_jac_lm_params_default(C.byref(self.params)))
        for k, v in params.items():
            if k not in dict(JacLmParams._fields_):
                raise TypeError("unknown LM parameter %r" % k)
            setattr(self.params, k, v)
        self._h = C.c_void_p()
        _check(lib().twr_jac_lm_create(batch._h, jac_lsq._h, C.byref(self.params), C.byref(self._h)))
        self.n_problems = jac_lsq.n_problems
        if solver != "cgls":   # (the default is what twr_jac_lm_create leaves)
            _check(lib().twr_jac_lm_set_solver(self._h, self.SOLVERS[solver]))

    def __del__(self):
        if getattr(self, "_h", None) and lib is not None:
            lib().twr_jac_lm_destroy(self._h)
            self._h = None

    def bytes(self):
        r = C.c_int64(0)
        _check(lib().twr_jac_lm_bytes(self._h, C.byref(r)))
        return dict(resident=r.value)

    def start_device(self, d_x, d_xlo, d_xup, d_g, d_jac, stream=0):
        """twr_jac_lm_start on raw device pointers (ints): binds them (they must stay alive while steps are taken), projects x
        onto the box, linearises and sets mu0."""
        _check(lib().twr_jac_lm_start(self._h, C.c_void_p(d_x), C.c_void_p(d_xlo), C.c_void_p(d_xup), C.c_void_p(d_g),
                                      C.c_void_p(d_jac), C.c_void_p(stream)))

    def step_device(self, stream=0):
        """twr_jac_lm_step: one step, one chain of launches on `stream`, capturable."""
        _check(lib().twr_jac_lm_step(self._h, C.c_void_p(stream)))

    def state_device(self, d_out, stream=0):
        """twr_jac_lm_state: REC doubles per problem to d_out (FIELDS)."""
        _check(lib().twr_jac_lm_state(self._h, C.c_void_p(d_out), C.c_void_p(stream)))
