/* towr_amd -- MI355X-native evaluation of towr's NLP constraint / Jacobian hot path.
 *
 * C ABI of libtowr_amd.so.  Plain pointers and sizes only; no C++/torch types.
 * Every entry point names the reference interface it replaces (file:line under
 * KaiNakamura/towr).  The reference has no C ABI: the path sits
 * behind the C++ virtual interface ifopt::ConstraintSet, so the binding a maintainer adds
 * is the small C++ adapter shown in INTEGRATION.md (towr_amd/csrc/ifopt_adapter.h).
 *
 * Conventions
 *   - all functions return TWR_OK (0) or a negative error code; twr_last_error() gives
 *     the message of the last failure on the calling thread.  No exceptions cross the ABI.
 *   - handles are thread-compatible: distinct handles may be used from distinct threads.
 *   - devices: a batch (and a twr_planes handle) lives on the device it was created for.  Every entry point makes
 *     that device current for its own HIP calls and restores the calling thread's current device before it
 *     returns; none reads or clears the thread's sticky HIP error.
 *   - "x" is the stacked ifopt variable vector in the reference order
 *        base-lin | base-ang | ee-motion_0.. | ee-force_0.. [| ee-schedule0..]   (nlp_formulation.cc:63-93)
 *     "g" are the stacked constraint values and "jac" the Jacobian non-zeros in the CSR
 *     order ifopt::Problem::EvalNonzerosOfJacobian copies out (row-major, columns
 *     ascending, explicit structural zeros kept), for the constraint sets
 *        terrain-ee-motion_e.. | dynamic | splineacc-base-lin | splineacc-base-ang |
 *        rangeofmotion-e.. | force-ee-force_e.. | swing-ee-motion_e.. | baseMotion | totalduration-e..
 *     i.e. params_.constraints_ order (parameters.cc:55-60); twr_params.constraint_sets selects
 *     which families exist (default: the four of the hot path).
 */
#ifndef TOWR_AMD_H_
#define TOWR_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TWR_MAX_EE 4
#define TWR_MAX_PHASES 32
#define TWR_NAME_LEN 40

enum { TWR_OK = 0, TWR_ERR_INVALID = -1, TWR_ERR_HIP = -2, TWR_ERR_NO_DEVICE = -3, TWR_ERR_INTERNAL = -4, TWR_ERR_UNSUPPORTED = -5 };

/* RobotModel::Robot (robot_model.h:70-75) */
enum { TWR_ROBOT_MONOPED = 0, TWR_ROBOT_BIPED, TWR_ROBOT_HYQ, TWR_ROBOT_ANYMAL, TWR_ROBOT_GO1 };
/* HeightMap::TerrainID (height_map.h:79-86) */
enum { TWR_TERRAIN_FLAT = 0, TWR_TERRAIN_BLOCK, TWR_TERRAIN_STAIRS, TWR_TERRAIN_GAP, TWR_TERRAIN_SLOPE,
       TWR_TERRAIN_CHIMNEY, TWR_TERRAIN_CHIMNEY_LR,
       /* HeightMapFromCSV (include/towr/terrain/height_map_from_csv.h): a gridded terrain, heights per 0.17 m
         * cell; needs a twr_terrain_grid handle, see twr_structure_create_with_grid */
       TWR_TERRAIN_CSV_GRID,
       /* Grid (include/towr/terrain/grid_height_map.h:15-60): the perception-driven terrain fpowr hands the solver
        * (fpowr/src/footstep_plan_server.cc:155) -- the float "elevation" layer of a ROS grid_map, bilinear
        * sample, central-difference slopes over resolution/6, FLT_MAX outside the map; needs a handle made by
        * twr_terrain_grid_map_create, see twr_structure_create_with_grid */
       TWR_TERRAIN_GRID_MAP };
enum { TWR_EVAL_VALUES = 1, TWR_EVAL_JACOBIAN = 2, TWR_EVAL_BOTH = 3,
       /* also run the per-problem NaN/Inf scan over the outputs of this evaluation (twr_batch_status) */
       TWR_EVAL_CHECK = 4 };
/* Parameters::ConstraintName entries of the default list (parameters.h:139-147, parameters.cc:55-60),
 * as bits of twr_params.constraint_sets.  The sets always appear in this (the reference's) order. */
enum {
  TWR_SET_TERRAIN = 1,   /* TerrainConstraint per ee          (nlp_formulation.cc:278-289) */
  TWR_SET_DYNAMIC = 2,   /* DynamicConstraint                 (nlp_formulation.cc:237-245) */
  TWR_SET_BASE_ACC = 4,  /* SplineAccConstraint base-lin/-ang (nlp_formulation.cc:319-331) */
  TWR_SET_ROM = 8,       /* RangeOfMotionConstraint per ee    (nlp_formulation.cc:247-262) */
  TWR_SET_FORCE = 16,    /* ForceConstraint per ee            (nlp_formulation.cc:291-304) */
  TWR_SET_SWING = 32,    /* SwingConstraint per ee            (nlp_formulation.cc:306-317) */
  /* Parameters::OptimizePhaseDurations() (parameters.cc:76-80): TotalDurationConstraint per ee
   * (nlp_formulation.cc:264-276) AND, because IsOptimizeTimings() becomes true (parameters.cc:128-135),
   * the phase durations join x as variable sets ee-schedule<e> (n_phases-1 each, after ee-force_*),
   * the ee splines become PhaseSplines (spline_holder.cc:48-52): every Jacobian row of an ee spline
   * holds all variables of its set, and dynamic / rangeofmotion rows gain the duration columns. */
  TWR_SET_TOTAL_TIME = 64,
  /* BaseMotionConstraint "baseMotion" (nlp_formulation.cc:229-235, base_motion_constraint.cc:38-99): not in the
   * default list; rows come after swing-* (where a caller's constraints_.push_back(BaseRom) lands) and before
   * totalduration-*.  Needs twr_params.dt_base_motion and .base_z_init. */
  TWR_SET_BASE_ROM = 128,
  TWR_SETS_HOT_PATH = 1 | 2 | 8 | 16,
  TWR_SETS_TOWR_DEFAULT = 63,
  TWR_SETS_ALL = 127,      /* default list + OptimizePhaseDurations() */
  TWR_SETS_EVERY = 255     /* every Parameters::ConstraintName */
};

/* Robot + terrain constants: the POD "model blob" that rank 0 broadcasts over RCCL.
 * Replaces towr::RobotModel {KinematicModel, DynamicModel} + HeightMap::Ptr
 * (robot_model.h:63-83, single_rigid_body_dynamics.h:66-77, height_map.h:71-137). */
typedef struct twr_model {
  int32_t n_ee;
  int32_t terrain_id;
  double mass;
  double inertia[6];                    /* Ixx,Iyy,Izz,Ixy,Ixz,Iyz as given to SingleRigidBodyDynamics() */
  double nominal_stance[TWR_MAX_EE][3]; /* KinematicModel::GetNominalStanceInBase */
  double max_dev[3];                    /* KinematicModel::GetMaximumDeviationFromNominal */
  double gravity;                       /* 9.80665, dynamic_model.cc:37 */
  double friction;                      /* 0.5, height_map.h:136 */
  double force_limit;                   /* Parameters::force_limit_in_normal_direction_, parameters.cc:48 */
  double flat_height;                   /* FlatGround(height) */
} twr_model;

/* Contact schedule of one candidate: Parameters::ee_phase_durations_ / ee_in_contact_at_start_
 * (parameters.h:168-171). */
typedef struct twr_schedule {
  int32_t n_ee;
  int32_t n_phases[TWR_MAX_EE];
  int32_t in_contact_at_start[TWR_MAX_EE];
  double phase_durations[TWR_MAX_EE][TWR_MAX_PHASES];
} twr_schedule;

/* Discretisation parameters (parameters.cc:43-51). */
typedef struct twr_params {
  double dt_dynamic;            /* dt_constraint_dynamic_ (0.1) */
  double dt_rom;                /* dt_constraint_range_of_motion_ (0.08) */
  double duration_base_poly;    /* duration_base_polynomial_ (0.1) */
  int32_t polys_per_swing;      /* ee_polynomials_per_swing_phase_ (2) */
  int32_t polys_per_stance_force; /* force_polynomials_per_stance_phase_ (3) */
  int32_t constraint_sets;      /* TWR_SET_* mask; twr_params_default: TWR_SETS_HOT_PATH */
  int32_t reserved_;            /* must be 0 */
  double dt_base_motion;        /* dt_constraint_base_motion_ (duration_base_polynomial_/4, parameters.cc:51) */
  double base_z_init;           /* initial base height: BaseMotionConstraint bounds z to [z-0.02, z+0.1]
                                   (base_motion_constraint.cc:51-55, read from the spline at construction).
                                   twr_params_default leaves it NaN; TWR_SET_BASE_ROM is rejected until it is set. */
} twr_params;

typedef struct twr_sizes {
  int32_t n_vars, n_rows, nnz;
  int32_t n_var_sets, n_con_sets;
  int32_t k_dynamic, k_rom;     /* TimeDiscretizationConstraint::GetNumberOfNodes */
} twr_sizes;

typedef struct twr_set_info {
  char name[TWR_NAME_LEN];      /* ifopt component name, e.g. "rangeofmotion-2" */
  int32_t offset;               /* first variable index / first row */
  int32_t size;                 /* variables / rows */
  int32_t nnz_offset, nnz;      /* constraint sets only */
} twr_set_info;

typedef struct twr_terrain_grid twr_terrain_grid; /* host copy of a gridded terrain, shared by structures */
typedef struct twr_structure twr_structure; /* host: index maps + CSR pattern of one candidate */
typedef struct twr_batch twr_batch;         /* device: tables of a batch of candidates */

const char* twr_last_error(void);

/* RobotModel(Robot) + HeightMap::MakeTerrain(id) + Parameters defaults (robot_model.cc:41-68,
 * height_map.cc:37-50, parameters.cc:40-73). */
int twr_model_preset(int robot, int terrain, twr_model* out);
int twr_params_default(twr_params* out);

/* GaitGenerator::MakeGaitGenerator(n_ee)->SetCombo(combo); GetPhaseDurations(T, ee);
 * IsInContactAtStart(ee)  (gait_generator.cc:43-111, {monoped,biped,quadruped}_gait_generator.cc).
 * swing_scale multiplies every table entry whose contact state has a foot in the air before the
 * renormalisation to t_total (1.0 = reference tables); used to enumerate candidates. */
int twr_gait_combo(int n_ee, int combo, double t_total, double swing_scale, twr_schedule* out);

/* What NlpFormulation::GetVariableSets + GetConstraints + ifopt's LinkWithVariables compute once per
 * problem (nlp_formulation.cc:63-93,200-331): variable index maps, time grids, active-polynomial
 * tables and the x-independent CSR pattern of the stacked Jacobian. */
int twr_structure_create(const twr_model* model, const twr_schedule* schedule, const twr_params* params,
                         twr_structure** out);
/* Gridded terrain of HeightMapFromCSV (height_map_from_csv.h:16-27): heights[y_cell * cols + x_cell], i.e. the
 * matrix the reference fills from the CSV file; cell size 0.17 m and slope window cell/50 as in :112-115.
 * Structures keep a reference to the grid (it may be destroyed right after they are created); a batch
 * uploads every distinct grid once. */
int twr_terrain_grid_create(const double* heights, int rows, int cols, twr_terrain_grid** out);
/* The "elevation" layer of a grid_map::GridMap for TWR_TERRAIN_GRID_MAP: elevation[i + j * size_x] is cell (i, j)
 * (the column-major float matrix grid_map keeps; i runs along -x, j along -y from the corner with the largest x
 * and y), cell size `resolution`, map centre (pos_x, pos_y) = GridMap::getPosition(); the map must have start
 * index (0,0) (GridMap::convertToDefaultStartIndex()).  Sampling follows grid_map's published
 * atPosition(..., INTER_LINEAR): bilinear over the 2x2 cells around the position, nearest cell in the half-cell
 * border band, std::out_of_range (-> FLT_MAX in Grid::GetHeight) outside the map. */
int twr_terrain_grid_map_create(const float* elevation, int size_x, int size_y, double resolution, double pos_x,
                                double pos_y, twr_terrain_grid** out);
/* A new map in an existing grid_map handle (fpowr builds a fresh Grid from the request's map on every plan request,
 * footstep_plan_server.cc:155): new content and centre, same size and resolution.  `elevation` is a layer of the handle's size
 * as grid_map keeps it after GridMap::move, a circular buffer with start index (start_x, start_y) (GridMap::getStartIndex(); (0,0)
 * for a map that was never moved); the handle keeps its own form, start index (0,0):
 *   stored[i, j] = elevation[(i + start_x) mod size_x, (j + start_y) mod size_y]      (grid_map's getBufferIndexFromIndex)
 * column-major like twr_terrain_grid_map_create; cells are copied bit for bit (a NaN cell stays that NaN).  Every structure that
 * shares the handle sees the new map in its host-side calls from then on (twr_structure_initial_guess,
 * twr_structure_variable_bounds; twr_terrain_grid_info: the `data` address stays the same), and a batch created afterwards
 * uploads it.  A batch that already holds the map keeps its device copy until twr_batch_grid_map_sync.
 * NOT safe against a concurrent host call on the handle or on a structure created with it: the caller serialises them.
 * TWR_ERR_INVALID, with twr_last_error naming the argument and the handle unchanged: g or elevation NULL, elevation not
 * 4-byte aligned, g a CSV grid, a start index outside [0, size), a non-finite position. */
int twr_terrain_grid_map_update(twr_terrain_grid* g, const float* elevation /* size_x * size_y */, int start_x, int start_y,
                                double pos_x, double pos_y);
void twr_terrain_grid_destroy(twr_terrain_grid* g);
/* As twr_structure_create for model->terrain_id == TWR_TERRAIN_CSV_GRID / TWR_TERRAIN_GRID_MAP (the grid must be
 * of the matching kind). */
int twr_structure_create_with_grid(const twr_model* model, const twr_schedule* schedule, const twr_params* params,
                                   const twr_terrain_grid* grid, twr_structure** out);
void twr_structure_destroy(twr_structure* s);
/* n candidates of one robot/terrain model at once (a sweep: SURVEY.md 8e "each rank builds descriptors for its
 * shard only"): structure i from schedules[i] / params[i], built on up to n_threads host threads (<= 0: all
 * hardware threads).  On failure nothing is left allocated and out[] is all NULL. */
int twr_structure_create_many(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n,
                              int n_threads, twr_structure** out);
/* The same for a gridded terrain (model->terrain_id == TWR_TERRAIN_CSV_GRID / TWR_TERRAIN_GRID_MAP): every structure
 * shares `grid` (one device copy per batch).  This is what a sweep over the perception-driven `Grid` terrain of
 * fpowr (footstep_plan_server.cc:155) uses; grid == NULL is twr_structure_create_many. */
int twr_structure_create_many_with_grid(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n,
                                        int n_threads, const twr_terrain_grid* grid, twr_structure** out);
/* Sharding a sweep over ranks / devices (contiguous shards balanced by BYTES, not counts -- candidates are
 * ragged).  twr_candidate_bytes: bytes[i] = 8 (n + m + nnz) of candidate i, the bytes one callback of it moves; builds
 * only the variable layout, the time tables and the CSR pattern (no device tables), on n_threads host threads (<= 0:
 * all).  Every rank computes the same numbers from the same candidate list, so no exchange is needed.
 * twr_shard_bounds: bounds[0..world], rank r owns candidates [bounds[r], bounds[r+1]); the boundary of rank r is the
 * prefix whose weight sum is closest to r / world of the total; never an empty shard; TWR_ERR_INVALID when n < world
 * (on every rank alike).  The reference has no counterpart: fpowr solves one gait per goal
 * (fpowr/src/footstep_plan_server.cc:191-200). */
int twr_candidate_bytes(const twr_model* model, const twr_schedule* schedules, const twr_params* params, int n, int n_threads,
                        int64_t* bytes /* n */);
int twr_shard_bounds(const double* weights /* n */, int n, int world, int32_t* bounds /* world + 1 */);
/* What a rank needs to rebuild a grid handle it received over the wire (towr_amd/dist.py broadcast_grid): kind (0: CSV
 * heights, double [rows][cols]; 1: grid_map elevation layer, float, column-major [size_x][size_y]), the two sizes,
 * resolution and map position (grid_map only), and the cell data (`data` points into the handle; valid until destroy). */
int twr_terrain_grid_info(const twr_terrain_grid* g, int32_t* kind, int32_t* rows_or_size_x, int32_t* cols_or_size_y,
                          double* resolution, double* pos_x, double* pos_y, const void** data);
int twr_structure_sizes(const twr_structure* s, twr_sizes* out);
/* Introspection of the values-only path (TWR_EVAL_VALUES; fixed timings, at most 2046 variables): the work items a problem
 * of this structure is cut into -- at most 64 consecutive time nodes of the "dynamic" resp. range-of-motion grid whose active
 * polynomials span at most eight polynomials per ee spline (time_discretization_constraint.cc:36-58 gives the grids,
 * spline.cc:48-78 the active polynomials).  *dynamic_takes_rom is 1 when the two grids coincide and the "dynamic" items
 * evaluate the "rangeofmotion-*" rows of their time nodes as well (then *n_rom_items is 0).  `items` may be NULL; otherwise
 * it receives (first time node, time nodes, polynomials of the widest window) per item, "dynamic" items first; a grid so coarse
 * that the windows would cut over a quarter more items than 64 time nodes each give (towr's default grids) is cut at 64 time
 * nodes alone, its lanes fetch their own polynomial records, and the third number is 0.  All counts are 0 for a structure that keeps
 * the Jacobian kernels' cut. */
int twr_structure_values_items(const twr_structure* s, int32_t* n_dynamic_items, int32_t* n_rom_items, int32_t* dynamic_takes_rom,
                               int32_t* items /* [n_dynamic_items + n_rom_items][3] or NULL */);
int twr_structure_var_set(const twr_structure* s, int i, twr_set_info* out);
int twr_structure_con_set(const twr_structure* s, int i, twr_set_info* out);
/* Library-owned, valid until twr_structure_destroy: CSR row_ptr[n_rows+1], col_idx[nnz]. */
const int32_t* twr_structure_row_ptr(const twr_structure* s);
const int32_t* twr_structure_col_idx(const twr_structure* s);
/* ConstraintSet::GetBounds of the stacked sets (dynamic_constraint.cc:66-71,
 * range_of_motion_constraint.cc:71-81, force_constraint.cc:91-105, terrain_constraint.cc:72-88). */
int twr_structure_bounds(const twr_structure* s, double* lower, double* upper);
/* Initial guess of NlpFormulation::Make{Base,Endeffector,Force}Variables (nlp_formulation.cc:95-181). */
int twr_structure_initial_guess(const twr_structure* s, const double init_base_lin[3],
                                const double init_base_ang[3], const double final_base_lin[3],
                                const double final_base_ang[3], const double* init_ee_pos /* n_ee*3 */,
                                double* x_out /* n_vars */);
/* Variable bounds (x_l, x_u) that the same functions put on the node variables: start state of base
 * and feet fixed, final base state fixed in the dimensions of Parameters::bounds_final_* (parameters.cc:65-69:
 * lin pos {x,y}, lin vel, ang pos, ang vel), everything else ifopt::NoBound (+-1e20)
 * (nlp_formulation.cc:109-122,151; nodes_variables.cc:152-181).  Base states are 12 doubles
 * {lin pos, lin vel, ang pos, ang vel}. */
int twr_structure_variable_bounds(const twr_structure* s, const double init_base[12], const double final_base[12],
                                  const double* init_ee_pos /* n_ee*3 */, double* lower /* n_vars */,
                                  double* upper /* n_vars */);
/* A planning request as ONE record of TWR_START_REC doubles -- what twr_structure_initial_guess and twr_structure_variable_bounds
 * take as five arrays:
 *   [0, 12)   init_base   {lin pos, lin vel, ang pos, ang vel}
 *   [12, 24)  final_base  (the same order)
 *   [24, 36)  init_ee_pos, 3 per end-effector (entries of feet the structure does not have are not read)
 * twr_structure_start_host gives x = twr_structure_initial_guess and lower / upper = twr_structure_variable_bounds of that
 * request, bit for bit, from the structure's START TABLE: one 8-byte record per variable that names where its value comes from
 * (a node of a spline -- the later one where two share the variable --, a phase duration, or zero) and where its bounds come
 * from (a slot of the request, the phase-duration box [0.2, 1.0], or ifopt::NoBound).  It is the host executor of the table
 * twr_batch_start runs on the device; each of x / lower / upper may be NULL. */
#define TWR_START_REC 36
int twr_structure_start_host(const twr_structure* s, const double request[TWR_START_REC], double* x /* n_vars or NULL */,
                             double* lower /* n_vars or NULL */, double* upper /* n_vars or NULL */);

/* Upload the tables of a batch: problem p uses structs[struct_of_problem[p]].  device is the HIP
 * device ordinal of this process (one process per GPU).  All structures of one batch must have the same
 * number of end-effectors (<= TWR_MAX_EE): the dynamic kernel is specialised per n_ee and a batch is one launch
 * of it; robots with different leg counts go into separate batches. */
int twr_batch_create(const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem,
                     int n_problems, int device, twr_batch** out);
void twr_batch_destroy(twr_batch* b);
int twr_batch_num_problems(const twr_batch* b);
/* Device memory of the batch's tables, in bytes (any pointer may be NULL): `resident` = what the batch holds for all its
 * structures; `dyn_layout` = the layout tables of the "dynamic" set (index maps, CSR positions: everything that does not
 * hold a time) as built, `dyn_layout_distinct` = what is left of them after the batch has merged byte-identical tables of
 * different structures (candidates of a sweep that differ only in their total time share all of them), i.e. what one
 * evaluation reads.  No reference counterpart: towr recomputes these indices inside every callback
 * (towr/src/nodes_variables_phase_based.cc:210-298, spline.cc:48-78). */
int twr_batch_table_bytes(const twr_batch* b, int64_t* resident, int64_t* dyn_layout, int64_t* dyn_layout_distinct);
/* 1 when the batch's Jacobian values leave the dynamic / range-of-motion kernels with non-temporal stores, else 0.  Chosen by
 * twr_batch_create from the shape of the batch alone (fewer than four problems per structure on average AND more than
 * 256 MB of output per evaluation: a sweep whose candidates all bring their own tables); the values written are the
 * same bits either way. */
int twr_batch_streaming_stores(const twr_batch* b);
/* Slices per problem of the "dynamic" set when every problem of the batch references the same structure with fixed
 * timings (a uniform batch: many x for one NLP), else 0.  With per-kernel launches (large batches, or profiling events)
 * such a batch is evaluated by a kernel whose waves each own one slice kind and load its tables once per launch, when the
 * resident grid divides into the kinds (eval_plan.h DynUniformCols); the values written are the same bits either way. */
int twr_batch_dyn_uniform_kinds(const twr_batch* b);
/* The launches a call on this batch would issue, in order, without issuing them: which kernel, which template instantiation
 * of it, grid, block and dynamic LDS.  Read-only: planned from the same shape and by the same planner as the call itself
 * (batch_plan.h MakeEvalShape / eval_plan.h PlanEval), so it is what the device runs, for this device's CU count and memory-side cache.
 *   request TWR_PLAN_EVAL:       twr_batch_eval(flags); events != 0: as between twr_batch_profile_begin and _end
 *   request TWR_PLAN_SCORES:     twr_batch_eval_scores      (flags and events are ignored: these record no events)
 *   request TWR_PLAN_SCORE_BEST: twr_batch_eval_score_best
 * Up to max_steps steps are written; *n_steps is the number the call issues (event records are not steps).
 *   kernel:        "dyn_kernel", "dyn_uniform_kernel", "rom_kernel", "eval_fused_kernel", "phase_locate_kernel",
 *                  "dyn_phase_kernel", "rom_phase_kernel", "node_kernel", "node_kernel2", "node_chunk_kernel",
 *                  "eval_values_kernel", "eval_scores_kernel", "score_fold_kernel", "score_kernel", "best_kernel"
 *   instantiation: the kernel with its template key, e.g. "eval_fused_kernel<34,xc2,GJNT>", "rom_kernel<26,J>",
 *                  "dyn_uniform_kernel<GJ,xc4>", "eval_values_kernel<5>"; the plain name of a kernel with one body
 *   store:         "G", "J", "GJ", "JNT", "GJNT" (NT: non-temporal copy-out stores); "" for a kernel without the parameter
 *   nit:           store instructions of the copy-out (0: run-time length); xc: 64-entry chunks of the dyn staging maps, or the
 *                  doubles of x per thread (NX) of the values-only / scoring kernels
 *   uniform_kinds: slice kinds of a dyn_uniform_kernel launch, else 0 */
enum { TWR_PLAN_EVAL = 0, TWR_PLAN_SCORES = 1, TWR_PLAN_SCORE_BEST = 2 };
typedef struct twr_launch_step {
  char kernel[32];
  char instantiation[48];
  char store[8];
  int32_t nit, xc;
  int32_t grid, block, lds_bytes;
  int32_t uniform_kinds;
} twr_launch_step;
int twr_batch_eval_plan(const twr_batch* b, int request, int flags, int events, twr_launch_step* steps, int max_steps, int* n_steps);
/* Ragged layout of the batch arrays, each n_problems+1 prefix sums in units of doubles:
 * problem p owns x[x_off[p]..x_off[p+1]), g[g_off[p]..), jac[jac_off[p]..). */
int twr_batch_layout(const twr_batch* b, int64_t* x_off, int64_t* g_off, int64_t* jac_off);
/* A new map for a live batch, in place: the batch's device copy of the grid_map layer behind handle `g` (a handle at least one
 * structure of the batch was created with) and the map centre in the header of every structure of the batch that reads it are
 * overwritten; the tables, work lists and plans of the batch, and everything built on it (twr_jac_ops, twr_jac_lsq, twr_jac_lm,
 * the Gram tables) depend on the schedules alone and stay.  The device copy keeps its ADDRESS, so an evaluation captured in a
 * hipGraph before the update sees the new map when it is replayed after it.  Structures of the batch on another map are not
 * touched.  Same size and resolution only: another size is a new handle and a new batch.
 *   twr_batch_grid_map_sync:          to the handle's current content and centre (twr_terrain_grid_map_update).  The host layer
 *                                     goes to a staging buffer the batch owns (allocated by the first call) and from there into
 *                                     the map by the same kernel.  Stream-ordered on hip_stream; NOT capturable (it reads
 *                                     host memory, and its first call allocates).
 *   twr_batch_grid_map_update_device: from a layer on the batch's device, as an elevation-mapping node leaves it: d_elevation
 *                                     float[size_x * size_y], column-major, circular with start index (start_x, start_y) as in
 *                                     twr_terrain_grid_map_update, and the centre (pos_x, pos_y).  One kernel launch and nothing
 *                                     else: asynchronous on hip_stream, capturable in a hipGraph.  d_elevation is only read, and
 *                                     read when the launch runs: keep it unchanged until then.  The HOST handle is NOT touched:
 *                                     twr_batch_start (below) makes x0 and the variable bounds of a request from the new map on
 *                                     the device; only a caller that also uses the host-side structure calls
 *                                     (twr_structure_initial_guess, twr_structure_variable_bounds, twr_structure_start_host) on
 *                                     the new map calls twr_terrain_grid_map_update as well.
 * Both count as a call on the batch: at most ONE update or evaluation of a batch in flight at a time (serialise them on one
 * stream; an evaluation enqueued before the update reads the old map, one enqueued after it the new one).  Device scope and sticky
 * error as twr_batch_eval.  TWR_ERR_INVALID, with twr_last_error naming the argument, before any device is touched: b, g or
 * d_elevation NULL, d_elevation not 4-byte aligned, g a CSV grid, g not a map of this batch, a start index outside [0, size),
 * a non-finite position; nothing is changed then. */
int twr_batch_grid_map_sync(twr_batch* b, const twr_terrain_grid* g, void* hip_stream);
int twr_batch_grid_map_update_device(twr_batch* b, const twr_terrain_grid* g, const float* d_elevation, int start_x, int start_y,
                                     double pos_x, double pos_y, void* hip_stream);
/* Start of a planning request for the whole batch, on the device: x0 (twr_structure_initial_guess) and x_l / x_u
 * (twr_structure_variable_bounds) of every problem from request records in device memory (TWR_START_REC doubles each, layout
 * above).  Problem p reads the record at d_request + p * request_stride; request_stride = 0: one record for all problems.
 * The outputs are in the layout of twr_batch_layout (x_off); each of d_x / d_xlo / d_xup may be NULL, not all three.
 * The terrain heights of the guess (the goal and every final foothold) are evaluated through the batch's tables, i.e. on the
 * map the batch holds NOW: after twr_batch_grid_map_update_device that is the new map, without the host handle.
 * Results: a request whose final yaw is 0 gives the bits of the host functions.  With a turn the device's sine and cosine are
 * its own (within 1.5 ulp of libm's), so the variables that descend from a final foothold (ee-motion positions and
 * velocities) differ from the host's by rounding, everything else is bit-identical.  A non-finite or huge entry of a record
 * reaches the variables that are made from it and nothing else (no index is computed from a request without a range check).
 *   twr_batch_reserve_start: plans the call and uploads the start tables of the batch's structures (byte-identical ones once)
 *                            and the work list, into device memory of their own (twr_batch_table_bytes does not count it).
 *   twr_batch_start:         ONE kernel launch, asynchronous on hip_stream, no host synchronisation.  After
 *                            twr_batch_reserve_start it allocates nothing and is capturable in a hipGraph; without it the
 *                            first call reserves (allocates and uploads) and is NOT capturable.
 * twr_batch_start counts as a call on the batch: at most ONE update, start or evaluation of a batch in flight at a time (a map
 * update enqueued before it is seen, one enqueued after it is not).  Device scope and sticky error as twr_batch_eval.
 * TWR_ERR_INVALID, with twr_last_error naming the argument, before any device is touched: b or d_request NULL, all three
 * outputs NULL, a request_stride that is neither 0 nor >= TWR_START_REC, a pointer that is not 8-byte aligned. */
int twr_batch_reserve_start(twr_batch* b);
int twr_batch_start(twr_batch* b, const double* d_request, int64_t request_stride, double* d_x, double* d_xlo, double* d_xup,
                    void* hip_stream);

/* One full NLP callback for every problem of the batch, device pointers in, device pointers out:
 *   ifopt::Problem::EvaluateConstraints(x)        -> g     (TWR_EVAL_VALUES)
 *   ifopt::Problem::EvalNonzerosOfJacobian(x,val) -> jac   (TWR_EVAL_JACOBIAN)
 * i.e. Composite::SetVariables + {Terrain,Dynamic,RangeOfMotion,Force}Constraint::
 * {GetValues, FillJacobianBlock}.  Asynchronous on `hip_stream` (hipStream_t, may be
 * NULL for the default stream); no host synchronisation, capturable in a hipGraph.  If the calling thread's current
 * device is not the batch's, the call switches to it for the launches and RESTORES the caller's device before it
 * returns; it neither reads nor clears the thread's sticky HIP error (every launch returns its own status, which is
 * what a TWR_ERR_HIP result reports).  At most ONE evaluation of a given batch may
 * be in flight at a time (batches with optimised timings keep per-batch scratch records; the profiling
 * counters are per batch too): serialise evaluations of one batch on one stream, use one batch per stream.
 * REPRODUCIBILITY: for a FIXED value of `flags` a given x gives bit-identical g / Jacobian values wherever the problem sits
 * in a batch, on every device and rank.  The kernels are instantiated per output selection, and the selections (values
 * only / Jacobian only / both) agree with each other to rounding (<= 1e-13 of the set scale), NOT bit for bit.  A sweep
 * that compares candidates across ranks or calls must therefore score all of them with the SAME flags (near-tied
 * candidates could otherwise be ranked differently); twr_batch_score / twr_batch_best are deterministic given g.
 * (Values only: a batch in which EVERY problem has fixed timings and at most 2046 variables takes the lane-per-time-node
 * kernel, see twr_structure_values_items; one problem that cannot keeps the whole batch on the values-only instantiation of
 * the Jacobian kernels.  The two agree to rounding, so the shards of one sweep -- which all take the same path -- compare
 * bit for bit, a batch of another composition to rounding.)  twr_batch_eval_scores without g: inf-norms bit-identical to
 * twr_batch_score over this path's g, 1-norms to rounding (<= 1e-12 relative), see there. */
int twr_batch_eval(twr_batch* b, const double* d_x, double* d_g, double* d_jac, int flags, void* hip_stream);
/* Failure detection (the reference only has Release-mode-silent asserts, spline.cc:52,65): after an evaluation with
 * TWR_EVAL_CHECK, h_status[p] has bit 0 set if a constraint value of problem p is NaN/Inf and bit 1 if a Jacobian
 * value is.  Waits for hip_stream (the stream of that evaluation). */
int twr_batch_status(twr_batch* b, int32_t* h_status /* n_problems */, void* hip_stream);
/* Measurement aid (bench.py): after _begin, the next max_evals calls of twr_batch_eval also record
 * HIP events on their launch stream around each of the three kernels (dynamic, range of motion,
 * force/terrain nodes); _end waits for the last one and returns the average duration of each. */
int twr_batch_profile_begin(twr_batch* b, int max_evals);
int twr_batch_profile_end(twr_batch* b, double avg_ms[3], int* n_evals);
/* Trajectory sampling of a batch of solutions, fpowr::GetTrajectory (fpowr/include/fpowr/footstep_plan_extractor.h:
 * 19-53): problem p's x sampled every dt while t <= T + 1e-5 (t accumulated).  One record per sample, end-effectors
 * in towr order:  [ t | base lin p v a (9) | quaternion w x y z | omega (3) | omega_dot (3) |
 *                  per ee: contact (0/1), ee-motion p v a (9), ee-force (3) ]   = 20 + 13 n_ee doubles.
 * twr_structure_sample_count gives the records per problem; problem p's records start at
 * d_out + p * problem_stride (doubles).  Asynchronous on hip_stream. */
int twr_structure_sample_count(const twr_structure* s, double dt, int32_t* n_samples);
int twr_batch_sample(twr_batch* b, const double* d_x, double dt, double* d_out, int64_t problem_stride, void* hip_stream);
/* fpowr::ExtractInitialGuess / ExtractInitialGuesses (fpowr/include/fpowr/initial_guess_extractor.h:17-48) for a batch of
 * solutions: every problem's x sampled at the n_times times d_times[] (device array, within [0, T]; the goal's
 * state_sample_times).  One record of 49 doubles per time:
 *   [ t | state (12): base-lin p, base-ang p (Euler angles), base-lin v, base-ang v (Euler rates) |
 *     controls (36): ee-motion acceleration of ee i at 3 i, twelve zeros ("joint torques"), ee-force of ee i at 24 + 3 i ]
 * problem p's records start at d_out + p * problem_stride (doubles, >= 49 n_times).  Asynchronous on hip_stream. */
int twr_batch_initial_guess(twr_batch* b, const double* d_x, const double* d_times, int32_t n_times, double* d_out,
                            int64_t problem_stride, void* hip_stream);

/* Candidate scoring of a sweep (new; the reference solves one NLP per goal and lets Ipopt judge feasibility): for
 * problem p and constraint family f -- the bit index of its TWR_SET_* flag: 0 terrain, 1 dynamic, 2 splineacc, 3
 * rangeofmotion, 4 force, 5 swing, 6 totalduration, 7 baseMotion -- over the family's rows, with the bounds of
 * ConstraintSet::GetBounds (twr_structure_bounds):
 *   d_scores[16 p + 2 f]     = max_i max(lower_i - g_i, g_i - upper_i, 0)        (inf-norm of the violation)
 *   d_scores[16 p + 2 f + 1] = sum_i max(lower_i - g_i, g_i - upper_i, 0)        (1-norm)
 * (0 for families the structure does not build; NaN if a constraint value of the family is NaN).  d_g is the output of
 * twr_batch_eval with TWR_EVAL_VALUES.  Asynchronous on hip_stream. */
int twr_batch_score(twr_batch* b, const double* d_g, double* d_scores /* 16 * n_problems */, void* hip_stream);
/* The planner's decision without leaving the device: the candidate with the smallest SUM over the chosen constraint
 * families (bit f of `families` = family f of twr_batch_score, i.e. the TWR_SET_* bit) of the inf-norm violations
 * d_scores[16 c + 2 f], c < n_candidates.  The table may be longer than this batch (after an all-gather of every rank's
 * score rows it holds the whole sweep; `b` only names the device and owns the scratch).  A NaN total loses, the first
 * index wins a tie.  d_best[0] = index (as a double), d_best[1] = its total; one 16-byte copy brings the decision to the
 * host.  Asynchronous on hip_stream, capturable; one call per batch in flight at a time.
 * Replaces the host arg-min of a sweep driver over time_discretization_constraint.cc:65-75-style constraint values
 * (fpowr runs ONE candidate, footstep_plan_server.cc:193-195; a sweep over gait_generator.cc:54-105 candidates needs the
 * choice). */
int twr_batch_best(twr_batch* b, const double* d_scores, int32_t n_candidates, uint32_t families, double* d_best /* 2 */,
                   void* hip_stream);
/* twr_batch_score and twr_batch_best over THIS batch's candidates behind one call (two stream-ordered launches):
 * d_scores as twr_batch_score, d_best[0] = index_offset + the winning problem's index in the batch
 * (index_offset = the shard's first candidate: the result is then a global candidate index), d_best[1] = its total.  A
 * multi-rank sweep all-gathers the ranks' 16-byte results (the smallest total, then the smallest index, wins) instead of
 * 128 bytes per candidate.  Asynchronous on hip_stream, capturable; shares the scratch of twr_batch_best. */
int twr_batch_score_best(twr_batch* b, const double* d_g, double* d_scores /* 16 * n_problems */, uint32_t families,
                         int64_t index_offset, double* d_best /* 2 */, void* hip_stream);
/* A planner step without g: the values-only evaluation reduced to twr_batch_score's table as it is computed.
 * twr_batch_scores_without_g: 1 if the batch scores without g -- every problem takes the values-only path (fixed timings,
 * at most 2046 variables; see twr_batch_eval) --, 0 if the scoring calls need d_g.
 * twr_batch_eval_scores: d_scores[16 p + 2 f] = inf-norm, [16 p + 2 f + 1] = 1-norm of the bound violation of family f,
 * exactly twr_batch_score's table (bounds of ConstraintSet::GetBounds, twr_structure_bounds; the constraint files
 * twr_batch_score cites): 0 for families the structure does not build, NaN if a constraint value of the family is NaN,
 * all zeros for a structure without rows.
 *   - scores without g (twr_batch_scores_without_g == 1): d_g may be NULL; if it is not, it is left untouched -- no g is
 *     written anywhere.  Two launches: the values-only kernel's scoring instantiation (every wave reduces its rows to a
 *     partial record in a scratch slab of the batch) and a fold of each problem's records in a fixed order.
 *   - otherwise (optimised timings, a batch mixing them with fixed timings, problems of more than 2046 variables): exactly
 *     twr_batch_eval(TWR_EVAL_VALUES) into d_g followed by twr_batch_score, bit for bit; d_g NULL is TWR_ERR_INVALID.
 * twr_batch_eval_score_best: the same, then this shard's decision as twr_batch_score_best (families mask, index_offset,
 * d_best = {index_offset + index, total}); it shares twr_batch_best's scratch.
 * Both are asynchronous and stream-ordered on hip_stream, capturable in a hipGraph, and count as an evaluation of the batch
 * (at most one in flight, see twr_batch_eval; _score_best: one call per batch in flight, as twr_batch_best).  Device scope
 * and errors as twr_batch_eval.  They record no per-kernel profiling events (twr_batch_profile_begin).
 * REPRODUCIBILITY (without g): a given x gives bit-identical scores wherever the problem sits in the batch and on every call.
 * The inf-norms are bit-identical to twr_batch_score over a TWR_EVAL_VALUES g of the same batch (same arithmetic, same
 * bounds); the 1-norms are summed in the scoring kernel's own fixed order (per lane, a fixed xor tree over the wave, then
 * the problem's partial records in planned order) and agree with twr_batch_score to rounding (<= 1e-12 relative). */
int twr_batch_scores_without_g(const twr_batch* b);
int twr_batch_eval_scores(twr_batch* b, const double* d_x, double* d_g /* may be NULL without g */, double* d_scores /* 16 * n_problems */,
                          void* hip_stream);
int twr_batch_eval_score_best(twr_batch* b, const double* d_x, double* d_g, double* d_scores /* 16 * n_problems */, uint32_t families,
                              int64_t index_offset, double* d_best /* 2 */, void* hip_stream);
/* fpowr::ExtractFootstepPlan (fpowr/include/fpowr/footstep_plan_extractor.h:69-133) for every problem of the batch,
 * up to the nearest-plane lookup (twr_batch_contact_planes below): the solution x sampled every dt
 * (GetTrajectory, :19-53), a footstep state at the first sample and wherever HasEndEffectorContactChanged (:55-67)
 * against the previous sample; duration = time to the next footstep state, the last one lasts until time_horizon.
 * Problem p's records start at d_out + p * max_steps * (2 + 4 n_ee):
 *   [ t_global | duration | contact flag per ee | ee-motion position (3) per ee ]
 * and d_counts[p] is the number of footstep states FOUND -- never more than twr_structure_contact_steps_max, but it
 * may exceed a smaller max_steps the caller chose: then only the first min(d_counts[p], max_steps) records are
 * valid (each with its duration; the last of them lasts until the first state that was dropped).  Asynchronous on
 * hip_stream. */
int twr_structure_contact_steps_max(const twr_structure* s, int32_t* max_steps);
int twr_batch_contact_plan(twr_batch* b, const double* d_x, double dt, double time_horizon, double* d_out, int32_t max_steps,
                           int32_t* d_counts, void* hip_stream);

/* fpowr::NearestPlaneLookup (fpowr/include/fpowr/nearest_plane_lookup.h:51-85), the last step of ExtractFootstepPlan
 * (footstep_plan_extractor.h:72-73,111-118): the planar regions of the goal's terrain message as polygons in world x, y
 * (PlanarRegionsToPolygons, :20-49: boundary point (x, y, 0) rotated by the region's orientation, shifted by its
 * position) and, for every footstep state of twr_batch_contact_plan and every end-effector in contact, the index of the
 * first polygon with the smallest boost::geometry::distance to the foot's x, y (0 inside or on the boundary, else the
 * distance to the nearest boundary segment; the boundary points are walked as given, no closing edge is added -- what
 * boost does with the reference's uncorrected polygons); -1 for a foot in the air, for footstep states past d_counts[p]
 * and when there are no regions -- or when no distance is below DBL_MAX, the reference's start value: a NaN, infinite or
 * overflowing (1e300) foothold over closed polygons.  Every product and sum is rounded on its own, as in the reference's build.
 *   regions:        n_regions x 7 doubles  [position x y z | orientation x y z w]   (plane_parameters)
 *   boundary_xy:    the outer_boundary points of all regions, x y each, region r = points [boundary_start[r],
 *                   boundary_start[r+1])
 *   d_plane_index:  n_problems x max_steps x n_ee int32, written by twr_batch_contact_planes from the d_out / d_counts
 *                   of twr_batch_contact_plan (same max_steps).  Asynchronous on hip_stream. */
typedef struct twr_planes twr_planes;
int twr_planes_create(const double* regions, const double* boundary_xy, const int32_t* boundary_start, int32_t n_regions,
                      int device, twr_planes** out);
void twr_planes_destroy(twr_planes* planes);
/* the polygons in world coordinates (x y per boundary point, in the order given), for inspection */
int twr_planes_world_xy(const twr_planes* planes, double* world_xy);
int twr_batch_contact_planes(twr_batch* b, const twr_planes* planes, const double* d_plan, const int32_t* d_counts,
                             int32_t max_steps, int32_t* d_plane_index, void* hip_stream);

/* Joint-space trajectories and reachability scores: the reference's Go1 leg inverse kinematics
 * (towr/src/go1/go1leg_inverse_kinematics.cc:16-115, inverse_kinematics_go1.cc:8-47), which it runs on the RobotStateCartesian
 * records of GetTrajectory (footstep_plan_server.cc:118-129), for every sample of every problem of a batch.
 *
 * twr_leg_kinematics describes one leg chain (HAA about x, HFE and KFE about y) and how the legs map onto the front-left one.
 * twr_leg_kinematics_preset fills the reference's Go1 constants as the doubles its expressions yield; every other robot is
 * TWR_ERR_UNSUPPORTED (the reference has no IK for them) -- a caller may fill the struct for their own robot.  Every call below
 * validates the descriptor before any device is touched, twr_last_error naming the field: n_ee in 1..4, mirrors exactly +-1,
 * bends 0/1, lengths finite and > 0, offsets finite, q_min <= q_max and neither NaN.
 *
 * Foot e in the base frame is R(q)^T (p_ee - p_base), R(q) = Eigen's toRotationMatrix of the normalised quaternion of the
 * sample record (xpp_vis CartesianJointConverter's frame change; a quaternion whose norm in doubles is 0, Inf or NaN cannot be
 * normalised and gives NaN angles with flag 32); then foot * mirror[e] - base_to_hip goes through
 * GetJointAngles + EnforceLimits restated operation for operation, the reference's quirks included: -atan2(y, -z) with its
 * signed zeros, the clamp std::max(lo, std::min(hi, v)) that turns a NaN cosine into +1, limits that leave a NaN alone.
 *
 * Joint record of a sample, TWR_JOINT_REC(n_ee) doubles:  [ t | per leg: q_HAA q_HFE q_KFE flags over_reach ]
 *   flags (an integer as a double): 1 the HFE cosine was clamped (!(-1 <= c && c <= 1), so a NaN counts), 2 the KFE cosine was,
 *     4 / 8 / 16 the HAA / HFE / KFE limit was enforced, 32 an angle is NaN
 *   over_reach: max(r - (thigh + shank), |thigh - shank| - r, 0) in metres, r the HFE-to-foot distance (NaN if r is): what the
 *     clamp hides and twr_batch_joint_scores reports, which the angles alone no longer tell
 * Scores of a problem, TWR_JOINT_SCORE_REC doubles:
 *   [0] samples   [1] leg-samples with flag 1 or 2 (unreachable)   [2] leg-samples with a limit enforced
 *   [3] max over_reach   [4] max over joints and samples s >= 1 of |q(s) - q(s-1)| / dt, raw, no unwrapping (0 with one sample)
 *   [5] min distance of an angle to its nearer limit over leg-samples with no flag set (1e20 if there are none)
 *   [6] leg-samples with flag 32   [7] index of the first sample with an unreachable leg, -1 if none
 *   [3], [4], [5] are NaN if a contributing value is NaN (twr_batch_score's rule).  Maxima, minima and counts only, folded in a
 *   fixed order without atomics: the same bits wherever the problem sits in a batch, on every call and stream.
 *
 * twr_batch_joints: the records of twr_batch_sample (same dt, hence the same sample counts; d_traj / traj_stride as given
 *   there) -> joint records at d_joints + p * joint_stride.
 * twr_batch_joint_scores: joint records -> scores at d_jscores + 8 p.
 * twr_batch_eval_joint_scores: x -> scores, bit-identical to the three calls in a row, without a trajectory buffer.  It counts as
 *   an evaluation of the batch (at most one in flight).
 * All three are asynchronous and stream-ordered on hip_stream and consist of kernel launches only (twr_batch_joints builds the
 * sample work list on its first call per dt / stride like twr_batch_sample: capture after one warm call).  TWR_ERR_INVALID before
 * any device is touched: NULL arguments, pointers not 8-byte aligned, traj_stride < n_samples * (20 + 13 n_ee) or joint_stride <
 * n_samples * TWR_JOINT_REC(n_ee) for some problem, kin->n_ee != the batch's, dt not finite or <= 0, a bad descriptor. */
typedef struct twr_leg_kinematics {
  int32_t n_ee;             /* 1..4, must equal the batch's n_ee */
  int32_t knee_bend[4];     /* 0 forward, 1 backward */
  double  mirror[4][3];     /* +-1: foot_B * mirror[e] maps leg e onto the front-left leg */
  double  base_to_hip[3];   /* of the front-left leg, subtracted after mirroring */
  double  hfe_to_haa[3];    /* added after the HAA rotation */
  double  length_thigh, length_shank;
  double  q_min[3], q_max[3];  /* HAA, HFE, KFE, radians */
} twr_leg_kinematics;
#define TWR_JOINT_REC(n_ee)  (1 + 5 * (n_ee))
#define TWR_JOINT_SCORE_REC  8
int twr_leg_kinematics_preset(int robot, twr_leg_kinematics* out);
int twr_batch_joints(twr_batch* b, const twr_leg_kinematics* kin, const double* d_traj, int64_t traj_stride, double dt,
                     double* d_joints, int64_t joint_stride, void* hip_stream);
int twr_batch_joint_scores(twr_batch* b, const twr_leg_kinematics* kin, const double* d_joints, int64_t joint_stride,
                           double dt, double* d_jscores /* 8 * n_problems */, void* hip_stream);
int twr_batch_eval_joint_scores(twr_batch* b, const twr_leg_kinematics* kin, const double* d_x, double dt,
                                double* d_jscores /* 8 * n_problems */, void* hip_stream);

/* Checks of a sampled trajectory BETWEEN the constraint nodes.  The constraints hold where towr places them (dynamics and range of
 * motion on their dt grids, terrain height and the friction pyramid at the spline nodes); these two calls evaluate the same
 * quantities at every sample record of twr_batch_sample, i.e. on the trajectory a planner publishes
 * (footstep_plan_server.cc:118-129, 286-294), and fold them per problem.
 *
 * twr_batch_checks reads the sample record [ t | base p v a | q wxyz | omega | omega_dot | per ee: contact, p v a, f ] and nothing
 * else of the trajectory, and writes one check record per sample, TWR_CHECK_REC(n_ee) doubles:
 *   [ t | dynamics residual: angular (3), linear (3) | per ee: contact, clearance, f_n, cone, rom ]
 *   t, contact  the sample record's own doubles (the contact flag is carried along because the scores below tell stance from swing
 *               and are folded from check records alone; with optimised timings only the trajectory knows the phase)
 *   residual    SingleRigidBodyDynamics::GetDynamicViolation (single_rigid_body_dynamics.cc:76-103) in its order:
 *                 angular  I_w omega_dot + omega x (I_w omega) - sum_e f_e x (p_base - p_e),   I_w = R I_b R^T
 *                 linear   m a - sum_e f_e, + m g on z
 *               R = the rotation of the record's normalised quaternion (as twr_batch_joints forms it); m, g and I_b are those of the
 *               problem's structure, the constants its constraints were built with
 *   clearance   p_e.z - h(p_e.x, p_e.y), h the terrain of the problem's structure; for a `Grid` batch the map the batch holds when
 *               the launch runs
 *   f_n         f_e . n
 *   cone        mu f_n - max(|f_e . t1|, |f_e . t2|): >= 0 inside the friction pyramid.  n, t1, t2: the normalised terrain basis at
 *               (p_e.x, p_e.y) as the force constraint forms it (height_map.cc:93-139), mu the structure's friction coefficient
 *   rom         max_d (|foot_B[d] - nominal_stance[e][d]| - max_dev[d]), foot_B = R^T (p_e - p_base): <= 0 inside the box of
 *               range_of_motion_constraint.cc:71-81
 * Of `model` only n_ee, nominal_stance, max_dev and force_limit are read.  force_limit enters nowhere but the validation: the
 * caller compares score [5] and the f_n of the records with it.
 * Order of operations: no operation is contracted, sums over the end-effectors run left to right from 0, I_w is formed as
 * (R I_b) R^T row by row, every dot product left to right (the header of csrc/kernels/checks.h lists every expression).  A check
 * record is thus a function of its sample record alone, the same bits in every batch, slot, call and stream, and a restatement in
 * plainly rounded doubles reproduces it bit for bit (tests/check_points.py).
 *
 * twr_batch_check_scores folds a problem's check records into TWR_CHECK_SCORE_REC doubles at d_cscores + 8 p:
 *   [0] samples   [1] max |linear residual component|   [2] max |angular residual component|
 *   [3] min clearance over leg-samples with contact 0 (1e20 if none)   [4] max |clearance| over leg-samples in contact (0 if none)
 *   [5] min f_n over leg-samples in contact (1e20 if none)   [6] min cone over leg-samples in contact (1e20 if none)
 *   [7] max rom over all leg-samples
 *   A leg-sample is in contact when its flag is not 0.  [1] - [7] are NaN if a contributing value is NaN (twr_batch_score's rule).
 *   Maxima, minima and counts only, one wave per problem in rounds of 64 samples, no atomics: the same bits wherever the problem
 *   sits in a batch.
 *
 * Both calls are asynchronous and stream-ordered on hip_stream and consist of kernel launches only.  twr_batch_checks walks the
 * sample work list of twr_batch_sample (same dt and traj_stride as given there, built on the first call per dt / stride): capturable
 * in a hipGraph after one warm call; twr_batch_check_scores is always capturable.  twr_batch_checks counts as a call on the batch,
 * because it reads the live map: a twr_batch_grid_map_update_device enqueued before it on the stream is seen, one enqueued after it
 * is not.  Device scope and sticky error as twr_batch_eval.
 * TWR_ERR_INVALID, with twr_last_error naming the argument or field, before any device is touched: a NULL argument, a pointer
 * that is not 8-byte aligned, traj_stride < n_samples * (20 + 13 n_ee) or check_stride < n_samples * TWR_CHECK_REC(n_ee) for some
 * problem, dt not finite or <= 0, model->n_ee != the batch's, a nominal_stance, max_dev or force_limit that is not finite,
 * a max_dev < 0.
 * Hostile records are contained: the only index computed from a record is the cell lookup of the terrain, behind its range checks;
 * a NaN / Inf / 1e300 foot or force reaches the fields of its own sample that are made from it (its leg's fields and the residual)
 * and nothing else; a quaternion that cannot be normalised (norm 0, Inf or NaN in doubles) gives a NaN angular residual and NaN
 * rom for that sample. */
#define TWR_CHECK_REC(n_ee)  (7 + 5 * (n_ee))
#define TWR_CHECK_SCORE_REC  8
int twr_batch_checks(twr_batch* b, const twr_model* model, const double* d_traj, int64_t traj_stride, double dt, double* d_checks,
                     int64_t check_stride, void* hip_stream);
int twr_batch_check_scores(twr_batch* b, const double* d_checks, int64_t check_stride, double dt,
                           double* d_cscores /* 8 * n_problems */, void* hip_stream);

/* Convenience for single-problem / adapter use: host buffers, synchronous (H2D, eval, D2H).  Runs on a NON-BLOCKING
 * stream the batch owns (created on first use), not on the NULL stream: it neither waits for nor holds up work the host
 * application has in flight on the NULL stream or on its own blocking streams; the call returns when its own chain is
 * done.  flags select what is evaluated and copied back (TWR_EVAL_VALUES alone moves no Jacobian over PCIe: the ifopt
 * adapter evaluates values for eval_g and adds the Jacobian only when eval_jac_g asks for it). */
int twr_batch_eval_host(twr_batch* b, const double* h_x, double* h_g, double* h_jac, int flags);
/* Page-locked host buffers owned by the batch (x, g, jac of the whole batch layout), allocated on first
 * use.  Passing exactly these pointers to twr_batch_eval_host makes the transfers DMA directly from / into
 * them (no staging through pageable memory): what an Ipopt callback should read g and the Jacobian
 * values from (the ifopt adapter does).  For batches of up to 32 MB of Jacobian values the kernels then store g and
 * the Jacobian values straight into these host buffers over PCIe (each value once, coalesced) instead of into HBM
 * followed by two copies: and gather x from them: 34 instead of 53 us for one quadruped problem (TWR_HOST_ZERO_COPY=0 switches it off). */
int twr_batch_host_buffers(twr_batch* b, double** h_x, double** h_g, double** h_jac);

/* Products with the Jacobian values of a batch, on the device (new; what every gradient-based use of a Jacobian needs):
 *   twr_jac_mul:  y[g_off[p] + r] = sum_k J_p[r][k] v[x_off[p] + k]    -- the directional derivative J v: Ipopt's first-order
 *                 derivative test (towr/test/hopper_example.cc:86), a Gauss-Newton / CG step
 *   twr_jac_tmul: z[x_off[p] + k] = sum_r J_p[r][k] w[g_off[p] + r]    -- J^T w: the gradient of SoftConstraint,
 *                 jac.transpose() * W * (g - b) (towr/src/soft_constraint.cc:61-66), of 1/2 |viol|^2 with w = viol, the
 *                 J^T lambda term of a KKT check
 * J_p = d_jac + jac_off[p]: the CSR values of problem p as twr_batch_eval writes them (TWR_EVAL_JACOBIAN or TWR_EVAL_BOTH, any
 * store policy, any launch path: the layout is the same).  A handle of its own: twr_jac_ops_create takes the same arguments as
 * twr_batch_create and its x / g / jac layout is exactly that batch's (twr_jac_ops_layout == twr_batch_layout); a batch that
 * never asks for products allocates nothing for them.  The handle owns the device copies of what it reads (the patterns,
 * byte-identical ones stored once, column indices in 16 bits, and its work lists), so it may outlive the batch and the
 * structures.  Both products are asynchronous and stream-ordered on hip_stream and capturable in a hipGraph; device scope,
 * error codes and the sticky HIP error as twr_batch_eval; NULL buffers are TWR_ERR_INVALID, and so are buffers that are not
 * 8-byte aligned.  At most ONE product per handle in flight (J^T w keeps its partials in the handle's slab); handles on
 * different streams are independent.  Outputs must not overlap inputs.
 * Summation order is a function of the problem's structure alone (jac_plan.h, twr::PlanJacOps): a problem's y and z have the
 * same bits wherever it sits in whatever batch, on every call, stream and device, and a NaN / Inf in one problem's J, v or w
 * reaches that problem's outputs only.  A structure without rows: J v writes nothing, J^T w writes zeros; a column without
 * entries gets an exact 0. */
typedef struct twr_jac_ops twr_jac_ops;
int twr_jac_ops_create(const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem, int n_problems, int device,
                       twr_jac_ops** out);
void twr_jac_ops_destroy(twr_jac_ops* ops);
int twr_jac_ops_layout(const twr_jac_ops* ops, int64_t* x_off, int64_t* g_off, int64_t* jac_off);
/* resident: device bytes the handle holds (tables, work lists, slab); distinct_patterns: the patterns its tables hold once each */
int twr_jac_ops_bytes(const twr_jac_ops* ops, int64_t* resident, int32_t* distinct_patterns);
int twr_jac_mul(twr_jac_ops* ops, const double* d_jac, const double* d_v, double* d_y, void* hip_stream);
int twr_jac_tmul(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_z, void* hip_stream);
/* Weighted squared column norms: d_out[x_off[p] + k] = sum_r w[g_off[p] + r] J_p[r][k]^2 (d_w NULL: unit weights) -- what
 * Marquardt's scaled damping (twr_jac_col_scale below), a Jacobi preconditioner and Ipopt-style variable scaling need.  It runs
 * over J^T w's work list, block maps, slab and fold, the values squared as they are staged, so everything said of twr_jac_tmul
 * holds word for word: the order of every sum is a function of the pattern alone (same bits wherever the problem sits, on every
 * call, stream and device), a column without entries gets an exact 0, a NaN / Inf stays in its problem, capturable, ONE call
 * per handle in flight (the slab), the same NULL / alignment / device-scope / sticky-error rules.  With w >= 0 every term is
 * non-negative: the result is 0 exactly when the column has no entry with w_r J_rk^2 != 0. */
int twr_jac_col_sqnorms(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_out, void* hip_stream);
/* The normal product in one pass over J: d_u[x_off[p] + k] = (J_p^T (w o (J_p v)))_k in the x layout and, unless d_y is NULL,
 * d_y = J v in the g layout (d_w NULL: unit weights) -- what an iteration of CG on the normal equations needs, with the
 * Jacobian values read from memory once instead of once per product.  Blocks of whole rows: a block's values are kept in LDS
 * while its rows' sums y_r are taken, multiplied by t_r = w_r y_r there, and summed per column into partials that the fold of
 * twr_jac_tmul adds in block order (jac_plan.h, twr::PlanJacNormal).  Everything said of the two products holds: no atomics,
 * the order of every sum a function of the pattern alone (same bits wherever the problem sits, on every call, stream and
 * device; d_y NULL does not change d_u), a column without entries gets an exact 0, a structure without rows writes no y and
 * zeros to u, J, v and w are only multiplied and added (a NaN / Inf stays in its problem), stream-ordered and capturable, ONE
 * call per handle in flight (the one-pass slab), the same NULL (d_w and d_y may be) / alignment / device-scope / sticky-error
 * rules.  u is not bit-identical to twr_jac_tmul of w o twr_jac_mul(v): the blocks differ.
 *   twr_jac_ops_reserve_normal: plans, uploads and allocates the one-pass tables, work list and slab, once; twr_jac_ops_bytes
 *                               counts them from then on, and a handle that never asks holds what it held before.  The calls
 *                               that need them (twr_jac_normal_mul, twr_jac_lsq_solve_onepass) call it themselves when it has
 *                               not been called: that one call allocates and can NOT be captured in a hipGraph -- reserve
 *                               before capturing.
 *   twr_jac_ops_reserve_normal_tile: the same with an LDS tile of tile_entries (1 .. 2048) entries instead of 2048, for tuning
 *                               and for tests (a small tile turns ordinary rows into rows longer than a tile).  Results
 *                               keep every property above; their bits depend on the tile.  TWR_ERR_INVALID once the tables
 *                               exist for another tile. */
int twr_jac_ops_reserve_normal(twr_jac_ops* ops);
int twr_jac_ops_reserve_normal_tile(twr_jac_ops* ops, int tile_entries);
int twr_jac_normal_mul(twr_jac_ops* ops, const double* d_jac, const double* d_w, const double* d_v, double* d_y, double* d_u,
                       void* hip_stream);
/* Host introspection: the CSC view of the CSR pattern -- col_ptr[n_vars + 1], and per entry row_idx[nnz] (ascending within a
 * column) and csr_pos[nnz], its position in the CSR value array (CSC values = csr_values[csr_pos]).  Any pointer may be NULL.
 * TWR_ERR_INVALID if a row's column indices do not ascend strictly (they always do for the patterns the factory builds; the
 * products rely on it). */
int twr_structure_transpose(const twr_structure* s, int32_t* col_ptr, int32_t* row_idx, int32_t* csr_pos);

/* The damped weighted least-squares step with the Jacobian values of a batch, on the device (new; the linear solve in the middle
 * of a Levenberg-Marquardt / damped Gauss-Newton method), per problem p and for the whole batch at once:
 *   d_p = argmin_d  sum_r w_r (J_p d - b_p)_r^2 + mu_p |d|^2     <=>   (J_p^T W_p J_p + mu_p I) d_p = J_p^T W_p b_p
 * by CGLS on top of twr_jac_mul / twr_jac_tmul: matrix-free, no factorisation, J^T J never formed (towr's J is rank deficient;
 * mu > 0 makes the step unique).  A handle of its own, created from a twr_jac_ops it BORROWS (ops must outlive it) and the
 * arguments ops was created with: a mismatch in the problem count or in any problem's n / m is TWR_ERR_INVALID, and so is a
 * NULL ops (checked before any device is touched).  The handle owns the solver's workspace and the device copy of the per-row
 * bounds (twr_structure_bounds; byte-identical tables stored once); a twr_jac_ops that never asks for a solve allocates nothing.
 * All three calls are asynchronous and stream-ordered on hip_stream and capturable in a hipGraph (kernel launches only); device
 * scope, error codes, the sticky HIP error, NULL and 8-byte alignment checks as twr_jac_mul.  At most ONE call per handle in
 * flight, and none together with a product on the borrowed ops (the solve uses the handle's workspace and the ops' slab).
 * Outputs must not overlap inputs.  No atomics: every per-problem sum is taken in an order fixed by the problem's sizes alone,
 * so a problem's outputs have the same bits wherever it sits in whatever batch, on every call and stream, and a NaN / Inf in
 * one problem's inputs reaches that problem's outputs only.
 *   twr_jac_dot:       d_out[p] = sum_i a_i b_i over the x layout (space 0) or the g layout (space 1)
 *   twr_jac_violation: d_r = g - min(max(g, lower), upper): |r_i| is the per-row quantity twr_batch_score reduces, a NaN g_i gives
 *                      a NaN r_i.  Optional (NULL to leave out): d_w weights (NULL = 1), d_w_active = w [r != 0] (the active-set
 *                      weights), d_merit[p] = 1/2 sum_i w_i r_i^2.
 *   twr_jac_lsq_solve: d_d (x layout) = the step above from d = 0: r = b, s = J^T(w o r), p = s, gamma = gamma0 = s^T s; repeat
 *                      q = J p, delta = q^T(w o q) + mu p^T p, alpha = gamma / delta, d += alpha p, r -= alpha q,
 *                      s = J^T(w o r) - mu d, gamma' = s^T s, beta = gamma' / gamma, p = s + beta p.  At most `iters` iterations; a
 *                      problem stops when gamma <= tol^2 gamma0, and from then on its d does not change whatever the rest of the
 *                      batch still does (a larger `iters` gives the same bits).  d_w NULL = unit weights.  d_mu: one mu >= 0 per
 *                      problem, read on the device; the launch sequence depends on iters alone, no scalar comes to the host.
 *                      d_info[4p ..]: iterations taken, |s| / |s0|, |s0|, status: 0 converged (also |s0| = 0: b = 0 or a structure
 *                      without rows, d = 0), 1 iteration cap, 2 bad input (mu < 0 or not finite, a non-finite |s0| or gamma, a
 *                      delta that is not a positive finite number); d is then what it was when the problem stopped, zeros if
 *                      that was at the start.  iters == 0 writes d = 0 and |s0|. */
typedef struct twr_jac_lsq twr_jac_lsq;
int twr_jac_lsq_create(twr_jac_ops* ops, const twr_structure* const* structs, int n_structs, const int32_t* struct_of_problem,
                       int n_problems, twr_jac_lsq** out);
void twr_jac_lsq_destroy(twr_jac_lsq* lsq);
/* resident: device bytes the handle holds (bound tables, work records, workspace; the scaled solve's once reserved) */
int twr_jac_lsq_bytes(const twr_jac_lsq* lsq, int64_t* resident);
int twr_jac_dot(twr_jac_lsq* lsq, int space, const double* d_a, const double* d_b, double* d_out, void* hip_stream);
int twr_jac_violation(twr_jac_lsq* lsq, const double* d_g, const double* d_w, double* d_r, double* d_w_active, double* d_merit,
                      void* hip_stream);
int twr_jac_lsq_solve(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu, int iters,
                      double tol, double* d_d, double* d_info, void* hip_stream);
/* Marquardt-scaled damping: towr's variables are metres, radians, m/s and newtons in one vector and the weighted column norms
 * of its Jacobian span nine orders of magnitude, so mu I damps some variables not at all and freezes others.  With
 * C = diag(c), c_k = 1 / (column norm k), the step
 *   d_p = argmin_d  sum_r w_r (J_p d - b_p)_r^2 + mu_p sum_k (d_k / c_k)^2    <=>   (J^T W J + mu C^-2) d = J^T W b
 * does not depend on the units of x.  Same rules as the calls above (stream order, capture, one call per handle in flight,
 * bits independent of the batch, containment, NULL / alignment checks).
 *   twr_jac_col_scale:        d_scale (x layout) from d_colsq (twr_jac_col_sqnorms): a_k = colsq_k, or, with d_colsq_max given
 *                             (in / out, x layout: the running maximum over the steps of an LM loop, start it at 0),
 *                             a_k = colsq_max_k = max(colsq_max_k, colsq_k); top = max_k a_k;
 *                             c_k = 1 / sqrt(max(a_k, rel_floor top)); c_k = 1 for every k of a problem with top == 0.  A NaN a_k
 *                             gives a NaN c_k for that k alone.  rel_floor outside (0, 1] is TWR_ERR_INVALID.
 *   twr_jac_lsq_solve_scaled: the iteration of twr_jac_lsq_solve on J C in e = d / c: s = c o J^T(w o r) - mu e, p = s + beta p,
 *                             q = J (c o p), delta = q^T(w o q) + mu p^T p, e += alpha p, d = c o e, r -= alpha q.  Stopping rule,
 *                             d_info, status codes, freezing of finished problems and the launch sequence as twr_jac_lsq_solve,
 *                             |s| and |s0| being the scaled quantities; with c = 1 it returns the bits of twr_jac_lsq_solve.  A c_k
 *                             that is not a positive finite number is bad input: status 2, d = 0.
 *   twr_jac_lsq_reserve_scaled: allocates the scaled solve's two extra vectors (x layout), once; twr_jac_lsq_bytes counts them
 *                             from then on.  twr_jac_lsq_solve_scaled calls it itself when it has not been called: that one call
 *                             allocates and can NOT be captured in a hipGraph -- reserve before capturing. */
int twr_jac_lsq_reserve_scaled(twr_jac_lsq* lsq);
int twr_jac_col_scale(twr_jac_lsq* lsq, const double* d_colsq, double* d_colsq_max, double rel_floor, double* d_scale, void* hip_stream);
int twr_jac_lsq_solve_scaled(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                             const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream);
/* The same step with J read once per iteration: the gradient is recurred instead of formed from r.  From d = 0: r = b,
 * s = J^T(w o b) (twr_jac_tmul), p = s, gamma = gamma0 = s^T s; repeat (q, u) = twr_jac_normal_mul(p),
 * delta = q^T(w o q) + mu p^T p, alpha = gamma / delta, d += alpha p, r -= alpha q, s -= alpha (u + mu p), gamma' = s^T s,
 * beta = gamma' / gamma, p = s + beta p: three launches per iteration (the one-pass product, its fold, one vector kernel)
 * instead of five.  In exact arithmetic these are the iterates of twr_jac_lsq_solve; in floating point the recurred s drifts
 * from the true gradient by rounding only, and d is close to, not bit-identical with, twr_jac_lsq_solve's.
 * d_scale NULL: the unscaled step.  Otherwise the Marquardt-scaled step of twr_jac_lsq_solve_scaled, the same iteration on J C
 * in e = d / c: s0 = c o J^T(w o b), the product reads c o p, u is multiplied by c, d = c o e; with c = 1 it returns the bits
 * of the unscaled one-pass solve.  Stopping rule, d_info, status codes, freezing of finished problems, iters == 0 and the bad
 * mu / bad c rules as twr_jac_lsq_solve[_scaled]; the launch sequence depends on iters alone; d has the same bits in any batch,
 * call and stream and under any larger iters.  The first call allocates (twr_jac_ops_reserve_normal on the borrowed ops, two
 * more vectors in the x layout here, twr_jac_lsq_reserve_scaled with d_scale) and can NOT be captured: before capturing, call
 * twr_jac_lsq_reserve_onepass (scaled != 0: for a d_scale as well), which makes all of them, once.  twr_jac_lsq_bytes and
 * twr_jac_ops_bytes count the additions from then on. */
int twr_jac_lsq_reserve_onepass(twr_jac_lsq* lsq, int scaled);
int twr_jac_lsq_solve_onepass(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                              const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream);

/* Variable bounds (new): a bound-constrained Levenberg-Marquardt step and its driver, by projected active-set LM (the way Ceres
 * and scipy's trf treat boxes).  towr fixes the start state, the final base state and the initial footholds with lo == up and,
 * with optimised timings, boxes every phase duration (twr_structure_variable_bounds); x + d of the free step leaves all of them.
 * Here the fixed and the blocked variables are taken out of the solve by an exact zero in the column scale, the trial point is
 * projected onto the box, and accept / reject and mu are decided per problem on the device.  Same rules as the calls above:
 * asynchronous and stream-ordered, capturable (kernel launches only), no atomics, every per-problem sum in an order fixed by the
 * problem's sizes alone (the same bits wherever the problem sits in whatever batch, on every call and stream), a NaN / Inf in
 * one problem's inputs stays in that problem, NULL / 8-byte alignment checks, one call per handle in flight.
 *   twr_jac_lsq_solve_masked: the iteration of twr_jac_lsq_solve_scaled (CGLS), where a c_k that is exactly 0 is legal and means
 *                             "variable k does not move": e_k stays 0, d_k is an exact +0, and |s|, |s0| are taken over the
 *                             free scaled space.  A c_k that is negative, NaN or Inf stays bad input (status 2).  With no zero
 *                             in c it returns the bits of twr_jac_lsq_solve_scaled.  Launch sequence, freezing, d_info, status
 *                             codes and the workspace (twr_jac_lsq_reserve_scaled) as twr_jac_lsq_solve_scaled.
 *   twr_jac_free_set:         d_scale_out[k] = blocked_k ? +0 : d_scale_in[k] (d_scale_in NULL: 1), with
 *                             blocked_k = (x_k <= lo_k && z_k <= 0) || (x_k >= up_k && z_k >= 0), z = J^T(w o b) the direction
 *                             of descent: a variable on a bound that the step would push outwards, and every variable with
 *                             lo == up that sits on its value.  d_nfree[p] = the number of free variables of problem p (as a
 *                             double).  x, lo, up, z and the scales are in the x layout; bounds of +-1e20 (ifopt's NoBound)
 *                             are ordinary numbers.  d_scale_out may be d_scale_in.
 * The driver, a handle of its own that BORROWS the batch, the twr_jac_lsq and, through it, its twr_jac_ops: all of them must
 * outlive it and share one layout and device (a mismatch is TWR_ERR_INVALID; NULL arguments are checked before any device is
 * touched).  It
 * owns its workspace (twr::PlanJacLm, jac_plan.h); twr_jac_lm_create also reserves the scaled solve's vectors of lsq.
 *   twr_jac_lm_start: binds the caller's buffers -- d_x (in / out), d_xlo, d_xup (x layout), d_g, d_jac (the caller's, g / jac
 *                     layout; the linearisation of the last step is left in them) --, projects x onto the box, linearises and
 *                     sets mu0 = clamp(tau lambda_max(C_f J^T W J C_f)), lambda_max from power_iters power iterations on the
 *                     device from a fixed start vector (power_iters == 0: mu0 = tau).  A problem whose x holds a NaN, an Inf
 *                     or a value beyond +-1e20 (ifopt's "no bound": not a number to the NLP), or whose bounds hold a NaN or
 *                     lo > up, is BAD from here on and its x is not touched, not even projected.
 *   twr_jac_lm_step:  one step as one chain of launches, no host synchronisation, no scalar to the host, the sequence a function
 *                     of the parameters alone (capturable after start, k steps as well): eval(BOTH) at x; violation (r, active
 *                     weights w, merit); b = -r; column norms and the scale c with the running maximum; z = J^T(w o b); free
 *                     set; masked solve; x_t = min(max(x + d, lo), up); eval(VALUES) at x_t; violation; accept per problem:
 *                     ok = merit_t < merit (a NaN rejects), x = x_t where ok, mu = clamp(mu mu_down) or clamp(mu mu_up).
 *                     A problem whose merit at the linearisation is <= merit_done is DONE: x and mu never change again.  A
 *                     non-finite merit at the linearisation or a solve status 2 makes it BAD: x stays as it is.  The merit
 *                     a trial is compared with is the recorded one (the first linearisation's, then the accepted trials'),
 *                     so a problem's recorded merit never rises.  The re-linearisation after a reject is not skipped.
 *   twr_jac_lm_state: copies the records to d_out (device, TWR_JAC_LM_REC doubles per problem), stream-ordered: merit at start,
 *                     current merit, mu, steps taken, steps accepted, free variables and CG iterations of the last step taken,
 *                     state (0 running, 1 done, 2 bad).
 *   twr_jac_lm_bytes: device bytes the handle owns. */
#define TWR_JAC_LM_REC 8
typedef struct twr_jac_lm_params {
  int32_t cg_iters;      /* 60: the iteration cap of the masked solve */
  int32_t power_iters;   /* 30 */
  double cg_tol;         /* 1e-8 */
  double mu_down;        /* 1/3: mu *= mu_down after an accepted step */
  double mu_up;          /* 10:  mu *= mu_up after a rejected one */
  double mu_min, mu_max; /* 1e-16, 1e16: mu is clamped to these, so a problem that keeps rejecting cannot run mu to Inf */
  double rel_floor;      /* 1e-12: twr_jac_col_scale */
  double tau;            /* 1e-2 */
  double merit_done;     /* 0 */
} twr_jac_lm_params;
typedef struct twr_jac_lm twr_jac_lm;
int twr_jac_lm_params_default(twr_jac_lm_params* out);
int twr_jac_lsq_solve_masked(twr_jac_lsq* lsq, const double* d_jac, const double* d_b, const double* d_w, const double* d_mu,
                             const double* d_scale, int iters, double tol, double* d_d, double* d_info, void* hip_stream);
int twr_jac_free_set(twr_jac_lsq* lsq, const double* d_x, const double* d_xlo, const double* d_xup, const double* d_z,
                     const double* d_scale_in, double* d_scale_out, double* d_nfree, void* hip_stream);
int twr_jac_lm_create(twr_batch* batch, twr_jac_lsq* lsq, const twr_jac_lm_params* params, twr_jac_lm** out);
void twr_jac_lm_destroy(twr_jac_lm* lm);
int twr_jac_lm_bytes(const twr_jac_lm* lm, int64_t* resident);
int twr_jac_lm_start(twr_jac_lm* lm, double* d_x, const double* d_xlo, const double* d_xup, double* d_g, double* d_jac,
                     void* hip_stream);
int twr_jac_lm_step(twr_jac_lm* lm, void* hip_stream);
int twr_jac_lm_state(twr_jac_lm* lm, double* d_out /* TWR_JAC_LM_REC * n_problems */, void* hip_stream);

/* The Gram matrix (new): N_p = J_p^T W_p J_p formed ONCE per linearisation and kept, and the damped step solved on it.  The CGLS
 * calls above read the Jacobian values twice per iteration (once with the one-pass product); N is small (C3: 70 552 stored values
 * against 102 896 of J) and an iteration of CG on it reads nothing else, so the whole solve is ONE launch with every vector in
 * LDS.  Where the duration columns are dense (optimised timings with every constraint set) N is larger than 2 nnz J and CGLS
 * stays the better solve: an alternative the caller picks, no existing call changes.  Planned on the host (jac_plan.h,
 * twr::PlanJacGram): per distinct pattern the pattern of N = J^T J as FULL symmetric CSR (structural: an explicit zero of J
 * counts, a column of J without entries is an empty row and column; column indices ascending, 16 bits on the device) and, per
 * stored entry (i, j) of the lower triangle, the list of its terms (row r, position of J_ri, position of J_rj) in ascending r,
 * packed in 64 bits; byte-identical patterns are stored once.
 * LIMITS, checked by twr_jac_ops_reserve_gram (TWR_ERR_UNSUPPORTED, twr_last_error says which): at most 65 536 rows and
 * 16 777 216 Jacobian entries per problem (16 + 24 + 24 bits of a term), fewer than 2^31 terms per pattern, and at most 3412
 * variables per problem (the solve keeps six vectors of n doubles in the 160 KiB of LDS one workgroup may have).
 * The rules of the calls above hold: asynchronous and stream-ordered on hip_stream, capturable in a hipGraph (kernel launches
 * only) once reserved, at most ONE call per handle in flight, outputs must not overlap inputs, NULL and 8-byte alignment are
 * checked before any device is touched, no atomics and the order of every sum a function of the pattern alone (a problem's
 * outputs have the same bits wherever it sits in whatever batch, on every call and stream), a NaN / Inf in one problem's inputs
 * stays in that problem, and a structure without rows has N = 0 (no stored value) and d = 0 with status 0.
 *   twr_structure_gram_pattern: host introspection, the pattern of N of one structure: row_ptr[n + 1], col_idx[nnz N].  Any
 *                             pointer may be NULL; *nnz alone gives the size.
 *   twr_jac_ops_reserve_gram: plans and uploads the tables and work lists, once; twr_jac_ops_bytes counts them from then on and a
 *                             handle that never asks holds what it held before.  The calls that need them call it themselves
 *                             when it has not been called: that one call allocates and can NOT be captured -- reserve first.
 *   twr_jac_ops_gram_layout:  gram_off[n_problems + 1] (doubles, every start on a 16-byte boundary): the values of N_p are
 *                             d_gram[gram_off[p] + k], k over the CSR pattern above.  The CALLER owns the value buffer of
 *                             gram_off[n_problems] doubles, as it owns d_jac: 4.6 GB for 8192 C3 problems.  Needs the reserve.
 *   twr_jac_gram:             d_gram = J^T W J for every problem (d_w NULL: unit weights, the same bits as weights of 1).  One
 *                             lane per entry of the lower triangle adds (w_r J_ri) J_rj in ascending r with fused multiply-adds
 *                             and stores the sum to (i, j) and (j, i): N_ij and N_ji carry the same bits.
 *   twr_jac_gram_mul:         d_u[x_off[p] + i] = sum_j N_p[i][j] v[x_off[p] + j] (x layout): power iterations, tests.
 *   twr_jac_lsq_solve_gram:   (C N C + mu I) e = c o z, d = c o e by CG from e = 0, z = J^T (w o b) from the caller
 *                             (twr_jac_tmul): s = c o z, p = s, gamma = gamma0 = s^T s; repeat u = c o (N (c o p)),
 *                             delta = p^T u + mu p^T p, alpha = gamma / delta, e += alpha p, s -= alpha (u + mu p),
 *                             gamma' = s^T s, beta = gamma' / gamma, p = s + beta p.  The gradient s is RECURRED, never formed
 *                             again from a residual (there is none): it drifts from the true gradient by rounding only, as in
 *                             twr_jac_lsq_solve_onepass, and d is close to, not bit-identical with, the CGLS calls'.  d_scale
 *                             NULL: c = 1 (the same bits as a scale of ones).  A c_k that is exactly 0 means "variable k does
 *                             not move", as in twr_jac_lsq_solve_masked: d_k is an exact +0 and |s|, |s0| are taken over the free
 *                             space; a negative, NaN or Inf c_k is bad input.  Stopping rule (gamma <= tol^2 gamma0), d_info,
 *                             status codes 0 / 1 / 2, the bad mu rule, iters == 0 (d = 0 and |s0|) and "a larger iters gives
 *                             the same bits" as twr_jac_lsq_solve_scaled; on bad input d_info[4p + 1] is sqrt(gamma / gamma0)
 *                             as it stood: 1 for a bad mu or c with a finite |s0|, or where N holds a NaN (the first delta),
 *                             NaN where |s0| itself is not finite.  One launch whose shape depends on the batch alone;
 *                             one workgroup per problem, which ends when its problem stops.  The solve multiplies, then adds
 *                             (no fused multiply-add), every sum in a stated order (jac/gram.h): scripts/gram_cpu.py
 *                             gram_cg_device restates it in numpy bit for bit, the iteration counts included. */
int twr_structure_gram_pattern(const twr_structure* s, int32_t* row_ptr /* n + 1 */, int32_t* col_idx, int64_t* nnz);
int twr_jac_ops_reserve_gram(twr_jac_ops* ops);
int twr_jac_ops_gram_layout(const twr_jac_ops* ops, int64_t* gram_off /* n_problems + 1 */);
int twr_jac_gram(twr_jac_ops* ops, const double* d_jac, const double* d_w, double* d_gram, void* hip_stream);
int twr_jac_gram_mul(twr_jac_ops* ops, const double* d_gram, const double* d_v, double* d_u, void* hip_stream);
int twr_jac_lsq_solve_gram(twr_jac_lsq* lsq, const double* d_gram, const double* d_z, const double* d_mu, const double* d_scale,
                           int iters, double tol, double* d_d, double* d_info, void* hip_stream);
/* The linear solve of the driver: TWR_JAC_LM_CGLS (the default: twr_jac_lsq_solve_masked) or TWR_JAC_LM_GRAM (twr_jac_gram on the
 * active-set weights, then twr_jac_lsq_solve_gram with the z and the free set of the linearisation; everything else about a
 * step -- records, DONE / BAD, capture of k steps, no scalar to the host -- is unchanged).  Legal between twr_jac_lm_create and
 * twr_jac_lm_start (TWR_ERR_INVALID later).  TWR_JAC_LM_GRAM reserves the Gram tables of the borrowed twr_jac_ops
 * (TWR_ERR_UNSUPPORTED where they have none) and allocates the driver's own N, which twr_jac_lm_bytes counts from then on.
 * The power iteration of twr_jac_lm_start runs on J with either solver.  twr_jac_lm_params keeps its layout. */
enum { TWR_JAC_LM_CGLS = 0, TWR_JAC_LM_GRAM = 1 };
int twr_jac_lm_set_solver(twr_jac_lm* lm, int solver);

/* Tuning knobs.  The DEFAULT build reads nothing from the environment: the values below are compiled in.  A build with
 * -DTWR_TUNING_KNOBS (make -C towr_amd/csrc TUNING=1) reads them, for A/B measurements (scripts/ab.py):
 * TWR_STREAM_NT when a batch is created, TWR_HOST_ZERO_COPY[_X] once per process, the launch knobs (the BPC, FUSED knobs) on
 * every twr_batch_eval, so that an experiment may change them between evaluations of one process.  They never change
 * results, only how the work is spread over the device:
 *   TWR_DYN_BPC, TWR_ROM_BPC        persistent workgroups per CU of dyn_kernel / rom_kernel (8 / 4: their LDS images fill a CU)
 *   TWR_NODE_BPC                    persistent waves per CU of node_chunk_kernel, all families together (16)
 *   TWR_PDYN_BPC, TWR_PROM_BPC      the same for dyn_phase_kernel / rom_phase_kernel (default: what their LDS images allow,
 *                                   at most 4 / 8)
 *   TWR_FUSED_MAX_ROM               rom slices up to which one fused launch replaces the three kernels (default: 20 rounds
 *                                   of the rom residency = 20 x TWR_ROM_BPC x number of CUs)
 *   TWR_FUSED_SPLIT                 eighths of the residency the fused launch gives the rom role when both roles do not fit
 *                                   (default: 5 up to 34/8 rounds of rom slices, 4 above; 8 = one role after the other)
 *   TWR_FUSED_GROM, TWR_FUSED_GDYN  explicit block counts of the two roles of the fused launch (experiments)
 *   TWR_STREAM_NT=0|1               overrides the store policy twr_batch_create picks (twr_batch_streaming_stores)
 *   TWR_HOST_ZERO_COPY[_X]=0        twr_batch_eval_host: copy through device buffers instead of letting the kernels store
 *                                   into (gather x from) the page-locked host buffers */

#ifdef __cplusplus
}
#endif
#endif /* TOWR_AMD_H_ */
