// TEST INFRASTRUCTURE ONLY -- CPU oracle for the towr NLP constraint/Jacobian path.
//
// A plain C++ restatement (no Eigen, no ifopt) of the reference algorithm in
// /root/reference/towr (KaiNakamura/towr @ 2025-05-23).  Only tests/,
// __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it; the product
// library (towr_amd/csrc) never includes, links or calls anything in oracle/.
//
// PARITY UNPINNED by the reference's own tests: the reference ships no golden
// vectors (towr/test/dynamic_model_test.cc:36-49 and dynamic_constraint_test.cc:40-43
// are empty stubs) and cannot be compiled here (needs Eigen3 + ifopt, both absent,
// no network).  What pins this oracle instead (tests/test_oracle_*.py):
//   * central finite differences of oracle g(x) vs oracle Jacobian,
//   * an independent mpmath implementation of g(x) with 40-digit numerical
//     differentiation (oracle/mp_ref.py -> tests/golden/mp_*.npz), for every constraint
//     set incl. optimised phase durations,
//   * hand known-answers derived from the cited reference lines.
//
// C interface (flat arrays, used from Python via ctypes).
#pragma once
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct orc_problem orc_problem;

// robot: 0 Monoped, 1 Biped, 2 Hyq, 3 Anymal, 4 Go1   (towr/src/robot_model.cc:41-68)
// terrain: 0 Flat,1 Block,2 Stairs,3 Gap,4 Slope,5 Chimney,6 ChimneyLR (height_map.h:79-86),
//          7 HeightMapFromCSV with the grid passed to orc_create (terrain/height_map_from_csv.h)
//          8 Grid (terrain/grid_height_map.h), see orc_set_grid_map
// phase_durations: concatenated per-ee phase durations, n_phases[ee] entries each.
orc_problem* orc_create(int robot, int terrain, int n_ee, const int* n_phases,
                        const double* phase_durations, const int* in_contact_at_start,
                        double dt_dynamic, double dt_rom, double duration_base_poly,
                        int polys_per_swing, int polys_per_stance_force,
                        double force_limit, int constraint_sets,
                        double dt_base_motion /* parameters.cc:51 */, double base_z_init /* base_motion_constraint.cc:51 */,
                        const double* grid /* terrain 7 (HeightMapFromCSV): rows x cols heights, grid[y_cell][x_cell] */,
                        int grid_rows, int grid_cols);
// terrain 8 = the fork's `Grid` height map (include/towr/terrain/grid_height_map.h:15-60): create the problem with
// terrain 8, then hand over the "elevation" layer of the grid_map before the first evaluation / initial guess:
// elevation[i + j * size_x] (column-major float matrix, as grid_map stores it; start index (0,0)), cell size
// `resolution`, map centre (pos_x, pos_y).  Returns 0, or -1 on bad arguments.
int orc_set_grid_map(orc_problem*, const float* elevation, int size_x, int size_y, double resolution, double pos_x,
                     double pos_y);
// height and the two slopes of the problem's terrain at (x, y)
void orc_terrain_probe(const orc_problem*, double x, double y, double out[3]);
void orc_terrain_probe_full(const orc_problem*, double x, double y, double out[31]);
// constraint_sets: which of the default sets (parameters.cc:55-60) to build, in that order
enum {
  ORC_SET_TERRAIN = 1, ORC_SET_DYNAMIC = 2, ORC_SET_BASE_ACC = 4, ORC_SET_ROM = 8, ORC_SET_FORCE = 16,
  ORC_SET_SWING = 32,
  ORC_SET_BASE_ROM = 128,   // BaseMotionConstraint "baseMotion" (not in the default list), placed before TotalTime
  ORC_SET_TOTAL_TIME = 64,  // Parameters::OptimizePhaseDurations (parameters.cc:76-80): timings become variables
  ORC_SETS_HOT_PATH = 1 | 2 | 8 | 16,
  ORC_SETS_TOWR_DEFAULT = 63
};
void orc_destroy(orc_problem*);

int orc_n_vars(const orc_problem*);
int orc_n_rows(const orc_problem*);
int orc_n_var_sets(const orc_problem*);
int orc_n_con_sets(const orc_problem*);
const char* orc_var_set_name(const orc_problem*, int i);
int orc_var_set_size(const orc_problem*, int i);
const char* orc_con_set_name(const orc_problem*, int i);
int orc_con_set_rows(const orc_problem*, int i);

// reference initial guess (nlp_formulation.cc:95-181); state arrays are 3 doubles.
void orc_initial_guess(orc_problem*, const double* base_lin0, const double* base_ang0,
                       const double* base_lin1, const double* base_ang1,
                       const double* ee_pos0 /* n_ee*3 */, double* x_out);

// variable bounds (x_l, x_u) of the same construction; init_base / final_base = {lin p, lin v, ang p, ang v}
void orc_variable_bounds(orc_problem*, const double* init_base /*12*/, const double* final_base /*12*/,
                         const double* ee_pos0 /* n_ee*3 */, double* lower, double* upper);

// one full callback: SetVariables(x); g = stacked GetValues(); J = stacked GetJacobian().
// Jacobian returned as CSR over the stacked rows (columns ascending in each row, explicit
// zeros kept) exactly as ifopt::Problem::EvalNonzerosOfJacobian would copy it out.
// Returns nnz.  Pass NULL outputs to query sizes only.
int orc_eval(orc_problem*, const double* x, double* g, int* row_ptr, int* col_idx, double* vals);
void orc_bounds(orc_problem*, double* lower, double* upper);

// fpowr::GetTrajectory (footstep_plan_extractor.h:19-53): samples of the solution x every dt; returns the
// number of samples (pass out = NULL to query it); record layout in towr_oracle.cc.
int orc_sample_trajectory(orc_problem*, const double* x, double dt, double* out, int max_samples);

// fpowr::PlanarRegionsToPolygons / NearestPlaneLookup::GetNearestPlaneIndex (nearest_plane_lookup.h:20-85); tf and
// boost::geometry restated from their published algorithms (notes in towr_oracle.cc)
void orc_planes_world_xy(const double* regions, const double* local_xy, const int* start, int n, double* out_xy);
int orc_nearest_plane(const double* world_xy, const int* start, int n_polys, double px, double py);
// per ring and point: covered_by (1 inside, 0 boundary, -1 outside) and the distance to the ring itself (n_points points x, y)
void orc_ring_side(const double* xy, int n, const double* points, int n_points, int* side);
void orc_ring_distance(const double* xy, int n, const double* points, int n_points, double* distance);

// fpowr::ExtractInitialGuess (initial_guess_extractor.h:17-34) at the given times: 49 doubles per time
// [t | state 12 | controls 36], layout in towr_oracle.cc
void orc_initial_guess_samples(orc_problem*, const double* x, const double* times, int n_times, double* out);

// fpowr::ExtractFootstepPlan (footstep_plan_extractor.h:69-133) up to the nearest-plane lookup (orc_nearest_plane): footstep states
// [t | duration | contact per ee | ee position per ee]; returns their number (out = NULL to query it).
int orc_contact_plan(orc_problem*, const double* x, double dt, double time_horizon, double* out, int max_steps);

// reference-shaped timing loop for bench.py's cpu_baseline: `iters` full callbacks on
// x (values + Jacobian), returns seconds.
double orc_time_callbacks(orc_problem*, const double* x, int iters);

// gait generator restatement (gait_generator.cc:54-105, *_gait_generator.cc).
// Fills per-ee phase durations for combo `combo` scaled to t_total; returns the
// number of doubles written to out (concatenated), n_phases[ee] and contact[ee].
int orc_gait(int n_ee, int combo, double t_total, int* n_phases, int* contact_at_start,
             double* out, int out_cap);

// probes of the closed forms the reference took from towr/matlab/*.m (tests/test_oracle_symbolic.py)
double orc_hermite_dpos_dT(double t, double T, double p0, double v0, double p1, double v1);
void orc_euler_probe(const double nodes[12], double T, double t, double* out /* 429 doubles, layout in towr_oracle.cc */);

// small probes used by known-answer tests
void orc_hermite_weights(double t, double T, double w[12]);   // d{p,v,a}/d{p0,v0,p1,v1}
// NodeSpline::GetLocalTime on n durations at each of n_t times: id[k], t_local[k]; returns the number of times for which no
// segment is found (id -1, t_local NaN)
int orc_locate(const double* durations, int n, const double* t, int n_t, int* id, double* t_local);
// PhaseDurations::SetVariables on n - 1 variables of n given durations, then NodesVars::PhaseToPolyDurations of the ee-motion and the
// ee-force nodes: ph[n], md / fd (room for n * max(pps, ppf) each); returns n_md | n_fd << 16
int orc_phase_poly_durations(int n, int contact_at_start, int pps, int ppf, const double* given, const double* vars, double* ph,
                             double* md, double* fd);
double orc_terrain_height(int terrain, double x, double y);
void orc_terrain_basis(int terrain, int which, double x, double y, double out[3]);
void orc_terrain_dbasis(int terrain, int which, int dim, double x, double y, double out[3]);

#ifdef __cplusplus
}
#endif
