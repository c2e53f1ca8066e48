// Host-side structure builder.  Closed-form restatement of the reference's setup-time
// logic; nothing here touches x.  Citations are file:line under /root/reference/towr/.
#include "structure.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <exception>
#include <limits>
#include <map>
#include <numeric>
#include <stdexcept>
#include <thread>
#include <tuple>
#include <unordered_map>

namespace twr {

namespace {

// Spline::GetSegmentID + GetLocalTime (src/spline.cc:48-78): eps 1e-10, the previous segment wins
// at junctions, local time by sequential subtraction.  Must be reproduced bit for bit because the
// active polynomial decides which Jacobian columns exist.
TimeNode Locate(double t_global, const std::vector<double>& durations) {
  const double eps = 1e-10;
  double t = 0;
  int id = -1;
  for (size_t i = 0; i < durations.size(); ++i) {
    t += durations[i];
    if (t >= t_global - eps) {
      id = (int)i;
      break;
    }
  }
  if (id < 0) throw std::runtime_error("time grid exceeds spline duration");
  double t_local = t_global;
  for (int i = 0; i < id; ++i) t_local -= durations[i];
  return {id, t_local};
}

// TimeDiscretizationConstraint ctor (src/time_discretization_constraint.cc:37-50)
std::vector<double> TimeGrid(double T, double dt) {
  if (!(dt > 0)) throw std::runtime_error("dt must be positive");
  double t = 0.0;
  std::vector<double> g = {t};
  for (int i = 0; i < std::floor(T / dt); ++i) {
    t += dt;
    g.push_back(t);
  }
  g.push_back(T);
  return g;
}

struct PolyPhase {
  int phase;
  bool constant;
  int n_in_phase;
};

// BuildPolyInfos (src/nodes_variables_phase_based.cc:38-58)
std::vector<PolyPhase> PhasePolys(int n_phases, bool first_constant, int n_changing) {
  std::vector<PolyPhase> v;
  bool c = first_constant;
  for (int ph = 0; ph < n_phases; ++ph) {
    if (c)
      v.push_back({ph, true, 1});
    else
      for (int j = 0; j < n_changing; ++j) v.push_back({ph, false, n_changing});
    c = !c;
  }
  return v;
}

// NodesVariablesEEMotion / NodesVariablesEEForce::GetPhaseBasedEEParameterization
// (src/nodes_variables_phase_based.cc:210-298) as a direct index assignment.
SplineLayout PhaseBasedLayout(const double* phase_durations, int n_phases, bool first_constant, int n_changing,
                              bool is_motion, int var_offset) {
  SplineLayout s;
  auto polys = PhasePolys(n_phases, first_constant, n_changing);
  for (auto& p : polys) {
    s.durations.push_back(phase_durations[p.phase] / p.n_in_phase);  // ConvertPhaseToPolyDurations :73-84
    s.poly_phase.push_back(p.phase);
  }
  s.n_nodes = (int)polys.size() + 1;
  s.idx.assign(s.n_nodes * 6, -1);
  s.node_constant.assign(s.n_nodes, 0);
  for (int n = 0; n < s.n_nodes; ++n) {  // IsConstantNode :99-111
    bool c = false;
    if (n > 0 && polys[n - 1].constant) c = true;
    if (n < s.n_nodes - 1 && polys[n].constant) c = true;
    s.node_constant[n] = c;
  }
  int idx = var_offset;
  auto set = [&](int node, int deriv, int dim, int v) { s.idx[(node * 2 + deriv) * 3 + dim] = v; };
  for (int n = 0; n < s.n_nodes; ++n) {
    if (!s.node_constant[n]) {
      for (int d = 0; d < 3; ++d) {
        set(n, 0, d, idx++);
        if (is_motion) {
          if (d != 2) set(n, 1, d, idx++);  // swing: z velocity fixed to zero
        } else {
          set(n, 1, d, idx++);
        }
      }
    } else {
      if (n + 1 >= s.n_nodes) throw std::runtime_error("dangling constant node");
      if (is_motion)
        for (int d = 0; d < 3; ++d) {  // one position shared by both nodes of the stance polynomial
          set(n, 0, d, idx);
          set(n + 1, 0, d, idx);
          idx++;
        }
      n += 1;
    }
  }
  s.var_offset = var_offset;
  s.var_size = idx - var_offset;
  return s;
}

// the dimension of every variable of a phase-based set, by index relative to the set's first (-1: none)
std::vector<int> DimOf(const SplineLayout& s) {
  std::vector<int> dim_of(s.var_size, -1);
  for (int n = 0; n < s.n_nodes; ++n)
    for (int dv = 0; dv < 2; ++dv)
      for (int d = 0; d < 3; ++d)
        if (s.at(n, dv, d) >= 0) dim_of[s.at(n, dv, d) - s.var_offset] = d;
  return dim_of;
}

PolyDesc MakeEePoly(const SplineLayout& s, int q) {
  PolyDesc p;
  std::memset(&p, 0, sizeof(p));
  p.iT = 1.0 / s.durations[q];
  int gi[12];
  bool shared = true;
  for (int d = 0; d < 3; ++d)
    if (s.at(q, 0, d) < 0 || s.at(q, 0, d) != s.at(q + 1, 0, d)) shared = false;
  std::vector<int> uniq;
  for (int j = 0; j < 4; ++j)
    for (int d = 0; d < 3; ++d) {
      int node = q + (j >= 2 ? 1 : 0), deriv = j & 1;
      int v = s.at(node, deriv, d);
      if (shared && j == 2) v = -1;  // folded into p0
      gi[j * 3 + d] = v;
      if (v >= 0) uniq.push_back(v);
    }
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  if (uniq.size() > 12) throw std::runtime_error("too many slots");
  const int nslots = (int)uniq.size();
  p.xbase = uniq.empty() ? 0 : uniq.front();
  for (size_t i = 0; i < uniq.size(); ++i)
    if (uniq[i] != p.xbase + (int)i) throw std::runtime_error("polynomial variables not contiguous");
  int dim_of_slot[12], cnt[3] = {0, 0, 0};
  for (int c = 0; c < 12; ++c)
    if (gi[c] >= 0) dim_of_slot[gi[c] - p.xbase] = c % 3;
  for (int sl = 0; sl < nslots; ++sl) cnt[dim_of_slot[sl]]++;
  for (int c = 0; c < 12; ++c) {
    if (gi[c] < 0) {
      p.cand[c] = 0xFFFF;
      continue;
    }
    int sl = gi[c] - p.xbase, d = c % 3;
    int ra = 0, rb = 0, rl = 0;
    for (int s2 = 0; s2 < sl; ++s2) {
      if (dim_of_slot[s2] != (d + 1) % 3) ra++;
      if (dim_of_slot[s2] != (d + 2) % 3) rb++;
      if (dim_of_slot[s2] == d) rl++;
    }
    p.cand[c] = (uint16_t)(sl | (ra << 4) | (rb << 8) | (rl << 12));
  }
  p.meta = (uint32_t)(nslots | (cnt[0] << 4) | (cnt[1] << 8) | (cnt[2] << 12) | ((shared ? 1 : 0) << 16));
  return p;
}

}  // namespace

// ------------------------------------------------------------------ variables
void Structure::BuildVariables() {
  n_ee = schedule.n_ee;
  if (n_ee < 1 || n_ee > kMaxEE || n_ee != model.n_ee) throw std::runtime_error("n_ee mismatch");
  for (int e = 0; e < n_ee; ++e)
    if (schedule.n_phases[e] < 1 || schedule.n_phases[e] > TWR_MAX_PHASES) throw std::runtime_error("bad phase count");
  // Parameters::GetTotalTime (src/parameters.cc:112-126): first foot is the reference
  T = std::accumulate(schedule.phase_durations[0], schedule.phase_durations[0] + schedule.n_phases[0], 0.0);
  for (int e = 0; e < n_ee; ++e) {
    double Te = std::accumulate(schedule.phase_durations[e], schedule.phase_durations[e] + schedule.n_phases[e], 0.0);
    if (std::fabs(Te - T) >= 1e-6) throw std::runtime_error("phase durations of the feet do not sum to the same T");
  }
  // Parameters::GetBasePolyDurations (src/parameters.cc:82-98)
  {
    double dt = params.duration_base_poly, t_left = T;
    if (!(dt > 0)) throw std::runtime_error("duration_base_poly must be positive");
    while (t_left > 1e-10) {
      base.durations.push_back(t_left > dt ? dt : t_left);
      t_left -= dt;
    }
  }
  // NodesVariablesAll (src/nodes_variables_all.cc:34-61): node-major, px py pz vx vy vz
  base.n_nodes = (int)base.durations.size() + 1;
  base.idx.resize(base.n_nodes * 6);
  for (int n = 0; n < base.n_nodes; ++n)
    for (int dv = 0; dv < 2; ++dv)
      for (int d = 0; d < 3; ++d) base.idx[(n * 2 + dv) * 3 + d] = 6 * n + 3 * dv + d;
  base.var_size = base.n_nodes * 6;
  // variable set order: NlpFormulation::GetVariableSets (src/nlp_formulation.cc:63-93)
  int off = 0;
  off_base_lin = off;
  var_sets.push_back({"base-lin", off, base.var_size, 0, 0});
  off += base.var_size;
  off_base_ang = off;
  var_sets.push_back({"base-ang", off, base.var_size, 0, 0});
  off += base.var_size;
  for (int e = 0; e < n_ee; ++e) {  // MakeEndeffectorVariables :127-156 (stance phases constant)
    motion.push_back(PhaseBasedLayout(schedule.phase_durations[e], schedule.n_phases[e],
                                      schedule.in_contact_at_start[e] != 0, params.polys_per_swing, true, off));
    var_sets.push_back({"ee-motion_" + std::to_string(e), off, motion.back().var_size, 0, 0});
    off += motion.back().var_size;
  }
  for (int e = 0; e < n_ee; ++e) {  // MakeForceVariables :158-181 (swing phases constant)
    force.push_back(PhaseBasedLayout(schedule.phase_durations[e], schedule.n_phases[e],
                                     schedule.in_contact_at_start[e] == 0, params.polys_per_stance_force, false, off));
    var_sets.push_back({"ee-force_" + std::to_string(e), off, force.back().var_size, 0, 0});
    off += force.back().var_size;
  }
  // MakeContactScheduleVariables (src/nlp_formulation.cc:183-198), part of x only when the timings are
  // optimised (:78-82); PhaseDurations holds n_phases-1 variables (src/phase_durations.cc:45)
  timings = (params.constraint_sets & TWR_SET_TOTAL_TIME) != 0;
  if (timings)
    for (int e = 0; e < n_ee; ++e) {
      if (schedule.n_phases[e] < 2) throw std::runtime_error("optimised timings need at least two phases per foot");
      off_schedule[e] = off;
      var_sets.push_back({"ee-schedule" + std::to_string(e), off, schedule.n_phases[e] - 1, 0, 0});
      off += schedule.n_phases[e] - 1;
    }
  n_vars = off;
  mpoly.resize(n_ee);
  fpoly.resize(n_ee);
  for (int e = 0; e < n_ee; ++e) {
    for (size_t q = 0; q < motion[e].durations.size(); ++q) mpoly[e].push_back(MakeEePoly(motion[e], (int)q));
    for (size_t q = 0; q < force[e].durations.size(); ++q) fpoly[e].push_back(MakeEePoly(force[e], (int)q));
  }
}

// ------------------------------------------------------------------ time tables
void Structure::BuildTimeTables() {
  grid_dyn = TimeGrid(T, params.dt_dynamic);  // DynamicConstraint ctor, dynamic_constraint.cc:37-51
  grid_rom = TimeGrid(T, params.dt_rom);      // RangeOfMotionConstraint ctor, range_of_motion_constraint.cc:35-50
  dyn_motion.resize(n_ee);
  dyn_force.resize(n_ee);
  rom_motion.resize(n_ee);
  for (double t : grid_dyn) {
    dyn_base.push_back(Locate(t, base.durations));
    for (int e = 0; e < n_ee; ++e) {
      dyn_motion[e].push_back(Locate(t, motion[e].durations));
      dyn_force[e].push_back(Locate(t, force[e].durations));
    }
  }
  for (double t : grid_rom) {
    rom_base.push_back(Locate(t, base.durations));
    for (int e = 0; e < n_ee; ++e) rom_motion[e].push_back(Locate(t, motion[e].durations));
  }
  if (params.constraint_sets & TWR_SET_BASE_ROM) {  // BaseMotionConstraint ctor, base_motion_constraint.cc:38-41
    grid_bm = TimeGrid(T, params.dt_base_motion);
    for (double t : grid_bm) bm_base.push_back(Locate(t, base.durations));
  }
  // force / terrain node tables
  force_nodes.resize(n_ee);
  terrain_rows.resize(n_ee);
  for (int e = 0; e < n_ee; ++e) {
    const SplineLayout& f = force[e];
    const SplineLayout& m = motion[e];
    for (int n = 0; n < f.n_nodes; ++n) {
      if (f.node_constant[n]) continue;  // GetIndicesOfNonConstantNodes, nodes_variables_phase_based.cc:119-129
      int adj_poly = n == 0 ? 0 : n - 1;  // GetPhase -> GetAdjacentPolyIds(node).front(), :131-138,163-179
      int phase = f.poly_phase[adj_poly];
      int start = -1;                     // GetNodeIDAtStartOfPhase, :140-161
      for (size_t q = 0; q < m.poly_phase.size(); ++q)
        if (m.poly_phase[q] == phase) {
          start = (int)q;
          break;
        }
      if (start < 0) throw std::runtime_error("stance phase missing in ee-motion");
      ForceNode fn;
      fn.fidx = f.at(n, 0, 0);
      fn.hidx = m.at(start, 0, 0);
      if (f.at(n, 0, 1) != fn.fidx + 2 || f.at(n, 0, 2) != fn.fidx + 4 || m.at(start, 0, 1) != fn.hidx + 1)
        throw std::runtime_error("unexpected force node layout");
      force_nodes[e].push_back(fn);
    }
    for (int n = 1; n < m.n_nodes; ++n) {  // terrain_constraint.cc:49-51
      TerrainRow tr;
      tr.idx = m.at(n, 0, 0);
      tr.stride = m.at(n, 0, 1) - tr.idx;
      if (m.at(n, 0, 2) != tr.idx + 2 * tr.stride) throw std::runtime_error("unexpected motion node layout");
      terrain_rows[e].push_back(tr);
    }
  }
  // splineacc-base-*: the two NodeSpline::GetJacobianWrtNodes rows of spline_acc_constraint.cc:67-81 at
  // t = T_j of polynomial j and t = 0 of polynomial j+1 (CubicHermitePolynomial::GetDerivativeWrt{Start,End}Node,
  // polynomial.cc:140-234, kAcc); they depend on the durations only.
  if (params.constraint_sets & TWR_SET_BASE_ACC)
    for (size_t j = 0; j + 1 < base.durations.size(); ++j) {
      const double Tp = base.durations[j], Tn = base.durations[j + 1];
      const double Tp2 = std::pow(Tp, 2), Tp3 = std::pow(Tp, 3), Tn2 = std::pow(Tn, 2), Tn3 = std::pow(Tn, 3);
      const double prev[4] = {(12 * Tp) / Tp3 - 6 / Tp2, (6 * Tp) / Tp2 - 4 / Tp, 6 / Tp2 - (12 * Tp) / Tp3, (6 * Tp) / Tp2 - 2 / Tp};
      const double next[4] = {(12 * 0.0) / Tn3 - 6 / Tn2, (6 * 0.0) / Tn2 - 4 / Tn, 6 / Tn2 - (12 * 0.0) / Tn3, (6 * 0.0) / Tn2 - 2 / Tn};
      AccJunction a;
      a.c[0] = prev[0]; a.c[1] = prev[1];
      a.c[2] = prev[2] - next[0]; a.c[3] = prev[3] - next[1];
      a.c[4] = 0.0 - next[2]; a.c[5] = 0.0 - next[3];
      acc_junctions.push_back(a);
    }
  // swing-ee-motion_e: GetIndicesOfNonConstantNodes + the neighbours' position variables
  swing_nodes.resize(n_ee);
  if (params.constraint_sets & TWR_SET_SWING)
    for (int e = 0; e < n_ee; ++e) {
      const SplineLayout& m = motion[e];
      for (int n = 0; n < m.n_nodes; ++n) {
        if (m.node_constant[n]) continue;
        // "assumes ... starting and ending in stance" (swing_constraint.cc:66): the reference indexes
        // nodes.at(node_id -+ 1) and throws otherwise
        if (n == 0 || n == m.n_nodes - 1) throw std::runtime_error("swing constraint needs schedules that start and end in stance");
        SwingNode sn;
        sn.cur = m.at(n, 0, 0);
        if (m.at(n, 1, 0) != sn.cur + 1 || m.at(n, 0, 1) != sn.cur + 2 || m.at(n, 1, 1) != sn.cur + 3)
          throw std::runtime_error("unexpected swing node layout");
        sn.prev_x = m.at(n - 1, 0, 0); sn.prev_y = m.at(n - 1, 0, 1);
        sn.next_x = m.at(n + 1, 0, 0); sn.next_y = m.at(n + 1, 0, 1);
        sn.pad = 0;
        if (sn.prev_x < 0 || sn.prev_y < 0 || sn.next_x < 0 || sn.next_y < 0) throw std::runtime_error("swing neighbour is not a variable");
        swing_nodes[e].push_back(sn);
      }
    }
}

// ------------------------------------------------------------------ CSR pattern + bounds
void Structure::BuildPattern() {
  const double inf = 1e20;
  // rows are emitted straight into col_idx / row_ptr (no per-row containers: this runs once per candidate of a
  // sweep)
  row_ptr.assign(1, 0);
  col_idx.clear();
  col_idx.reserve(1 << 17);
  std::vector<int32_t>& c = col_idx;
  auto end_row = [&]() {
    if (!std::is_sorted(col_idx.begin() + row_ptr.back(), col_idx.end())) throw std::runtime_error("row not sorted");
    row_ptr.push_back((int32_t)col_idx.size());
  };
  auto emit = [&](std::initializer_list<int> cols) {
    col_idx.insert(col_idx.end(), cols.begin(), cols.end());
    end_row();
  };
  auto begin_set = [&](const std::string& name, int n) {
    SetInfo s;
    s.name = name;
    s.offset = (int)row_ptr.size() - 1;
    s.size = n;
    con_sets.push_back(s);
  };
  auto slots_cols = [&](const PolyDesc& p, int want_dim, bool equal, std::vector<int32_t>& out) {
    // columns of the slots whose dim ==/!= want_dim, ascending
    int dim_of_slot[12];
    for (int c = 0; c < 12; ++c)
      if (p.cand[c] != 0xFFFF) dim_of_slot[p.cand[c] & 0xF] = c % 3;
    const int nslots = p.meta & 0xF;
    for (int s = 0; s < nslots; ++s)
      if ((dim_of_slot[s] == want_dim) == equal) out.push_back(p.xbase + s);
  };
  auto set_cols = [&](const SplineLayout& s, int want_dim, bool equal, std::vector<int32_t>& out) {
    // all variables of a phase-based set whose dim ==/!= want_dim, ascending
    const std::vector<int> dim_of = DimOf(s);
    for (int i = 0; i < s.var_size; ++i)
      if ((dim_of[i] == want_dim) == equal) out.push_back(s.var_offset + i);
  };
  auto sched_cols = [&](int e, std::vector<int32_t>& out) {
    for (int i = 0; i < schedule.n_phases[e] - 1; ++i) out.push_back(off_schedule[e] + i);
  };
  const int sets = params.constraint_sets;
  // --- terrain-ee-motion_e  (terrain_constraint.cc:90-108): [x, y, z] of node id = row+1
  for (int e = 0; e < n_ee && (sets & TWR_SET_TERRAIN); ++e) {
    begin_set("terrain-ee-motion_" + std::to_string(e), (int)terrain_rows[e].size());
    for (size_t r = 0; r < terrain_rows[e].size(); ++r) {
      const TerrainRow& tr = terrain_rows[e][r];
      emit({tr.idx, tr.idx + tr.stride, tr.idx + 2 * tr.stride});
      bool constant = motion[e].node_constant[r + 1];
      lower.push_back(0.0);
      upper.push_back(constant ? 0.0 : inf);  // terrain_constraint.cc:72-88
    }
  }
  // --- dynamic (dynamic_constraint.cc:73-117, single_rigid_body_dynamics.cc:103-192)
  if (sets & TWR_SET_DYNAMIC) begin_set("dynamic", (int)grid_dyn.size() * 6);
  for (size_t k = 0; k < grid_dyn.size() && (sets & TWR_SET_DYNAMIC); ++k) {
    int q = dyn_base[k].poly;
    for (int r = 0; r < 3; ++r) {  // AX, AY, AZ
      for (int node = q; node <= q + 1; ++node)  // -sum [f]x J_pos: dims != r, pos then vel per node
        for (int dv = 0; dv < 2; ++dv)
          for (int d = 0; d < 3; ++d)
            if (d != r) c.push_back(off_base_lin + 6 * node + 3 * dv + d);
      for (int i = 0; i < 12; ++i) c.push_back(off_base_ang + 6 * q + i);  // structurally full
      if (!timings) {
        for (int e = 0; e < n_ee; ++e) slots_cols(mpoly[e][dyn_motion[e][k].poly], r, false, c);  // [f]x J_p
        for (int e = 0; e < n_ee; ++e) slots_cols(fpoly[e][dyn_force[e][k].poly], r, false, c);   // [r]x J_f
      } else {  // PhaseSpline: every variable of the set (phase_spline.cc:44-51), then the duration columns
        for (int e = 0; e < n_ee; ++e) set_cols(motion[e], r, false, c);
        for (int e = 0; e < n_ee; ++e) set_cols(force[e], r, false, c);
        for (int e = 0; e < n_ee; ++e) sched_cols(e, c);  // dynamic_constraint.cc:107-113
      }
      end_row();
      lower.push_back(0.0);
      upper.push_back(0.0);
    }
    for (int d = 0; d < 3; ++d) {  // LX, LY, LZ
      for (int j = 0; j < 4; ++j) c.push_back(off_base_lin + 6 * q + 3 * j + d);  // m J_acc
      if (!timings) {
        for (int e = 0; e < n_ee; ++e) slots_cols(fpoly[e][dyn_force[e][k].poly], d, true, c);  // -J_f
      } else {
        for (int e = 0; e < n_ee; ++e) set_cols(force[e], d, true, c);
        for (int e = 0; e < n_ee; ++e) sched_cols(e, c);
      }
      end_row();
      lower.push_back(0.0);
      upper.push_back(0.0);
    }
  }
  // --- splineacc-base-lin, splineacc-base-ang (spline_acc_constraint.cc:67-88): the sparse difference
  // acc_prev - acc_next keeps the union pattern: both value kinds of nodes j, j+1, j+2 in dimension d
  // (the shared node's position entry is a structural non-zero even when the durations are equal and
  // its value cancels)
  if (sets & TWR_SET_BASE_ACC)
    for (int which = 0; which < 2; ++which) {
      const int off = which == 0 ? off_base_lin : off_base_ang;
      begin_set(which == 0 ? "splineacc-base-lin" : "splineacc-base-ang", 3 * (int)acc_junctions.size());
      for (size_t j = 0; j < acc_junctions.size(); ++j)
        for (int d = 0; d < 3; ++d) {
          for (int i = 0; i < 6; ++i) c.push_back(off + 6 * (int)j + 3 * i + d);
          end_row();
          lower.push_back(0.0);
          upper.push_back(0.0);
        }
    }
  // --- rangeofmotion-e (range_of_motion_constraint.cc:83-109)
  for (int e = 0; e < n_ee && (sets & TWR_SET_ROM); ++e) {
    begin_set("rangeofmotion-" + std::to_string(e), (int)grid_rom.size() * 3);
    for (size_t k = 0; k < grid_rom.size(); ++k) {
      int q = rom_base[k].poly;
      const PolyDesc& mp = mpoly[e][rom_motion[e][k].poly];
      for (int r = 0; r < 3; ++r) {
        for (int i = 0; i < 12; ++i) c.push_back(off_base_lin + 6 * q + i);  // -R^T J_c
        for (int i = 0; i < 12; ++i)  // DerivOfRotVecMult(inverse): row 0 does not depend on roll
          if (!(r == 0 && i % 3 == 0)) c.push_back(off_base_ang + 6 * q + i);
        if (!timings) {
          for (int s = 0; s < (int)(mp.meta & 0xF); ++s) c.push_back(mp.xbase + s);  // R^T J_p
        } else {  // b_R_w (dense) times the all-variables PhaseSpline rows, then the duration columns (:106-108)
          for (int i = 0; i < motion[e].var_size; ++i) c.push_back(motion[e].var_offset + i);
          sched_cols(e, c);
        }
        end_row();
        lower.push_back(model.nominal_stance[e][r] - model.max_dev[r]);  // :71-81
        upper.push_back(model.nominal_stance[e][r] + model.max_dev[r]);
      }
    }
  }
  // --- force-ee-force_e (force_constraint.cc:107-171)
  for (int e = 0; e < n_ee && (sets & TWR_SET_FORCE); ++e) {
    begin_set("force-ee-force_" + std::to_string(e), (int)force_nodes[e].size() * 5);
    for (const ForceNode& fn : force_nodes[e]) {
      for (int r = 0; r < 5; ++r) emit({fn.hidx, fn.hidx + 1, fn.fidx, fn.fidx + 2, fn.fidx + 4});
      lower.push_back(0.0);  upper.push_back(model.force_limit);  // :91-105
      lower.push_back(-inf); upper.push_back(0.0);
      lower.push_back(0.0);  upper.push_back(inf);
      lower.push_back(-inf); upper.push_back(0.0);
      lower.push_back(0.0);  upper.push_back(inf);
    }
  }
  // --- swing-ee-motion_e (swing_constraint.cc:86-121): rows x-pos, x-vel, y-pos, y-vel per swing node
  for (int e = 0; e < n_ee && (sets & TWR_SET_SWING); ++e) {
    begin_set("swing-ee-motion_" + std::to_string(e), 4 * (int)swing_nodes[e].size());
    for (const SwingNode& sn : swing_nodes[e]) {
      emit({sn.prev_x, sn.cur, sn.next_x});
      emit({sn.prev_x, sn.cur + 1, sn.next_x});
      emit({sn.prev_y, sn.cur + 2, sn.next_y});
      emit({sn.prev_y, sn.cur + 3, sn.next_y});
      for (int r = 0; r < 4; ++r) {
        lower.push_back(0.0);
        upper.push_back(0.0);
      }
    }
  }
  // --- baseMotion (base_motion_constraint.cc:60-90): rows AX..AZ = base-ang position, LX..LZ = base-lin position
  if (sets & TWR_SET_BASE_ROM) {
    begin_set("baseMotion", 6 * (int)grid_bm.size());
    const double dev_rad = 0.05, z0 = params.base_z_init;
    for (size_t k = 0; k < grid_bm.size(); ++k) {
      const int q = bm_base[k].poly;
      for (int r6 = 0; r6 < 6; ++r6) {
        const int off = r6 < 3 ? off_base_ang : off_base_lin, d = r6 % 3;
        emit({off + 6 * q + d, off + 6 * q + 3 + d, off + 6 * q + 6 + d, off + 6 * q + 9 + d});
      }
      lower.push_back(-dev_rad); upper.push_back(dev_rad);   // AX
      lower.push_back(-dev_rad); upper.push_back(dev_rad);   // AY
      lower.push_back(-inf);     upper.push_back(inf);       // AZ
      lower.push_back(-inf);     upper.push_back(inf);       // LX
      lower.push_back(-inf);     upper.push_back(inf);       // LY
      lower.push_back(z0 - 0.02); upper.push_back(z0 + 0.1); // LZ
    }
  }
  // --- totalduration-e (total_duration_constraint.cc:50-72): sum of the optimised durations
  for (int e = 0; e < n_ee && (sets & TWR_SET_TOTAL_TIME); ++e) {
    begin_set("totalduration-" + std::to_string(e), 1);
    sched_cols(e, c);
    end_row();
    lower.push_back(0.1);
    upper.push_back(T - 0.2);  // min_duration_last_phase
  }
  n_rows = (int)row_ptr.size() - 1;
  nnz = row_ptr[n_rows];
  for (auto& s : con_sets) {
    s.nnz_offset = row_ptr[s.offset];
    s.nnz = row_ptr[s.offset + s.size] - s.nnz_offset;
  }
}

// ------------------------------------------------------------------ device blob
namespace {

// The blob's alignment rules (device_tables.h): the DevStruct header, then the tables on 16-byte boundaries and the layout
// tables of dyn_kernel on 64-byte lines (a blob starts on a 256-byte line); the whole is a multiple of 16 bytes.
class BlobWriter {
 public:
  // the layout tables are recorded in `layout`: a batch stores byte-identical ones once
  explicit BlobWriter(std::vector<Structure::TableRef>& layout) : blob_(sizeof(DevStruct)), layout_(layout) { layout_.clear(); }
  uint32_t Put(const void* src, size_t bytes, size_t align = 16) {
    const size_t off = (blob_.size() + align - 1) / align * align;
    blob_.resize(off + bytes);
    if (bytes) std::memcpy(blob_.data() + off, src, bytes);
    return (uint32_t)off;
  }
  template <class T>
  uint32_t Put(const std::vector<T>& v, size_t align = 16) { return Put(v.data(), v.size() * sizeof(T), align); }
  template <class T>
  uint32_t PutLayout(const std::vector<T>& v) {
    layout_.push_back({Put(v, 64), (uint32_t)(v.size() * sizeof(T))});
    return layout_.back().off;
  }
  std::vector<char> Finish(const DevStruct& h) {
    std::memcpy(blob_.data(), &h, sizeof(h));
    blob_.resize((blob_.size() + 15) / 16 * 16);
    return std::move(blob_);
  }

 private:
  std::vector<char> blob_;
  std::vector<Structure::TableRef>& layout_;
};

// the base-spline point of a time node: local time in the active polynomial, 1 / its duration, and 6 * its index (the offset
// of its first node in base-lin / base-ang); the records assign it to their named fields with std::tie
std::tuple<double, double, int32_t> BaseAt(const SplineLayout& base, const TimeNode& n) {
  return std::make_tuple(n.t_local, 1.0 / base.durations[n.poly], 6 * n.poly);
}

// start time of every polynomial: the running sum Spline::GetSegmentID compares t against (spline.cc:52-57)
std::vector<double> StartTimes(const std::vector<double>& durations) {
  std::vector<double> t0(durations.size() + 1, 0.0);
  for (size_t q = 0; q < durations.size(); ++q) t0[q + 1] = t0[q] + durations[q];
  return t0;
}

// the ee-motion polynomial of a range-of-motion record (RomRec, RomSeg): 1 / duration, first x index, meta and the 48-bit
// slot word (12 x 4 bit: the slot of candidate c, 0xF = absent)
template <class R>
void SetRomPoly(R& r, const PolyDesc& p) {
  r.iTm = p.iT;
  r.xbase = p.xbase;
  r.meta = p.meta;
  uint64_t slots = 0;
  for (int c = 0; c < 12; ++c) slots |= (uint64_t)(p.cand[c] & 0xF) << (4 * c);
  r.slots[0] = (uint32_t)slots;
  r.slots[1] = (uint32_t)(slots >> 32);
}

// Cuts the time nodes [0, K) into consecutive runs from the left, each as long as fits(k0, k1) allows for the run [k0, k1):
// (first node, count) per run, or none when a single time node does not fit.
template <class Fits>
std::vector<std::pair<int, int>> CutRuns(int K, const Fits& fits) {
  std::vector<std::pair<int, int>> runs;
  for (int k0 = 0; k0 < K;) {
    int k1 = k0;
    while (k1 < K && fits(k0, k1 + 1)) ++k1;
    if (k1 == k0) return {};
    runs.push_back({k0, k1 - k0});
    k0 = k1;
  }
  return runs;
}

// the per-ee sets of one family are adjacent in g / jac: one flat list
template <class T>
std::vector<T> FlatFamily(const Structure& S, const std::string& prefix, int rows_per_item, const std::vector<std::vector<T>>& per_ee,
                          int32_t& row0, int32_t& nnz0, int32_t& count) {
  std::vector<T> all;
  for (int e = 0; e < S.n_ee; ++e) {
    const SetInfo* si = S.FindSet(prefix + std::to_string(e));
    if (!si) break;
    if (e == 0) { row0 = si->offset; nnz0 = si->nnz_offset; }
    if (si->offset != row0 + rows_per_item * (int)all.size()) throw std::runtime_error(prefix + " sets not adjacent");
    all.insert(all.end(), per_ee[e].begin(), per_ee[e].end());
  }
  count = (int32_t)all.size();
  return all;
}

// the node head (device_tables.h): first 64 terrain rows, first 64 force nodes, at fixed offsets behind the header
void PutNodeHead(BlobWriter& w, const std::vector<TerrainRow>& rows, const std::vector<ForceNode>& forces) {
  std::vector<char> head(kNodeHeadBytes, 0);
  if (!rows.empty()) std::memcpy(head.data(), rows.data(), std::min<size_t>(64, rows.size()) * sizeof(TerrainRow));
  if (!forces.empty())
    std::memcpy(head.data() + 64 * sizeof(TerrainRow), forces.data(), std::min<size_t>(64, forces.size()) * sizeof(ForceNode));
  if (w.Put(head.data(), head.size()) != kNodeHeadTerrainOff) throw std::runtime_error("node head is not the first table of the blob");
}

// optimised timings: the polynomial table of one ee spline (device_tables.h PhasePoly)
std::vector<PhasePoly> PhasePolyTable(const SplineLayout& sl, const std::vector<PolyDesc>& pd) {
  std::vector<PhasePoly> out(pd.size());
  const std::vector<int> dim_of = DimOf(sl);
  int in_phase = 0;
  for (size_t q = 0; q < pd.size(); ++q) {
    PhasePoly& pp = out[q];
    in_phase = (q > 0 && sl.poly_phase[q] == sl.poly_phase[q - 1]) ? in_phase + 1 : 0;
    int n_in = 0;
    for (size_t q2 = 0; q2 < pd.size(); ++q2) n_in += sl.poly_phase[q2] == sl.poly_phase[q];
    pp.phase = sl.poly_phase[q];
    pp.n_in_phase = n_in;
    pp.poly_in_phase = in_phase;
    pp.xbase = pd[q].xbase;
    pp.meta = pd[q].meta;
    std::memcpy(pp.cand, pd[q].cand, sizeof(pp.cand));
    const int before = (pd[q].meta & 0xF) ? pd[q].xbase - sl.var_offset : 0;
    for (int i = 0; i < before; ++i) {
      for (int r = 0; r < 3; ++r) {
        if (dim_of[i] != r) pp.base_ne[r]++;
        if (dim_of[i] == r) pp.base_eq[r]++;
      }
    }
    pp.base_all = (uint16_t)before;
  }
  return out;
}

// the dynamic row, relative to a time node's first, of value i of a candidate of dimension d: the two angular rows, then the
// linear row (ee-force)
int CandRow(int d, int i) { return i < 2 ? (d + 1 + i) % 3 : 3 + d; }

// optimised timings: where the W values of each candidate of one ee polynomial go inside a time node's expanded dynamic
// rows (PhasePutM, PhasePutF); `trash` for absent candidates, unused entries and dummy records (p = nullptr)
template <int W, class Put, class Pos>
Put PhasePutOf(const PolyDesc* p, uint16_t trash, const Pos& pos) {
  Put r;
  for (auto& row : r.off)
    for (uint16_t& v : row) v = trash;
  for (int c = 0; c < 12 && p; ++c) {
    if (p->cand[c] == 0xFFFF) continue;
    const int j = c / 3, d = c % 3, col = p->xbase + (p->cand[c] & 0xF);
    for (int i = 0; i < W; ++i) r.off[j][W * d + i] = (uint16_t)(8 * pos(CandRow(d, i), col));
  }
  return r;
}

// dyn_kernel's tables of the dynamic set, fixed timings (device_tables.h)
struct DynTables {
  int row = 0;                                 // first row of the set
  std::vector<DynPolyT> polys_t;
  std::vector<DynPolyL> polys;
  std::vector<std::vector<int>> rec_of[2];     // [kind][ee][q] -> record index (kind 0: ee-motion, 1: ee-force)
  std::vector<DynNodeT> nodes_t;
  std::vector<DynNodeL> nodes;
  std::vector<DynSel> sel;
  std::vector<DynTile> tiles;                  // four per (slice, polynomial combination)
};

// position in col_idx of column `col` of CSR row `row` (exact) or of the first column after it
int ColumnPos(const Structure& S, int row, int col, bool exact) {
  const int32_t* b = S.col_idx.data() + S.row_ptr[row];
  const int32_t* e = S.col_idx.data() + S.row_ptr[row + 1];
  const int32_t* it = std::lower_bound(b, e, col);
  if (exact && (it == e || *it != col)) throw std::runtime_error("dynamic pattern lacks an expected column");
  return (int)(it - S.col_idx.data());
}

// candidate scoring: family and bounds of every row (device_tables.h, ScoreTables)
void PutScoreRecord(const Structure& S, BlobWriter& w, DevStruct& h) {
  if (S.con_sets.size() > (size_t)kMaxConSets) throw std::runtime_error("too many constraint sets");
  std::vector<double> pairs;
  std::map<std::pair<uint64_t, uint64_t>, int> pair_index;   // distinct (lower, upper), by bit pattern
  std::vector<uint16_t> meta((size_t)S.n_rows, 0);
  int slot_of[8] = {-1, -1, -1, -1, -1, -1, -1, -1}, n_slots = 0;
  // (sets in row order: the slots are handed out in the order the families first appear along the rows)
  std::vector<size_t> by_row(S.con_sets.size());
  std::iota(by_row.begin(), by_row.end(), (size_t)0);
  std::sort(by_row.begin(), by_row.end(), [&](size_t a, size_t b) { return S.con_sets[a].offset < S.con_sets[b].offset; });
  for (size_t i : by_row) {
    const std::string& nm = S.con_sets[i].name;
    auto starts = [&](const char* p) { return nm.rfind(p, 0) == 0; };
    const int fam = starts("terrain-") ? 0 : starts("dynamic") ? 1 : starts("splineacc-") ? 2 : starts("rangeofmotion-") ? 3
                  : starts("force-") ? 4 : starts("swing-") ? 5 : starts("totalduration-") ? 6 : starts("baseMotion") ? 7 : -1;
    if (fam < 0) throw std::runtime_error("constraint set of an unknown family");
    if (S.con_sets[i].size > 0 && slot_of[fam] < 0) slot_of[fam] = n_slots++;
    if (S.con_sets[i].size > 0 && slot_of[fam] != n_slots - 1) throw std::runtime_error("the sets of a constraint family are not adjacent in g");
    for (int r = S.con_sets[i].offset; r < S.con_sets[i].offset + S.con_sets[i].size; ++r) {
      uint64_t kl, ku;
      std::memcpy(&kl, &S.lower[r], 8);
      std::memcpy(&ku, &S.upper[r], 8);
      auto it = pair_index.find({kl, ku});
      if (it == pair_index.end()) {
        it = pair_index.emplace(std::make_pair(kl, ku), (int)(pairs.size() / 2)).first;
        pairs.push_back(S.lower[r]);
        pairs.push_back(S.upper[r]);
      }
      if (it->second >= kScoreMaxPairs) throw std::runtime_error("more than 127 distinct constraint bounds in one structure");
      meta[r] = (uint16_t)(slot_of[fam] << 12 | it->second);
    }
  }
  ScoreTables sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.n_rows = S.n_rows;
  sc.n_pairs = (int)(pairs.size() / 2);
  for (int f = 0; f < 8; ++f) sc.slot_of_family[f] = (int8_t)slot_of[f];
  // [ ScoreTables | pairs | zero padding to kScoreHeadBytes ][ meta words ] at a FIXED offset behind the node head: score_kernel
  // asks for all of it without having seen a single field of the header
  if (sizeof(sc) + pairs.size() * sizeof(double) > (size_t)kScoreHeadBytes) throw std::runtime_error("score record head overflows");
  std::vector<char> rec(kScoreHeadBytes + (meta.size() * sizeof(uint16_t) + 15) / 16 * 16, 0);
  std::memcpy(rec.data(), &sc, sizeof(sc));
  if (!pairs.empty()) std::memcpy(rec.data() + sizeof(sc), pairs.data(), pairs.size() * sizeof(double));
  if (!meta.empty()) std::memcpy(rec.data() + kScoreHeadBytes, meta.data(), meta.size() * sizeof(uint16_t));
  h.o_score = w.Put(rec.data(), rec.size());
  if (h.o_score != kScoreOff) throw std::runtime_error("score record is not at its fixed offset");
}

// the node families: force, terrain, splineacc, baseMotion, swing
void PutNodeFamilies(const Structure& S, BlobWriter& w, DevStruct& h, const std::vector<TerrainRow>& rows, const std::vector<ForceNode>& forces,
                                const std::vector<SwingNode>& swings) {
  if (const SetInfo* si = S.FindSet("splineacc-base-lin")) {
    const SetInfo* sa = S.FindSet("splineacc-base-ang");
    if (!sa || sa->offset != si->offset + si->size || S.off_base_lin != 0) throw std::runtime_error("splineacc sets not adjacent");
    h.row_acc = si->offset;
    h.nnz_acc = si->nnz_offset;
    h.n_junctions = (int)S.acc_junctions.size();
  }
  h.o_force_nodes = w.Put(forces);
  h.o_terrain_rows = w.Put(rows);
  h.o_acc = w.Put(S.acc_junctions);
  if (const SetInfo* si = S.FindSet("baseMotion")) {
    std::vector<BaseNode> bn(S.grid_bm.size());
    for (size_t k = 0; k < S.grid_bm.size(); ++k) std::tie(bn[k].t, bn[k].iT, bn[k].q6) = BaseAt(S.base, S.bm_base[k]);
    h.row_bm = si->offset;
    h.nnz_bm = si->nnz_offset;
    h.n_bm_nodes = (int)bn.size();
    h.o_bm = w.Put(bn);
  }
  h.o_swing_nodes = w.Put(swings);
}

// --- DynPolyT / DynPolyL: one record pair per polynomial of every ee spline, ordered by start time, so that the records a slice
// (a short time window) reads sit next to each other and an 8-bit index relative to the slice's first record
// reaches all of them
void DynPolyRecords(const Structure& S, DynTables& t) {
  struct PolyRef {
    double t0;
    int e, kind, q;   // kind 0: ee-motion, 1: ee-force
  };
  std::vector<PolyRef> order;
  for (auto& r : t.rec_of) r.resize(S.n_ee);
  for (int e = 0; e < S.n_ee; ++e)
    for (int kind = 0; kind < 2; ++kind) {
      const std::vector<double> t0 = StartTimes(kind == 0 ? S.motion[e].durations : S.force[e].durations);
      for (size_t q = 0; q + 1 < t0.size(); ++q) order.push_back({t0[q], e, kind, (int)q});
      t.rec_of[kind][e].resize(t0.size() - 1);
    }
  std::stable_sort(order.begin(), order.end(), [](const PolyRef& a, const PolyRef& b) { return a.t0 < b.t0; });
  t.polys_t.resize(order.size());
  t.polys.resize(order.size());
  for (size_t i = 0; i < order.size(); ++i) {
    const PolyRef& pr = order[i];
    t.rec_of[pr.kind][pr.e][pr.q] = (int)i;
    const PolyDesc& pd = pr.kind == 0 ? S.mpoly[pr.e][pr.q] : S.fpoly[pr.e][pr.q];
    t.polys_t[i].t0 = pr.t0;
    t.polys_t[i].iT = pd.iT;
    DynPolyL& P = t.polys[i];
    int slot_of[12];
    for (int c = 0; c < 12; ++c) {
      slot_of[c] = pd.cand[c] == 0xFFFF ? -1 : (pd.cand[c] & 0xF);
      if (slot_of[c] >= 0) {
        P.rel[c] = (uint8_t)slot_of[c];
        P.pres[c] = 0xFF;
      }
    }
    // 8 * the position of candidate src's slot among the slots of its two angular rows / its linear row: the ranks MakeEePoly
    // stored in PolyDesc::cand, valid here because every src below has the dimension of the candidate c it stands in for
    auto code = [&](int src, int r) { return (uint8_t)(8 * ((pd.cand[src] >> (4 + 4 * r)) & 0xF)); };
    if (pr.kind == 0) {
      if ((pd.meta >> 16) & 1) P.flags |= 1;
      for (int d = 0; d < 3; ++d)
        if (slot_of[d] < 0) throw std::runtime_error("ee-motion node position that is not a variable");
      for (int c = 0; c < 12; ++c) {
        const int src = slot_of[c] >= 0 ? c : c % 3;   // not a variable: p0's slots (stored last by the kernel)
        for (int r = 0; r < 2; ++r) P.code[2 * c + r] = code(src, r);
      }
      continue;
    }
    bool present[4];
    for (int j = 0; j < 4; ++j) {
      present[j] = slot_of[3 * j] >= 0;
      for (int d = 1; d < 3; ++d)
        if ((slot_of[3 * j + d] >= 0) != present[j]) throw std::runtime_error("ee-force node value that is a variable in some dimensions only");
    }
    if (present[0] != present[1] || present[2] != present[3]) throw std::runtime_error("ee-force node with a constant position or velocity only");
    if (!present[0]) P.flags |= 2;
    if (!present[2]) P.flags |= 4;
    for (int c = 0; c < 12; ++c) {
      const int d = c % 3, j = c / 3;
      if ((pd.meta & 0xF) == 0) continue;             // no variables at all: codes 0, the tile starts point at trash
      const int src = present[j] ? c : (j ^ 2) * 3 + d;   // constant node: the other node's value of the same kind
      if (slot_of[src] < 0) throw std::runtime_error("ee-force polynomial layout not understood");
      for (int r = 0; r < 3; ++r) P.code[3 * c + r] = code(src, r);
    }
  }
}

// the per-node records of one dynamic slice and the tile records of its polynomial combinations (shift: PutDynTables' stage)
void DynSliceNodes(const Structure& S, DynTables& t, const Structure::DynSlice& sl, const int (&shift)[2][kMaxEE]) {
  const int qmin = S.dyn_base[sl.k0].poly, nbase = 6 * (S.dyn_base[sl.k0 + sl.cnt - 1].poly - qmin + 2);   // base-lin doubles staged
  std::vector<int> combo_key;   // active polynomial ids of the last combination: a new slice has its own staging layout, its
                                // first node opens a new combination
  for (int k = sl.k0; k < sl.k0 + sl.cnt; ++k) {
    const int row0 = t.row + 6 * k, v0 = S.row_ptr[row0];
    DynNodeL& N = t.nodes[k];
    t.nodes_t[k].t = S.grid_dyn[k];
    std::tie(t.nodes_t[k].tb, t.nodes_t[k].iTb, std::ignore) = BaseAt(S.base, S.dyn_base[k]);
    N.sb_lin = (uint16_t)(8 * (2 + 6 * (S.dyn_base[k].poly - qmin)));
    N.sb_ang = (uint16_t)(8 * (2 + nbase + 6 * (S.dyn_base[k].poly - qmin)));
    const int node_rel = v0 - S.row_ptr[t.row + 6 * sl.k0];
    N.nb = (uint16_t)(8 * node_rel);
    N.rs1 = (uint16_t)(8 * (S.row_ptr[row0 + 1] - v0));
    N.rs2 = (uint16_t)(8 * (S.row_ptr[row0 + 2] - v0));
    for (int d = 0; d < 3; ++d) N.rl[d] = (uint16_t)(8 * (S.row_ptr[row0 + 3 + d] - v0));
    // where a tile starts in a row, relative to the node's first value: the position of the polynomial's first
    // variable in the CSR row (read off the pattern itself, so kernel and pattern cannot disagree)
    auto pos = [&](int row, int col, bool exact) { return ColumnPos(S, row0 + row, col, exact) - v0; };
    // the tile starts depend on the node only through the active polynomials: one record set per combination
    std::vector<int> key;
    for (int e = 0; e < S.n_ee; ++e) {
      key.push_back(S.dyn_motion[e][k].poly);
      key.push_back(S.dyn_force[e][k].poly);
    }
    const bool new_combo = key != combo_key;
    if (new_combo) {
      combo_key = key;
      t.tiles.resize(t.tiles.size() + 4);
    }
    const size_t tile0 = t.tiles.size() - 4;
    if (tile0 + 3 > 0xFFFF) throw std::runtime_error("too many polynomial combinations for 16-bit tile indices");
    for (int role = 0; role < 4; ++role) {
      DynSel& Sx = t.sel[(size_t)k * 4 + role];
      DynTile T = {};
      Sx.tile = (uint16_t)(tile0 + role);
      Sx.dm = Sx.df = (uint8_t)kDynPolyDummy;
      // trash: base-lin entry `role` of every row (the rows' first four entries are base-lin values, which the same
      // wave writes after the tiles); the dummy record's codes are 0
      const int row_start[6] = {0, N.rs1, N.rs2, N.rl[0], N.rl[1], N.rl[2]};
      for (int r = 0; r < 3; ++r) T.base_m[r] = (uint16_t)(row_start[r] + 8 * role);
      for (int r = 0; r < 6; ++r) T.base_f[r] = (uint16_t)(row_start[r] + 8 * role);
      if (role < S.n_ee) {
        const int e = role;
        const int qm = S.dyn_motion[e][k].poly, qf = S.dyn_force[e][k].poly;
        const PolyDesc& mp = S.mpoly[e][qm];
        const PolyDesc& fp = S.fpoly[e][qf];
        const int rm = t.rec_of[0][e][qm], rf = t.rec_of[1][e][qf];
        Sx.dm = (uint8_t)(rm - sl.poly0);
        Sx.df = (uint8_t)(rf - sl.poly0);
        if (rm - sl.poly0 >= kDynPolyDummy || rf - sl.poly0 >= kDynPolyDummy || rm < sl.poly0 || rf < sl.poly0)
          throw std::runtime_error("polynomial record index does not fit the slice");
        T.s_m = (uint8_t)(shift[0][e] + mp.xbase);
        if ((mp.meta & 0xF) == 0) throw std::runtime_error("ee-motion polynomial without variables");
        for (int r = 0; r < 3; ++r) T.base_m[r] = (uint16_t)(8 * pos(r, mp.xbase, false));
        if ((fp.meta & 0xF) != 0) {
          T.s_f = (uint8_t)(shift[1][e] + fp.xbase);
          for (int r = 0; r < 6; ++r) T.base_f[r] = (uint16_t)(8 * pos(r, fp.xbase, false));
        }
        // self-check of the decomposition  offset = tile start + 8 * rank  against the pattern, value by value (once per
        // polynomial combination: the nodes of a combination share their tile records, asserted below)
        auto check = [&](const PolyDesc& p, const uint16_t* tile, const DynPolyL& P, int W, const char* what) {
          for (int c = 0; c < 12 && new_combo; ++c)
            for (int i = 0; i < W && p.cand[c] != 0xFFFF; ++i) {
              const int row = CandRow(c % 3, i);
              if (tile[row] + P.code[W * c + i] != 8 * pos(row, p.xbase + (p.cand[c] & 0xF), true)) throw std::runtime_error(what);
            }
        };
        check(mp, T.base_m, t.polys[rm], 2, "ee-motion tile offsets disagree with the CSR pattern");
        check(fp, T.base_f, t.polys[rf], 3, "ee-force tile offsets disagree with the CSR pattern");
      }
      if (!new_combo && std::memcmp(&t.tiles[tile0 + role], &T, sizeof(T)) != 0)
        throw std::runtime_error("tile starts differ inside one polynomial combination");
      t.tiles[tile0 + role] = T;
    }
  }
}

// --- dynamic, fixed timings: slices, staging maps and per-lane records with every index resolved to an LDS
// byte offset (device_tables.h).  The put offsets are read off the CSR pattern itself, so kernel and
// pattern cannot disagree.
void PutDynTables(Structure& S, BlobWriter& w) {
  const SetInfo* dyn = S.FindSet("dynamic");
  if (!dyn) return;
  const int K = (int)S.grid_dyn.size();
  DynTables t;
  t.row = dyn->offset;
  DynPolyRecords(S, t);
  // the doubles of x the nodes [k0, k1) read, in staging order (xs index 2 + entry): the nodes of their base-lin, then base-ang
  // polynomials, then the variables of each ee's active motion (kind 0) and force (kind 1) polynomials.  With `xidx`: the
  // x index of every entry, and shift[kind][e] such that x index i of that ee range is staged at xs index i + shift
  auto stage = [&](int k0, int k1, std::vector<int>* xidx, int (*shift)[kMaxEE]) {
    const int qmin = S.dyn_base[k0].poly, nbase = 6 * (S.dyn_base[k1 - 1].poly - qmin + 2);
    for (int i = 0; xidx && i < nbase; ++i) xidx->push_back(S.off_base_lin + 6 * qmin + i);
    for (int i = 0; xidx && i < nbase; ++i) xidx->push_back(S.off_base_ang + 6 * qmin + i);
    int n = 2 * nbase;
    for (int e = 0; e < S.n_ee; ++e)
      for (int kind = 0; kind < 2; ++kind) {
        const std::vector<PolyDesc>& pd = kind == 0 ? S.mpoly[e] : S.fpoly[e];
        const std::vector<TimeNode>& at = kind == 0 ? S.dyn_motion[e] : S.dyn_force[e];
        int lo = 1 << 30, hi = -1;
        for (int q = at[k0].poly; q <= at[k1 - 1].poly; ++q) {
          const int ns = (int)(pd[q].meta & 0xF);
          if (!ns) continue;
          lo = std::min(lo, pd[q].xbase);
          hi = std::max(hi, pd[q].xbase + ns);
        }
        if (hi < 0) lo = hi = 0;
        if (xidx) shift[kind][e] = 2 + n - lo;
        for (int i = lo; xidx && i < hi; ++i) xidx->push_back(i);
        n += hi - lo;
      }
    return n;
  };
  auto nvals_of = [&](int k0, int k1) { return S.row_ptr[t.row + 6 * k1] - S.row_ptr[t.row + 6 * k0]; };
  auto first_rec = [&](int k) {   // the first polynomial record time node k reads
    int lo = 1 << 30;
    for (int e = 0; e < S.n_ee; ++e) lo = std::min({lo, t.rec_of[0][e][S.dyn_motion[e][k].poly], t.rec_of[1][e][S.dyn_force[e][k].poly]});
    return lo;
  };
  auto rec_span_ok = [&](int k0, int k1) {   // the 8-bit record indices of a slice (255 = dummy)
    int hi = -1;
    for (int e = 0; e < S.n_ee; ++e)
      for (int k : {k0, k1 - 1}) hi = std::max({hi, t.rec_of[0][e][S.dyn_motion[e][k].poly], t.rec_of[1][e][S.dyn_force[e][k].poly]});
    return hi - first_rec(k0) < kDynPolyDummy;
  };
  t.nodes_t.resize(K);
  t.nodes.resize(K);
  t.sel.resize((size_t)K * 4);
  S.dyn_slices.clear();
  S.dyn_staged_max = 0;
  // Slices that stage at most 128 doubles of x read the 256-byte form of their staging map and gather x with two loads per
  // lane instead of four (dyn_body XC = 2) -- if EVERY slice of a batch does.  Fine discretisations do anyway (a 12..15-node
  // slice of a K = 200 problem stages 90-130); where the general capacity would let a few slices stage a little more, they
  // are cut at 128 instead, as long as that costs at most one more slice per eight.
  auto cut = [&](int cap) {
    return CutRuns(K, [&](int k0, int k1) {
      return k1 - k0 <= kDynNodes && nvals_of(k0, k1) <= kDynImage && stage(k0, k1, nullptr, nullptr) <= cap && rec_span_ok(k0, k1);
    });
  };
  const auto general = cut(kDynXsCap), small = cut(std::min(kDynXsCap, 128));
  const int n_general = general.empty() ? 1 << 30 : (int)general.size(), n_small = small.empty() ? 1 << 30 : (int)small.size();
  const auto& runs = n_small <= n_general + (n_general + 7) / 8 ? small : general;
  if (runs.empty()) throw std::runtime_error("one time node of the dynamic set exceeds the LDS staging capacity");
  for (const auto& run : runs) {
    const int k0 = run.first, k1 = run.first + run.second;
    if (nvals_of(k0, k1) < 16) throw std::runtime_error("a time-node run with fewer than 16 Jacobian values cannot be staged");
    // staging layout of the slice
    std::vector<int> xidx;
    int shift[2][kMaxEE];
    stage(k0, k1, &xidx, shift);
    if ((int)xidx.size() > kDynXsCap) throw std::runtime_error("staging count inconsistent");
    for (int x : xidx)
      if (x < 0 || x > 0xFFFF) throw std::runtime_error("x index does not fit the staging map");
    auto staging_map = [&](int chunks) {   // lane l holds entries l, 64 + l, ...; unused entries stage x[0] (harmless)
      std::vector<uint16_t> map(64 * chunks, 0);
      for (size_t e = 0; e < xidx.size(); ++e) map[(e % 64) * chunks + e / 64] = (uint16_t)xidx[e];
      return map;
    };
    Structure::DynSlice sl;
    sl.k0 = k0;
    sl.cnt = k1 - k0;
    sl.nvals = nvals_of(k0, k1);
    sl.map = w.PutLayout(staging_map(4));
    sl.map2 = sl.map;
    S.dyn_staged_max = std::max(S.dyn_staged_max, (int)xidx.size());
    if (xidx.size() <= 128) sl.map2 = w.PutLayout(staging_map(2));   // the 256-byte form (what a batch of such slices reads)
    sl.poly0 = first_rec(k0);
    S.dyn_slices.push_back(sl);
    DynSliceNodes(S, t, sl, shift);
  }
  // times first, then the layout tables (twr_batch_create stores byte-identical layout tables of a batch once)
  S.off_dyn_nodes_t = w.Put(t.nodes_t);
  S.off_dyn_poly_t = w.Put(t.polys_t);
  S.off_dyn_nodes_l = w.PutLayout(t.nodes);
  S.off_dyn_sel = w.PutLayout(t.sel);
  S.off_dyn_tile = w.PutLayout(t.tiles);
  S.off_dyn_poly_l = w.PutLayout(t.polys);
}

// --- rangeofmotion-<ee>, fixed timings: per-node records shared by all ee, slices, per-(slice, polynomial) segments
void PutRomTables(Structure& S, BlobWriter& w) {
  if (!S.FindSet("rangeofmotion-0")) return;
  const int K = (int)S.grid_rom.size();
  std::vector<RomNode> nodes(K);
  for (int k = 0; k < K; ++k) {
    nodes[k].t = S.grid_rom[k];
    std::tie(nodes[k].tb, nodes[k].iTb, nodes[k].q6) = BaseAt(S.base, S.rom_base[k]);
  }
  for (int e = 0; e < S.n_ee; ++e) {
    const int row0 = S.FindSet("rangeofmotion-" + std::to_string(e))->offset;
    auto vals = [&](int k0, int k1) { return S.row_ptr[row0 + 3 * k1] - S.row_ptr[row0 + 3 * k0]; };
    auto segs = [&](int k0, int k1) {   // polynomials of the ee spline active in nodes [k0, k1)
      int n = 1;
      for (int k = k0 + 1; k < k1; ++k) n += S.rom_motion[e][k].poly != S.rom_motion[e][k - 1].poly;
      return n;
    };
    // Balanced runs: the fewest runs that respect the limits (<= 64 time nodes = lanes, the LDS image, kRomMaxSeg
    // polynomials), of (nearly) equal length -- K = 200 gives 4 x 50 rather than 64 + 64 + 64 + 8: the kernel has a
    // compile-time number of copy-out stores and pays the full count for a short tail run too.
    auto cut = [&](int limit) {
      return CutRuns(K, [&](int k0, int k1) { return k1 - k0 <= limit && vals(k0, k1) <= kRomStage && segs(k0, k1) <= kRomMaxSeg; });
    };
    std::vector<std::pair<int, int>> best = cut(64);
    if (best.empty()) throw std::runtime_error("one time node exceeds the LDS staging capacity");
    for (int limit = (K + (int)best.size() - 1) / (int)best.size(); limit < 64; ++limit) {
      auto runs = cut(limit);   // the smallest run length that still needs no more runs
      if (runs.size() == best.size()) {
        best = std::move(runs);
        break;
      }
    }
    const std::vector<double> t0 = StartTimes(S.motion[e].durations);
    for (const auto& r : best) {
      Structure::RomSlice sl;
      sl.k0 = r.first;
      sl.cnt = r.second;
      sl.nvals = vals(r.first, r.first + r.second);
      // copy_out_fixed clamps its tail iterations to the last complete pair of the slice: a slice must hold one
      if (sl.nvals < 4) throw std::runtime_error("a time-node run with fewer than 4 Jacobian values cannot be staged");
      std::memset(sl.first, 255, sizeof(sl.first));
      std::vector<RomSeg> sg;
      for (int k = sl.k0; k < sl.k0 + sl.cnt; ++k) {
        const int q = S.rom_motion[e][k].poly;
        if (k == sl.k0 || q != S.rom_motion[e][k - 1].poly) {
          const PolyDesc& mp = S.mpoly[e][q];
          RomSeg seg = {};
          seg.t0 = t0[q];
          SetRomPoly(seg, mp);
          seg.voff0 = vals(sl.k0, k);
          seg.kfirst = k - sl.k0;
          seg.node_vals = vals(k, k + 1);
          if (seg.node_vals != 68 + 3 * (int)(mp.meta & 0xF)) throw std::runtime_error("rangeofmotion row lengths inconsistent");
          sl.first[sg.size()] = (uint8_t)(k - sl.k0);
          sg.push_back(seg);
        }
        // every node of a segment has the same row lengths: voff = voff0 + (k - kfirst) * node_vals (checked); which segment of
        // this ee's slice node k reads: three bits per ee
        const RomSeg& last = sg.back();
        if (vals(sl.k0, k) != last.voff0 + (k - sl.k0 - last.kfirst) * last.node_vals) throw std::runtime_error("rangeofmotion segment layout inconsistent");
        nodes[k].seg |= (uint32_t)(sg.size() - 1) << (3 * e);
      }
      sl.segs = w.Put(sg);
      S.rom_slices[e].push_back(sl);
    }
  }
  S.off_rom_nodes = w.Put(nodes);   // (after the loop: it fills RomNode::seg)
}

// --- optimised timings: per-node record templates, polynomial tables, set-wide counts, global grid times
uint32_t PutPhaseTables(Structure& S, BlobWriter& w) {
  const SetInfo* dyn = S.FindSet("dynamic");
  const SetInfo* rom[kMaxEE] = {nullptr, nullptr, nullptr, nullptr};
  for (int e = 0; e < S.n_ee; ++e) rom[e] = S.FindSet("rangeofmotion-" + std::to_string(e));
  const bool have_rom = rom[0] != nullptr;
  if (dyn) {   // dynamic: the base-spline part of the per-node record (the rest depends on x)
    std::vector<DynShared> sh(S.grid_dyn.size());
    for (size_t k = 0; k < S.grid_dyn.size(); ++k) {
      std::tie(sh[k].tb, sh[k].iTb, sh[k].q6) = BaseAt(S.base, S.dyn_base[k]);
      sh[k].voff = S.row_ptr[dyn->offset + 6 * k] - dyn->nnz_offset;
    }
    S.off_dyn_shared = w.Put(sh);
  }
  // rangeofmotion-<ee>: the record templates (the pre-pass fills in the x-dependent part)
  for (int e = 0; e < S.n_ee && have_rom; ++e) {
    std::vector<RomRec> rc(S.grid_rom.size());
    for (size_t k = 0; k < S.grid_rom.size(); ++k) {
      RomRec& R = rc[k];
      const PolyDesc& mp = S.mpoly[e][S.rom_motion[e][k].poly];
      std::tie(R.tb, R.iTb, R.q6) = BaseAt(S.base, S.rom_base[k]);
      R.tm = S.rom_motion[e][k].t_local;
      R.voff = S.row_ptr[rom[e]->offset + 3 * k] - rom[e]->nnz_offset;
      SetRomPoly(R, mp);
    }
    S.off_rom_recs[e] = w.Put(rc);
  }
  PhaseTables& pt = S.phase_tables;
  std::memset(&pt, 0, sizeof(pt));
  for (int e = 0; e < S.n_ee; ++e) {
    pt.off_sched[e] = S.off_schedule[e];
    pt.n_phases[e] = S.schedule.n_phases[e];
    pt.t_total[e] = std::accumulate(S.schedule.phase_durations[e], S.schedule.phase_durations[e] + S.schedule.n_phases[e], 0.0);
    const auto mp = PhasePolyTable(S.motion[e], S.mpoly[e]), fp = PhasePolyTable(S.force[e], S.fpoly[e]);
    pt.n_mpoly[e] = (int)mp.size();
    pt.n_fpoly[e] = (int)fp.size();
    pt.o_mpoly[e] = w.Put(mp);
    pt.o_fpoly[e] = w.Put(fp);
    const std::vector<int> dm = DimOf(S.motion[e]), df = DimOf(S.force[e]);
    for (int r = 0; r < 3; ++r) {
      for (int v : dm) pt.mne[e][r] += v != r;
      for (int v : df) { pt.fne[e][r] += v != r; pt.feq[e][r] += v == r; }
    }
    pt.msize[e] = S.motion[e].var_size;
  }
  int sched_total = 0;
  for (int e = 0; e < S.n_ee; ++e) sched_total += S.schedule.n_phases[e] - 1;
  for (int r = 0; r < 3; ++r) {
    pt.len_ang[r] = 20 + sched_total;
    pt.len_lin[r] = 4 + sched_total;
    for (int e = 0; e < S.n_ee; ++e) {
      pt.len_ang[r] += pt.mne[e][r] + pt.fne[e][r];
      pt.len_lin[r] += pt.feq[e][r];
    }
    pt.node_vals += pt.len_ang[r] + pt.len_lin[r];
  }
  for (int e = 0; e < S.n_ee; ++e) {
    for (int r = 0; r < 3; ++r) {
      pt.rom_len[e][r] = 12 + (r == 0 ? 8 : 12) + pt.msize[e] + S.schedule.n_phases[e] - 1;
      pt.rom_node_vals[e] += pt.rom_len[e][r];
    }
    if (have_rom) {
      pt.row_rom[e] = rom[e]->offset;
      pt.nnz_rom[e] = rom[e]->nnz_offset;
    }
    // rom_phase_kernel assembles whole expanded time nodes in LDS: one node must fit the 160 KB of a CU
    // (the dynamic set has the matching guard below; without it the batch is created and every evaluation fails to launch)
    if (have_rom && pt.rom_node_vals[e] > 160 * 128)
      throw std::runtime_error("optimised timings: a time node of rangeofmotion-" + std::to_string(e) + " has more than 20480 Jacobian values");
  }
  pt.o_tdyn = w.Put(S.grid_dyn);
  pt.o_trom = w.Put(S.grid_rom);
  pt.k_dyn = dyn ? (int)S.grid_dyn.size() : 0;
  pt.k_rom = have_rom ? (int)S.grid_rom.size() : 0;
  pt.row_dyn = dyn ? dyn->offset : 0;
  pt.nnz_dyn = dyn ? dyn->nnz_offset : 0;
  pt.off_lin = S.off_base_lin;
  pt.off_ang = S.off_base_ang;
  pt.o_dyn_shared = S.off_dyn_shared;
  for (int e = 0; e < S.n_ee; ++e) {
    pt.o_rom_recs[e] = S.off_rom_recs[e];
    if (pt.n_mpoly[e] > kMaxPhasePolys || pt.n_fpoly[e] > kMaxPhasePolys) throw std::runtime_error("too many polynomials per ee spline for optimised timings");
  }
  if (const SetInfo* si = S.FindSet("totalduration-0")) {
    pt.row_total = si->offset;
    pt.nnz_total = si->nnz_offset;
  }
  // dynamic: byte offset of every ee value inside a time node's expanded rows, read off the CSR pattern of time
  // node 0 (the rows hold all variables of every ee set, so the ee part of the layout is the same at every node)
  if (dyn) {
    if (pt.node_vals > 8191) throw std::runtime_error("optimised timings: a time node of the dynamic set has more than 8191 Jacobian values");
    const int v0 = S.row_ptr[dyn->offset];
    auto find = [&](int row, int col) { return ColumnPos(S, dyn->offset + row, col, true) - v0; };
    std::vector<PhasePutM> pm_all;
    std::vector<PhasePutF> pf_all;
    for (int e = 0; e < S.n_ee; ++e) {
      const uint16_t trash = (uint16_t)(8 * (8 + e));   // base-ang entry of row AX, rewritten after the tiles
      pt.mput_base[e] = (int)pm_all.size();
      pt.fput_base[e] = (int)pf_all.size();
      for (const PolyDesc& p : S.mpoly[e]) pm_all.push_back(PhasePutOf<2, PhasePutM>(&p, trash, find));
      for (const PolyDesc& p : S.fpoly[e]) pf_all.push_back(PhasePutOf<3, PhasePutF>(&p, trash, find));
      pt.ee[e].ns = S.schedule.n_phases[e] - 1;
      for (int r = 0; r < 3; ++r) {
        pt.ee[e].dur_ang[r] = 8 * find(r, S.off_schedule[e]);
        pt.ee[e].dur_lin[r] = 8 * find(3 + r, S.off_schedule[e]);
      }
    }
    pt.n_mput = (int)pm_all.size();
    pt.n_fput = (int)pf_all.size();
    for (int e = 0; e < kMaxEE; ++e) {   // dummy records
      pm_all.push_back(PhasePutOf<2, PhasePutM>(nullptr, (uint16_t)(8 * (8 + e)), find));
      pf_all.push_back(PhasePutOf<3, PhasePutF>(nullptr, (uint16_t)(8 * (8 + e)), find));
    }
    pt.o_mput = w.Put(pm_all);
    pt.o_fput = w.Put(pf_all);
    for (int r = 1; r < 6; ++r) pt.dyn_row_off[r - 1] = 8u * (uint32_t)(S.row_ptr[dyn->offset + r] - v0);
    if (S.params.polys_per_swing > 15 || S.params.polys_per_stance_force > 15)
      throw std::runtime_error("optimised timings: at most 15 polynomials per phase");
  }
  // the pattern builder and these closed forms must agree
  if (dyn && dyn->nnz != pt.node_vals * (int)S.grid_dyn.size()) throw std::runtime_error("dynamic row lengths inconsistent");
  for (int e = 0; e < S.n_ee && have_rom; ++e)
    if (rom[e]->nnz != pt.rom_node_vals[e] * (int)S.grid_rom.size())
      throw std::runtime_error("rangeofmotion row lengths inconsistent");
  return w.Put(&pt, sizeof(pt));
}

// trajectory sampling tables
uint32_t PutSampleTables(const Structure& S, BlobWriter& w) {
  SampleTables st;
  std::memset(&st, 0, sizeof(st));
  st.n_base = (int)S.base.durations.size();
  st.o_bdur = w.Put(S.base.durations);
  st.off_lin = S.off_base_lin;
  st.off_ang = S.off_base_ang;
  st.t_total = std::accumulate(S.base.durations.begin(), S.base.durations.end(), 0.0);  // spline.cc:118-123
  for (int e = 0; e < S.n_ee; ++e) {
    st.n_phases[e] = S.schedule.n_phases[e];
    st.contact0[e] = S.schedule.in_contact_at_start[e] != 0;
    st.n_mpoly[e] = (int)S.mpoly[e].size();
    st.n_fpoly[e] = (int)S.fpoly[e].size();
    st.o_phdur[e] = w.Put(S.schedule.phase_durations[e], S.schedule.n_phases[e] * sizeof(double));
    st.o_mdur[e] = w.Put(S.motion[e].durations);
    st.o_fdur[e] = w.Put(S.force[e].durations);
    st.o_mdesc[e] = w.Put(S.mpoly[e]);
    st.o_fdesc[e] = w.Put(S.fpoly[e]);
    if (st.n_mpoly[e] > kMaxPhasePolys || st.n_fpoly[e] > kMaxPhasePolys) st.n_base = -1;  // sampling unsupported
  }
  if (st.n_base > 2 * kMaxPhasePolys) st.n_base = -1;
  return w.Put(&st, sizeof(st));
}

// values-only evaluation of dynamic / rangeofmotion-* with one lane per time node (device_tables.h FlatNode): fixed
// timings only -- with optimised timings the active polynomials depend on x and the phase kernels keep that path
void PutFlatTables(Structure& S, BlobWriter& w, DevStruct& h) {
  const SetInfo* dyn = S.FindSet("dynamic");
  const bool have_rom = S.FindSet("rangeofmotion-0") != nullptr;
  S.flat_items_rom.clear();
  S.flat_items_dyn.clear();
  S.flat_with_rom = false;
  size_t n_flat_polys = 0;
  for (int e = 0; e < S.n_ee; ++e) n_flat_polys += S.mpoly[e].size() + S.fpoly[e].size();
  // x is staged in LDS (16-bit byte offsets); window starts are 16-bit indices
  if (S.timings || S.n_vars > kFlatXCap || n_flat_polys >= 65536 || !(have_rom || dyn)) return;
  S.flat_row_dyn = dyn ? dyn->offset : 0;
  std::vector<FlatPoly> fp;
  int first[2 * kMaxEE] = {0};   // spline s = 2 e (ee-motion_e), 2 e + 1 (ee-force_e): its first record in fp
  auto flat_polys = [&](int s, const std::vector<PolyDesc>& polys, const std::vector<double>& durations) {
    first[s] = (int)fp.size();
    const std::vector<double> t0 = StartTimes(durations);
    for (size_t q = 0; q < polys.size(); ++q) {
      FlatPoly r = {};
      r.t0 = t0[q];
      r.iT = polys[q].iT;
      const bool shared = (polys[q].meta >> 16) & 1;
      for (int c = 0; c < 12; ++c) {
        const int src = shared && c >= 6 && c < 9 ? c - 6 : c;   // stance: p1 is the same variable as p0
        const int sl = polys[q].cand[src] & 0xF;
        r.off[c] = (uint16_t)(sl != 0xF ? 8 * (2 + polys[q].xbase + sl) : 0);
      }
      fp.push_back(r);
    }
  };
  for (int e = 0; e < S.n_ee; ++e) {
    if (have_rom) S.flat_row_rom[e] = S.FindSet("rangeofmotion-" + std::to_string(e))->offset;
    flat_polys(2 * e, S.mpoly[e], S.motion[e].durations);
    flat_polys(2 * e + 1, S.fpoly[e], S.force[e].durations);
  }
  S.off_flat_polys = h.o_flat = w.Put(fp);
  // items: <= 64 consecutive time nodes whose active polynomials span <= kFlatWindow per spline.  On a COARSE grid (towr's
  // defaults: 0.1 / 0.08 s against polynomials of that length) the time nodes hardly share polynomials and the windows would
  // cut items of a few time nodes: such a grid is cut at 64 time nodes alone and its lanes fetch their own records
  // (FlatWork::gather; the indices stay relative to the item's first polynomials, 8 bits)
  auto flat_items = [&](const std::vector<double>& grid, const std::vector<TimeNode>& at_base, const std::vector<std::vector<TimeNode>>& at_motion,
                        const std::vector<std::vector<TimeNode>>* at_force, std::vector<Structure::FlatItem>& items) {
    auto poly_at = [&](int s, size_t k) { return (s & 1) ? (*at_force)[s >> 1][k].poly : at_motion[s >> 1][k].poly; };
    const int step = at_force ? 1 : 2;   // range of motion: the ee-motion splines only
    auto cut = [&](int window) {
      return CutRuns((int)grid.size(), [&](int k0, int k1) {
        if (k1 - k0 > 64) return false;
        for (int s = 0; s < 2 * S.n_ee; s += step)
          if (poly_at(s, k1 - 1) - poly_at(s, k0) >= window) return false;
        return true;
      });
    };
    std::vector<std::pair<int, int>> runs = cut(kFlatWindow);
    // (an item costs about the same whatever it holds, fetching the records per lane a quarter more: the windows stay while
    // they cut at most a quarter more items than 64 time nodes each would)
    const bool gather = 4 * runs.size() > 5 * ((grid.size() + 63) / 64);
    if (gather) runs = cut(256);
    std::vector<FlatNode> fn(grid.size());
    items.clear();
    for (const auto& r : runs) {
      const int k0 = r.first, k1 = r.first + r.second;
      Structure::FlatItem it;
      it.k0 = k0;
      it.cnt = r.second;
      it.gather = gather;
      for (int k = k0; k < k1; ++k) {
        fn[k].t = grid[k];
        std::tie(fn[k].tb, fn[k].iTb, fn[k].q6) = BaseAt(S.base, at_base[k]);
      }
      for (int s = 0; s < 2 * S.n_ee; s += step) {
        const int lo = poly_at(s, k0), hi = poly_at(s, k1 - 1);
        it.start[s >> 2] |= (uint64_t)(first[s] + lo) << (16 * (s & 3));
        it.count |= (uint64_t)(hi - lo + 1) << (8 * s);
        for (int k = k0; k < k1; ++k) ((s & 1) ? fn[k].qf[s >> 1] : fn[k].qm[s >> 1]) = (uint8_t)(poly_at(s, k) - lo);
      }
      items.push_back(it);
    }
    return w.Put(fn);
  };
  // coinciding grids (the BASELINE configurations choose one dt for both; towr's defaults are 0.1 / 0.08 s): the "dynamic"
  // items evaluate the range-of-motion rows of their time nodes as well -- same base point, rotation and ee positions
  S.flat_with_rom = have_rom && dyn && S.grid_rom == S.grid_dyn;
  if (have_rom && !S.flat_with_rom) S.off_flat_rom = flat_items(S.grid_rom, S.rom_base, S.rom_motion, nullptr, S.flat_items_rom);
  if (dyn) S.off_flat_dyn = flat_items(S.grid_dyn, S.dyn_base, S.dyn_motion, &S.dyn_force, S.flat_items_dyn);
}

// the header's grid fields and model constants
void SetHeader(const Structure& S, DevStruct& h) {
  if (S.model.terrain_id == TWR_TERRAIN_CSV_GRID || S.model.terrain_id == TWR_TERRAIN_GRID_MAP) {
    if (!S.grid) throw std::runtime_error("gridded terrains need twr_structure_create_with_grid");
    if (S.grid->grid_map != (S.model.terrain_id == TWR_TERRAIN_GRID_MAP))
      throw std::runtime_error("the grid handle is of the other kind (CSV heights vs grid_map elevation layer)");
    h.grid_rows = S.grid->rows;
    h.grid_cols = S.grid->cols;
    h.grid_res = S.grid->res;
    h.grid_eps = S.grid->eps;
    h.grid_px = S.grid->pos_x;
    h.grid_py = S.grid->pos_y;
  }
  h.n_ee = S.n_ee;
  h.terrain_id = S.model.terrain_id;
  h.off_base_ang = S.off_base_ang;
  h.inv_t_swing = 1.0 / 0.3;  // t_swing_avg_, swing_constraint.h:68
  h.mass = S.model.mass; h.gravity = S.model.gravity; h.mu = S.model.friction; h.flat_height = S.model.flat_height;
  // BuildInertiaTensor (single_rigid_body_dynamics.cc:36-44): off-diagonals are the negated products of inertia
  const double* I = S.model.inertia;  // Ixx,Iyy,Izz,Ixy,Ixz,Iyz
  h.Ib[0] = I[0]; h.Ib[1] = -I[3]; h.Ib[2] = -I[4]; h.Ib[3] = I[1]; h.Ib[4] = -I[5]; h.Ib[5] = I[2];
}

}  // namespace

// one builder per table group, called in the order the blob holds them
void Structure::PackBlob() {
  DevStruct h;
  std::memset(&h, 0, sizeof(h));
  BlobWriter w(dyn_layout_tables);
  const auto rows = FlatFamily(*this, "terrain-ee-motion_", 1, terrain_rows, h.row_terrain, h.nnz_terrain, h.n_terrain_rows);
  const auto forces = FlatFamily(*this, "force-ee-force_", 5, force_nodes, h.row_force, h.nnz_force, h.n_force_nodes);
  const auto swings = FlatFamily(*this, "swing-ee-motion_", 4, swing_nodes, h.row_swing, h.nnz_swing, h.n_swing_nodes);
  PutNodeHead(w, rows, forces);
  PutScoreRecord(*this, w, h);
  PutNodeFamilies(*this, w, h, rows, forces, swings);
  rom_slices.assign(n_ee, {});
  if (timings) {
    h.timings = 1;
    h.o_phase = PutPhaseTables(*this, w);
  } else {
    PutDynTables(*this, w);
    PutRomTables(*this, w);
  }
  h.o_sample = PutSampleTables(*this, w);
  PutFlatTables(*this, w, h);
  SetHeader(*this, h);
  blob = w.Finish(h);
}

const SetInfo* Structure::FindSet(const std::string& name) const {
  for (const SetInfo& s : con_sets)
    if (s.name == name) return &s;
  return nullptr;
}

void Structure::Build() {
  BuildVariables();
  BuildTimeTables();
  BuildPattern();
  PackBlob();
}
void Structure::BuildSizes() {
  BuildVariables();
  BuildTimeTables();
  BuildPattern();
}

// ------------------------------------------------------------------ terrain height (host, setup only)
// HeightMap::GetHeight of the example terrains (src/height_map_examples.cc:35-197,
// include/towr/terrain/examples/height_map_examples.h:45-166).
// HeightMapFromCSV::GetHeight (include/towr/terrain/height_map_from_csv.h:29-37).  static_cast<size_t>(x / res)
// truncates toward zero; a quotient <= -1 wraps to a huge size_t in the reference (formally undefined) and
// fails the range check -- here a signed cell index that is invalid when negative.
// Grid::GetHeight (include/towr/terrain/grid_height_map.h:29-46) over grid_map's published
// atPosition(INTER_LINEAR) (restated in the device code, kernels.hip gridmap_sample; this host copy serves the
// initial guess only): bilinear in double, rounded to float; nearest cell in the border band; FLT_MAX outside.
static float GridMapSample(const TerrainGrid& g, double x, double y) {
  const int sx = g.rows, sy = g.cols;
  const double res = g.res, lx = sx * res, ly = sy * res;
  auto in = [&](long i, long j) { return i >= 0 && j >= 0 && i < sx && j < sy; };
  auto at = [&](long i, long j) { return g.elevation[(size_t)i + (size_t)j * (size_t)sx]; };
  const long i0 = (long)(-((x - 0.5 * lx - g.pos_x) / res)), j0 = (long)(-((y - 0.5 * ly - g.pos_y) / res));
  const double tx = g.pos_x + 0.5 * lx - x, ty = g.pos_y + 0.5 * ly - y;
  const bool inside = tx >= 0.0 && ty >= 0.0 && tx < lx && ty < ly;
  const double cx0 = g.pos_x + 0.5 * lx - 0.5 * res - res * (double)i0, cy0 = g.pos_y + 0.5 * ly - 0.5 * res - res * (double)j0;
  const long ia = x >= cx0 ? i0 : i0 + 1, ja = y >= cy0 ? j0 : j0 + 1, ib = ia - 1, jb = ja - 1;
  if (in(ia, ja) && in(ib, jb)) {
    const double px = g.pos_x + 0.5 * lx - 0.5 * res - res * (double)ia, py = g.pos_y + 0.5 * ly - 0.5 * res - res * (double)ja;
    const double rx = (x - px) / res, ry = (y - py) / res, fx = 1.0 - rx, fy = 1.0 - ry;
    return (float)(at(ia, ja) * fx * fy + at(ib, ja) * rx * fy + at(ia, jb) * fx * ry + at(ib, jb) * rx * ry);
  }
  if (inside && in(i0, j0)) return at(i0, j0);
  return std::numeric_limits<float>::max();
}

double TerrainGrid::Height(double x, double y) const {
  if (grid_map) return GridMapSample(*this, x, y);
  const long xc = (long)(x / res), yc = (long)(y / res);
  if (xc < 0 || yc < 0 || xc >= cols || yc >= rows) return 0.0;
  return heights[(size_t)yc * cols + xc];
}

double TerrainHeightHost(const twr_model& m, const TerrainGrid* grid, double x, double y) {
  switch (m.terrain_id) {
    case TWR_TERRAIN_CSV_GRID:
    case TWR_TERRAIN_GRID_MAP:
      if (!grid) throw std::runtime_error("gridded terrain without a grid");
      return grid->Height(x, y);
    case TWR_TERRAIN_FLAT: return m.flat_height;
    case TWR_TERRAIN_BLOCK: {
      const double start = 0.7, len = 3.5, height = 0.5, eps = 0.03, slope = height / eps;
      double h = 0.0;
      if (start <= x && x <= start + eps) h = slope * (x - start);
      if (start + eps <= x && x <= start + len) h = height;
      return h;
    }
    case TWR_TERRAIN_STAIRS: {
      double h = 0.0;
      if (x >= 1.0) h = 0.2;
      if (x >= 1.0 + 0.4) h = 0.4;
      if (x >= 1.0 + 0.4 + 1.0) h = 0.0;
      return h;
    }
    case TWR_TERRAIN_GAP: {
      const double gs = 1.0, w = 0.5, hh = 1.5, xc = gs + w / 2.0, ge = gs + w;
      const double a = (4 * hh) / (w * w), b = -(8 * hh * xc) / (w * w), c = -(hh * (w - 2 * xc) * (w + 2 * xc)) / (w * w);
      return (gs <= x && x <= ge) ? a * x * x + b * x + c : 0.0;
    }
    case TWR_TERRAIN_SLOPE: {
      const double ss = 1.0, up = 1.0, dn = 1.0, hc = 0.7, xd = ss + up, xf = xd + dn, sl = hc / up;
      double z = 0.0;
      if (x >= ss) z = sl * (x - ss);
      if (x >= xd) z = hc - sl * (x - xd);
      if (x >= xf) z = 0.0;
      return z;
    }
    case TWR_TERRAIN_CHIMNEY: {
      const double xs = 1.0, len = 1.5, ys = 0.5, sl = 3.0;
      return (xs <= x && x <= xs + len) ? sl * (y - ys) : 0.0;
    }
    case TWR_TERRAIN_CHIMNEY_LR: {
      const double xs = 0.5, len = 1.0, ys = 0.5, sl = 2, xe1 = xs + len, xe2 = xs + 2 * len;
      double z = 0.0;
      if (xs <= x && x <= xe1) z = sl * (y - ys);
      if (xe1 <= x && x <= xe2) z = -sl * (y + ys);
      return z;
    }
  }
  throw std::runtime_error("unknown terrain id");
}

// ------------------------------------------------------------------ initial guess
// NlpFormulation::Make{Base,Endeffector,Force}Variables (src/nlp_formulation.cc:95-181) with
// NodesVariables::SetByLinearInterpolation + GetValues (src/nodes_variables.cc:52-62,126-150):
// a variable shared by two nodes ends up with the value written for the later node.
void Structure::InitialGuess(const double* lin0, const double* ang0, const double* lin1, const double* ang1,
                             const double* ee0, double* x) const {
  auto interpolate = [&](const SplineLayout& s, int var_off_delta, const double* a, const double* b) {
    double dp[3], vel[3];
    for (int d = 0; d < 3; ++d) {
      dp[d] = b[d] - a[d];
      vel[d] = dp[d] / T;
    }
    for (int n = 0; n < s.n_nodes; ++n)
      for (int d = 0; d < 3; ++d) {
        int ip = s.at(n, 0, d), iv = s.at(n, 1, d);
        if (ip >= 0) x[ip + var_off_delta] = a[d] + n / static_cast<double>(s.n_nodes - 1) * dp[d];
        if (iv >= 0) x[iv + var_off_delta] = vel[d];
      }
  };
  for (int i = 0; i < n_vars; ++i) x[i] = 0.0;
  double fl[3] = {lin1[0], lin1[1], TerrainHeightHost(model, grid.get(), lin1[0], lin1[1]) - model.nominal_stance[0][2]};
  interpolate(base, off_base_lin, lin0, fl);
  interpolate(base, off_base_ang, ang0, ang1);
  for (int e = 0; e < n_ee; ++e) {
    double yaw = ang1[2];
    // GetRotationMatrixBaseToWorld((0,0,yaw)) * nominal stance (nlp_formulation.cc:141-148)
    double cz = std::cos(yaw), sz = std::sin(yaw), c0 = std::cos(0.0), s0 = std::sin(0.0);
    const double* nb = model.nominal_stance[e];
    double R[3][3] = {{c0 * cz, cz * s0 * s0 - c0 * sz, s0 * sz + c0 * cz * s0},
                      {c0 * sz, c0 * cz + s0 * s0 * sz, c0 * s0 * sz - cz * s0},
                      {-s0, c0 * s0, c0 * c0}};
    double fe[3];
    for (int i = 0; i < 3; ++i) fe[i] = lin1[i] + (R[i][0] * nb[0] + R[i][1] * nb[1] + R[i][2] * nb[2]);
    fe[2] = TerrainHeightHost(model, grid.get(), fe[0], fe[1]);
    interpolate(motion[e], 0, ee0 + 3 * e, fe);
  }
  for (int e = 0; e < n_ee; ++e) {
    double f[3] = {0.0, 0.0, model.mass * model.gravity / n_ee};
    interpolate(force[e], 0, f, f);
  }
  if (timings)  // PhaseDurations::GetValues (src/phase_durations.cc:66-75): the given durations but the last
    for (int e = 0; e < n_ee; ++e)
      for (int i = 0; i < schedule.n_phases[e] - 1; ++i) x[off_schedule[e] + i] = schedule.phase_durations[e][i];
}

// ------------------------------------------------------------------ trajectory sampling
// fpowr::GetTrajectory (fpowr/include/fpowr/footstep_plan_extractor.h:19-53): `while (t <= T + 1e-5) { ...; t += dt; }`
int SampleCount(double t_total, double dt) {
  if (!(dt > 0)) throw std::runtime_error("dt must be positive");
  int n = 0;
  for (double t = 0.0; t <= t_total + 1e-5; t += dt)
    if (++n > 10000000) throw std::runtime_error("too many samples");
  return n;
}
int Structure::SampleCount(double dt) const {
  return twr::SampleCount(std::accumulate(base.durations.begin(), base.durations.end(), 0.0), dt);
}

// ------------------------------------------------------------------ variable bounds
// NodesVariables::AddStartBound / AddFinalBound as called by NlpFormulation::MakeBaseVariables and
// MakeEndeffectorVariables (src/nlp_formulation.cc:109-122,151; src/nodes_variables.cc:152-181) with the
// bounded dimensions of src/parameters.cc:65-69.  A bound on a node value that is not an optimisation
// variable is silently dropped (AddBound only scans existing variables).
void Structure::VariableBounds(const double* init_base, const double* final_base, const double* ee0, double* lower,
                               double* upper) const {
  const double inf = 1e20;  // ifopt::NoBound
  for (int i = 0; i < n_vars; ++i) {
    lower[i] = -inf;
    upper[i] = inf;
  }
  auto fix = [&](const SplineLayout& s, int delta, int node, int deriv, int dim, double val) {
    int i = s.at(node, deriv, dim);
    if (i >= 0) lower[i + delta] = upper[i + delta] = val;
  };
  const int last = base.n_nodes - 1;
  for (int d = 0; d < 3; ++d) {
    fix(base, off_base_lin, 0, 0, d, init_base[d]);
    fix(base, off_base_lin, 0, 1, d, init_base[3 + d]);
    if (d != 2) fix(base, off_base_lin, last, 0, d, final_base[d]);  // bounds_final_lin_pos_ = {X,Y}
    fix(base, off_base_lin, last, 1, d, final_base[3 + d]);
    fix(base, off_base_ang, 0, 0, d, init_base[6 + d]);
    fix(base, off_base_ang, 0, 1, d, init_base[9 + d]);
    fix(base, off_base_ang, last, 0, d, final_base[6 + d]);
    fix(base, off_base_ang, last, 1, d, final_base[9 + d]);
    for (int e = 0; e < n_ee; ++e) fix(motion[e], 0, 0, 0, d, ee0[3 * e + d]);
  }
  if (timings)  // PhaseDurations::GetBounds with Parameters::bound_phase_duration_ (parameters.cc:52)
    for (int e = 0; e < n_ee; ++e)
      for (int i = 0; i < schedule.n_phases[e] - 1; ++i) {
        lower[off_schedule[e] + i] = 0.2;
        upper[off_schedule[e] + i] = 1.0;
      }
}

// ------------------------------------------------------------------ presets
// RobotModel(Robot) (src/robot_model.cc:41-68) with the constants of
// include/towr/models/examples/{monoped,biped,hyq,anymal}_model.h and models/go1/go1_model.h.
void ModelPreset(int robot, int terrain, twr_model* m) {
  std::memset(m, 0, sizeof(*m));
  auto quad = [&](double xn, double yn, double zn) {
    double s[4][3] = {{xn, yn, zn}, {xn, -yn, zn}, {-xn, yn, zn}, {-xn, -yn, zn}};  // LF RF LH RH
    std::memcpy(m->nominal_stance, s, sizeof(s));
  };
  auto set = [&](int n_ee, double mass, double ixx, double iyy, double izz, double ixy, double ixz, double iyz,
                 double dx, double dy, double dz) {
    m->n_ee = n_ee;
    m->mass = mass;
    double I[6] = {ixx, iyy, izz, ixy, ixz, iyz};
    std::memcpy(m->inertia, I, sizeof(I));
    m->max_dev[0] = dx; m->max_dev[1] = dy; m->max_dev[2] = dz;
  };
  switch (robot) {
    case TWR_ROBOT_MONOPED:
      set(1, 20, 1.2, 5.5, 6.0, 0.0, -0.2, -0.01, 0.25, 0.15, 0.2);
      m->nominal_stance[0][2] = -0.58;
      break;
    case TWR_ROBOT_BIPED:
      set(2, 20, 1.209, 5.583, 6.056, 0.005, -0.190, -0.012, 0.25, 0.15, 0.15);
      m->nominal_stance[0][1] = 0.20;  m->nominal_stance[0][2] = -0.65;
      m->nominal_stance[1][1] = -0.20; m->nominal_stance[1][2] = -0.65;
      break;
    case TWR_ROBOT_HYQ:
      set(4, 83, 4.26, 8.97, 9.88, -0.0063, 0.193, 0.0126, 0.25, 0.20, 0.10);
      quad(0.31, 0.29, -0.58);
      break;
    case TWR_ROBOT_ANYMAL:
      set(4, 29.5, 0.946438, 1.94478, 2.01835, 0.000938112, -0.00595386, -0.00146328, 0.15, 0.1, 0.10);
      quad(0.34, 0.19, -0.42);
      break;
    case TWR_ROBOT_GO1:
      set(4, 12.84, 0.0168128557, 0.063009565, 0.0716547275, -0.0002296769, -0.0002945293, -0.0000418731, 0.16, 0.12, 0.06);
      quad(0.1881, 0.04675 + 0.08, -0.3);
      break;
    default: throw std::runtime_error("unknown robot id");
  }
  if (terrain < TWR_TERRAIN_FLAT || terrain > TWR_TERRAIN_GRID_MAP) throw std::runtime_error("unknown terrain id");
  m->terrain_id = terrain;
  m->gravity = 9.80665;     // dynamic_model.cc:37
  m->friction = 0.5;        // height_map.h:136
  m->force_limit = 1000.0;  // parameters.cc:48
  m->flat_height = 0.0;
}

// ------------------------------------------------------------------ gait generator
namespace {
struct Stride {
  std::vector<double> times;
  std::vector<unsigned> contacts;  // bit e set = ee e in contact
};
enum G { Stand = 0, Flight, Walk1, Walk2, Walk2E, Run2, Run2E, Run1, Run1E, Run3, Run3E, Hop1, Hop1E, Hop2, Hop3, Hop3E, Hop5, Hop5E };

Stride DropTransition(Stride s) {  // GaitGenerator::RemoveTransition (gait_generator.cc:131-144)
  double last = s.times.back();
  s.times.pop_back();
  s.times.back() += last;
  s.contacts.pop_back();
  return s;
}
// quadruped contact states, ee bits LF=1 RF=2 LH=4 RH=8 (quadruped_gait_generator.cc:39-74)
constexpr unsigned II = 0, PI = 4, bI = 8, IP = 1, Ib = 2, Pb = 4 | 2, bP = 8 | 1, BI = 12, IB = 3, PP = 4 | 1, bb = 8 | 2,
                   Bb = 12 | 2, BP = 12 | 1, bB = 8 | 3, PB = 4 | 3, BB = 15;
Stride QuadStride(int g) {  // quadruped_gait_generator.cc:89-366
  switch (g) {
    case Stand: return {{0.3}, {BB}};
    case Flight: return {{0.3}, {Bb}};
    case Walk1: return {{0.3, 0.2, 0.3, 0.2, 0.3, 0.2, 0.3, 0.2}, {bB, BB, Bb, BB, PB, BB, BP, BB}};
    case Walk2: return {{0.25, 0.13, 0.25, 0.13, 0.25, 0.13, 0.25, 0.13}, {bB, bb, Bb, Pb, PB, PP, BP, bP}};
    case Walk2E: return DropTransition(QuadStride(Walk2));
    case Run1: return {{0.3, 0.2, 0.3, 0.2}, {bP, BB, Pb, BB}};
    case Run2: return {{0.4, 0.1, 0.4, 0.1}, {bP, II, Pb, II}};
    case Run2E: return {{0.4}, {bP}};
    case Run3: return {{0.3, 0.1, 0.3, 0.1}, {PP, II, bb, II}};
    case Run3E: return {{0.3}, {PP}};
    case Hop1: return {{0.3, 0.1, 0.3, 0.1}, {BI, II, IB, II}};
    case Hop1E: return {{0.3}, {BI}};
    case Hop2: return {{0.3, 0.4, 0.3}, {BB, II, BB}};
    case Hop3: return {{0.2, 0.3, 0.2, 0.2, 0.2, 0.3, 0.2, 0.2}, {Bb, BI, BP, bP, bB, IB, PB, Pb}};
    case Hop3E: return DropTransition(QuadStride(Hop3));
    case Hop5: return {{0.1, 0.2, 0.1, 0.1, 0.2, 0.1}, {Bb, BB, IP, Bb, BB, IP}};
  }
  throw std::runtime_error("quadruped gait not implemented");
}
Stride BipedStride(int g) {  // biped_gait_generator.cc:64-226, bits L=1 R=2
  const unsigned I = 0, P = 1, b = 2, B = 3;
  switch (g) {
    case Stand: return {{0.2}, {B}};
    case Flight: return {{0.5}, {I}};
    case Walk1: case Walk2: return {{0.3, 0.05, 0.3, 0.05}, {b, B, P, B}};
    case Run1: case Run3: return {{0.15, 0.4, 0.15 + 0.15, 0.4, 0.15}, {b, I, P, I, b}};
    case Hop1: return {{0.15, 0.5, 0.15}, {B, I, B}};
    case Hop2: return {{0.15, 0.4, 0.15}, {b, I, b}};
    case Hop3: return {{0.2, 0.2, 0.2}, {P, I, P}};
    case Hop5: return {{0.2, 0.3, 0.2, 0.2}, {P, I, b, B}};
  }
  throw std::runtime_error("biped gait not implemented");
}
Stride MonoStride(int g) {  // monoped_gait_generator.cc:50-120
  switch (g) {
    case Stand: return {{0.5}, {1}};
    case Flight: return {{0.5}, {0}};
    case Hop1: return {{0.3, 0.3}, {1, 0}};
    case Hop2: return {{0.2, 0.3}, {1, 0}};
  }
  throw std::runtime_error("monoped gait not implemented");
}
std::vector<int> ComboGaits(int n_ee, int combo) {
  static const std::vector<int> quad[5] = {{Stand, Walk2, Walk2, Walk2, Walk2E, Stand},   // quadruped_gait_generator.cc:76-87
                                           {Stand, Run2, Run2, Run2, Run2E, Stand},
                                           {Stand, Run3, Run3, Run3, Run3E, Stand},
                                           {Stand, Hop1, Hop1, Hop1, Hop1E, Stand},
                                           {Stand, Hop3, Hop3, Hop3, Hop3E, Stand}};
  static const std::vector<int> biped[5] = {{Stand, Walk1, Walk1, Walk1, Walk1, Stand},   // biped_gait_generator.cc:51-62
                                            {Stand, Run1, Run1, Run1, Run1, Stand},
                                            {Stand, Hop1, Hop1, Hop1, Stand},
                                            {Stand, Hop1, Hop2, Hop2, Stand},
                                            {Stand, Hop5, Hop5, Hop5, Stand}};
  static const std::vector<int> mono[5] = {{Stand, Hop1, Hop1, Hop1, Hop1, Stand},        // monoped_gait_generator.cc:37-48
                                           {Stand, Hop1, Hop1, Hop1, Stand},
                                           {Stand, Hop1, Hop1, Hop1, Hop1, Stand},
                                           {Stand, Hop2, Hop2, Hop2, Stand},
                                           {Stand, Hop2, Hop2, Hop2, Hop2, Hop2, Stand}};
  if (combo < 0 || combo > 4) throw std::runtime_error("combo must be 0..4");
  if (n_ee == 1) return mono[combo];
  if (n_ee == 2) return biped[combo];
  if (n_ee == 4) return quad[combo];
  throw std::runtime_error("no gait generator for this leg count");  // gait_generator.cc:43-52
}
}  // namespace

void GaitCombo(int n_ee, int combo, double t_total, double swing_scale, twr_schedule* out) {
  std::vector<double> times;
  std::vector<unsigned> contacts;
  for (int g : ComboGaits(n_ee, combo)) {  // SetGaits (gait_generator.cc:113-129)
    Stride s = n_ee == 1 ? MonoStride(g) : n_ee == 2 ? BipedStride(g) : QuadStride(g);
    times.insert(times.end(), s.times.begin(), s.times.end());
    contacts.insert(contacts.end(), s.contacts.begin(), s.contacts.end());
  }
  const unsigned all = (1u << n_ee) - 1;
  for (size_t i = 0; i < times.size(); ++i)
    if (contacts[i] != all) times[i] *= swing_scale;  // candidate enumeration knob (1.0 = reference)
  std::memset(out, 0, sizeof(*out));
  out->n_ee = n_ee;
  // GetPhaseDurations() (gait_generator.cc:76-105)
  std::vector<std::vector<double>> foot(n_ee);
  std::vector<double> acc(n_ee, 0.0);
  for (size_t ph = 0; ph + 1 < contacts.size(); ++ph)
    for (int e = 0; e < n_ee; ++e) {
      acc[e] += times[ph];
      bool cur = (contacts[ph] >> e) & 1, nxt = (contacts[ph + 1] >> e) & 1;
      if (cur != nxt) {
        foot[e].push_back(acc[e]);
        acc[e] = 0.0;
      }
    }
  for (int e = 0; e < n_ee; ++e) foot[e].push_back(acc[e] + times.back());
  for (int e = 0; e < n_ee; ++e) {
    if (foot[e].size() > TWR_MAX_PHASES) throw std::runtime_error("too many phases");
    // GetNormalizedPhaseDurations + GetPhaseDurations(T, ee) (gait_generator.cc:54-74)
    double total = std::accumulate(foot[e].begin(), foot[e].end(), 0.0);
    out->n_phases[e] = (int)foot[e].size();
    out->in_contact_at_start[e] = (contacts.front() >> e) & 1;  // IsInContactAtStart :107-111
    for (size_t i = 0; i < foot[e].size(); ++i) out->phase_durations[e][i] = (foot[e][i] / total) * t_total;
  }
}

LayoutShare ShareLayoutTables(const std::vector<const Structure*>& structs) {
  struct Seen {
    const char* bytes;
    uint32_t n;
    LayoutShare::Ref ref;
  };
  auto hash = [](const char* p, size_t n) {   // FNV-1a over 8-byte words (a bucket key only: equality is decided by memcmp)
    uint64_t h = 1469598103934665603ull;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      std::memcpy(&w, p + i, 8);
      h = (h ^ w) * 1099511628211ull;
      h ^= h >> 29;
    }
    for (; i < n; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
    return h;
  };
  LayoutShare out;
  out.of.resize(structs.size());
  std::unordered_map<uint64_t, std::vector<Seen>> by_hash;
  for (size_t i = 0; i < structs.size(); ++i) {
    const Structure& S = *structs[i];
    for (const Structure::TableRef& tr : S.dyn_layout_tables) {
      if ((size_t)tr.off + tr.bytes > S.blob.size()) throw std::runtime_error("layout table outside its blob");
      const char* src = S.blob.data() + tr.off;
      std::vector<Seen>& bucket = by_hash[hash(src, tr.bytes) ^ tr.bytes];
      LayoutShare::Ref ref{(int)i, tr.off};
      bool found = false;
      for (const Seen& sn : bucket)
        if (sn.n == tr.bytes && std::memcmp(sn.bytes, src, tr.bytes) == 0) {
          ref = sn.ref;
          found = true;
          break;
        }
      if (!found) {
        bucket.push_back({src, tr.bytes, ref});
        out.bytes_distinct += tr.bytes;
      }
      out.bytes_built += tr.bytes;
      out.of[i].push_back(ref);
    }
  }
  return out;
}

std::vector<size_t> BlobOffsets(const std::vector<const Structure*>& structs) {
  std::vector<size_t> off(structs.size() + 1, 0);
  for (size_t i = 0; i < structs.size(); ++i) off[i + 1] = off[i] + (structs[i]->blob.size() + 255) / 256 * 256;
  return off;
}

namespace {
// XCD-aware order.  Workgroups are dealt round-robin over the 8 XCDs and the persistent grids are multiples of 8, so list
// position j runs on XCD j % 8 (eval_fused_kernel's slice mapping relies on it, kernels.hip).  Interleaving the problems in
// groups of 8 puts all items of one problem on ONE XCD (same L2): its x is fetched from HBM once per kernel instead of once
// per XCD.  (Speed only; ragged item counts merely loosen the alignment.)  first: first item of every problem (+ end).
template <class W>
void Interleave(std::vector<W>& items, const std::vector<int>& first) {
  const std::vector<W> src = items;
  const int n = (int)first.size() - 1;
  size_t out = 0;
  for (int p0 = 0; p0 < n; p0 += 8) {
    const int np = std::min(8, n - p0);
    for (int s = 0;; ++s) {
      bool any = false;
      for (int k = 0; k < np; ++k)
        if (first[p0 + k] + s < first[p0 + k + 1]) {
          items[out++] = src[first[p0 + k] + s];
          any = true;
        }
      if (!any) break;
    }
  }
}
}  // namespace

void BatchPlan::PlaceRecords(uint64_t base) {
  for (auto& lw : lists.ploc) {
    if (lw.recs) lw.recs += base - 1;
    if (lw.dyn_loc) lw.dyn_loc += base - 1;
  }
  for (auto& rw : lists.prom) rw.recs += base;
  for (auto& pw : lists.pdyn) pw.loc += base;
}

BatchPlan PlanBatch(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem,
                    const std::vector<uint64_t>& blob_at, int n_cu, int64_t cache_bytes, int force_chunk) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  BatchPlan b;
  BatchPlan::Lists& L = b.lists;
  // Layout tables of dyn_kernel (device_tables.h) are stored once per distinct CONTENT: a structure whose table is
  // byte-identical to one of an earlier structure of the batch reads that one (its own copy stays in the arena, unread).
  // Candidates of a sweep that differ in the total time only share all of them, and an evaluation then reads 24 B per
  // time node + 16 B per polynomial of such a candidate instead of ~35 KB.  The model constants (DevStruct header) are
  // taken from the first structure of the batch that has the same ones.
  std::vector<std::unordered_map<uint32_t, uint64_t>> layout_at(n_structs);   // [structure][blob offset of the table] -> device address
  std::vector<uint64_t> model_hdr(n_structs);
  const LayoutShare share = ShareLayoutTables(structs);
  b.dyn_layout_bytes = share.bytes_built;
  b.dyn_layout_distinct_bytes = share.bytes_distinct;
  for (int i = 0; i < n_structs; ++i) {
    const auto& tabs = structs[i]->dyn_layout_tables;
    for (size_t t = 0; t < tabs.size(); ++t) layout_at[i][tabs[t].off] = blob_at[share.of[i][t].owner] + share.of[i][t].off;
    const DevStruct* H = reinterpret_cast<const DevStruct*>(structs[i]->blob.data());
    model_hdr[i] = blob_at[i];
    for (int q = 0; q < i; ++q) {
      const DevStruct* Q = reinterpret_cast<const DevStruct*>(structs[q]->blob.data());
      if (model_hdr[q] == blob_at[q] && Q->mass == H->mass && Q->gravity == H->gravity && std::memcmp(Q->Ib, H->Ib, sizeof(H->Ib)) == 0) {
        model_hdr[i] = model_hdr[q];
        break;
      }
    }
    if (structs[i]->dyn_staged_max > 128) b.dyn_map_chunks = 4;
  }
  b.x_off.assign(n_problems + 1, 0);
  b.g_off.assign(n_problems + 1, 0);
  b.j_off.assign(n_problems + 1, 0);
  std::vector<int> flat_group_p;             // the problem of every group of four flat items
  bool flat_ok = true;
  std::vector<int> dyn_first, rom_first, pdyn_first;   // first work item of every problem (+ end; pdyn: optimised timings only)
  // (families that are switched off -- twr_params.constraint_sets -- simply have no work items; problems with
  // optimised timings get PDynWork / LocWork / RomPhaseWork items instead of DynWork / RomWork)
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    const Structure& S = *structs[si];
    const DevStruct* H = reinterpret_cast<const DevStruct*>(S.blob.data());
    const uint64_t blob = blob_at[si];
    const SampleTables* st = reinterpret_cast<const SampleTables*>(S.blob.data() + H->o_sample);
    b.blob_of_problem.push_back(blob);
    b.t_total.push_back(st->t_total);
    b.sample_ok.push_back(st->n_base >= 0);
    b.x_off[p + 1] = b.x_off[p] + S.n_vars;
    b.g_off[p + 1] = b.g_off[p] + S.n_rows;
    b.j_off[p + 1] = b.j_off[p] + S.nnz;
    dyn_first.push_back((int)L.dyn.size());
    rom_first.push_back((int)L.rom.size());
    const SetInfo* dsp = S.FindSet("dynamic");
    const SetInfo ds = dsp ? *dsp : SetInfo();
    for (const auto& sl : S.dyn_slices) {   // fixed timings only (empty otherwise)
      DynWork w;
      std::memset(&w, 0, sizeof(w));
      const auto& lay = layout_at[si];
      w.nodes_t = blob + S.off_dyn_nodes_t + sizeof(DynNodeT) * (size_t)sl.k0;
      w.nodes_l = lay.at(S.off_dyn_nodes_l) + sizeof(DynNodeL) * (size_t)sl.k0;
      w.sel = lay.at(S.off_dyn_sel) + sizeof(DynSel) * (size_t)sl.k0 * 4;
      w.tile = lay.at(S.off_dyn_tile);   // (records are addressed through DynSel::tile)
      w.poly_t = blob + S.off_dyn_poly_t + sizeof(DynPolyT) * (size_t)sl.poly0;
      w.poly_l = lay.at(S.off_dyn_poly_l) + sizeof(DynPolyL) * (size_t)sl.poly0;
      w.map = lay.at(b.dyn_map_chunks == 2 ? sl.map2 : sl.map);
      w.hdr = model_hdr[si];
      w.x_off = b.x_off[p];
      w.g_off = b.g_off[p] + ds.offset + 6 * sl.k0;
      w.j_off = b.j_off[p] + S.row_ptr[ds.offset + 6 * sl.k0];
      w.cnt = sl.cnt;
      w.nvals = sl.nvals;
      L.dyn.push_back(w);
    }
    for (int e = 0; e < (int)S.rom_slices.size(); ++e) {   // fixed timings only (empty otherwise)
      if (S.rom_slices[e].empty()) continue;
      const SetInfo& rs = *S.FindSet("rangeofmotion-" + std::to_string(e));
      for (const auto& sl : S.rom_slices[e]) {
        RomWork w;
        std::memset(&w, 0, sizeof(w));
        w.nodes = blob + S.off_rom_nodes + sizeof(RomNode) * (size_t)sl.k0;
        w.segs = blob + sl.segs;
        w.x_off = b.x_off[p];
        w.g_off = b.g_off[p] + rs.offset + 3 * sl.k0;
        w.j_off = b.j_off[p] + S.row_ptr[rs.offset + 3 * sl.k0];
        w.off_lin = S.off_base_lin;
        w.off_ang = S.off_base_ang;
        w.cnt = sl.cnt;
        w.nvals = sl.nvals;
        w.ee = e;
        b.rom_max_vals = std::max(b.rom_max_vals, w.nvals);
        L.rom.push_back(w);
      }
    }
    if (S.timings) {
      const int Kd = (int)S.grid_dyn.size();
      const size_t loc_off = b.records_bytes;   // DynLoc[4 * Kd] of this problem, then its RomRec arrays
      const PhaseTables& pt = S.phase_tables;
      if (dsp) {
        // dyn_phase_kernel: a pass = the time nodes whose expanded rows fit the LDS image (four at sixteen lanes each,
        // fewer when a node has more than 5120 values: the image then takes the whole 160 KB of a CU)
        b.records_bytes += sizeof(DynLoc) * 4 * (size_t)Kd;
        const int nv = pt.node_vals;
        const int run = std::max(1, std::min(4, (160 * 128) / nv));
        b.pdyn_img_cap = std::max(b.pdyn_img_cap, run * nv);
        pdyn_first.push_back((int)L.pdyn.size());
        for (int k0 = 0; k0 < Kd; k0 += run) {
          PDynWork pw;
          std::memset(&pw, 0, sizeof(pw));
          pw.hdr = blob;
          pw.loc = loc_off + sizeof(DynLoc) * (size_t)k0;
          pw.loc_stride = (int32_t)(sizeof(DynLoc) * (size_t)Kd);
          pw.shared = blob + pt.o_dyn_shared + sizeof(DynShared) * (size_t)k0;
          pw.mput = blob + pt.o_mput;
          pw.fput = blob + pt.o_fput;
          pw.ee = blob + H->o_phase + offsetof(PhaseTables, ee);
          pw.x_off = b.x_off[p];
          pw.g_off = b.g_off[p] + dsp->offset + 6 * k0;
          pw.j_off = b.j_off[p] + dsp->nnz_offset + (int64_t)k0 * nv;
          pw.cnt = std::min(run, Kd - k0);
          pw.node_vals = nv;
          pw.off_lin = S.off_base_lin;
          pw.off_ang = S.off_base_ang;
          pw.n_ee = S.n_ee;
          pw.n_mput = pt.n_mput;
          pw.n_fput = pt.n_fput;
          for (int q = 0; q < 5; ++q) pw.row_off[q] = pt.dyn_row_off[q];
          L.pdyn.push_back(pw);
        }
      }
      for (int e = 0; e < S.n_ee; ++e) {
        const SetInfo* rs = S.FindSet("rangeofmotion-" + std::to_string(e));
        if (!rs && !dsp) continue;
        LocWork lw;
        std::memset(&lw, 0, sizeof(lw));
        lw.blob = blob;
        lw.recs = rs ? b.records_bytes + 1 : 0;   // (+1: see BatchPlan::records_bytes)
        lw.dyn_loc = dsp ? loc_off + sizeof(DynLoc) * (size_t)Kd * (size_t)e + 1 : 0;
        lw.x_off = b.x_off[p];
        lw.ee = e;
        L.ploc.push_back(lw);
        if (!rs) continue;
        const int K = (int)S.grid_rom.size(), nv = pt.rom_node_vals[e];
        const int run_max = std::max(1, std::min(16, (160 * 128) / nv));   // time nodes per pass (four lanes each)
        const int n_pass = (K + run_max - 1) / run_max;
        const int run = (K + n_pass - 1) / n_pass;                  // balanced: no short tail pass (it pays the full copy-out)
        b.prom_img_cap = std::max(b.prom_img_cap, run * nv);
        for (int k0 = 0; k0 < K; k0 += run) {
          RomPhaseWork rw;
          rw.recs = b.records_bytes + sizeof(RomRec) * (size_t)k0;
          rw.x_off = b.x_off[p];
          rw.g_off = b.g_off[p] + rs->offset + 3 * k0;
          rw.j_off = b.j_off[p] + rs->nnz_offset + (int64_t)k0 * nv;
          rw.off_lin = S.off_base_lin;
          rw.off_ang = S.off_base_ang;
          rw.cnt = std::min(run, K - k0);
          rw.msize = pt.msize[e];
          rw.ns = S.schedule.n_phases[e] - 1;
          rw.node_vals = nv;
          L.prom.push_back(rw);
        }
        b.records_bytes += sizeof(RomRec) * (size_t)K;
      }
    }
    // values-only work items (device_tables.h FlatWork): 64 time nodes of the dynamic / range-of-motion grid each
    if (S.timings) flat_ok = false;
    if (S.off_flat_polys) {
      auto items = [&](uint32_t off_nodes, const std::vector<Structure::FlatItem>& list, bool dynamic) {
        for (const auto& it : list) {
          FlatWork fw;
          std::memset(&fw, 0, sizeof(fw));
          fw.nodes = blob + off_nodes + sizeof(FlatNode) * (size_t)it.k0;
          fw.polys = blob + S.off_flat_polys;
          fw.x_off = b.x_off[p];
          fw.g_off = b.g_off[p];
          fw.k0 = it.k0;
          fw.cnt = it.cnt;
          fw.start[0] = it.start[0];
          fw.start[1] = it.start[1];
          fw.count = it.count;
          fw.n_x = S.n_vars;
          fw.n_ee = S.n_ee;
          fw.off_lin = S.off_base_lin;
          fw.off_ang = S.off_base_ang;
          for (int e = 0; e < kMaxEE; ++e) fw.row_rom[e] = S.flat_row_rom[e];
          fw.dynamic = dynamic ? 1 : 0;
          fw.gather = it.gather ? 1 : 0;
          if (dynamic) {
            fw.row_dyn = S.flat_row_dyn;
            fw.with_rom = S.flat_with_rom ? 1 : 0;
            fw.mass = H->mass;
            fw.gravity = H->gravity;
            for (int i = 0; i < 6; ++i) fw.Ib[i] = H->Ib[i];
          }
          L.flat.push_back(fw);
        }
      };
      b.flat_max_x = std::max(b.flat_max_x, S.n_vars);
      items(S.off_flat_dyn, S.flat_items_dyn, true);
      items(S.off_flat_rom, S.flat_items_rom, false);
      while (L.flat.size() % 4 != 0) {   // whole groups: empty items that still carry the problem's x (the group copies it
        FlatWork fw;                     // to LDS with all its threads)
        std::memset(&fw, 0, sizeof(fw));
        fw.x_off = b.x_off[p];
        fw.n_x = S.n_vars;
        L.flat.push_back(fw);
      }
      flat_group_p.resize(L.flat.size() / 4, p);
    } else if (S.FindSet("rangeofmotion-0") || dsp) {
      flat_ok = false;
    }
    NodeWork nw;
    nw.blob = blob;
    nw.x_off = b.x_off[p];
    nw.g_off = b.g_off[p];
    nw.j_off = b.j_off[p];
    L.node.push_back(nw);
  }
  // one entry past the end carries the totals: a kernel reads a problem's row count as work[p + 1].g_off - work[p].g_off
  // from the work list alone (score_kernel requests g before the structure's header has arrived)
  L.node.push_back(NodeWork{0, b.x_off[n_problems], b.g_off[n_problems], b.j_off[n_problems]});
  dyn_first.push_back((int)L.dyn.size());
  rom_first.push_back((int)L.rom.size());
  pdyn_first.push_back((int)L.pdyn.size());
  Interleave(L.dyn, dyn_first);
  Interleave(L.rom, rom_first);
  // Uniform dyn list: one structure with fixed timings for every problem -- in the flagship batch and in its real use, many
  // x for one NLP -- so problem p's slice of a kind is problem 0's with x, g and jac moved on by p strides.  (By structure
  // INDEX: two equal structures are two tables in the arena, and a batch of them takes the general kernel.)  The interleaved
  // order puts problem 0's slices min(8, n) positions apart.
  {
    bool one = n_problems > 0;
    for (int si : struct_of_problem) one = one && si == struct_of_problem[0];
    if (one) {
      const Structure& S = *structs[struct_of_problem[0]];
      const int s = (int)S.dyn_slices.size();
      if (!S.timings && s > 0 && L.dyn.size() == (size_t)s * (size_t)n_problems)
        b.dyn_uniform = DynUniform{s, 0, std::min(8, n_problems), n_problems, S.n_vars, S.n_rows, S.nnz, 0};
    }
  }
  Interleave(L.pdyn, pdyn_first);
  // Store policy of the copy-out (kernels.hip copy_out_fixed): non-temporal when the batch is SWEEP-LIKE -- fewer than four
  // problems per structure on average, so every evaluation re-reads tables (and x) that only that problem uses -- AND one
  // evaluation writes more than the device's memory-side cache holds (256 MB on an MI355X; by architecture name, structure.h), so that plain stores would flush those
  // tables out of it between two evaluations.  Measured (one box, no per-kernel events): the C5 sweep at 512 /
  // 1024 candidates 116-118 / 223-224 -> 99 / 209-211 us per step; at 256 candidates (220 MB of output, absorbed by the
  // Infinity Cache as it is) 52 -> 55 us, and 8192 problems of ONE structure lose 15 % in rom_kernel -- hence the two conditions.
  std::vector<char> used(n_structs, 0);
  int n_used = 0;
  for (int si : struct_of_problem)
    if (!used[si]) {
      used[si] = 1;
      ++n_used;
    }
  b.stream_nt = StreamNonTemporal(n_used, n_problems, 8 * (b.g_off[n_problems] + b.j_off[n_problems]), cache_bytes);
  b.node_families = 2;
  for (const Structure* S : structs)
    if (S->params.constraint_sets & ~(TWR_SET_TERRAIN | TWR_SET_DYNAMIC | TWR_SET_ROM | TWR_SET_FORCE)) b.node_families = 4;
  if (!flat_ok) {
    L.flat.clear();
  } else {
    // One problem, one XCD: workgroup r of the launch runs on XCD r modulo 8 and takes group r.  The groups of problem p go to
    // workgroups = p modulo 8: its x comes from HBM once and from that XCD's L2 for its other groups.
    std::vector<size_t> queue[8];   // queue c: the groups that go to the list positions = c modulo 8
    for (size_t i = 0; i < flat_group_p.size(); ++i) queue[flat_group_p[i] % 8].push_back(i);
    std::vector<FlatWork> out;
    out.reserve(L.flat.size());
    std::vector<size_t> order;      // the groups in list order
    order.reserve(flat_group_p.size());
    auto emit = [&](size_t group) {
      out.insert(out.end(), L.flat.begin() + 4 * group, L.flat.begin() + 4 * group + 4);
      order.push_back(group);
    };
    size_t depth = 0, k = 0;
    for (const auto& q : queue) depth = std::max(depth, q.size());
    for (; k < depth; ++k) {   // whole rounds of eight; a round in which a queue has run dry ends the interleaving
      bool whole = true;
      for (const auto& q : queue) whole = whole && k < q.size();
      if (!whole) break;
      for (const auto& q : queue) emit(q[k]);
    }
    for (const auto& q : queue)
      for (size_t i = k; i < q.size(); ++i) emit(q[i]);
    // candidate scoring without g: where every group went, then per problem its partial records in a fixed order (its groups
    // in the order the structure lists its items, so the fold's sums do not depend on where the problem sits in the batch)
    std::vector<int32_t> pos(flat_group_p.size());
    for (size_t i = 0; i < order.size(); ++i) pos[order[i]] = (int32_t)i;
    const int32_t n_groups = (int32_t)flat_group_p.size();
    L.score_blob.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) L.score_blob[i] = b.blob_of_problem[flat_group_p[order[i]]];
    L.score_first.assign(1, 0);
    size_t i = 0;
    for (int p = 0; p < n_problems; ++p) {
      for (; i < flat_group_p.size() && flat_group_p[i] == p; ++i)
        for (int w = 0; w < kFlatGroup; ++w)
          if (L.flat[kFlatGroup * i + w].cnt > 0) L.score_slot.push_back(kFlatGroup * pos[i] + w);   // (L.flat: still in list order)
      for (int w = 0; w < b.node_families; ++w) L.score_slot.push_back(kFlatGroup * (n_groups + p) + w);
      L.score_first.push_back((int32_t)L.score_slot.size());
    }
    b.score_fused = true;
    b.score_slab = (int64_t)kFlatGroup * (n_groups + n_problems);
    L.flat.swap(out);
  }
  // Large batches whose node-based sets are terrain / force / splineacc / swing only: per-family chunk lists for the
  // persistent node_chunk_kernel (baseMotion and totalduration rows, and small batches -- where the fused launch or the
  // one-workgroup-per-problem kernel is as good -- stay with node_kernel).
  // (hot-path batches -- terrain and force rows only -- are faster on node_kernel2: 0.041 vs 0.047 ms per 8192 C3 problems)
  // (from eight problems per CU on -- 2048 on the 256 CUs of an MI355X, where the cut-over was measured: below that the
  // one-workgroup-per-problem kernel has enough waves in flight and no persistent loop to fill)
  bool eligible = n_problems >= 8 * n_cu && b.node_families == 4;
  for (const Structure* S : structs)
    if (S->params.constraint_sets & (TWR_SET_BASE_ROM | TWR_SET_TOTAL_TIME)) eligible = false;
  for (int p = 0; p < n_problems && eligible; ++p) {
    const DevStruct* H = reinterpret_cast<const DevStruct*>(structs[struct_of_problem[p]]->blob.data());
    auto add = [&](int f, int count, uint32_t table_off, size_t rec_bytes, int row0, int rows_per, int nnz0, int vals_per) {
      const int chunk = f == 1 ? force_chunk : 64;
      for (int i0 = 0; i0 < count; i0 += chunk) {
        FamWork w;
        std::memset(&w, 0, sizeof(w));
        w.blob = b.blob_of_problem[p];
        w.table = w.blob + table_off + (f == 2 ? 0 : rec_bytes * (size_t)i0);
        w.x_off = b.x_off[p];
        w.g_off = b.g_off[p] + row0 + (int64_t)rows_per * i0;
        w.j_off = b.j_off[p] + nnz0 + (int64_t)vals_per * i0;
        w.cnt = std::min(chunk, count - i0);
        w.i0 = f == 2 ? i0 : 0;
        w.aux0 = 3 * H->n_junctions;
        w.aux1 = H->off_base_ang;
        w.inv_t_swing = H->inv_t_swing;
        L.fam[f].push_back(w);
      }
    };
    add(0, H->n_terrain_rows, H->o_terrain_rows, sizeof(TerrainRow), H->row_terrain, 1, H->nnz_terrain, 3);
    add(1, H->n_force_nodes, H->o_force_nodes, sizeof(ForceNode), H->row_force, 5, H->nnz_force, 25);
    add(2, 6 * H->n_junctions, H->o_acc, sizeof(AccJunction), H->row_acc, 1, H->nnz_acc, 6);
    add(3, H->n_swing_nodes, H->o_swing_nodes, sizeof(SwingNode), H->row_swing, 4, H->nnz_swing, 12);
  }
  return b;
}

// The dyn / rom grids are persistent: as many workgroups as are resident at once.  Residency is LDS bound; the occupancy API
// over-reports it for the dynamic kernel (measured: 7 x 22.5 KB resident, an 8th starts a second round), so the per-CU
// counts are fixed (LaunchTuning) rather than queried.  (Running dyn and rom concurrently on two streams was measured and is
// slower than back to back.)
EvalPlan PlanEval(const EvalShape& s) {
  EvalPlan plan;
  const LaunchTuning& t = s.tuning;
  auto add = [&](Launch k, int store, int nit, int xc, int items, int grid, int block, int lds = 0) -> LaunchStep& {
    LaunchStep& p = plan.step[plan.n++];
    p.kernel = k;
    p.store = store;
    p.nit = nit;
    p.xc = xc;
    p.grid = std::min(items, grid);
    p.block = block;
    p.lds = lds;
    return p;
  };
  auto event = [&](int i) {
    if (s.events) plan.step[plan.n++].arg[0] = i;
  };
  const bool wg = s.flags & 1, wj = s.flags & 2;
  const int store = wg && wj ? kStoreGJ : wj ? kStoreJ : kStoreG;   // non-temporal stores only go with the Jacobian
  const int store_nt = !(s.stream_nt && wj) ? store : wg ? kStoreGJNT : kStoreJNT;
  const int xc = s.dyn_map_chunks == 2 ? 2 : 4;
  const int n_chunks = s.fam[0] + s.fam[1] + s.fam[2] + s.fam[3];
  auto nodes = [&]() {   // the node-based sets (terrain-*, force-*, splineacc-*, swing-*, ...): last launch of every path
    if (n_chunks > 0) {
      // persistent waves per CU for ALL families together, shared out by their chunk counts (by count, not by bytes: an iteration
      // costs about the same whatever the family -- weighting the force chunks 1.5 x ... 3 x was 4-15 % slower)
      const int res = t.node_bpc * s.n_cu;
      int gf[4], sum = 0;
      for (int f = 0; f < 4; ++f) {
        gf[f] = s.fam[f] == 0 ? 0 : std::min(s.fam[f], std::max(1, (int)((long long)res * s.fam[f] / n_chunks)));
        sum += gf[f];
      }
      LaunchStep& p = add(Launch::kChunk, store, 0, 0, sum, sum, 64);
      std::copy(gf, gf + 4, p.arg);
    } else if (s.node > 0) {
      add(s.node_families == 2 ? Launch::kNode2 : Launch::kNode, store, 0, 0, s.node, s.node, s.node_families == 2 ? 128 : 256);
    }
  };
  // Candidate scores (twr_batch_eval_scores): with score_fused the values-only launch in its scoring instantiation
  // (eval_scores_kernel: every wave reduces its rows to a partial record, the node-based sets always by the launch's own
  // node waves -- node_chunk_kernel writes g) and the fold of the partial records into the score rows; otherwise exactly
  // twr_batch_eval(TWR_EVAL_VALUES) and twr_batch_score.  Then twr_batch_best's launch if asked for.  No per-kernel events.
  if (s.flags & kEvalScores) {
    if (s.score_fused) {
      const int nx = (s.flat_max_x + 64 * kFlatGroup - 1) / (64 * kFlatGroup);
      const int n_groups = s.flat / kFlatGroup, items = n_groups + s.node;
      LaunchStep& p = add(Launch::kScores, kStoreG, 0, nx <= 3 ? 3 : nx <= 5 ? 5 : 8, items, items, 64 * kFlatGroup, flat_lds_bytes(s.flat_max_x));
      p.arg[0] = n_groups;
      p.arg[1] = s.node_families;
      p.arg[2] = flat_x_bytes(s.flat_max_x);
      const int fold = (kFoldThreads * s.node + 255) / 256;
      add(Launch::kFold, kStoreG, 0, 0, fold, fold, 256).arg[0] = s.node;
    } else {
      EvalShape v = s;
      v.flags = 1;   // TWR_EVAL_VALUES
      v.events = false;
      plan = PlanEval(v);
      add(Launch::kScoreG, kStoreG, 0, 0, s.node, s.node, 256).arg[0] = s.node;
    }
    if (s.flags & kEvalBest) {   // (launch_best's grid: four candidates per thread, at most 256 workgroups)
      const int blocks = std::max(1, std::min((s.node + 1023) / 1024, 256));
      add(Launch::kBest, kStoreG, 0, 0, blocks, blocks, 256).arg[0] = s.node;
    }
    return plan;
  }
  // Values only (no Jacobian), every problem with fixed timings and at most kFlatXCap variables: "dynamic" and "rangeofmotion-*"
  // with one lane per time node (flat items), the node-based sets -- one launch (eval_values_kernel); with per-kernel events three.
  if (wg && !wj && s.flat > 0 && s.pdyn == 0 && s.prom == 0 && s.ploc == 0) {
    const int nf = !s.events && n_chunks == 0 ? s.node_families : 0;   // (large batches: the chunk kernel takes the node sets;
                                                                        // with per-kernel events they are a launch of their own)
    const int nx = (s.flat_max_x + 64 * kFlatGroup - 1) / (64 * kFlatGroup);
    static_assert(kFlatXCap <= 8 * 64 * kFlatGroup, "largest instantiation of the values-only kernel");
    const int n_groups = s.flat / kFlatGroup, items = n_groups + (nf > 0 ? s.node : 0);
    event(0);
    LaunchStep& p = add(Launch::kValues, kStoreG, 0, nx <= 3 ? 3 : nx <= 5 ? 5 : 8, items, items, 64 * kFlatGroup, flat_lds_bytes(s.flat_max_x));
    p.arg[0] = n_groups;
    p.arg[1] = nf;
    p.arg[2] = flat_x_bytes(s.flat_max_x);
    event(1);   // (the two flat families are one launch: the second interval is empty)
    event(2);
    if (nf == 0) nodes();
    event(3);
    return plan;
  }
  const int cap = t.rom_bpc * s.n_cu;
  // The fused launch (the dyn, rom and node roles as blocks of one launch) is used while the rom role needs at most TWENTY
  // rounds of its residency (rom_bpc workgroups per CU x n_cu).  Round-3 re-tune on one box, ragged sweep, fused vs three
  // launches: 320 / 400 / 512 candidates 75 / 98 / 126 vs 83 / 104 / 128 us per step, 768 / 1024: 187 / 250 vs 183 / 235;
  // round 4: 512 candidates 115 vs 124, 768 / 1024 equal.  The 512 candidates of a two-GPU shard of the C5 sweep are ~8500
  // rom slices (the enumeration is ragged: 16.6 slices per candidate), 8.3 rounds on the 256 CUs of an MI355X.  With
  // non-temporal stores (sweep-like batches) the fused launch stays ahead for longer -- 768 / 896 / 1024 candidates of the
  // C5 sweep (12.7 / 14.9 / 17 thousand rom slices): 160-165 / 179 / 210 us as three launches, 148 / 166 / 202 us fused --
  // twenty rounds there (the enumeration ends at 1040 candidates; nothing larger was measured).  Round 5, with the roles
  // always co-resident: batches that share one structure, plain stores, 640 / 1024 / 2048 problems 129.5 / 193.5 / 365 us as
  // three launches, 120 / 188 / 376 us fused -- twenty rounds for both store policies.  The thresholds are in units of the
  // device's residency, not constants of one chip.
  const int fused_max = t.fused_max_rom > 0 ? t.fused_max_rom : 20 * cap;
  if (!s.events && s.pdyn == 0 && s.prom == 0 && s.rom > 0 && s.dyn > 0 && s.rom <= fused_max) {
    const int half_dyn = (s.dyn + 1) / 2;
    int g_rom = std::min(s.rom, cap), g_dyn = std::min(half_dyn, cap);
    // When the two persistent roles do not fit the CUs together, the blocks of the later role only start as the earlier
    // ones retire, i.e. the roles run one after the other.  For up to 2560 rom slices (160 quadruped candidates of
    // K = 200) it pays to give each role half of the residency instead, so that the latency-bound dyn waves and the
    // store-bound rom waves overlap from the start (64 / 128 / 160 candidates: 18.7 / 30.1 / 35.2 -> 17.5 / 27.8 /
    // 31.6 us per step; from 200 candidates on the extra rounds cost more than the overlap gains).
    // (round 3: five eighths for rom up to 3200 slices -- 128 / 160 / 200 candidates 27.5 / 33.5 / 40.5 us against 27.7 / 33.9 /
    // 44.0 us with the round-2 rule "half each up to 2560"; from 256 candidates on unsplit was as good or better THEN.)
    // Round 5, re-measured with the round-4 kernels (split tables, nt stores; one box, ragged sweep, us per step unsplit ->
    // split): 256 candidates 53.8 -> 47.2 (five eighths; 48.6 at four), 320: 69.3 -> 62.5 (four), 384: 81.7 -> 74.5, 512:
    // 100.9 -> 92.6, 768: 155.8 -> 145.9, 1024: 206.0 -> 194.1; six eighths loses everywhere.  The two roles are ALWAYS
    // co-resident now: the latency-bound dyn waves fill the holes of the store-bound rom stream.
    const int split = t.fused_split > 0 ? t.fused_split : (8 * s.rom <= 34 * cap ? 5 : 4);   // (4352 slices on 256 CUs)
    if (split < 8 && g_rom + g_dyn > cap) {   // split = eighths of the residency given to rom (8 = never split)
      g_rom = std::min(g_rom, cap * split / 8);
      g_dyn = std::min(g_dyn, cap - cap * split / 8);
    }
    if (t.fused_grom > 0) g_rom = std::min(t.fused_grom, s.rom);
    if (t.fused_gdyn > 0) g_dyn = std::min(t.fused_gdyn, half_dyn);
    if (g_dyn >= 8) g_dyn &= ~7;   // (the XCD-aware slice mapping of the dyn role, eval_fused_kernel)
    const int need = (s.rom_max_vals + 1 + 2 + 127) / 128;   // copy-out length of the rom role (as for rom_kernel below)
    const int grid = g_rom + g_dyn + 2 * s.node;
    LaunchStep& p = add(Launch::kFused, store_nt, need <= 34 ? 34 : kRomNitMax, xc, grid, grid, 128);
    p.arg[0] = g_rom;
    p.arg[1] = g_dyn;
    return plan;
  }
  event(0);
  if (s.dyn > 0) {
    LaunchStep& p = add(Launch::kDyn, store_nt, 0, xc, s.dyn, t.dyn_bpc * s.n_cu, 64);
    // A uniform list (BatchPlan::dyn_uniform) goes to dyn_uniform_kernel, whose waves own one slice kind each and load its
    // records once per launch, when the grid divides into kinds without idling the residency (DynUniformCols).
    const int cols = DynUniformCols(s.dyn_uniform.s, s.dyn_uniform.n_problems, t.dyn_bpc * s.n_cu);
    if (cols > 0 && s.dyn == s.dyn_uniform.s * s.dyn_uniform.n_problems) {
      p.uni = s.dyn_uniform;
      p.uni.cols = cols;
      p.grid = 8 * p.uni.s * cols;
    }
  }
  // optimised-timings problems: the pre-pass (segment lookup -> records), then the persistent kernels; their LDS per
  // workgroup is the image of one pass, and their residency follows from it
  if (s.ploc > 0) add(Launch::kLocate, store, 0, 0, s.ploc, s.ploc, kLocateThreads);
  auto phase_bpc = [&](int lds, int most, int knob) { return knob > 0 ? knob : std::max(1, std::min(most, 160 * 1024 / lds)); };
  if (s.pdyn > 0) {   // (at most one wave per SIMD: the kernel uses the AGPR half of the register file as well)
    const int lds = 8 * ((s.pdyn_img_cap + 1) & ~1);
    add(Launch::kDynPhase, store, s.pdyn_img_cap <= 40 * 128 ? 40 : 0, 0, s.pdyn, phase_bpc(lds, 4, t.pdyn_bpc) * s.n_cu, 64, lds);
  }
  event(1);
  if (s.prom > 0) {
    const int lds = 8 * ((s.prom_img_cap + 1) & ~1), img = s.prom_img_cap;
    const int nit = img <= 24 * 128 ? 24 : img <= 32 * 128 ? 32 : img <= 40 * 128 ? 40 : 0;
    add(Launch::kRomPhase, store, nit, 0, s.prom, phase_bpc(lds, 8, t.prom_bpc) * s.n_cu, 64, lds);
  }
  if (s.rom > 0) {
    // NIT = store instructions of rom_kernel's copy-out: the smallest instantiation that covers the largest slice of the
    // batch (+ parity shift, rounded up to whole store instructions).  The stores past the end of a slice are re-stores of its
    // last pair -- no HBM traffic, but requests all the same: C3's balanced 50-node slices need 34, and 34 instead of 38 is
    // worth 4 % of the kernel (A/B on one box: 0.925 -> 0.883 ms together with the balanced slices; five 40-node slices with
    // 27 stores each: 0.965 ms -- large slices win).
    const int need = (s.rom_max_vals + 1 + 2 + 127) / 128;
    add(Launch::kRom, store_nt, need <= 26 ? 26 : need <= 30 ? 30 : need <= 34 ? 34 : kRomNitMax, 0, s.rom, cap, 64);
  }
  event(2);
  nodes();
  event(3);
  return plan;
}

EvalCounts CountsOf(const BatchPlan& P) {
  const BatchPlan::Lists& L = P.lists;
  EvalCounts c;
  c.dyn = (int)L.dyn.size(), c.rom = (int)L.rom.size(), c.node = std::max(0, (int)L.node.size() - 1), c.flat = (int)L.flat.size();
  for (int f = 0; f < 4; ++f) c.fam[f] = (int)L.fam[f].size();
  c.pdyn = (int)L.pdyn.size(), c.ploc = (int)L.ploc.size(), c.prom = (int)L.prom.size();
  return c;
}

EvalShape MakeEvalShape(const BatchPlan& P, const EvalCounts& c, int n_cu, int flags, bool events, const LaunchTuning& tuning) {
  const bool scoring = flags & kEvalScores;
  EvalShape s;
  s.n_cu = n_cu;
  s.dyn = c.dyn, s.rom = c.rom, s.node = c.node, s.flat = c.flat, s.pdyn = c.pdyn, s.ploc = c.ploc, s.prom = c.prom;
  for (int f = 0; f < 4; ++f) s.fam[f] = c.fam[f];
  s.rom_max_vals = P.rom_max_vals, s.flat_max_x = P.flat_max_x, s.dyn_map_chunks = P.dyn_map_chunks, s.node_families = P.node_families;
  s.pdyn_img_cap = P.pdyn_img_cap, s.prom_img_cap = P.prom_img_cap, s.stream_nt = P.stream_nt;
  if (!scoring) s.dyn_uniform = P.dyn_uniform;
  s.flags = scoring ? flags & (kEvalScores | kEvalBest) : flags & 3;
  s.events = events && !scoring;
  s.score_fused = scoring && P.score_fused;
  s.tuning = tuning;
  return s;
}

const char* StoreName(int store) {
  switch (store) {
    case kStoreG: return "G";
    case kStoreJ: return "J";
    case kStoreGJ: return "GJ";
    case kStoreJNT: return "JNT";
    case kStoreGJNT: return "GJNT";
  }
  return "?";
}

const char* KernelName(const LaunchStep& p) {
  switch (p.kernel) {
    case Launch::kEvent: return "";
    case Launch::kDyn: return p.uni.s > 0 ? "dyn_uniform_kernel" : "dyn_kernel";
    case Launch::kRom: return "rom_kernel";
    case Launch::kFused: return "eval_fused_kernel";
    case Launch::kLocate: return "phase_locate_kernel";
    case Launch::kDynPhase: return "dyn_phase_kernel";
    case Launch::kRomPhase: return "rom_phase_kernel";
    case Launch::kNode: return "node_kernel";
    case Launch::kNode2: return "node_kernel2";
    case Launch::kChunk: return "node_chunk_kernel";
    case Launch::kValues: return "eval_values_kernel";
    case Launch::kScores: return "eval_scores_kernel";
    case Launch::kFold: return "score_fold_kernel";
    case Launch::kScoreG: return "score_kernel";
    case Launch::kBest: return "best_kernel";
  }
  return "?";
}

std::string InstantiationName(const LaunchStep& p) {
  const std::string k = KernelName(p), st = StoreName(p.store);
  switch (p.kernel) {
    case Launch::kDyn: return k + "<" + st + ",xc" + std::to_string(p.xc) + ">";
    case Launch::kRom:
    case Launch::kDynPhase:
    case Launch::kRomPhase: return k + "<" + std::to_string(p.nit) + "," + st + ">";
    case Launch::kFused: return k + "<" + std::to_string(p.nit) + ",xc" + std::to_string(p.xc) + "," + st + ">";
    case Launch::kChunk: return k + "<" + st + ">";
    case Launch::kValues:
    case Launch::kScores: return k + "<" + std::to_string(p.xc) + ">";
    default: return k;
  }
}

// ---------------------------------------------------------------- products with the Jacobian values (jac_products.hip)
namespace {
void CheckPattern(const Structure& S) {
  const int n = S.n_vars, m = S.n_rows;
  if ((int)S.row_ptr.size() != m + 1 || (int)S.col_idx.size() != S.nnz || S.row_ptr[0] != 0 || S.row_ptr[m] != S.nnz)
    throw std::runtime_error("CSR pattern does not match its sizes");
  if (n > 65536) throw std::runtime_error("more than 65536 variables: column indices do not fit 16 bits");
  for (int r = 0; r < m; ++r) {
    if (S.row_ptr[r + 1] < S.row_ptr[r]) throw std::runtime_error("row_ptr descends");
    for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
      const int c = S.col_idx[k];
      if (c < 0 || c >= n) throw std::runtime_error("column index outside [0, n_vars)");
      if (k > S.row_ptr[r] && c <= S.col_idx[k - 1])
        throw std::runtime_error("row " + std::to_string(r) + ": column indices not strictly ascending (unsorted or duplicate entries)");
    }
  }
}

template <class T>
uint64_t AppendTable(std::vector<char>& out, const T* data, size_t count) {
  const size_t at = (out.size() + 15) / 16 * 16;
  out.resize(at + count * sizeof(T));
  if (count) std::memcpy(out.data() + at, data, count * sizeof(T));
  return at;
}

uint64_t HashWords(uint64_t h, const void* data, size_t bytes) {   // FNV-1a over 8-byte words (a bucket key only)
  const char* p = static_cast<const char*>(data);
  size_t i = 0;
  for (; i + 8 <= bytes; i += 8) {
    uint64_t w;
    std::memcpy(&w, p + i, 8);
    h = (h ^ w) * 1099511628211ull;
    h ^= h >> 29;
  }
  for (; i < bytes; ++i) h = (h ^ (unsigned char)p[i]) * 1099511628211ull;
  return h;
}

struct JacTables {   // one distinct pattern: byte offsets into JacOpsPlan::tables, its blocks, partials per problem
  uint64_t col = 0, row_ptr = 0, fold_ptr = 0, fold_slot = 0;
  std::vector<std::pair<int, int>> rows;   // J v blocks [r0, r1)
  struct TBlock {
    int k0, k1, r_first, span, ncols;
    uint64_t map;
    int64_t slot;                          // first partial, relative to the problem's
  };
  std::vector<TBlock> tblocks;
  int64_t slots = 0;
};

JacTables BuildJacTables(const Structure& S, JacOpsPlan& J) {
  const int n = S.n_vars, m = S.n_rows, nnz = S.nnz;
  JacTables P;
  const std::vector<uint16_t> col(S.col_idx.begin(), S.col_idx.end());   // < 65536: CheckPattern
  P.col = AppendTable(J.tables, col.data(), col.size());
  P.row_ptr = AppendTable(J.tables, S.row_ptr.data(), S.row_ptr.size());
  J.table_bytes_mul += 2 * (int64_t)nnz + 4 * (int64_t)(m + 1);
  for (int r0 = 0; r0 < m;) {
    int r1 = r0 + 1;
    while (r1 < m && r1 - r0 < kJacMulRows && S.row_ptr[r1 + 1] - S.row_ptr[r0] <= kJacMulNnz) ++r1;
    P.rows.push_back({r0, r1});
    r0 = r1;
  }
  std::vector<int> row_of(nnz);
  for (int r = 0; r < m; ++r) std::fill(row_of.begin() + S.row_ptr[r], row_of.begin() + S.row_ptr[r + 1], r);
  std::vector<int> stamp(n, -1);
  std::vector<std::vector<int32_t>> slots_of(n);   // the partials of every column, in block order
  int64_t tbytes = 4 * (int64_t)(m + 1);
  for (int k0 = 0; k0 < nnz;) {
    const int b = (int)P.tblocks.size();
    int k1 = k0, ncols = 0;
    while (k1 < nnz && k1 - k0 < kJacTNnz && row_of[k1] - row_of[k0] < kJacTSpan) {
      const int c = S.col_idx[k1];
      if (stamp[c] != b) {
        if (ncols == kJacTCols) break;
        stamp[c] = b;
        ++ncols;
      }
      ++k1;
    }
    std::vector<std::pair<int, int>> e;   // (column, entry - k0), sorted: the block's columns ascending, each in row order
    for (int k = k0; k < k1; ++k) e.push_back({S.col_idx[k], k - k0});
    std::sort(e.begin(), e.end());
    std::vector<uint16_t> map(ncols + 1 + e.size());
    int j = -1;
    for (size_t i = 0; i < e.size(); ++i) {
      if (i == 0 || e[i].first != e[i - 1].first) {
        map[++j] = (uint16_t)i;
        slots_of[e[i].first].push_back((int32_t)(P.slots + j));
      }
      map[ncols + 1 + i] = (uint16_t)e[i].second;
    }
    map[ncols] = (uint16_t)e.size();
    const uint64_t at = AppendTable(J.tables, map.data(), map.size());
    tbytes += 2 * (int64_t)map.size();
    P.tblocks.push_back({k0, k1, row_of[k0], row_of[k1 - 1] - row_of[k0] + 1, ncols, at, P.slots});
    P.slots += ncols;
    k0 = k1;
  }
  std::vector<int32_t> fptr(n + 1, 0), fslot;
  for (int c = 0; c < n; ++c) {
    fslot.insert(fslot.end(), slots_of[c].begin(), slots_of[c].end());
    fptr[c + 1] = (int32_t)fslot.size();
  }
  P.fold_ptr = AppendTable(J.tables, fptr.data(), fptr.size());
  P.fold_slot = AppendTable(J.tables, fslot.data(), fslot.size());
  J.table_bytes_tmul += tbytes + 4 * (int64_t)(fptr.size() + fslot.size());
  return P;
}
}  // namespace

CscPattern TransposePattern(const Structure& S) {
  CheckPattern(S);
  CscPattern t;
  t.col_ptr.assign(S.n_vars + 1, 0);
  for (int k = 0; k < S.nnz; ++k) ++t.col_ptr[S.col_idx[k] + 1];
  for (int c = 0; c < S.n_vars; ++c) t.col_ptr[c + 1] += t.col_ptr[c];
  t.row_idx.resize(S.nnz);
  t.csr_pos.resize(S.nnz);
  std::vector<int32_t> next(t.col_ptr.begin(), t.col_ptr.end() - 1);
  for (int r = 0; r < S.n_rows; ++r)
    for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
      const int q = next[S.col_idx[k]]++;
      t.row_idx[q] = r;
      t.csr_pos[q] = k;
    }
  return t;
}

void JacOpsPlan::Place(uint64_t base) {
  for (auto& w : mul) w.col += base, w.row_ptr += base;
  for (auto& w : tmul) w.map += base, w.row_ptr += base;
  for (auto& w : fold) w.ptr += base, w.slot += base;
}

JacOpsPlan PlanJacOps(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  JacOpsPlan J;
  std::vector<JacTables> pats;
  std::vector<const Structure*> first;   // the first structure of every distinct pattern
  std::unordered_map<uint64_t, std::vector<int>> by_hash;
  J.pattern_of_struct.resize(n_structs);
  for (int i = 0; i < n_structs; ++i) {
    const Structure& S = *structs[i];
    CheckPattern(S);
    uint64_t h = HashWords(1469598103934665603ull ^ (uint64_t)S.n_vars, S.row_ptr.data(), S.row_ptr.size() * sizeof(int32_t));
    h = HashWords(h, S.col_idx.data(), S.col_idx.size() * sizeof(int32_t));
    std::vector<int>& bucket = by_hash[h];
    int pid = -1;
    for (int q : bucket)
      if (first[q]->n_vars == S.n_vars && first[q]->row_ptr == S.row_ptr && first[q]->col_idx == S.col_idx) pid = q;
    if (pid < 0) {
      pid = (int)pats.size();
      bucket.push_back(pid);
      first.push_back(&S);
      pats.push_back(BuildJacTables(S, J));
    }
    J.pattern_of_struct[i] = pid;
  }
  J.distinct_patterns = (int)pats.size();
  J.x_off.assign(n_problems + 1, 0);
  J.g_off.assign(n_problems + 1, 0);
  J.j_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    const Structure& S = *structs[si];
    const JacTables& P = pats[J.pattern_of_struct[si]];
    J.x_off[p + 1] = J.x_off[p] + S.n_vars;
    J.g_off[p + 1] = J.g_off[p] + S.n_rows;
    J.j_off[p + 1] = J.j_off[p] + S.nnz;
    for (const auto& rb : P.rows) J.mul.push_back({J.x_off[p], J.g_off[p], J.j_off[p], P.col, P.row_ptr, rb.first, rb.second, S.n_vars, 0});
    for (const auto& tb : P.tblocks)
      J.tmul.push_back({J.g_off[p], J.j_off[p], J.slab + tb.slot, tb.map, P.row_ptr, tb.k0, tb.k1, tb.r_first, tb.span, tb.ncols, 0});
    for (int c0 = 0; c0 < S.n_vars; c0 += kJacFoldCols)
      J.fold.push_back({J.x_off[p], J.slab, P.fold_ptr, P.fold_slot, c0, std::min(S.n_vars, c0 + kJacFoldCols)});
    J.slab += P.slots;
    if (S.n_vars <= kJacLdsX) J.mul_lds_x = std::max(J.mul_lds_x, S.n_vars);
  }
  return J;
}

// ---------------------------------------------------------------- the one-pass normal product (jac_products.hip jac_normal_kernel)
namespace {
struct JacNormalTables {   // one distinct pattern: byte offsets into JacNormalPlan::tables, its blocks, partials per problem
  uint64_t fold_ptr = 0, fold_slot = 0;
  struct Block {
    int r0, r1, ncols, is_long;
    uint64_t map;
    int64_t slot;   // first partial, relative to the problem's
  };
  std::vector<Block> blocks;
  int64_t slots = 0;
};

JacNormalTables BuildJacNormalTables(const Structure& S, JacNormalPlan& N, int tile) {
  const int n = S.n_vars, m = S.n_rows;
  JacNormalTables P;
  std::vector<std::vector<int32_t>> slots_of(n);   // the partials of every column, in block order
  for (int r0 = 0; r0 < m;) {
    int r1 = r0 + 1;
    while (r1 < m && r1 - r0 < kJacThreads && S.row_ptr[r1 + 1] - S.row_ptr[r0] <= tile) ++r1;
    const int k0 = S.row_ptr[r0], k1 = S.row_ptr[r1];
    if (k1 - k0 > tile) {   // one long row: a partial per entry, in column order
      for (int k = k0; k < k1; ++k) slots_of[S.col_idx[k]].push_back((int32_t)(P.slots + (k - k0)));
      P.blocks.push_back({r0, r1, k1 - k0, 1, 0, P.slots});
      P.slots += k1 - k0;
    } else if (k1 > k0) {
      std::vector<std::pair<int, int>> e;   // (column, entry - k0), sorted: the block's columns ascending, each in row order
      for (int k = k0; k < k1; ++k) e.push_back({S.col_idx[k], k - k0});
      std::sort(e.begin(), e.end());
      int ncols = 0;
      for (size_t i = 0; i < e.size(); ++i) ncols += i == 0 || e[i].first != e[i - 1].first;
      std::vector<uint16_t> map(ncols + 1 + e.size());
      int j = -1;
      for (size_t i = 0; i < e.size(); ++i) {
        if (i == 0 || e[i].first != e[i - 1].first) {
          map[++j] = (uint16_t)i;
          slots_of[e[i].first].push_back((int32_t)(P.slots + j));
        }
        map[ncols + 1 + i] = (uint16_t)e[i].second;
      }
      map[ncols] = (uint16_t)e.size();
      P.blocks.push_back({r0, r1, ncols, 0, AppendTable(N.tables, map.data(), map.size()), P.slots});
      P.slots += ncols;
    } else {
      P.blocks.push_back({r0, r1, 0, 0, 0, P.slots});   // rows without entries: y = 0 is still theirs to write
    }
    r0 = r1;
  }
  std::vector<int32_t> fptr(n + 1, 0), fslot;
  for (int c = 0; c < n; ++c) {
    fslot.insert(fslot.end(), slots_of[c].begin(), slots_of[c].end());
    fptr[c + 1] = (int32_t)fslot.size();
  }
  P.fold_ptr = AppendTable(N.tables, fptr.data(), fptr.size());
  P.fold_slot = AppendTable(N.tables, fslot.data(), fslot.size());
  return P;
}
}  // namespace

void JacNormalPlan::Place(uint64_t ops_base, uint64_t base) {
  for (auto& w : work) w.col += ops_base, w.row_ptr += ops_base, w.map += base;
  for (auto& w : fold) w.ptr += base, w.slot += base;
}

std::vector<JacPatternPlace> JacPatternPlaces(const JacOpsPlan& J, const std::vector<int32_t>& struct_of_problem) {
  std::vector<JacPatternPlace> at(J.distinct_patterns, JacPatternPlace{-1, 0, 0});
  size_t k = 0;
  for (size_t p = 0; p < struct_of_problem.size(); ++p) {   // J.mul is problem by problem; a problem without rows has no record
    while (k < J.mul.size() && J.mul[k].x_off < J.x_off[p]) ++k;
    JacPatternPlace& a = at[J.pattern_of_struct[struct_of_problem[p]]];
    if (a.first_struct >= 0) continue;
    a.first_struct = struct_of_problem[p];
    if (k < J.mul.size() && J.mul[k].x_off == J.x_off[p]) a.col = J.mul[k].col, a.row_ptr = J.mul[k].row_ptr;
  }
  return at;
}

JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& patterns, const std::vector<JacPatternPlace>& places,
                            const std::vector<int32_t>& pattern_of_problem, int tile) {
  const int n_patterns = (int)patterns.size(), n_problems = (int)pattern_of_problem.size();
  if (tile < 1 || tile > kJacNormNnz) throw std::runtime_error("the one-pass tile is 1 .. kJacNormNnz entries");
  if (places.size() != patterns.size()) throw std::runtime_error("one place per pattern");
  JacNormalPlan N;
  N.tile = tile;
  std::vector<JacNormalTables> npats;
  for (const Structure* S : patterns) {
    CheckPattern(*S);
    npats.push_back(BuildJacNormalTables(*S, N, tile));
  }
  N.x_off.assign(n_problems + 1, 0);
  N.g_off.assign(n_problems + 1, 0);
  N.j_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int q = pattern_of_problem[p];
    if (q < 0 || q >= n_patterns) throw std::runtime_error("pattern_of_problem out of range");
    const Structure& S = *patterns[q];
    const JacNormalTables& Q = npats[q];
    N.x_off[p + 1] = N.x_off[p] + S.n_vars;
    N.g_off[p + 1] = N.g_off[p] + S.n_rows;
    N.j_off[p + 1] = N.j_off[p] + S.nnz;
    for (const auto& b : Q.blocks)
      N.work.push_back({N.x_off[p], N.g_off[p], N.j_off[p], N.slab + b.slot, places[q].col, places[q].row_ptr, b.map, b.r0, b.r1,
                        S.n_vars, b.ncols, b.is_long, 0});
    for (int c0 = 0; c0 < S.n_vars; c0 += kJacFoldCols)
      N.fold.push_back({N.x_off[p], N.slab, Q.fold_ptr, Q.fold_slot, c0, std::min(S.n_vars, c0 + kJacFoldCols)});
    N.slab += Q.slots;
    if (S.n_vars <= kJacLdsX) N.lds_x = std::max(N.lds_x, S.n_vars);
  }
  return N;
}

JacNormalPlan PlanJacNormal(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem, int tile) {
  const JacOpsPlan J = PlanJacOps(structs, struct_of_problem);   // (checks the patterns and struct_of_problem)
  const std::vector<JacPatternPlace> places = JacPatternPlaces(J, struct_of_problem);
  std::vector<const Structure*> patterns(places.size(), nullptr);   // (a pattern no problem has is still a structure's)
  for (size_t i = 0; i < structs.size(); ++i)
    if (!patterns[J.pattern_of_struct[i]]) patterns[J.pattern_of_struct[i]] = structs[i];
  std::vector<int32_t> pattern_of_problem;
  for (int32_t si : struct_of_problem) pattern_of_problem.push_back(J.pattern_of_struct[si]);
  return PlanJacNormal(patterns, places, pattern_of_problem, tile);
}

// ---------------------------------------------------------------- the Gram matrix N = J^T W J (jac_gram.hip)
void GramPattern(const Structure& S, std::vector<int32_t>* row_ptr, std::vector<int32_t>* col_idx) {
  const CscPattern T = TransposePattern(S);   // (checks the pattern)
  const int n = S.n_vars;
  row_ptr->assign(n + 1, 0);
  col_idx->clear();
  std::vector<int> stamp(n, -1);
  std::vector<int32_t> cols;
  for (int i = 0; i < n; ++i) {   // row i of N: the columns of every row of J that has an entry in column i
    cols.clear();
    for (int q = T.col_ptr[i]; q < T.col_ptr[i + 1]; ++q) {
      const int r = T.row_idx[q];
      for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1]; ++k) {
        const int c = S.col_idx[k];
        if (stamp[c] != i) stamp[c] = i, cols.push_back(c);
      }
    }
    std::sort(cols.begin(), cols.end());
    if (col_idx->size() + cols.size() > (size_t)INT32_MAX) throw JacGramUnsupported("the Gram matrix has more than 2^31 - 1 entries");
    col_idx->insert(col_idx->end(), cols.begin(), cols.end());
    (*row_ptr)[i + 1] = (int32_t)col_idx->size();
  }
}

namespace {
// One pattern's tables, appended to `tables` (offsets into it)
JacGramPattern BuildGramTables(const Structure& S, std::vector<char>& tables) {
  const int n = S.n_vars;
  if (S.n_rows > kGramMaxRows)
    throw JacGramUnsupported("the Gram tables hold a row of J in 16 bits: " + std::to_string(S.n_rows) + " rows, at most " + std::to_string(kGramMaxRows));
  if (S.nnz > kGramMaxNnz)
    throw JacGramUnsupported("the Gram tables hold a position in J in 24 bits: " + std::to_string(S.nnz) + " entries, at most " + std::to_string(kGramMaxNnz));
  if (n > kGramMaxVars)
    throw JacGramUnsupported("the Gram solve keeps " + std::to_string(kGramSolveVectors) + " vectors of n doubles in one workgroup's LDS (" +
                             std::to_string(kGramLdsBytes) + " bytes): " + std::to_string(n) + " variables, at most " + std::to_string(kGramMaxVars));
  JacGramPattern P;
  std::vector<int32_t> rp, ci;
  GramPattern(S, &rp, &ci);
  const CscPattern T = TransposePattern(S);
  P.n = n;
  P.nnz = (int32_t)ci.size();
  // the lower entries in CSR order, and every one's terms in ascending row
  std::vector<int32_t> lpos, lmirror;
  std::vector<std::vector<uint64_t>> terms;
  std::vector<int32_t> where(n, -1);   // column -> lower entry of the row in hand
  for (int i = 0; i < n; ++i) {
    for (int e = rp[i]; e < rp[i + 1] && ci[e] <= i; ++e) {
      const int j = ci[e];
      where[j] = (int32_t)lpos.size();
      lpos.push_back(e);
      lmirror.push_back((int32_t)(std::lower_bound(ci.begin() + rp[j], ci.begin() + rp[j + 1], i) - ci.begin()));
      terms.emplace_back();
    }
    for (int q = T.col_ptr[i]; q < T.col_ptr[i + 1]; ++q) {
      const int r = T.row_idx[q];
      for (int k = S.row_ptr[r]; k < S.row_ptr[r + 1] && S.col_idx[k] <= i; ++k)
        terms[where[S.col_idx[k]]].push_back((uint64_t)r << 48 | (uint64_t)T.csr_pos[q] << 24 | (uint64_t)k);
    }
  }
  P.lower = (int32_t)lpos.size();
  std::vector<int32_t> order(P.lower);
  for (int e = 0; e < P.lower; ++e) order[e] = e;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return terms[a].size() > terms[b].size(); });
  P.slices = (P.lower + kGramSlice - 1) / kGramSlice;
  std::vector<int32_t> pos(P.lower), mirror(P.lower), cnt(P.lower), slice_ptr(P.slices + 1, 0);
  std::vector<uint64_t> words;
  for (int s = 0; s < P.slices; ++s) {
    const int e0 = s * kGramSlice, e1 = std::min(P.lower, e0 + kGramSlice);
    const size_t width = terms[order[e0]].size(), at = words.size();
    if (at + width * kGramSlice > (size_t)INT32_MAX) throw JacGramUnsupported("the Gram contribution table has more than 2^31 - 1 words");
    words.resize(at + width * kGramSlice, kGramPad);
    for (int e = e0; e < e1; ++e) {
      const std::vector<uint64_t>& t = terms[order[e]];
      pos[e] = lpos[order[e]], mirror[e] = lmirror[order[e]], cnt[e] = (int32_t)t.size();
      for (size_t k = 0; k < t.size(); ++k) words[at + k * kGramSlice + (e - e0)] = t[k];
      P.products += (int64_t)t.size();
    }
    slice_ptr[s + 1] = (int32_t)words.size();
  }
  P.n_words = (int64_t)words.size();
  std::vector<uint16_t> col(ci.begin(), ci.end());
  P.row_ptr = AppendTable(tables, rp.data(), rp.size());
  P.col = AppendTable(tables, col.data(), col.size());
  P.pos = AppendTable(tables, pos.data(), pos.size());
  P.mirror = AppendTable(tables, mirror.data(), mirror.size());
  P.cnt = AppendTable(tables, cnt.data(), cnt.size());
  P.slice_ptr = AppendTable(tables, slice_ptr.data(), slice_ptr.size());
  P.words = AppendTable(tables, words.data(), words.size());
  return P;
}
}  // namespace

void JacGramPlan::Place(uint64_t base) {
  for (auto& w : form) w.pos += base, w.mirror += base, w.cnt += base, w.slice_ptr += base, w.words += base;
  for (auto& w : mul) w.row_ptr += base, w.col += base;
  for (auto& w : solve) w.row_ptr += base, w.col += base;
}

JacGramPlan PlanJacGram(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  JacGramPlan G;
  std::vector<const Structure*> first;   // the first structure of every distinct pattern
  std::unordered_map<uint64_t, std::vector<int>> by_hash;
  G.pattern_of_struct.resize(n_structs);
  for (int i = 0; i < n_structs; ++i) {
    const Structure& S = *structs[i];
    CheckPattern(S);
    uint64_t h = HashWords(1469598103934665603ull ^ (uint64_t)S.n_vars, S.row_ptr.data(), S.row_ptr.size() * sizeof(int32_t));
    h = HashWords(h, S.col_idx.data(), S.col_idx.size() * sizeof(int32_t));
    std::vector<int>& bucket = by_hash[h];
    int pid = -1;
    for (int q : bucket)
      if (first[q]->n_vars == S.n_vars && first[q]->row_ptr == S.row_ptr && first[q]->col_idx == S.col_idx) pid = q;
    if (pid < 0) {
      pid = (int)G.patterns.size();
      bucket.push_back(pid);
      first.push_back(&S);
      G.patterns.emplace_back();
    }
    G.pattern_of_struct[i] = pid;
  }
  // The distinct patterns are planned side by side (a sweep has a thousand of them at a third of a second each), every one into
  // tables of its own, which are then laid end to end in pattern order: the plan does not depend on the number of threads.
  const int n_pat = (int)first.size();
  std::vector<std::vector<char>> local(n_pat);
  std::vector<std::exception_ptr> failed(n_pat);
  std::atomic<int> next{0};
  const auto worker = [&] {
    for (int q = next++; q < n_pat; q = next++) {
      try {
        G.patterns[q] = BuildGramTables(*first[q], local[q]);
      } catch (...) {
        failed[q] = std::current_exception();
      }
    }
  };
  const int n_threads = std::max(1, std::min({n_pat, kGramPlanThreads, (int)std::thread::hardware_concurrency()}));
  std::vector<std::thread> pool;
  for (int t = 1; t < n_threads; ++t) pool.emplace_back(worker);
  worker();
  for (std::thread& t : pool) t.join();
  for (int q = 0; q < n_pat; ++q)
    if (failed[q]) std::rethrow_exception(failed[q]);   // the first pattern that failed, whatever thread had it
  for (int q = 0; q < n_pat; ++q) {
    const uint64_t base = AppendTable(G.tables, local[q].data(), local[q].size());
    JacGramPattern& P = G.patterns[q];
    P.row_ptr += base, P.col += base, P.pos += base, P.mirror += base, P.cnt += base, P.slice_ptr += base, P.words += base;
    std::vector<char>().swap(local[q]);
  }
  G.x_off.assign(n_problems + 1, 0);
  G.g_off.assign(n_problems + 1, 0);
  G.j_off.assign(n_problems + 1, 0);
  G.gram_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    const Structure& S = *structs[si];
    const JacGramPattern& P = G.patterns[G.pattern_of_struct[si]];
    G.x_off[p + 1] = G.x_off[p] + S.n_vars;
    G.g_off[p + 1] = G.g_off[p] + S.n_rows;
    G.j_off[p + 1] = G.j_off[p] + S.nnz;
    G.gram_off[p + 1] = G.gram_off[p] + (P.nnz + 1) / 2 * 2;
    for (int e0 = 0; e0 < P.lower; e0 += kGramThreads)
      G.form.push_back({G.g_off[p], G.j_off[p], G.gram_off[p], P.pos, P.mirror, P.cnt, P.slice_ptr, P.words, e0, std::min(P.lower, e0 + kGramThreads)});
    for (int r0 = 0; r0 < S.n_vars; r0 += kGramThreads)
      G.mul.push_back({G.x_off[p], G.gram_off[p], P.row_ptr, P.col, r0, std::min(S.n_vars, r0 + kGramThreads)});
    G.solve.push_back({G.x_off[p], G.gram_off[p], P.row_ptr, P.col, S.n_vars, 0});
    G.max_n = std::max(G.max_n, S.n_vars);
  }
  return G;
}

void JacLsqPlan::Place(uint64_t base) {
  for (auto& w : work) w.lower += base, w.upper += base;
}

JacLsqPlan PlanJacLsq(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  JacLsqPlan L;
  struct Table {
    const Structure* first;
    uint64_t lower, upper;
  };
  std::vector<Table> tabs;
  std::unordered_map<uint64_t, std::vector<int>> by_hash;
  L.bounds_of_struct.resize(n_structs);
  for (int i = 0; i < n_structs; ++i) {
    const Structure& S = *structs[i];
    if ((int)S.lower.size() != S.n_rows || (int)S.upper.size() != S.n_rows) throw std::runtime_error("bounds do not match the rows");
    uint64_t h = HashWords(1469598103934665603ull ^ (uint64_t)S.n_rows, S.lower.data(), S.lower.size() * sizeof(double));
    h = HashWords(h, S.upper.data(), S.upper.size() * sizeof(double));
    std::vector<int>& bucket = by_hash[h];
    const size_t bytes = (size_t)S.n_rows * sizeof(double);
    int tid = -1;
    for (int q : bucket) {   // byte-identical, not ==: -0.0 and 0.0 are different tables, NaN bounds equal themselves
      const Structure& F = *tabs[q].first;
      if (F.n_rows == S.n_rows && (bytes == 0 || (std::memcmp(F.lower.data(), S.lower.data(), bytes) == 0 &&
                                                  std::memcmp(F.upper.data(), S.upper.data(), bytes) == 0)))
        tid = q;
    }
    if (tid < 0) {
      tid = (int)tabs.size();
      bucket.push_back(tid);
      const uint64_t lo = AppendTable(L.bounds, S.lower.data(), S.lower.size());
      tabs.push_back({&S, lo, AppendTable(L.bounds, S.upper.data(), S.upper.size())});
    }
    L.bounds_of_struct[i] = tid;
  }
  L.distinct_bounds = (int)tabs.size();
  L.x_off.assign(n_problems + 1, 0);
  L.g_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    const Structure& S = *structs[si];
    const Table& T = tabs[L.bounds_of_struct[si]];
    L.work.push_back({L.x_off[p], L.g_off[p], T.lower, T.upper, S.n_vars, S.n_rows});
    L.x_off[p + 1] = L.x_off[p] + S.n_vars;
    L.g_off[p + 1] = L.g_off[p] + S.n_rows;
    if (S.n_vars <= kJacLdsX) L.lds_x = std::max(L.lds_x, S.n_vars);
  }
  const auto even = [](int64_t v) { return (v + 1) / 2 * 2; };
  const int64_t X = even(L.x_off[n_problems]), G = even(L.g_off[n_problems]);
  L.ws_p = 0;
  L.ws_z = L.ws_p + X;
  L.ws_q = L.ws_z + X;
  L.ws_r = L.ws_q + G;
  L.ws_t = L.ws_r + G;
  L.ws_rec = L.ws_t + G;
  L.ws_doubles = L.ws_rec + (int64_t)kLsqRec * n_problems;
  L.ws2_e = 0;
  L.ws2_cp = L.ws2_e + X;
  L.ws2_doubles = L.ws2_cp + X;
  L.ws3_s = 0;
  L.ws3_u = L.ws3_s + X;
  L.ws3_doubles = L.ws3_u + X;
  return L;
}

JacLmPlan PlanJacLm(const std::vector<const Structure*>& structs, const std::vector<int32_t>& struct_of_problem) {
  const int n_structs = (int)structs.size(), n_problems = (int)struct_of_problem.size();
  JacLmPlan L;
  L.x_off.assign(n_problems + 1, 0);
  L.g_off.assign(n_problems + 1, 0);
  for (int p = 0; p < n_problems; ++p) {
    const int si = struct_of_problem[p];
    if (si < 0 || si >= n_structs) throw std::runtime_error("struct_of_problem out of range");
    L.x_off[p + 1] = L.x_off[p] + structs[si]->n_vars;
    L.g_off[p + 1] = L.g_off[p] + structs[si]->n_rows;
  }
  const auto even = [](int64_t v) { return (v + 1) / 2 * 2; };
  const int64_t X = even(L.x_off[n_problems]), G = even(L.g_off[n_problems]), P = even(n_problems);
  int64_t at = 0;
  const auto take = [&](int64_t& seg, int64_t len) { seg = at, at += len; };
  for (int64_t* s : {&L.ws_xt, &L.ws_d, &L.ws_z, &L.ws_colsq, &L.ws_colmax, &L.ws_c, &L.ws_cf}) take(*s, X);
  for (int64_t* s : {&L.ws_r, &L.ws_b, &L.ws_wa, &L.ws_gt, &L.ws_rt}) take(*s, G);
  take(L.ws_rec, even((int64_t)kLmRec * n_problems));
  for (int64_t* s : {&L.ws_mu, &L.ws_merit_t, &L.ws_merit_lin, &L.ws_nfree}) take(*s, P);
  take(L.ws_info, even((int64_t)4 * n_problems));
  L.ws_doubles = at;
  return L;
}

}  // namespace twr
