// Host-side structure builder.  Closed-form restatement of the reference's setup-time
// logic; nothing here touches x.  Citations are file:line under /root/reference/towr/.
#include "structure.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <stdexcept>
#include <tuple>

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
  BuildStartTable();
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
// atPosition(INTER_LINEAR) (restated in the device code, kernels/terrain.h gridmap_sample; this host copy serves the
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

// ------------------------------------------------------------------ start table (start_table.h)
// InitialGuess and VariableBounds above as ONE record per variable: the loops are theirs, in their order, writing records where
// they write numbers -- so a variable shared by two nodes keeps the record of the later node, as it keeps that node's value, and
// a bound on a node value that is no variable leaves no trace.
void Structure::BuildStartTable() {
  std::vector<StartRec> rec(n_vars, StartRec{0, 0, 0, kStartZero, kStartNoBound, 0, 0});
  std::vector<double> dur;
  StartHeader h{};
  h.n_vars = n_vars;
  h.n_ee = n_ee;
  h.T = T;
  h.mass = model.mass;
  h.gravity = model.gravity;
  for (int e = 0; e < n_ee; ++e)
    for (int d = 0; d < 3; ++d) h.stance[e][d] = model.nominal_stance[e][d];
  auto values = [&](const SplineLayout& s, int delta, int spline) {   // `interpolate` of InitialGuess
    if (s.n_nodes - 1 > 0xFFFF) throw std::runtime_error("too many nodes per spline for the start table");
    h.nm1[spline] = s.n_nodes - 1;
    for (int n = 0; n < s.n_nodes; ++n)
      for (int d = 0; d < 3; ++d)
        for (int dv = 0; dv < 2; ++dv) {
          const int i = s.at(n, dv, d);
          if (i < 0) continue;
          StartRec& r = rec[i + delta];
          r.node = (uint16_t)n;
          r.spline = (uint8_t)spline;
          r.comp = (uint8_t)(3 * dv + d);
          r.value = kStartNode;
        }
  };
  values(base, off_base_lin, 0);
  values(base, off_base_ang, 1);
  for (int e = 0; e < n_ee; ++e) values(motion[e], 0, 2 + e);
  for (int e = 0; e < n_ee; ++e) values(force[e], 0, 2 + kMaxEE + e);
  auto fix = [&](const SplineLayout& s, int delta, int node, int deriv, int dim, int slot) {   // `fix` of VariableBounds
    const int i = s.at(node, deriv, dim);
    if (i < 0) return;
    rec[i + delta].bound = kStartFixed;
    rec[i + delta].slot = (uint8_t)slot;
  };
  const int last = base.n_nodes - 1;
  for (int d = 0; d < 3; ++d) {
    fix(base, off_base_lin, 0, 0, d, d);
    fix(base, off_base_lin, 0, 1, d, 3 + d);
    if (d != 2) fix(base, off_base_lin, last, 0, d, 12 + d);
    fix(base, off_base_lin, last, 1, d, 12 + 3 + d);
    fix(base, off_base_ang, 0, 0, d, 6 + d);
    fix(base, off_base_ang, 0, 1, d, 9 + d);
    fix(base, off_base_ang, last, 0, d, 12 + 6 + d);
    fix(base, off_base_ang, last, 1, d, 12 + 9 + d);
    for (int e = 0; e < n_ee; ++e) fix(motion[e], 0, 0, 0, d, 24 + 3 * e + d);
  }
  if (timings)
    for (int e = 0; e < n_ee; ++e)
      for (int i = 0; i < schedule.n_phases[e] - 1; ++i) {
        StartRec& r = rec[off_schedule[e] + i];
        r = StartRec{(uint16_t)dur.size(), 0, 0, kStartDuration, kStartDurationBox, 0, 0};
        dur.push_back(schedule.phase_durations[e][i]);
      }
  h.n_dur = (int32_t)dur.size();
  h.o_dur = (uint32_t)sizeof(StartHeader);
  h.o_rec = h.o_dur + (uint32_t)(dur.size() * sizeof(double));
  auto table = std::make_shared<std::vector<char>>(h.o_rec + rec.size() * sizeof(StartRec));
  std::memcpy(table->data(), &h, sizeof(h));
  if (!dur.empty()) std::memcpy(table->data() + h.o_dur, dur.data(), dur.size() * sizeof(double));
  if (!rec.empty()) std::memcpy(table->data() + h.o_rec, rec.data(), rec.size() * sizeof(StartRec));
  start_table = std::move(table);
}

void Structure::StartHost(const double* request, double* x, double* lower, double* upper) const {
  if (!start_table) throw std::runtime_error("structure without a start table");
  const char* t = start_table->data();
  const StartHeader& h = *reinterpret_cast<const StartHeader*>(t);
  const double* dur = reinterpret_cast<const double*>(t + h.o_dur);
  const StartRec* rec = reinterpret_cast<const StartRec*>(t + h.o_rec);
  StartEnd ends[kStartSplines] = {};
  if (x) {   // the per-spline endpoints: 1 + n_ee terrain heights, one sine and one cosine
    const double *lin0 = request, *ang0 = request + 6, *lin1 = request + 12, *ang1 = request + 18, *ee0 = request + 24;
    double fl[3], f[3];
    start_final_base(lin1, TerrainHeightHost(model, grid.get(), lin1[0], lin1[1]), h.stance[0], fl);
    start_end(lin0, fl, h.T, ends[0]);
    start_end(ang0, ang1, h.T, ends[1]);
    const double cz = std::cos(ang1[2]), sz = std::sin(ang1[2]);
    start_force(h.mass, h.gravity, h.n_ee, f);
    for (int e = 0; e < h.n_ee; ++e) {
      double fe[3];
      start_foothold(lin1, sz, cz, h.stance[e], fe);
      fe[2] = TerrainHeightHost(model, grid.get(), fe[0], fe[1]);
      start_end(ee0 + 3 * e, fe, h.T, ends[2 + e]);
      start_end(f, f, h.T, ends[2 + kMaxEE + e]);
    }
  }
  for (int i = 0; i < h.n_vars; ++i) {
    if (x) x[i] = start_value(rec[i], ends, h.nm1, dur);
    double lo, up;
    start_bounds(rec[i], request, lo, up);
    if (lower) lower[i] = lo;
    if (upper) upper[i] = up;
  }
}

}  // namespace twr
