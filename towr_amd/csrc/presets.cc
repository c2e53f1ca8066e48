// Robot and terrain presets and the gait generator: the reference's RobotModel and GaitGenerator as tables.
// Citations are file:line of the reference's towr/ tree, as in structure.cc.
#include <cmath>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "structure.h"

namespace twr {

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

// Go1legInverseKinematics / InverseKinematicsGo1 (include/towr/models/go1/go1leg_inverse_kinematics.h:47-49,
// inverse_kinematics_go1.h:34, src/go1/go1leg_inverse_kinematics.cc:86-108, src/go1/inverse_kinematics_go1.cc:23-37): every
// constant as the double the reference's expression yields.  Returns false for a robot the reference has no IK for.
bool LegKinematicsPreset(int robot, twr_leg_kinematics* k) {
  if (robot != TWR_ROBOT_GO1) return false;
  std::memset(k, 0, sizeof(*k));
  const double pi = 3.14159265358979323846;   // M_PI
  k->n_ee = 4;
  const double mirror[4][3] = {{1, 1, 1}, {1, -1, 1}, {-1, 1, 1}, {-1, -1, 1}};   // LF RF LH RH
  std::memcpy(k->mirror, mirror, sizeof(mirror));
  k->knee_bend[2] = k->knee_bend[3] = 1;   // hind legs: Backward
  k->base_to_hip[0] = 0.1881;
  k->base_to_hip[1] = 0.04675 + 0.08;
  k->length_thigh = k->length_shank = 0.213;
  const double lo[3] = {-180, -90, -180}, hi[3] = {90, 90, 0};
  for (int j = 0; j < 3; ++j) {
    k->q_min[j] = lo[j] / 180.0 * pi;
    k->q_max[j] = hi[j] / 180.0 * pi;
  }
  return true;
}
// What every joint call requires of a descriptor; throws naming the field.
void CheckLegKinematics(const twr_leg_kinematics& k) {
  auto bad = [](const std::string& what) { throw std::runtime_error("twr_leg_kinematics: " + what); };
  if (k.n_ee < 1 || k.n_ee > 4) bad("n_ee must be 1..4");
  for (int e = 0; e < k.n_ee; ++e) {
    if (k.knee_bend[e] != 0 && k.knee_bend[e] != 1) bad("knee_bend must be 0 or 1");
    for (int d = 0; d < 3; ++d)
      if (k.mirror[e][d] != 1.0 && k.mirror[e][d] != -1.0) bad("mirror must be +1 or -1");
  }
  for (int d = 0; d < 3; ++d) {
    if (!std::isfinite(k.base_to_hip[d])) bad("base_to_hip must be finite");
    if (!std::isfinite(k.hfe_to_haa[d])) bad("hfe_to_haa must be finite");
  }
  if (!std::isfinite(k.length_thigh) || !(k.length_thigh > 0)) bad("length_thigh must be finite and > 0");
  if (!std::isfinite(k.length_shank) || !(k.length_shank > 0)) bad("length_shank must be finite and > 0");
  for (int j = 0; j < 3; ++j)
    if (!(k.q_min[j] <= k.q_max[j])) bad("q_min <= q_max is required, neither NaN");
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

}  // namespace twr
