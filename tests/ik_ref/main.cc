// TEST INFRASTRUCTURE ONLY -- records what the reference's Go1 inverse kinematics computes.  Linked with the reference's own
// go1leg_inverse_kinematics.cc and inverse_kinematics_go1.cc, compiled where they lie against the stand-ins under shim/
// (tests/ik_ref/record.py).
//   ik_ref <in> <out>     files of doubles
//   in:   n_leg, then n_leg x (x y z bend) feet in the hip frame; n_body, then n_body x 12 feet in the base frame (LF RF LH RH)
//   out:  8 constants (base2hip_LF_ 3, hfe_to_haa_z 3, length_thigh, length_shank), n_leg x 3 angles of GetJointAngles,
//         n_body x 12 angles of GetAllJointAngles
#include <cmath>
#include <cstdio>
#include <map>
#include <vector>

#include <Eigen/Dense>
#include <xpp_vis/inverse_kinematics.h>

#define private public   // the constants are private members; the layout is unchanged
#include <towr/models/go1/go1leg_inverse_kinematics.h>
#include <towr/models/go1/inverse_kinematics_go1.h>
#undef private

static bool read_all(const char* path, std::vector<double>& v) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  double buf[4096];
  size_t n;
  while ((n = std::fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: ik_ref <in> <out>\n");
    return 2;
  }
  std::vector<double> in, out;
  if (!read_all(argv[1], in) || in.empty()) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  size_t at = 0;
  const size_t n_leg = (size_t)in[at++];
  if (in.size() < at + 4 * n_leg + 1) {
    std::fprintf(stderr, "truncated input\n");
    return 2;
  }
  xpp::InverseKinematicsGo1 body;
  const xpp::Go1legInverseKinematics& leg = body.leg;
  for (int d = 0; d < 3; ++d) out.push_back(body.base2hip_LF_[d]);
  for (int d = 0; d < 3; ++d) out.push_back(leg.hfe_to_haa_z[d]);
  out.push_back(leg.length_thigh);
  out.push_back(leg.length_shank);
  for (size_t i = 0; i < n_leg; ++i, at += 4) {
    const Eigen::Vector3d p(in[at], in[at + 1], in[at + 2]);
    const Eigen::Vector3d q =
        leg.GetJointAngles(p, in[at + 3] != 0.0 ? xpp::Go1legInverseKinematics::Backward : xpp::Go1legInverseKinematics::Forward);
    for (int j = 0; j < 3; ++j) out.push_back(q[j]);
  }
  const size_t n_body = (size_t)in[at++];
  if (in.size() != at + 12 * n_body) {
    std::fprintf(stderr, "truncated input\n");
    return 2;
  }
  for (size_t i = 0; i < n_body; ++i, at += 12) {
    std::vector<Eigen::Vector3d> feet;
    for (int e = 0; e < 4; ++e) feet.emplace_back(in[at + 3 * e], in[at + 3 * e + 1], in[at + 3 * e + 2]);
    const xpp::Joints q = body.GetAllJointAngles(xpp::EndeffectorsPos(feet));
    for (const Eigen::VectorXd& l : q.legs())
      for (int j = 0; j < 3; ++j) out.push_back(l[j]);
  }
  std::FILE* f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
    std::fprintf(stderr, "cannot write %s\n", argv[2]);
    return 2;
  }
  std::fclose(f);
  return 0;
}
