// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_vis/inverse_kinematics.h with the two xpp_states containers it hands around:
// feet in the base frame in, the legs' joint angles out.
#pragma once
#include <Eigen/Dense>
#include <vector>

namespace xpp {
class EndeffectorsPos {
 public:
  explicit EndeffectorsPos(std::vector<Eigen::Vector3d> p) : p_(std::move(p)) {}
  std::vector<Eigen::Vector3d> ToImpl() const { return p_; }

 private:
  std::vector<Eigen::Vector3d> p_;
};
class Joints {
 public:
  explicit Joints(std::vector<Eigen::VectorXd> q) : q_(std::move(q)) {}
  const std::vector<Eigen::VectorXd>& legs() const { return q_; }

 private:
  std::vector<Eigen::VectorXd> q_;
};
class InverseKinematics {
 public:
  using Vector3d = Eigen::Vector3d;
  InverseKinematics() = default;
  virtual ~InverseKinematics() = default;
  virtual Joints GetAllJointAngles(const EndeffectorsPos& pos_b) const = 0;
  virtual int GetEECount() const = 0;
};
}  // namespace xpp
