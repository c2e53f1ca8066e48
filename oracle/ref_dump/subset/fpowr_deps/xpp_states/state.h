// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/state.h (see ../ros/ros.h for the rules of these stand-ins).
// Published behaviour (xpp, github.com/leggedrobotics/xpp, xpp_states/include/xpp_states/state.h):
//   StateLinXd    position p_, velocity v_, acceleration a_ of a given dimension, zero after construction
//   StateLin3d    the 3-dimensional StateLinXd; can be built from / assigned a StateLinXd of dimension 3
//   StateAng3d    orientation q (Eigen::Quaterniond, identity after construction), angular velocity w, acceleration wd
//   State3d       lin (StateLin3d) and ang (StateAng3d)
#pragma once
#include <Eigen/Dense>
#include <cassert>

namespace xpp {

class StateLinXd {
 public:
  Eigen::VectorXd p_, v_, a_;
  explicit StateLinXd(int dim = 0) : p_(Eigen::VectorXd::Zero(dim)), v_(Eigen::VectorXd::Zero(dim)), a_(Eigen::VectorXd::Zero(dim)) {}
};

class StateLin3d : public StateLinXd {
 public:
  StateLin3d() : StateLinXd(3) {}
  StateLin3d(const StateLinXd& s) : StateLinXd(3) {   // NOLINT: xpp converts implicitly, asserting the dimension
    assert(s.p_.rows() == 3);
    p_ = s.p_;
    v_ = s.v_;
    a_ = s.a_;
  }
};

class StateAng3d {
 public:
  Eigen::Quaterniond q;   // (the Quaternion of the Eigen in use starts as it does there; GetTrajectory assigns it)
  Eigen::Vector3d w = Eigen::Vector3d::Zero(), wd = Eigen::Vector3d::Zero();
};

class State3d {
 public:
  StateLin3d lin;
  StateAng3d ang;
};

}  // namespace xpp
