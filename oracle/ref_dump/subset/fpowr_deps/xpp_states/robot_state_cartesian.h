// TEST INFRASTRUCTURE ONLY -- stand-in for xpp_states/robot_state_cartesian.h (see ../ros/ros.h for the rules).
// Published behaviour (xpp_states/src/robot_state_cartesian.cc): RobotStateCartesian(n_ee) sizes ee_motion_,
// ee_forces_ and ee_contact_ to n_ee, sets every contact flag to true and t_global_ to 0; base_ is a State3d.
#pragma once
#include <xpp_states/endeffectors.h>
#include <xpp_states/state.h>

namespace xpp {

class RobotStateCartesian {
 public:
  explicit RobotStateCartesian(int n_ee) : ee_motion_(n_ee), ee_forces_(n_ee), ee_contact_(n_ee, true) {
    ee_forces_.SetAll(Eigen::Vector3d::Zero());
  }
  State3d base_;
  EndeffectorsMotion ee_motion_;
  Endeffectors<Eigen::Vector3d> ee_forces_;
  EndeffectorsContact ee_contact_;
  double t_global_ = 0.0;
};

}  // namespace xpp
