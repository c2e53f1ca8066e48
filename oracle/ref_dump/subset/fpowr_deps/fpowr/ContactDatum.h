// TEST INFRASTRUCTURE ONLY -- stand-in for the message header ROS generates for fpowr's ContactDatum (see
// ../ros/ros.h for the rules): a plain struct with the two members footstep_plan_extractor.h fills.
#pragma once
#include <vector>

namespace fpowr {
struct ContactDatum {
  std::vector<int> contact_set;   // one plane index per end-effector, -1 = in the air
  double duration = 0.0;
};
}  // namespace fpowr
