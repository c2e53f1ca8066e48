// TEST INFRASTRUCTURE ONLY -- stand-in for the generated header of fpowr's FootstepPlan message (see ../ros/ros.h).
#pragma once
#include <vector>

#include <fpowr/ContactDatum.h>

namespace fpowr {
struct FootstepPlan {
  std::vector<ContactDatum> contact_data;
};
}  // namespace fpowr
