// TEST INFRASTRUCTURE ONLY -- stand-in for the generated header of fpowr's InitialGuess message (see ../ros/ros.h).
#pragma once
#include <vector>

namespace fpowr {
struct InitialGuess {
  double time = 0.0;
  std::vector<double> state, controls;
};
}  // namespace fpowr
