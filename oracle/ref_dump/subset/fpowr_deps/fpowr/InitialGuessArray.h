// TEST INFRASTRUCTURE ONLY -- stand-in for the generated header of fpowr's InitialGuessArray message (see ../ros/ros.h).
#pragma once
#include <vector>

#include <fpowr/InitialGuess.h>

namespace fpowr {
struct InitialGuessArray {
  std::vector<InitialGuess> initial_guesses;
};
}  // namespace fpowr
