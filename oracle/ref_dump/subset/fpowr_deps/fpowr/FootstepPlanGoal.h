// TEST INFRASTRUCTURE ONLY -- stand-in for the goal type actionlib generates for fpowr's FootstepPlan action (see
// ../ros/ros.h for the rules).  Members as the extractors use them: args->terrain (the planar terrain message),
// args->start_state.{LF,RF,LH,RH}_ee_point.{x,y} (read for the log line of the start planes only) and
// args->state_sample_times (iterated as doubles).  roscpp's <Message>ConstPtr is a shared pointer to the const message
// (boost::shared_ptr there; the extractors only dereference it).
#pragma once
#include <memory>
#include <vector>

#include <convex_plane_decomposition_msgs/PlanarTerrain.h>

namespace fpowr {
struct FootstepPlanGoal {
  struct Point {
    double x = 0.0, y = 0.0, z = 0.0;
  };
  struct {
    Point LF_ee_point, RF_ee_point, LH_ee_point, RH_ee_point;
  } start_state;
  convex_plane_decomposition_msgs::PlanarTerrain terrain;
  std::vector<double> state_sample_times;
};
using FootstepPlanGoalConstPtr = std::shared_ptr<const FootstepPlanGoal>;
}  // namespace fpowr
