// TEST INFRASTRUCTURE ONLY -- stand-in for convex_plane_decomposition_msgs/PlanarTerrain.h (see ../ros/ros.h for the
// rules).  What nearest_plane_lookup.h reads of the message: terrain.planarRegions, and per region
// plane_parameters.{position.{x,y,z}, orientation.{x,y,z,w}} (a geometry_msgs/Pose: float64 fields) and
// boundary.outer_boundary.points[i].{x,y} (Point2d of the published package: float32 fields; the recorded fixtures
// use boundary points that float32 holds exactly, so nothing depends on the width).  `gridmap` (a grid_map_msgs/GridMap
// there) is the member the `Grid` terrain reads; it is not used here and stays an empty placeholder.
#pragma once
#include <vector>

namespace convex_plane_decomposition_msgs {

struct Point2d {
  float x = 0.0f, y = 0.0f;
};
struct Polygon2d {
  std::vector<Point2d> points;
};
struct Polygon2dWithHoles {
  Polygon2d outer_boundary;
};
struct Pose {
  struct { double x = 0.0, y = 0.0, z = 0.0; } position;
  struct { double x = 0.0, y = 0.0, z = 0.0, w = 1.0; } orientation;
};
struct PlanarRegion {
  Pose plane_parameters;
  Polygon2dWithHoles boundary;
};
struct PlanarTerrain {
  std::vector<PlanarRegion> planarRegions;
  struct {} gridmap;
};

}  // namespace convex_plane_decomposition_msgs
