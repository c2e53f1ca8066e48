// TEST INFRASTRUCTURE ONLY -- stand-in for <boost/geometry.hpp> (see ../ros/ros.h for the rules of these stand-ins):
// model::d2::point_xy<double>, model::polygon<point> (the default: clockwise, closed), append(ring, point) and
// distance(point, polygon), the members fpowr's nearest_plane_lookup.h uses.  It is a statement of its own of what
// oracle/towr_oracle.cc restates for the oracle; the two are kept apart on purpose, and tests/test_ros_subset.py checks
// this one against a brute-force numpy computation.
//
// Published behaviour (Boost.Geometry 1.71: algorithms/detail/distance/point_to_geometry.hpp,
// strategies/cartesian/point_in_poly_winding.hpp, strategies/cartesian/distance_projected_point.hpp,
// algorithms/detail/within/point_in_geometry.hpp):
//   * nothing corrects the polygon: without bg::correct the points of the outer ring are walked in the order given and
//     only consecutive points form an edge -- a ring whose last point does not repeat the first has no closing edge,
//     and the orientation of the ring plays no role (the winding count is compared with zero);
//   * distance(point, polygon) is 0 when the point is inside or on the outer ring (no inner rings here), otherwise the
//     distance from the point to the outer ring;
//   * inside / on / outside is the winding strategy over the given edges: a ring of fewer than 4 points (the minimum of
//     a closed ring) holds nothing; an edge that spans the point's x strictly counts +2 or -2 by its x direction, an
//     edge with exactly one end at the point's x counts +1 or -1, in both cases only when the point lies on the positive
//     side for that direction, i.e. strictly above the edge; an edge with both ends at the point's x counts nothing;
//     a point on an edge is "on"; a non-zero total is "inside";
//   * the distance to a ring is the smallest projected-point distance over the given edges (compared squared, one
//     square root at the end): with v = b - a, w = p - a, c1 = w . v, c2 = v . v the closest point of edge a b is a when
//     c1 <= 0, b when c2 <= c1, else a + (c1 / c2) v; an empty ring is at distance 0, a single point is its own edge.
// Deviation: Boost compares coordinates and the side determinant with a tolerance of a few ulps; here the comparisons
// are exact.  It only matters for a point within rounding of an edge, where either answer is a distance of almost 0.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace boost {
namespace geometry {

namespace model {
namespace d2 {
template <typename T>
class point_xy {
 public:
  point_xy() = default;
  point_xy(T x, T y) : x_(x), y_(y) {}
  T x() const { return x_; }
  T y() const { return y_; }

 private:
  T x_ = T(), y_ = T();
};
}  // namespace d2

template <typename Point>
class polygon {
 public:
  using ring_type = std::vector<Point>;
  ring_type& outer() { return outer_; }
  const ring_type& outer() const { return outer_; }

 private:
  ring_type outer_;
};
}  // namespace model

template <typename Point>
void append(std::vector<Point>& ring, const Point& p) {
  ring.push_back(p);
}

namespace standin {

// > 0 when p is left of the directed line a -> b, < 0 right, 0 on it (side_by_triangle)
template <typename Point>
double side(const Point& a, const Point& b, const Point& p) {
  return (b.x() - a.x()) * (p.y() - a.y()) - (b.y() - a.y()) * (p.x() - a.x());
}

// +1 inside, 0 on an edge, -1 outside: the winding count in half turns over the edges as given
template <typename Point>
int covered(const std::vector<Point>& ring, const Point& p) {
  if (ring.size() < 4) return -1;
  int half_turns = 0;
  for (std::size_t i = 0; i + 1 < ring.size(); ++i) {
    const Point &a = ring[i], &b = ring[i + 1];
    const bool a_on = a.x() == p.x(), b_on = b.x() == p.x();
    if (a_on && b_on) {   // an edge along the vertical through p
      const double lo = a.y() < b.y() ? a.y() : b.y(), hi = a.y() < b.y() ? b.y() : a.y();
      if (lo <= p.y() && p.y() <= hi) return 0;
      continue;
    }
    if (a_on || b_on) {   // one end on the vertical: half a turn, decided by that end alone
      const Point& e = a_on ? a : b;
      if (p.y() == e.y()) return 0;
      const bool rightwards = a_on ? b.x() > p.x() : a.x() < p.x();
      if (p.y() > e.y()) half_turns += rightwards ? 1 : -1;
      continue;
    }
    const bool rightwards = a.x() < p.x() && p.x() < b.x(), leftwards = b.x() < p.x() && p.x() < a.x();
    if (!rightwards && !leftwards) continue;
    const double s = side(a, b, p);
    if (s == 0.0) return 0;
    if (rightwards && s > 0.0) half_turns += 2;    // above an edge that runs to the right: on its left
    if (leftwards && s < 0.0) half_turns -= 2;     // above an edge that runs to the left: on its right
  }
  return half_turns != 0 ? 1 : -1;
}

template <typename Point>
double squared_to_edge(const Point& a, const Point& b, const Point& p) {
  const double vx = b.x() - a.x(), vy = b.y() - a.y(), wx = p.x() - a.x(), wy = p.y() - a.y();
  const double c1 = wx * vx + wy * vy;
  double qx = a.x(), qy = a.y();
  if (!(c1 <= 0.0)) {   // (as published: `c1 <= 0` takes a, so a NaN c1 -- an infinite coordinate -- goes on to the projection)
    const double c2 = vx * vx + vy * vy;
    if (c2 <= c1) {
      qx = b.x();
      qy = b.y();
    } else {
      const double f = c1 / c2;
      qx = a.x() + f * vx;
      qy = a.y() + f * vy;
    }
  }
  return (p.x() - qx) * (p.x() - qx) + (p.y() - qy) * (p.y() - qy);
}

template <typename Point>
double to_ring(const std::vector<Point>& ring, const Point& p) {
  if (ring.empty()) return 0.0;
  if (ring.size() == 1) return std::sqrt(squared_to_edge(ring[0], ring[0], p));
  double best = squared_to_edge(ring[0], ring[1], p);
  for (std::size_t i = 1; i + 1 < ring.size(); ++i) {
    const double d = squared_to_edge(ring[i], ring[i + 1], p);
    if (d < best) best = d;
  }
  return std::sqrt(best);
}

}  // namespace standin

template <typename Point>
double distance(const Point& p, const model::polygon<Point>& poly) {
  if (standin::covered(poly.outer(), p) >= 0) return 0.0;
  return standin::to_ring(poly.outer(), p);
}

}  // namespace geometry
}  // namespace boost
