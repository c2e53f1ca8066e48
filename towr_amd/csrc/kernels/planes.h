// Nearest plane of a footstep (twr_batch_contact_planes): the device functions under plane_kernel of util_tu.hip, includable on
// their own (tests/plane_probe.hip runs them per ring and per point).
#pragma once
#include <stdint.h>

#include "common.h"

namespace twr {
// fpowr::NearestPlaneLookup::GetNearestPlaneIndex (nearest_plane_lookup.h:62-84) for every (problem, footstep state,
// end-effector) of a contact plan: boost::geometry::distance(point, polygon) restated from Boost 1.71 (winding
// strategy for covered_by, projected-point distance to the ring's consecutive points, no closing edge added; exact
// coordinate comparisons where boost allows a few ulp).  One thread per foot, polygons read from global memory.
// Every product and sum below is one correctly rounded operation, as in the reference's build: contraction is switched off in
// each body and the operators are written plainly -- __dmul_rn and its kin are ordinary operators compiled with the header's
// own setting in this toolchain, and were fused into multiply-adds once inlined.  The sign of a tiny determinant and the order of
// two almost equal distances must not depend on that.
TWR_DEV int ring_side(const double* __restrict__ xy, int n, double px, double py) {   // 1 inside, 0 boundary, -1 outside
#pragma clang fp contract(off)
  if (n < 4) return -1;
  int count = 0;
  for (int i = 0; i + 1 < n; ++i) {
    const double s1x = xy[2 * i], s1y = xy[2 * i + 1], s2x = xy[2 * i + 2], s2y = xy[2 * i + 3];
    const bool eq1 = s1x == px, eq2 = s2x == px;
    int c = 0;
    if (eq1 && eq2) {
      if ((s1y <= py && s2y >= py) || (s2y <= py && s1y >= py)) return 0;
    } else {
      c = eq1 ? (s2x > px ? 1 : -1) : eq2 ? (s1x > px ? -1 : 1) : (s1x < px && s2x > px) ? 2 : (s2x < px && s1x > px) ? -2 : 0;
    }
    if (c != 0) {
      int side;
      if (c == 1 || c == -1) {
        const double sey = eq1 ? s1y : s2y;
        side = py == sey ? 0 : (py > sey ? c : -c);   // (a NaN py is neither on the end nor above it)
      } else {
        const double det = (s2x - s1x) * (py - s1y) - (s2y - s1y) * (px - s1x);
        if (det != det) continue;                     // a NaN py: neither on the edge nor on a side of it
        side = det > 0 ? 1 : (det < 0 ? -1 : 0);
      }
      if (side == 0) return 0;
      if (side * c > 0) count += c;
    }
  }
  return count == 0 ? -1 : 1;
}
TWR_DEV double ring_distance(const double* __restrict__ xy, int n, double px, double py) {
#pragma clang fp contract(off)
  if (n == 0) return 0.0;
  auto comparable = [&](double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
    const double vx = bx - ax, vy = by - ay, wx = px - ax, wy = py - ay;
    const double c1 = wx * vx + wy * vy;
    if (c1 <= 0) return wx * wx + wy * wy;
    const double c2 = vx * vx + vy * vy;
    if (c2 <= c1) return (px - bx) * (px - bx) + (py - by) * (py - by);
    const double b = c1 / c2, qx = ax + b * vx, qy = ay + b * vy;
    return (px - qx) * (px - qx) + (py - qy) * (py - qy);
  };
  if (n == 1) return sqrt(comparable(xy[0], xy[1], xy[0], xy[1]));
  double best = comparable(xy[0], xy[1], xy[2], xy[3]);
  for (int i = 0; i + 1 < n; ++i) {
    const double c = comparable(xy[2 * i], xy[2 * i + 1], xy[2 * i + 2], xy[2 * i + 3]);
    if (c == 0.0) return 0.0;
    if (c < best) best = c;
  }
  return sqrt(best);
}
// the first polygon with the smallest distance to (px, py), -1 without one (or when no distance is below DBL_MAX); polygon i is
// the points poly_start[i] .. poly_start[i + 1] of poly_xy
TWR_DEV int nearest_plane(const double* __restrict__ poly_xy, const int32_t* __restrict__ poly_start, int n_polys, double px, double py) {
  int nearest = -1;
  double min_distance = 1.7976931348623157e308;
  for (int i = 0; i < n_polys; ++i) {
    const double* xy = poly_xy + 2 * poly_start[i];
    const int n = poly_start[i + 1] - poly_start[i];
    const double distance = ring_side(xy, n, px, py) >= 0 ? 0.0 : ring_distance(xy, n, px, py);
    if (distance < min_distance) {
      min_distance = distance;
      nearest = i;
    }
  }
  return nearest;
}
}  // namespace twr
