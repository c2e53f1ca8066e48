#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"

namespace twr {
// ---------------------------------------------------------------- terrain
// HeightMap example terrains: height, slopes, second derivative (height_map_examples.{h,cc}).
// Only Gap has curvature (GetHeightDerivWrtXX); Stairs overrides only GetHeight (zero slope).
struct Terr {
  double h, hx, hy, hxx;
};
// HeightMapFromCSV (include/towr/terrain/height_map_from_csv.h:29-109): piecewise-constant heights per cell;
// the "slope" is the step to the next / previous cell smeared over eps on the lower side of the step, checked
// in the reference's order (next cell first); second derivatives are the base class's zeros.
// Every threshold is the reference's: two separately rounded operations (x_end = cell * res, then x_end - eps).  A fused
// multiply-add rounds (c + 1) res - eps once and lands on another double for about a quarter of the cells, which turns a slope
// of diff / eps into 0 (or back) for a foothold on the threshold: no contraction in this function.
TWR_DEV Terr grid_eval(const DevStruct* __restrict__ S, double x, double y) {
#pragma clang fp contract(off)
  Terr t = {0.0, 0.0, 0.0, 0.0};
  const double* __restrict__ grid = reinterpret_cast<const double*>(S->grid_ptr);
  const int rows = S->grid_rows, cols = S->grid_cols;
  const double res = S->grid_res, eps = S->grid_eps;
  const long xc = (long)(x / res), yc = (long)(y / res);   // truncation toward zero, like static_cast<size_t>
  if (xc < 0 || yc < 0 || xc >= cols || yc >= rows) return t;
  const double h0 = grid[yc * cols + xc];
  t.h = h0;
#pragma unroll
  for (int dim = 0; dim < 2; ++dim) {
    const double v = dim == 0 ? x : y;
    const long c = dim == 0 ? xc : yc, n = dim == 0 ? cols : rows;
    const long stride = dim == 0 ? 1 : cols;
    double d = 0.0;
    bool done = false;
    if (c + 1 < n) {
      const double diff_end = grid[yc * cols + xc + stride] - h0;
      const double v_end = (double)(c + 1) * res;
      if (diff_end > 0 && v <= v_end && v >= v_end - eps) { d = diff_end / eps; done = true; }
    }
    if (!done && c - 1 >= 0) {
      const double diff_start = h0 - grid[yc * cols + xc - stride];
      const double v_start = (double)c * res;
      if (diff_start < 0 && v >= v_start && v <= v_start + eps) d = diff_start / eps;
    }
    if (dim == 0) t.hx = d; else t.hy = d;
  }
  return t;
}
// Grid (include/towr/terrain/grid_height_map.h:15-60) over the float "elevation" layer of a ROS grid_map.
// gridmap_sample = grid_map's published GridMap::atPosition(layer, position, INTER_LINEAR) for a map with start
// index (0,0) (third party, absent and unpinned in the reference: restated from its published algorithm --
// atPositionLinearInterpolated, GridMapMath getIndexFromPosition / getPositionFromIndex / checkIfPositionWithinMap):
// cell (i,j) centre = map position + length/2 - (index + 1/2) res; index = trunc((position + length/2 - p) / res);
// bilinear over the 2x2 cells around p evaluated in double and rounded to FLOAT; if one of the four cells lies outside
// the map: the nearest cell when p is inside the map, otherwise std::out_of_range, which Grid::GetHeight turns into
// numeric_limits<float>::max() (:41-45).
// No contraction in this function either: the cell centres cx0 / px end in "- res * index", and on a centre line the +- eps
// samples carry weights 1/6 and 5/6, so one exact value in six sits on a float rounding midpoint where the last bit of px decides.
TWR_DEV float gridmap_sample(const DevStruct* __restrict__ S, double x, double y) {
#pragma clang fp contract(off)
  const float* __restrict__ el = reinterpret_cast<const float*>(S->grid_ptr);
  const int sx = S->grid_rows, sy = S->grid_cols;
  const double res = S->grid_res, lx = sx * res, ly = sy * res, mx = S->grid_px, my = S->grid_py;
  const long i0 = (long)(-((x - 0.5 * lx - mx) / res)), j0 = (long)(-((y - 0.5 * ly - my) / res));
  const double tx = mx + 0.5 * lx - x, ty = my + 0.5 * ly - y;
  const bool inside = tx >= 0.0 && ty >= 0.0 && tx < lx && ty < ly;
  const double cx0 = mx + 0.5 * lx - 0.5 * res - res * (double)i0, cy0 = my + 0.5 * ly - 0.5 * res - res * (double)j0;
  const long ia = x >= cx0 ? i0 : i0 + 1, ja = y >= cy0 ? j0 : j0 + 1, ib = ia - 1, jb = ja - 1;
  if (ib >= 0 && jb >= 0 && ia < sx && ja < sy) {
    const double px = mx + 0.5 * lx - 0.5 * res - res * (double)ia, py = my + 0.5 * ly - 0.5 * res - res * (double)ja;
    const double rx = (x - px) / res, ry = (y - py) / res, fx = 1.0 - rx, fy = 1.0 - ry;
    const double f0 = el[ia + ja * (long)sx], f1 = el[ib + ja * (long)sx], f2 = el[ia + jb * (long)sx], f3 = el[ib + jb * (long)sx];
    // the reference's products and sums are separately rounded doubles: plain operators under the pragma above.  (HIP's
    // __dmul_rn / __dadd_rn are inline `*` and `+` that carry the unit's own contraction: the sum written with them
    // compiled to three fused multiply-adds.)
    return (float)(f0 * fx * fy + f1 * rx * fy + f2 * fx * ry + f3 * rx * ry);
  }
  if (inside && i0 >= 0 && j0 >= 0 && i0 < sx && j0 < sy) return el[i0 + j0 * (long)sx];
  return 3.402823466e+38f;  // numeric_limits<float>::max()
}
TWR_DEV Terr gridmap_eval(const DevStruct* __restrict__ S, double x, double y) {
  Terr t = {0.0, 0.0, 0.0, 0.0};
  const double eps = S->grid_eps;
  t.h = (double)gridmap_sample(S, x, y);
  // grid_height_map.h:48-60: the two heights are floats, their difference is a float, the quotient a double
  t.hx = (double)(gridmap_sample(S, x + eps, y) - gridmap_sample(S, x - eps, y)) / (2 * eps);
  t.hy = (double)(gridmap_sample(S, x, y + eps) - gridmap_sample(S, x, y - eps)) / (2 * eps);
  return t;
}
// The analytic maps round like the reference as well: Gap's 2a x + b cancels (62.8 - 60 at x = 1.31), so a fused slope differs from
// the reference's by up to 11 ulp, which every force row on that foothold then carries.
TWR_DEV Terr terrain_eval(const DevStruct* __restrict__ S, int id, double flat_height, double x, double y) {
#pragma clang fp contract(off)
  Terr t = {0.0, 0.0, 0.0, 0.0};
  switch (id) {
    case 7: return grid_eval(S, x, y);
    case 8: return gridmap_eval(S, x, y);
    case 0: t.h = flat_height; break;
    case 1: {  // Block (height_map_examples.cc:40-65)
      const double start = 0.7, len = 3.5, height = 0.5, eps = 0.03, slope = height / eps;
      if (start <= x && x <= start + eps) { t.h = slope * (x - start); t.hx = slope; }
      if (start + eps <= x && x <= start + len) t.h = height;
      break;
    }
    case 2: {  // Stairs (:69-84)
      if (x >= 1.0) t.h = 0.2;
      if (x >= 1.0 + 0.4) t.h = 0.4;
      if (x >= 1.0 + 0.4 + 1.0) t.h = 0.0;
      break;
    }
    case 3: {  // Gap (:88-120, height_map_examples.h:96-111)
      const double gs = 1.0, w = 0.5, hh = 1.5, xc = gs + w / 2.0, ge = gs + w;
      const double a = (4 * hh) / (w * w), b = -(8 * hh * xc) / (w * w), c = -(hh * (w - 2 * xc) * (w + 2 * xc)) / (w * w);
      if (gs <= x && x <= ge) { t.h = a * x * x + b * x + c; t.hx = 2 * a * x + b; t.hxx = 2 * a; }
      break;
    }
    case 4: {  // Slope (:124-157)
      const double ss = 1.0, up = 1.0, dn = 1.0, hc = 0.7, xd = ss + up, xf = xd + dn, sl = hc / up;
      if (x >= ss) { t.h = sl * (x - ss); t.hx = sl; }
      if (x >= xd) { t.h = hc - sl * (x - xd); t.hx = -sl; }
      if (x >= xf) { t.h = 0.0; t.hx = 0.0; }
      break;
    }
    case 5: {  // Chimney (:161-181)
      const double xs = 1.0, len = 1.5, ys = 0.5, sl = 3.0;
      if (xs <= x && x <= xs + len) { t.h = sl * (y - ys); t.hy = sl; }
      break;
    }
    case 6: {  // ChimneyLR (:185-211)
      const double xs = 0.5, len = 1.0, ys = 0.5, sl = 2, xe1 = xs + len, xe2 = xs + 2 * len;
      if (xs <= x && x <= xe1) { t.h = sl * (y - ys); t.hy = sl; }
      if (xe1 <= x && x <= xe2) { t.h = -sl * (y + ys); t.hy = -sl; }
      break;
    }
  }
  return t;
}

// ForceConstraint::{GetValues, FillJacobianBlock} (force_constraint.cc:62-171) for one stance force
// node; terrain basis and its "derivative" per height_map.cc:62-148 (component-wise product, as is).
TWR_DEV void force_core(const DevStruct* __restrict__ S, const double f[3], double px, double py, double* __restrict__ g5,
                        double* __restrict__ st25, bool want_g, bool want_j);
TWR_DEV void force_item(const DevStruct* __restrict__ S, const ForceNode fn, const double* __restrict__ xp,
                        double* __restrict__ g5, double* __restrict__ st25, bool want_g, bool want_j) {
  const double f[3] = {xp[fn.fidx], xp[fn.fidx + 2], xp[fn.fidx + 4]};
  force_core(S, f, xp[fn.hidx], xp[fn.hidx + 1], g5, st25, want_g, want_j);
}
// (f: the node's force, px / py: the stance foothold; the single body of the force rows for node_kernel and node_chunk_kernel)
TWR_DEV void force_core(const DevStruct* __restrict__ S, const double f[3], double px, double py, double* __restrict__ g5,
                        double* __restrict__ st25, bool want_g, bool want_j) {
  const Terr t = terrain_eval(S, S->terrain_id, S->flat_height, px, py);
  const double mu = S->mu;
  const double vb[3][3] = {{-t.hx, -t.hy, 1.0}, {1.0, 0.0, t.hx}, {0.0, 1.0, t.hy}};  // n, t1, t2 (height_map.cc:93-139)
  double nb[3][3], sq[3], nr[3], inv_nr[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    sq[b] = vb[b][0] * vb[b][0] + vb[b][1] * vb[b][1] + vb[b][2] * vb[b][2];
    nr[b] = sqrt(sq[b]);
#pragma unroll
    for (int i = 0; i < 3; ++i) nb[b][i] = vb[b][i] / nr[b];
    inv_nr[b] = nb[b][b == 0 ? 2 : b - 1];  // the component whose entry is 1: n.z, t1.x, t2.y
  }
  double rowv[5][3];  // the five pyramid directions
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    rowv[0][i] = nb[0][i];
    rowv[1][i] = nb[1][i] - mu * nb[0][i];
    rowv[2][i] = nb[1][i] + mu * nb[0][i];
    rowv[3][i] = nb[2][i] - mu * nb[0][i];
    rowv[4][i] = nb[2][i] + mu * nb[0][i];
  }
  if (want_g) {
#pragma unroll
    for (int r = 0; r < 5; ++r) g5[r] = f[0] * rowv[r][0] + f[1] * rowv[r][1] + f[2] * rowv[r][2];
  }
  if (!want_j) return;
  // second derivatives: only h_xx can be non-zero (GetSecondDerivativeOfHeightWrt, height_map.cc:150-163)
  double drow[2][5];  // [dim][row]: f . d(direction)/d(foothold dim)
#pragma unroll
  for (int dim = 0; dim < 2; ++dim) {
    const double hx_d = dim == 0 ? t.hxx : 0.0;  // d(hx)/d(dim)
    const double hy_d = 0.0;                     // d(hy)/d(dim)
    const double dv[3][3] = {{-hx_d, -hy_d, 0.0}, {0.0, 0.0, hx_d}, {0.0, 0.0, hy_d}};
    double db[3][3];
#pragma unroll
    for (int b = 0; b < 3; ++b)
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        // (1 / sq) (|v| unit - v[dim] v[i] / |v|).  On the diagonal that is |v| - v[dim]^2 / |v|, which cancels where the slope
        // is steep (all but 1 / 145 of it at Gap's edges); written as the sum of the other two squares over |v| it does not
        const double rest = vb[b][1 - dim] * vb[b][1 - dim] + vb[b][2] * vb[b][2];
        const double inner = i == dim ? rest * inv_nr[b] : 0.0 - vb[b][dim] * nb[b][i];
        const double outer = (1.0 / sq[b]) * inner;
        db[b][i] = outer * dv[b][i];
      }
    double dr[5][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      dr[0][i] = db[0][i];
      dr[1][i] = db[1][i] - mu * db[0][i];
      dr[2][i] = db[1][i] + mu * db[0][i];
      dr[3][i] = db[2][i] - mu * db[0][i];
      dr[4][i] = db[2][i] + mu * db[0][i];
    }
#pragma unroll
    for (int r = 0; r < 5; ++r) drow[dim][r] = f[0] * dr[r][0] + f[1] * dr[r][1] + f[2] * dr[r][2];
  }
#pragma unroll
  for (int r = 0; r < 5; ++r) {  // columns: foothold x, y (ee-motion) then force px, py, pz
    st25[5 * r + 0] = drow[0][r];
    st25[5 * r + 1] = drow[1][r];
    st25[5 * r + 2] = rowv[r][0];
    st25[5 * r + 3] = rowv[r][1];
    st25[5 * r + 4] = rowv[r][2];
  }
}
}  // namespace twr
