#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../device_tables.h"
#include "common.h"
#include "spline_math.h"

namespace twr {
// ---------------------------------------------------------------- range-of-motion item
// RangeOfMotionConstraint::{UpdateConstraintAtInstance, UpdateJacobianAtInstance}
// (range_of_motion_constraint.cc:58-109) for one (time node, ee).
struct RomX {
  double bl[12], ba[12], m[12];
};
TWR_DEV uint64_t rom_slots(const RomRec& r) { return ((uint64_t)r.slots[1] << 32) | r.slots[0]; }
// What a lane of rom_kernel carries through the pipeline, as loaded (raw: nothing is computed from the records at issue
// time, so a prefetch never waits): its time node's record -- fetched THREE slices ahead, because it also says which segment
// record the lane reads -- and its segment's record, fetched two slices ahead.
TWR_DEV RomNode rom_load_node(const RomWork& w, int lane) { return gptr<RomNode>(w.nodes)[min(lane, w.cnt - 1)]; }
TWR_DEV RomSeg rom_load_seg(const RomWork& w, const RomNode& nd) { return gptr<RomSeg>(w.segs)[(nd.seg >> (3 * w.ee)) & 7u]; }
// the lane's view in the form the math is written for (fields of the optimised-timings record RomRec)
TWR_DEV RomRec rom_rec_of(const RomWork& w, const RomNode& nd, const RomSeg& sg, int lane) {
  RomRec r;
  r.tb = nd.tb; r.iTb = nd.iTb;
  r.tm = nd.t - sg.t0; r.iTm = sg.iTm;
  r.q6 = nd.q6;
  r.xbase = sg.xbase;
  r.voff = sg.voff0 + (min(lane, w.cnt - 1) - sg.kfirst) * sg.node_vals;   // relative to the slice's first value
  r.meta = sg.meta;
  r.slots[0] = sg.slots[0]; r.slots[1] = sg.slots[1];
  r.pad[0] = r.pad[1] = 0;
  return r;
}
TWR_DEV void rom_load_x(const RomWork& w, const RomNode& nd, const RomSeg& sg, const double* __restrict__ x, RomX& X) {
  const double* xp = x + w.x_off;
  const double* xl = xp + w.off_lin + nd.q6;
  const double* xa = xp + w.off_ang + nd.q6;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    X.bl[i] = xl[i];
    X.ba[i] = xa[i];
  }
  gather12(xp, sg.xbase, ((uint64_t)sg.slots[1] << 32) | sg.slots[0], X.m);
}
TWR_DEV void rom_item(const RomWork& w, const RomRec& r, const RomX& X, double* __restrict__ gst, double* __restrict__ stage,
                      int par, int vbase, int trash, int lane, bool want_g, bool want_j) {
  const int soff = par + r.voff - vbase;
  double wP[4];
  hermite_pos(r.tb, r.iTb, wP);
  double c[3], e[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    c[d] = wP[0] * X.bl[d] + wP[1] * X.bl[3 + d] + wP[2] * X.bl[6 + d] + wP[3] * X.bl[9 + d];
    e[d] = wP[0] * X.ba[d] + wP[1] * X.ba[3 + d] + wP[2] * X.ba[6 + d] + wP[3] * X.ba[9 + d];
  }
  const uint64_t slots = rom_slots(r);
  double wm[4], p[3], v[3];
  ee_point(slots, meta_shared(r.meta), r.tm, r.iTm, X.m, wm, p);
#pragma unroll
  for (int d = 0; d < 3; ++d) v[d] = p[d] - c[d];
  Rot ro;
  rotation(e, ro);
  if (want_g) {
    double gv[3];
    matTvec(ro.R, v, gv);  // b_R_w (p - c)
    double* go = gst + 3 * lane;  // staged in LDS, written out coalesced with the Jacobian slice
    go[0] = gv[0]; go[1] = gv[1]; go[2] = gv[2];
  }
  if (!want_j) return;
  // DerivOfRotVecMult(t, v, inverse=true) = d(R^T v)/d e_d (euler_converter.cc:223-239).  With
  // dR/d e_d = [M_d]x R (M_d = rotation axis d of the ZYX sequence = column d of M) this is R^T (v x M_d).
  double ux[3], uy[3], uz[3];
  {
    const double Mx[3] = {ro.cy * ro.cz, ro.cy * ro.sz, -ro.sy}, My[3] = {-ro.sz, ro.cz, 0.0};
    double tx[3], ty[3];
    cross3(v, Mx, tx);
    cross3(v, My, ty);
    const double tz[3] = {v[1], -v[0], 0.0};  // v x e_z
    matTvec(ro.R, tx, ux);
    matTvec(ro.R, ty, uy);
    matTvec(ro.R, tz, uz);
  }
  const int nm = meta_nslots(r.meta);
  const int rs[3] = {soff, soff + 20 + nm, soff + 44 + 2 * nm};
  const int mo[3] = {20, 24, 24};
#pragma unroll
  for (int row = 0; row < 3; ++row) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int d = 0; d < 3; ++d) TWR_ROM_PUT(rs[row] + 3 * j + d, -ro.R[d][row] * wP[j]);  // -R^T J_c
      if (row == 0) {  // row 0 of R^T v does not depend on roll
        TWR_ROM_PUT(rs[0] + 12 + 2 * j + 0, wP[j] * uy[0]);
        TWR_ROM_PUT(rs[0] + 12 + 2 * j + 1, wP[j] * uz[0]);
      } else {
        TWR_ROM_PUT(rs[row] + 12 + 3 * j + 0, wP[j] * ux[row]);
        TWR_ROM_PUT(rs[row] + 12 + 3 * j + 1, wP[j] * uy[row]);
        TWR_ROM_PUT(rs[row] + 12 + 3 * j + 2, wP[j] * uz[row]);
      }
#pragma unroll
      for (int d = 0; d < 3; ++d) {  // R^T J_p
        const int sl = (int)((slots >> (4 * (j * 3 + d))) & 0xF);
        TWR_ROM_PUT(sl != 0xF ? rs[row] + mo[row] + sl : trash, ro.R[d][row] * wm[j]);
      }
    }
  }
}
}  // namespace twr
