#pragma once
#include <stdint.h>

#include "../start_table.h"
#include "common.h"
#include "spline_math.h"
#include "terrain.h"

namespace twr {
// ---------------------------------------------------------------- x0, x_l, x_u of a planning request (twr_batch_start)
// Structure::InitialGuess + VariableBounds for a whole batch from request records in device memory: the start table of every
// structure (start_table.h) says where each variable's value and bounds come from, and the decode is the header's, the same
// functions Structure::StartHost runs on the CPU.
//
// A workgroup (kStartItem = 256 threads) takes one work item, a run of <= 256 consecutive variables of one problem:
//   1. the problem's request record goes to LDS (36 doubles);
//   2. thread e < n_ee forms the endpoints of ee-motion e and ee-force e -- the final foothold is the goal plus the nominal
//      stance turned by the goal's yaw, its z the terrain's -- and thread 64 (another wave: it runs beside the feet) those of
//      base-lin and base-ang, whose final z is the terrain at the goal minus the stance height.  1 + n_ee terrain evaluations
//      through the structure's DevStruct, so through the map pointer and centre a live update leaves there;
//   3. after the barrier thread t decodes variable v0 + t from its 8-byte record and stores x0 / x_l / x_u: three coalesced
//      8-byte stores per lane, every output element written once, no atomics.  24 bytes written, 8 read per variable.
// Trigonometry: sincos_fast (spline_math.h; within 1.51 ulp of sin / cos), exact at yaw = 0 (s = +-0, c = 1), so that
// a request without a turn gives the host's bits; with a turn the footholds differ from libm's by rounding.
// Containment: the request enters as VALUES only.  The one place an index is computed from it is terrain_eval, whose cell
// lookups carry their own range checks (terrain.h) -- a NaN, infinite or huge goal, yaw or foot position gives NaN / the
// out-of-map height in the variables that descend from it and nothing else; every table index (spline, node, slot, duration)
// comes from the host-built record.
TWR_DEV void start_foot_ends(const StartHeader* __restrict__ H, const DevStruct* __restrict__ S, const double* __restrict__ rq, int e,
                             StartEnd* __restrict__ ends) {
  const double *lin1 = rq + 12, *ang1 = rq + 18, *ee0 = rq + 24;
  double sz, cz, fe[3], f[3];
  sincos_fast(ang1[2], &sz, &cz);
  const double nb[3] = {H->stance[e][0], H->stance[e][1], H->stance[e][2]};
  start_foothold(lin1, sz, cz, nb, fe);
  fe[2] = terrain_eval(S, S->terrain_id, S->flat_height, fe[0], fe[1]).h;
  const double a[3] = {ee0[3 * e], ee0[3 * e + 1], ee0[3 * e + 2]};
  StartEnd m, fo;
  start_end(a, fe, H->T, m);
  start_force(H->mass, H->gravity, H->n_ee, f);
  start_end(f, f, H->T, fo);
  ends[2 + e] = m;
  ends[2 + kMaxEE + e] = fo;
}
TWR_DEV void start_base_ends(const StartHeader* __restrict__ H, const DevStruct* __restrict__ S, const double* __restrict__ rq,
                             StartEnd* __restrict__ ends) {
  const double lin0[3] = {rq[0], rq[1], rq[2]}, ang0[3] = {rq[6], rq[7], rq[8]};
  const double lin1[3] = {rq[12], rq[13], rq[14]}, ang1[3] = {rq[18], rq[19], rq[20]};
  const double stance0[3] = {H->stance[0][0], H->stance[0][1], H->stance[0][2]};
  double fl[3];
  start_final_base(lin1, terrain_eval(S, S->terrain_id, S->flat_height, lin1[0], lin1[1]).h, stance0, fl);
  StartEnd l, a;
  start_end(lin0, fl, H->T, l);
  start_end(ang0, ang1, H->T, a);
  ends[0] = l;
  ends[1] = a;
}
// variable i of the problem: decode and store (x / lower / upper: the problem's, each may be null)
TWR_DEV void start_put(const StartHeader* __restrict__ H, const char* __restrict__ table, const StartEnd* __restrict__ ends,
                       const int32_t* __restrict__ nm1, const double* __restrict__ rq, int i, double* __restrict__ x,
                       double* __restrict__ lower, double* __restrict__ upper) {
  const StartRec r = tbl<StartRec>(table, H->o_rec)[i];
  if (x) x[i] = start_value(r, ends, nm1, tbl<double>(table, H->o_dur));
  double lo, up;
  start_bounds(r, rq, lo, up);
  if (lower) lower[i] = lo;
  if (upper) upper[i] = up;
}
}  // namespace twr
