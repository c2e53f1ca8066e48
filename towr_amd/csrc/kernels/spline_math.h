#pragma once
#include <stdint.h>

#include "common.h"

namespace twr {
// ---------------------------------------------------------------- cubic Hermite weights
// d{pos,vel,acc}/d{p0,v0,p1,v1} of CubicHermitePolynomial (src/polynomial.cc:140-234); iT = 1/T comes
// from the tables (one IEEE division on the host instead of one per lane and spline).
TWR_DEV void hermite_pos(double t, double iT, double w[4]) {
  const double iT2 = iT * iT, iT3 = iT2 * iT;
  const double t2 = t * t, t3 = t2 * t;
  w[0] = 2.0 * t3 * iT3 - 3.0 * t2 * iT2 + 1.0;
  w[1] = t - 2.0 * t2 * iT + t3 * iT2;
  w[2] = 3.0 * t2 * iT2 - 2.0 * t3 * iT3;
  w[3] = t3 * iT2 - t2 * iT;
}
TWR_DEV void hermite_all(double t, double iT, double wp[4], double wv[4], double wa[4]) {
  hermite_pos(t, iT, wp);
  const double iT2 = iT * iT, iT3 = iT2 * iT;
  const double t2 = t * t;
  wv[0] = 6.0 * t2 * iT3 - 6.0 * t * iT2;
  wv[1] = 3.0 * t2 * iT2 - 4.0 * t * iT + 1.0;
  wv[2] = 6.0 * t * iT2 - 6.0 * t2 * iT3;
  wv[3] = 3.0 * t2 * iT2 - 2.0 * t * iT;
  wa[0] = 12.0 * t * iT3 - 6.0 * iT2;
  wa[1] = 6.0 * t * iT2 - 4.0 * iT;
  wa[2] = 6.0 * iT2 - 12.0 * t * iT3;
  wa[3] = 6.0 * t * iT2 - 2.0 * iT;
}

// ---------------------------------------------------------------- candidate descriptors
TWR_DEV int meta_nslots(uint32_t meta) { return meta & 0xF; }
TWR_DEV bool meta_shared(uint32_t meta) { return (meta >> 16) & 1; }
// all 12 candidate loads are issued unconditionally (absent candidates read slot 0 and later get
// weight 0): one memory round trip, no branches (Spline::GetPoint needs at most these 12 values)
template <class Slot>   // slot(c): the 4-bit slot of candidate c, 0xF = absent
TWR_DEV void gather12_by(const double* __restrict__ xp, int xbase, Slot slot, double v[12]) {
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    const int sl = slot(c);
    v[c] = xp[xbase + (sl != 0xF ? sl : 0)];
  }
}
TWR_DEV void gather12(const double* __restrict__ xp, int xbase, uint64_t slots, double v[12]) {
  gather12_by(xp, xbase, [&](int c) { return (int)((slots >> (4 * c)) & 0xF); }, v);
}
// Position of an ee spline from its gathered node values (Spline::GetPoint, src/spline.cc:80-93, in
// Hermite basis form).  A stance ee-motion polynomial keeps one shared position variable for both
// nodes: w_p1 is folded into w_p0.
TWR_DEV void ee_point(uint64_t slots, bool shared, double tl, double iT, const double v[12], double w[4], double out[3]) {
  hermite_pos(tl, iT, w);
  if (shared) w[0] += w[2];
  out[0] = out[1] = out[2] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const bool valid = ((slots >> (4 * (j * 3 + d))) & 0xF) != 0xF;
      out[d] = fma(valid ? w[j] : 0.0, v[j * 3 + d], out[d]);
    }
}
TWR_DEV void gather12c(const double* __restrict__ xp, int xbase, const uint16_t cand[12], double v[12]) {
  gather12_by(xp, xbase, [&](int c) { return cand[c] & 0xF; }, v);
}
TWR_DEV uint64_t slots_of(const uint16_t cand[12]) {
  uint64_t s = 0;
#pragma unroll
  for (int c = 0; c < 12; ++c) s |= (uint64_t)(cand[c] & 0xF) << (4 * c);
  return s;
}
// the three slots (one per dimension, 12 bits) of node value j from the two dwords of such a word
TWR_DEV uint32_t slots12(uint32_t lo, uint32_t hi, int j) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (12 * j)) & 0xFFFu; }

// entry (r,d), r != d, of the cross-product matrix [v]x (single_rigid_body_dynamics.cc:46-57)
template <int R, int D>
TWR_DEV double crs(const double v[3]) {
  static_assert(R != D, "diagonal of a cross matrix is structurally absent");
  constexpr int o = 3 - R - D;
  constexpr bool pos = (R == 0 && D == 2) || (R == 1 && D == 0) || (R == 2 && D == 1);
  return pos ? v[o] : -v[o];
}
TWR_DEV void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// A constant of the trigonometry passes through an empty asm: it is then materialised where it is used -- two s_mov -- instead
// of being hoisted out of the persistent loops, where the register allocator ends up spilling it to scratch and reloading
// it in the loop.  That holds for the cold side as well: its constants are hoisted just the same.
struct InPlace {
  TWR_DEV double operator()(double c) const {
    asm volatile("" : "+s"(c));
    return c;
  }
};
// The fdlibm minimax kernels (k_sin.c / k_cos.c coefficients) on a reduced argument |r| <= pi/4.
TWR_DEV void sincos_reduced(double r, double& sr, double& cr) {
  const InPlace K;
  const double z = r * r;
  double ps = fma(z, K(1.58969099521155010221e-10), K(-2.50507602534068634195e-08));
  ps = fma(z, ps, K(2.75573137070700676789e-06));
  ps = fma(z, ps, K(-1.98412698298579493134e-04));
  ps = fma(z, ps, K(8.33333333332248946124e-03));
  ps = fma(z, ps, K(-1.66666666666666324348e-01));
  sr = fma(z * r, ps, r);
  double pc = fma(z, K(-1.13596475577881948265e-11), K(2.08757232129817482790e-09));
  pc = fma(z, pc, K(-2.75573143513906633035e-07));
  pc = fma(z, pc, K(2.48015872894767294178e-05));
  pc = fma(z, pc, K(-1.38888888888741095749e-03));
  pc = fma(z, pc, K(4.16666666666666019037e-02));
  cr = fma(z * z, pc, fma(z, -0.5, 1.0));
}
// sin and cos of the reduced argument of quadrant q = n mod 4, where x = n * pi/2 + r
TWR_DEV void sincos_quadrant(int q, double sr, double cr, double* __restrict__ s, double* __restrict__ c) {
  const double ss = (q & 1) ? cr : sr, cc = (q & 1) ? sr : cr;
  *s = (q & 2) ? -ss : ss;
  *c = ((q + 1) & 2) ? -cc : cc;
}

// sin and cos of a finite |x| >= 1e5 (the cold side of sincos_fast): Payne-Hanek reduction in integers.  |x| = m * 2^e with a
// 53-bit m; the digits of 2/pi that weigh 4 or more in x * 2/pi only add multiples of 2 pi, so a window of 192 digits from
// weight 2 downwards times m, modulo 2^192, is (x * 2/pi mod 4) * 2^190 to within 2^53 units.  No double lies closer to a
// multiple of pi/2 than 2^-61 of its size (6381956970095103 * 2^797 does), which leaves 2^-76 of the reduced argument: it is
// carried as a double-double through the multiplication by pi/2 into the kernels' first-order corrections.  The library
// sincos keeps an absolute 2^-104 here and misses that case's cosine by 405 ulp; this stays within 1.5 ulp (tests/test_trig_probe.py).
// The digits come from v_trig_preop_f64, four segments of 53, which starts at the digit of weight 2 itself once the biased
// exponent exceeds 1077 and at the first digit below that.  No memory is read: a load here, cold as it is, sits inside the
// persistent loops of every evaluation kernel and cost the flagship 4 % (a table of 2/pi was tried first).
TWR_DEV void sincos_far(double x, double* __restrict__ s, double* __restrict__ c) {
  const double ax = fabs(x);
  const uint64_t bits = (uint64_t)__double_as_longlong(ax);
  const int eb = (int)(bits >> 52);         // biased exponent: 1039 .. 2046
  const uint64_t m = (bits & 0xFFFFFFFFFFFFFull) | (1ull << 52);
  const int lead = eb > 1077 ? eb - 1077 : 0;                  // digits the instruction skips
  const int back = 53 + lead - (eb >= 1968 ? 128 : 0);         // segment j is an integer below 2^53 times 2^-(back + 53 j)
  const uint64_t c0 = (uint64_t)ldexp(__builtin_amdgcn_trig_preop(ax, 0), back);
  const uint64_t c1 = (uint64_t)ldexp(__builtin_amdgcn_trig_preop(ax, 1), back + 53);
  const uint64_t c2 = (uint64_t)ldexp(__builtin_amdgcn_trig_preop(ax, 2), back + 106);
  const uint64_t c3 = (uint64_t)ldexp(__builtin_amdgcn_trig_preop(ax, 3), back + 159);
  // the 212 digits as (w3:w2:w1:w0), then the 192 from the digit of weight 2 on: below exponent 1077 that digit lies
  // 1077 - eb places in front of the first one (zeros)
  const uint64_t w0 = c3 | (c2 << 53), w1 = (c2 >> 11) | (c1 << 42), w2 = (c1 >> 22) | (c0 << 31), w3 = c0 >> 33;
  const int sh = 20 + (eb < 1077 ? 1077 - eb : 0);             // 20 .. 58
  const uint64_t p0 = (w0 >> sh) | (w1 << (64 - sh)), p1 = (w1 >> sh) | (w2 << (64 - sh)), p2 = (w2 >> sh) | (w3 << (64 - sh));
  // y = (m * (p2:p1:p0)) mod 2^192 = (y2:y1:y0), x * 2/pi mod 4 = y / 2^190
  uint64_t y0 = m * p0;
  const uint64_t mid = m * p1;
  uint64_t y1 = mid + __umul64hi(m, p0);
  uint64_t y2 = m * p2 + __umul64hi(m, p1) + (y1 < mid ? 1u : 0u);
  const uint64_t n = (y2 + (1ull << 61)) >> 62;   // nearest integer (4 stands for 0)
  y2 -= n << 62;                                  // the signed remainder, |y| <= 2^189
  const bool neg = (int64_t)y2 < 0;
  if (neg) {                                      // magnitude and sign
    y0 = ~y0 + 1;
    y1 = ~y1 + (y0 == 0 ? 1u : 0u);
    y2 = ~y2 + ((y0 == 0 && y1 == 0) ? 1u : 0u);
  }
  int shift = 0;                                  // normalise: the leading one to bit 63 of y2
  if (y2 == 0) { y2 = y1; y1 = y0; y0 = 0; shift = 64; }
  if (y2 == 0) { y2 = y1; y1 = 0; shift = 128; }
  double fh = 0.0, fl = 0.0;                      // y / 2^190 = fh + fl
  if (y2 != 0) {
    const int lz = __clzll((long long)y2);
    const uint64_t a = lz ? (y2 << lz) | (y1 >> (64 - lz)) : y2;
    const uint64_t lo = lz ? (y1 << lz) | (y0 >> (64 - lz)) : y1;
    shift += lz;
    fh = ldexp((double)(a >> 11), -51 - shift);                           // 53 digits: exact
    fl = ldexp((double)(((a & 0x7FFull) << 53) | (lo >> 11)), -115 - shift);
  }
  if (neg) { fh = -fh; fl = -fl; }
  const InPlace K;
  const double pio2_h = K(1.5707963267948966e+00), pio2_l = K(6.1232339957367660e-17);
  const double rh = fh * pio2_h;
  const double rl = fma(fh, pio2_l, fl * pio2_h) + fma(fh, pio2_h, -rh);
  double sr, cr;
  sincos_reduced(rh, sr, cr);
  double sa, ca;                                  // of |x|: sin(rh + rl) = sin rh + rl cos rh, cos(rh + rl) = cos rh - rl sin rh
  sincos_quadrant((int)(n & 3), fma(rl, cr, sr), fma(-rl, sr, cr), &sa, &ca);
  *s = x < 0.0 ? -sa : sa;
  *c = ca;
}

// sin and cos of one Euler angle.  Cody-Waite reduction by pi/2 in three FMA steps and the fdlibm
// minimax kernels, ~35 FP64 instructions for both results; a larger finite |x| takes sincos_far.
// Measured against a 60-digit reference (tests/test_trig_probe.py): within 1.51 ulp for |x| < 1e5
// and within 1.47 ulp above.  +-Inf and NaN give NaN.
// The reference calls libm sin/cos (euler_converter.cc:133-221); the difference is rounding level.
TWR_DEV void sincos_fast(double x, double* __restrict__ s, double* __restrict__ c) {
  if (!(fabs(x) < 1.0e5)) {
    if (fabs(x) < __builtin_inf()) sincos_far(x, s, c);
    else *s = *c = x - x;
    return;
  }
  const InPlace K;
  // On |x|, the sign of x going onto the sine at the end: every step is odd in x, so this is the same bits as reducing x
  // itself -- except at -0, where the reduction (-0 - (-0) * pi/2) and the polynomial (r + r^3 * p) both lose the sign of
  // zero that the sine has to keep.
  const double ax = fabs(x);
  const double n = rint(ax * K(6.36619772367581382433e-01));
  double r = fma(-n, K(1.5707963267948966e+00), ax);
  r = fma(-n, K(6.1232339957367574e-17), r);
  r = fma(-n, K(8.4784276603688985e-32), r);
  double sr, cr, sa;
  sincos_reduced(r, sr, cr);
  sincos_quadrant((int)n & 3, sr, cr, &sa, c);
  *s = __builtin_signbit(x) ? -sa : sa;
}

// ---------------------------------------------------------------- quad helpers
// The dynamic kernel maps FOUR lanes to one time node (a "quad" = lanes 4i..4i+3); they exchange
// scalars with DPP quad permutes (no LDS, no memory).
template <int CTRL>
TWR_DEV double quad_perm(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
TWR_DEV double quad_sum(double v) {
  v += quad_perm<0xB1>(v);  // lane ^ 1
  v += quad_perm<0x4E>(v);  // lane ^ 2
  return v;
}
TWR_DEV double sel3(int i, double a, double b, double c) { return i == 0 ? a : (i == 1 ? b : c); }

// ZYX Euler rotation base->world (euler_converter.cc:207-221).
struct Rot {
  double R[3][3];
  double sx, cx, sy, cy, sz, cz;
};
TWR_DEV void rot_fill(double sx, double cx, double sy, double cy, double sz, double cz, Rot& o) {
  o.sx = sx; o.cx = cx; o.sy = sy; o.cy = cy; o.sz = sz; o.cz = cz;
  o.R[0][0] = cy * cz; o.R[0][1] = cz * sx * sy - cx * sz; o.R[0][2] = sx * sz + cx * cz * sy;
  o.R[1][0] = cy * sz; o.R[1][1] = cx * cz + sx * sy * sz; o.R[1][2] = cx * sy * sz - cz * sx;
  o.R[2][0] = -sy;     o.R[2][1] = cy * sx;                o.R[2][2] = cx * cy;
}
TWR_DEV void rotation(const double e[3], Rot& o) {
  double sx, cx, sy, cy, sz, cz;
  sincos_fast(e[0], &sx, &cx);
  sincos_fast(e[1], &sy, &cy);
  sincos_fast(e[2], &sz, &cz);
  rot_fill(sx, cx, sy, cy, sz, cz, o);
}
// rotation() by the four lanes of a quad that hold the same e: lanes j = 0..2 evaluate one sincos each and broadcast it
TWR_DEV void rotation_quad(int j, const double e[3], Rot& o) {
  double my_s, my_c;
  sincos_fast(sel3(j, e[0], e[1], e[2]), &my_s, &my_c);
  rot_fill(quad_perm<0x00>(my_s), quad_perm<0x00>(my_c), quad_perm<0x55>(my_s), quad_perm<0x55>(my_c), quad_perm<0xAA>(my_s), quad_perm<0xAA>(my_c), o);
}
TWR_DEV void matvec(const double A[3][3], const double v[3], double o[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2];
}
TWR_DEV void matTvec(const double A[3][3], const double v[3], double o[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = A[0][i] * v[0] + A[1][i] * v[1] + A[2][i] * v[2];
}
TWR_DEV void symmul(const double I[6], const double v[3], double o[3]) {  // I = (00,01,02,11,12,22)
  o[0] = I[0] * v[0] + I[1] * v[1] + I[2] * v[2];
  o[1] = I[1] * v[0] + I[3] * v[1] + I[4] * v[2];
  o[2] = I[2] * v[0] + I[4] * v[1] + I[5] * v[2];
}

// ---------------------------------------------------------------- optimised timings helpers
// Spline::GetSegmentID + GetLocalTime (src/spline.cc:48-78) on durations that depend on x: the same
// double-precision accumulation, eps and sequential subtraction as the reference (and the host Locate).
TWR_DEV int locate_segment(const double* __restrict__ d, int n, double t, double& t_local) {
  // Branch-free on purpose: with the reference's early `break` every iteration's load waits for the previous compare
  // (a chain of dependent LDS round trips); predicated, the loads of an unrolled block go out together and only the
  // additions are sequential.  Same additions and subtractions in the same order, so the same bits.
  const double eps = 1e-10;
  double acc = 0.0, tl = t;
  int id = n - 1;  // (the reference asserts that a segment is found)
  bool found = false;
#pragma unroll 8
  for (int i = 0; i < n; ++i) {
    const double di = d[i];
    acc += di;
    const bool hit = !found && acc >= t - eps;
    id = hit ? i : id;
    found = found || hit;
    if (!found && i < n - 1) tl -= di;   // t_local = t - sum of the durations BEFORE the segment, sequentially
  }
  t_local = tl;
  return id;
}
// node values (p0,v0,p1,v1)[dim] of the active polynomial from its gathered candidates: values that are
// not optimised are the constant 0, a stance ee-motion polynomial has p1 = p0
TWR_DEV void node_values(uint64_t slots, bool shared, const double v[12], double nv[4][3]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const bool valid = ((slots >> (4 * (j * 3 + d))) & 0xF) != 0xF;
      nv[j][d] = valid ? v[j * 3 + d] : 0.0;
    }
  if (shared) {
#pragma unroll
    for (int d = 0; d < 3; ++d) nv[2][d] = nv[0][d];
  }
}
}  // namespace twr
