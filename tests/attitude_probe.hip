// Test program (nothing in the product links it): runs quat_of_rotation, base_frame_rotation and base_frame of kernels/joints.h
// and sample_angular of kernels/sample.h on a file of points and writes the raw results, so that tests/test_attitude_probe.py
// can hold them to the reference's recorded answers and to the restatement of tests/attitude_points.py.
//
//   attitude_probe quat  IN OUT   IN: n, then n x 9 (R row-major).                       OUT per point: q as x y z w
//   attitude_probe euler IN OUT   IN: n, then n x 9 (Euler angles, rates, accelerations). OUT per point: the R of rotation() (9,
//                                 row-major), then q (x y z w), omega (3) and omega_dot (3) of sample_angular: 19 doubles
//   attitude_probe frame IN OUT   IN: n, then n x 10 (q as w x y z, p_base, p_ee).        OUT per point: the R of
//                                 base_frame_rotation (9, row-major), then the vector of base_frame (3): 12 doubles
//
// One thread handles one point.  Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/joints.h"
#include "kernels/sample.h"

#define PROBE_NAME "attitude_probe"
#include "probe_host.h"

namespace {
constexpr int BLOCK = 64;

__global__ __launch_bounds__(BLOCK) void quat_probe(const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double m[3][3], q[4];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) m[r][c] = p[9 * i + 3 * r + c];
  twr::quat_of_rotation(m, q);
  for (int k = 0; k < 4; ++k) out[4 * i + k] = q[k];
}
__global__ __launch_bounds__(BLOCK) void euler_probe(const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  twr::BaseSample B;
  for (int d = 0; d < 3; ++d) {
    B.p[d] = B.v[d] = B.a[d] = 0.0;
    B.e3[d] = p[9 * i + d];
    B.ed[d] = p[9 * i + 3 + d];
    B.edd[d] = p[9 * i + 6 + d];
  }
  twr::Rot ro;
  twr::rotation(B.e3, ro);
  twr::BaseAngular A;
  twr::sample_angular(B, A);
  double* o = out + 19 * i;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = ro.R[r][c];
  for (int k = 0; k < 4; ++k) o[9 + k] = A.q[k];
  for (int d = 0; d < 3; ++d) {
    o[13 + d] = A.omega[d];
    o[16 + d] = A.omega_dot[d];
  }
}
__global__ __launch_bounds__(BLOCK) void frame_probe(const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double* in = p + 10 * i;
  double R[3][3], v[3];
  const double base[3] = {in[4], in[5], in[6]}, ee[3] = {in[7], in[8], in[9]};
  twr::base_frame_rotation(in[0], in[1], in[2], in[3], R);
  twr::base_frame(R, base, ee, v);
  double* o = out + 12 * i;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) o[3 * r + c] = R[r][c];
  for (int d = 0; d < 3; ++d) o[9 + d] = v[d];
}
}  // namespace

int main(int argc, char** argv) {
  const char* modes[3] = {"quat", "euler", "frame"};
  const size_t per_in[3] = {9, 9, 10}, per_out[3] = {4, 19, 12};
  int mode = -1;
  for (int k = 0; k < 3 && argc == 4; ++k)
    if (!std::strcmp(argv[1], modes[k])) mode = k;
  if (mode < 0) {
    std::fprintf(stderr, "usage: attitude_probe quat|euler|frame IN OUT\n");
    return probe::REFUSED;
  }
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  // parse on the host first: the count is checked against what the file holds before anything reaches the device
  if (!in.have(1)) return in.bad("truncated: no point count");
  const double count = in.next();
  if (!(count >= 1.0 && count <= (double)(1L << 22)) || count != (double)(long)count) return in.bad("point count");
  const long n = (long)count;
  const size_t n_in = per_in[mode] * (size_t)n;
  if (!in.have(n_in)) return in.bad("truncated points");
  if (in.at + n_in != in.v.size()) return in.bad("trailing data");
  if (!probe::have_device()) return probe::NO_DEVICE;
  std::vector<double> out(per_out[mode] * (size_t)n);
  probe::Device dev;
  double *d_p = nullptr, *d_out = nullptr;
  if (!dev.upload(&d_p, in.here(), n_in) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
  const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK);
  if (mode == 0) quat_probe<<<blocks, BLOCK>>>(d_p, n, d_out);
  else if (mode == 1) euler_probe<<<blocks, BLOCK>>>(d_p, n, d_out);
  else frame_probe<<<blocks, BLOCK>>>(d_p, n, d_out);
  if (!probe::collect(out.data(), d_out, out.size()) || !dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}
