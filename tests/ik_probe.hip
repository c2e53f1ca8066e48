// Test program (nothing in the product links it): runs leg_ik and leg_ik_of_foot of kernels/joints.h on a file of feet and
// writes the raw results, so that tests/test_ik_probe.py can hold them to the reference's recorded answers.
//
//   ik_probe leg  IN OUT   IN: the descriptor, n, then n x (x y z bend) feet in the hip frame
//   ik_probe body IN OUT   IN: the descriptor, n, then n x 12 feet in the base frame (four legs)
//
// The descriptor is 31 doubles in the order of twr_leg_kinematics: n_ee, knee_bend[4], mirror[4][3], base_to_hip[3],
// hfe_to_haa[3], length_thigh, length_shank, q_min[3], q_max[3].  OUT (raw doubles), per leg: q_HAA q_HFE q_KFE flags
// cos_beta cos_gamma r over_reach.
//
// Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/joints.h"

#define PROBE_NAME "ik_probe"
#include "probe_host.h"

namespace {
constexpr int BLOCK = 64, OUT = 8, KIN = 31;

__device__ void put(double* __restrict__ o, const twr::LegIk& k, const twr_leg_kinematics& K) {
  o[0] = k.q[0]; o[1] = k.q[1]; o[2] = k.q[2];
  o[3] = (double)k.flags;
  o[4] = k.cos_beta; o[5] = k.cos_gamma; o[6] = k.r;
  o[7] = twr::over_reach(k.r, K);
}
__global__ __launch_bounds__(BLOCK) void leg_probe(const double* __restrict__ p, long n, double* __restrict__ out, twr_leg_kinematics K) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double foot[3] = {p[4 * i], p[4 * i + 1], p[4 * i + 2]};
  twr::LegIk k;
  twr::leg_ik(foot, p[4 * i + 3] != 0.0 ? 1 : 0, K, k);
  put(out + OUT * i, k, K);
}
__global__ __launch_bounds__(BLOCK) void body_probe(const double* __restrict__ p, long n, double* __restrict__ out, twr_leg_kinematics K) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  for (int e = 0; e < 4; ++e) {
    const double foot[3] = {p[12 * i + 3 * e], p[12 * i + 3 * e + 1], p[12 * i + 3 * e + 2]};
    twr::LegIk k;
    twr::leg_ik_of_foot(foot, e, K, k);
    put(out + OUT * (4 * i + e), k, K);
  }
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4 || (std::strcmp(argv[1], "leg") && std::strcmp(argv[1], "body"))) {
    std::fprintf(stderr, "usage: ik_probe leg|body IN OUT\n");
    return probe::REFUSED;
  }
  const bool body = !std::strcmp(argv[1], "body");
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  // parse on the host first: the count is checked against what the file holds before anything reaches the device
  if (!in.have((size_t)KIN + 1)) return in.bad("truncated descriptor");
  twr_leg_kinematics K;
  std::memset(&K, 0, sizeof K);
  K.n_ee = (int32_t)in.next();
  for (int e = 0; e < 4; ++e) K.knee_bend[e] = (int32_t)in.next();
  for (int e = 0; e < 4; ++e)
    for (int d = 0; d < 3; ++d) K.mirror[e][d] = in.next();
  for (int d = 0; d < 3; ++d) K.base_to_hip[d] = in.next();
  for (int d = 0; d < 3; ++d) K.hfe_to_haa[d] = in.next();
  K.length_thigh = in.next();
  K.length_shank = in.next();
  for (int j = 0; j < 3; ++j) K.q_min[j] = in.next();
  for (int j = 0; j < 3; ++j) K.q_max[j] = in.next();
  const long n = (long)in.next();
  const size_t per = body ? 12 : 4;
  if (n < 1 || n > (1L << 22)) return in.bad("point count");
  if (!in.have(per * (size_t)n)) return in.bad("truncated points");
  if (in.at + per * (size_t)n != in.v.size()) return in.bad("trailing data");
  if (body && K.n_ee != 4) return in.bad("body mode needs four legs");
  if (!probe::have_device()) return probe::NO_DEVICE;
  std::vector<double> out((size_t)OUT * (body ? 4 : 1) * (size_t)n);
  probe::Device dev;
  double *d_p = nullptr, *d_out = nullptr;
  if (!dev.upload(&d_p, in.here(), per * (size_t)n) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
  const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK);
  if (body) body_probe<<<blocks, BLOCK>>>(d_p, n, d_out, K);
  else leg_probe<<<blocks, BLOCK>>>(d_p, n, d_out, K);
  if (!probe::collect(out.data(), d_out, out.size()) || !dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}
