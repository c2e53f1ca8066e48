// Test program (nothing in the product links it): runs the device trigonometry of kernels/spline_math.h on a file of
// doubles and writes the raw results, so that tests/test_trig_probe.py can hold them to a 60-digit reference.
//
//   trig_probe sincos  IN OUT   IN: n doubles          OUT: n x (sin, cos), one lane per input calling sincos_fast
//   trig_probe rot     IN OUT   IN: n x 3 Euler angles OUT: n x (R[3][3] row-major, sx, cx, sy, cy, sz, cz), one lane per triple
//                                                           calling rotation()
//   trig_probe rotquad IN OUT   IN: n x 3 Euler angles OUT: n x 4 x the same 15 values, four lanes per triple calling
//                                                           rotation_quad(lane & 3, ...); every lane writes what it holds
//
// Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/spline_math.h"

#define PROBE_NAME "trig_probe"
#include "probe_host.h"

namespace {
constexpr int ROT_VALUES = 15;
constexpr int BLOCK = 256;

__device__ void put_rot(const twr::Rot& ro, double* __restrict__ o) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o[3 * r + c] = ro.R[r][c];
  o[9] = ro.sx; o[10] = ro.cx; o[11] = ro.sy; o[12] = ro.cy; o[13] = ro.sz; o[14] = ro.cz;
}

__global__ void sincos_probe(const double* __restrict__ x, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double s, c;
  twr::sincos_fast(x[i], &s, &c);
  out[2 * i] = s;
  out[2 * i + 1] = c;
}

__global__ void rot_probe(const double* __restrict__ e, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double ang[3] = {e[3 * i], e[3 * i + 1], e[3 * i + 2]};
  twr::Rot ro;
  twr::rotation(ang, ro);
  put_rot(ro, out + ROT_VALUES * i);
}

// the grid covers whole quads only and no lane leaves before the broadcast: a quad past the end recomputes the last triple
__global__ void rotquad_probe(const double* __restrict__ e, long n, double* __restrict__ out) {
  const long lane = (long)blockIdx.x * BLOCK + threadIdx.x;
  const long quad = lane >> 2;
  const long t = quad < n ? quad : n - 1;
  const double ang[3] = {e[3 * t], e[3 * t + 1], e[3 * t + 2]};
  twr::Rot ro;
  twr::rotation_quad((int)(lane & 3), ang, ro);
  if (quad < n) put_rot(ro, out + ROT_VALUES * lane);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: trig_probe sincos|rot|rotquad IN OUT\n");
    return probe::REFUSED;
  }
  const bool m_sincos = !std::strcmp(argv[1], "sincos"), m_rot = !std::strcmp(argv[1], "rot"), m_quad = !std::strcmp(argv[1], "rotquad");
  if (!m_sincos && !m_rot && !m_quad) {
    std::fprintf(stderr, "trig_probe: unknown mode %s\n", argv[1]);
    return probe::REFUSED;
  }
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  const long per_item = m_sincos ? 1 : 3;
  if (in.v.empty() || in.v.size() % per_item) {
    std::fprintf(stderr, "trig_probe: %zu doubles in %s do not make whole inputs\n", in.v.size(), argv[2]);
    return probe::REFUSED;
  }
  const long n = (long)in.v.size() / per_item;
  const long lanes = m_quad ? 4 * n : n;
  std::vector<double> out(m_sincos ? 2 * n : ROT_VALUES * lanes);

  if (!probe::have_device()) return probe::NO_DEVICE;
  probe::Device dev;
  double *d_in = nullptr, *d_out = nullptr;
  if (!dev.upload(&d_in, in.v) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
  const unsigned blocks = (unsigned)((lanes + BLOCK - 1) / BLOCK);
  if (m_sincos) sincos_probe<<<blocks, BLOCK>>>(d_in, n, d_out);
  else if (m_rot) rot_probe<<<blocks, BLOCK>>>(d_in, n, d_out);
  else rotquad_probe<<<blocks, BLOCK>>>(d_in, n, d_out);
  if (!probe::collect(out.data(), d_out, out.size()) || !dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}

