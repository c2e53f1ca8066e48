// Test program (nothing in the product links it): runs ring_side, ring_distance and nearest_plane of kernels/planes.h on a file
// of scenes and writes the raw results, so that tests/test_plane_probe.py can hold them to the reference's recorded answers,
// to the oracle and to an exact computation.
//
//   plane_probe side     IN OUT   OUT: per scene, point and ring (point-major) ring_side as a double
//   plane_probe distance IN OUT   OUT: per scene, point and ring (point-major) ring_distance, whether the point is inside or not
//   plane_probe nearest  IN OUT   OUT: per scene and point nearest_plane as a double
//
// IN (raw doubles): the number of scenes; per scene the number of rings, per ring its length k (0 .. 4096) and its k world
// (x, y), then the number of points and their (x, y).  One thread per (ring, point) or per point.
//
// Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/planes.h"

#define PROBE_NAME "plane_probe"
#include "probe_host.h"

namespace {
constexpr int BLOCK = 256;
constexpr long MAX_RING = 4096, MAX_RINGS = 1024, MAX_SCENES = 4096, MAX_POINTS = 1L << 20, MAX_ITEMS = 1L << 24;

struct PairWork {     // one ring and one point: the ring is xy[2 * xy_at .. 2 * (xy_at + n))
  int32_t xy_at, n;
  double px, py;
};
struct PointWork {    // one scene and one point: the scene's rings start at xy + 2 * xy_at, its n_polys + 1 starts at starts + start_at
  int32_t xy_at, start_at, n_polys, pad;
  double px, py;
};

__global__ __launch_bounds__(BLOCK) void pair_probe(const PairWork* __restrict__ work, long n, const double* __restrict__ xy,
                                                    double* __restrict__ out, int distance) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const PairWork w = work[i];
  const double* ring = xy + 2 * (size_t)w.xy_at;
  out[i] = distance ? twr::ring_distance(ring, w.n, w.px, w.py) : (double)twr::ring_side(ring, w.n, w.px, w.py);
}

__global__ __launch_bounds__(BLOCK) void nearest_probe(const PointWork* __restrict__ work, long n, const double* __restrict__ xy,
                                                       const int32_t* __restrict__ starts, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const PointWork w = work[i];
  out[i] = (double)twr::nearest_plane(xy + 2 * (size_t)w.xy_at, starts + w.start_at, w.n_polys, w.px, w.py);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: plane_probe side|distance|nearest IN OUT\n");
    return probe::REFUSED;
  }
  const bool m_side = !std::strcmp(argv[1], "side"), m_distance = !std::strcmp(argv[1], "distance"), m_nearest = !std::strcmp(argv[1], "nearest");
  if (!m_side && !m_distance && !m_nearest) {
    std::fprintf(stderr, "plane_probe: unknown mode %s\n", argv[1]);
    return probe::REFUSED;
  }
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  // parse on the host first: every count is checked against what the file holds before anything reaches the device, and every
  // index the kernels use is built here from those counts
  if (!in.have(1)) return in.bad("empty");
  const long n_scenes = (long)in.next();
  if (n_scenes < 1 || n_scenes > MAX_SCENES) return in.bad("scene count");
  std::vector<double> xy;
  std::vector<int32_t> starts;
  std::vector<PairWork> pairs;
  std::vector<PointWork> points;
  for (long s = 0; s < n_scenes; ++s) {
    if (!in.have(1)) return in.bad("truncated scene header");
    const long n_rings = (long)in.next();
    if (n_rings < 0 || n_rings > MAX_RINGS) return in.bad("ring count");
    const int32_t scene_xy_at = (int32_t)(xy.size() / 2), scene_start_at = (int32_t)starts.size();
    starts.push_back(0);
    for (long r = 0; r < n_rings; ++r) {
      if (!in.have(1)) return in.bad("truncated ring header");
      const long k = (long)in.next();
      if (k < 0 || k > MAX_RING) return in.bad("ring length");
      if (!in.have(2 * (size_t)k)) return in.bad("truncated ring");
      xy.insert(xy.end(), in.here(), in.here() + 2 * k);
      in.at += 2 * (size_t)k;
      starts.push_back((int32_t)(xy.size() / 2) - scene_xy_at);
    }
    if (xy.size() / 2 > (size_t)MAX_ITEMS) return in.bad("more ring points than the probe takes");
    if (!in.have(1)) return in.bad("truncated scene: no point count");
    const long n_points = (long)in.next();
    if (n_points < 0 || n_points > MAX_POINTS) return in.bad("point count");
    if (!in.have(2 * (size_t)n_points)) return in.bad("truncated points");
    for (long k = 0; k < n_points; ++k) {
      const double px = in[2 * k], py = in[2 * k + 1];
      if (m_nearest) {
        points.push_back({scene_xy_at, scene_start_at, (int32_t)n_rings, 0, px, py});
      } else {
        for (long r = 0; r < n_rings; ++r) {
          const int32_t a = starts[scene_start_at + r], b = starts[scene_start_at + r + 1];
          pairs.push_back({scene_xy_at + a, b - a, px, py});
        }
      }
    }
    in.at += 2 * (size_t)n_points;
    if (pairs.size() > (size_t)MAX_ITEMS || points.size() > (size_t)MAX_ITEMS) return in.bad("more items than the probe takes");
  }
  if (!in.at_end()) return in.bad("trailing data");
  const long n = (long)(m_nearest ? points.size() : pairs.size());
  std::vector<double> out((size_t)n);
  if (n == 0) return probe::write_out(argv[3], out);
  if (!probe::have_device()) return probe::NO_DEVICE;
  probe::Device dev;
  double *d_out = nullptr, *d_xy = nullptr;
  if (!dev.upload(&d_xy, xy) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
  const unsigned blocks = (unsigned)((n + BLOCK - 1) / BLOCK);
  if (m_nearest) {
    PointWork* d_work = nullptr;
    int32_t* d_starts = nullptr;
    if (!dev.upload(&d_work, points) || !dev.upload(&d_starts, starts)) return probe::HIP_FAILED;
    nearest_probe<<<blocks, BLOCK>>>(d_work, n, d_xy, d_starts, d_out);
  } else {
    PairWork* d_work = nullptr;
    if (!dev.upload(&d_work, pairs)) return probe::HIP_FAILED;
    pair_probe<<<blocks, BLOCK>>>(d_work, n, d_xy, d_out, m_distance ? 1 : 0);
  }
  if (!probe::collect(out.data(), d_out, out.size()) || !dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}
