// Test program (nothing in the product links it): runs terrain_eval and force_core of kernels/terrain.h on a file of points
// and writes the raw results, so that tests/test_terrain_probe.py can hold them to the reference's recorded answers.
//
//   terrain_probe eval    IN OUT   OUT: per point (h, hx, hy, hxx) of terrain_eval
//   terrain_probe force   IN OUT   OUT: per point g5[5] then st25[25] of force_core with want_g and want_j set
//   terrain_probe force_g IN OUT   OUT: per point g5[5] of force_core with want_g set and want_j off
//
// IN (raw doubles): the number of maps; per map: kind (7: CSV heights[rows][cols] in double, 8: `Grid` elevation
// [i + j * rows] in float), rows, cols, res, eps, px, py, then rows * cols values; the number of groups; per group:
// terrain_id, map index (-1: none), mu, flat_height, n, then n points -- (x, y) for eval, (fx, fy, fz, x, y) for the
// force modes.  Each group runs on a DevStruct of its own, filled by hand with the fields the terrain reads.
//
// Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/terrain.h"

#define PROBE_NAME "terrain_probe"
#include "probe_host.h"

namespace {
constexpr int BLOCK = 256;
constexpr int FORCE_OUT = 30;

__global__ void eval_probe(const twr::DevStruct* __restrict__ S, const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const twr::Terr t = twr::terrain_eval(S, S->terrain_id, S->flat_height, p[2 * i], p[2 * i + 1]);
  out[4 * i] = t.h;
  out[4 * i + 1] = t.hx;
  out[4 * i + 2] = t.hy;
  out[4 * i + 3] = t.hxx;
}

template <bool WANT_J>
__global__ void force_probe(const twr::DevStruct* __restrict__ S, const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  const double f[3] = {p[5 * i], p[5 * i + 1], p[5 * i + 2]};
  double g5[5], st25[25];
  twr::force_core(S, f, p[5 * i + 3], p[5 * i + 4], g5, st25, true, WANT_J);
  double* __restrict__ o = out + (WANT_J ? FORCE_OUT : 5) * i;
#pragma unroll
  for (int r = 0; r < 5; ++r) o[r] = g5[r];
  if (WANT_J) {
#pragma unroll
    for (int k = 0; k < 25; ++k) o[5 + k] = st25[k];
  }
}

struct Map {
  int kind, rows, cols;
  double res, eps, px, py;
  void* dev;
};
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: terrain_probe eval|force|force_g IN OUT\n");
    return probe::REFUSED;
  }
  const bool m_eval = !std::strcmp(argv[1], "eval"), m_force = !std::strcmp(argv[1], "force"), m_g = !std::strcmp(argv[1], "force_g");
  if (!m_eval && !m_force && !m_g) {
    std::fprintf(stderr, "terrain_probe: unknown mode %s\n", argv[1]);
    return probe::REFUSED;
  }
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  // parse on the host first: every count is checked against what the file holds before anything reaches the device
  if (!in.have(1)) return in.bad("empty");
  const long n_maps = (long)in.next();
  if (n_maps < 0 || n_maps > 64) return in.bad("map count");
  std::vector<Map> maps;
  std::vector<size_t> map_at;
  for (long m = 0; m < n_maps; ++m) {
    if (!in.have(7)) return in.bad("truncated map header");
    Map mp = {(int)in[0], (int)in[1], (int)in[2], in[3], in[4], in[5], in[6], nullptr};
    in.at += 7;
    if ((mp.kind != 7 && mp.kind != 8) || mp.rows < 1 || mp.cols < 1 || mp.rows > 4096 || mp.cols > 4096 || !(mp.res > 0) || !(mp.eps > 0))
      return in.bad("map header");
    if (!in.have((size_t)mp.rows * mp.cols)) return in.bad("truncated map");
    map_at.push_back(in.at);
    in.at += (size_t)mp.rows * mp.cols;
    maps.push_back(mp);
  }
  struct Group {
    int terrain_id, map;
    double mu, flat_height;
    long n;
    size_t at;
  };
  const long per_in = m_eval ? 2 : 5, per_out = m_eval ? 4 : m_force ? FORCE_OUT : 5;
  if (!in.have(1)) return in.bad("no groups");
  const long n_groups = (long)in.next();
  if (n_groups < 1 || n_groups > 4096) return in.bad("group count");
  std::vector<Group> groups;
  long total = 0;
  for (long g = 0; g < n_groups; ++g) {
    if (!in.have(5)) return in.bad("truncated group header");
    Group gr = {(int)in[0], (int)in[1], in[2], in[3], (long)in[4], in.at + 5};
    in.at += 5;
    if (gr.terrain_id < 0 || gr.terrain_id > 8 || gr.n < 1 || gr.n > (1L << 24)) return in.bad("group header");
    if ((gr.terrain_id >= 7) != (gr.map >= 0) || gr.map >= n_maps) return in.bad("group map index");
    if (gr.map >= 0 && maps[gr.map].kind != gr.terrain_id) return in.bad("group map kind");
    if (!in.have((size_t)gr.n * per_in)) return in.bad("truncated group");
    in.at += (size_t)gr.n * per_in;
    total += gr.n;
    groups.push_back(gr);
  }
  if (!in.at_end()) return in.bad("trailing data");

  if (!probe::have_device()) return probe::NO_DEVICE;
  probe::Device map_dev;   // the maps live as long as the groups; a kind-8 map goes up as floats
  for (size_t m = 0; m < maps.size(); ++m) {
    Map& mp = maps[m];
    const size_t cells = (size_t)mp.rows * mp.cols;
    if (mp.kind == 7) {
      double* d = nullptr;
      if (!map_dev.upload(&d, in.v.data() + map_at[m], cells)) return probe::HIP_FAILED;
      mp.dev = d;
    } else {
      std::vector<float> el(cells);
      for (size_t k = 0; k < cells; ++k) el[k] = (float)in.v[map_at[m] + k];
      float* d = nullptr;
      if (!map_dev.upload(&d, el)) return probe::HIP_FAILED;
      mp.dev = d;
    }
  }
  std::vector<double> out((size_t)total * per_out);
  size_t out_at = 0;
  for (const Group& gr : groups) {
    twr::DevStruct S;
    std::memset(&S, 0, sizeof S);
    S.terrain_id = gr.terrain_id;
    S.flat_height = gr.flat_height;
    S.mu = gr.mu;
    if (gr.map >= 0) {
      const Map& mp = maps[gr.map];
      S.grid_ptr = (uint64_t)(uintptr_t)mp.dev;
      S.grid_rows = mp.rows;
      S.grid_cols = mp.cols;
      S.grid_res = mp.res;
      S.grid_eps = mp.eps;
      S.grid_px = mp.px;
      S.grid_py = mp.py;
    }
    probe::Device dev;   // this group's header, points and results, freed before the next group
    twr::DevStruct* d_S = nullptr;
    double *d_in = nullptr, *d_out = nullptr;
    const size_t n_in = (size_t)gr.n * per_in, n_out = (size_t)gr.n * per_out;
    if (!dev.upload(&d_S, &S, 1) || !dev.upload(&d_in, in.v.data() + gr.at, n_in) || !dev.results(&d_out, n_out)) return probe::HIP_FAILED;
    const unsigned blocks = (unsigned)((gr.n + BLOCK - 1) / BLOCK);
    if (m_eval) eval_probe<<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    else if (m_force) force_probe<true><<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    else force_probe<false><<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    if (!probe::collect(out.data() + out_at, d_out, n_out) || !dev.release()) return probe::HIP_FAILED;
    out_at += n_out;
  }
  if (!map_dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}
