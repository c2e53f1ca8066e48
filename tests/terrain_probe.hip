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
// Exit status: 0 done, 2 usage / file error, 3 no HIP device, 4 a HIP call failed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/terrain.h"

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

bool ok(hipError_t err, const char* what) {
  if (err == hipSuccess) return true;
  std::fprintf(stderr, "terrain_probe: %s: %s\n", what, hipGetErrorString(err));
  return false;
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
    return 2;
  }
  const bool m_eval = !std::strcmp(argv[1], "eval"), m_force = !std::strcmp(argv[1], "force"), m_g = !std::strcmp(argv[1], "force_g");
  if (!m_eval && !m_force && !m_g) {
    std::fprintf(stderr, "terrain_probe: unknown mode %s\n", argv[1]);
    return 2;
  }
  std::vector<double> in;
  {
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) {
      std::fprintf(stderr, "terrain_probe: cannot read %s\n", argv[2]);
      return 2;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(f);
  }
  // parse on the host first: every count is checked against what the file holds before anything reaches the device
  size_t at = 0;
  auto have = [&](size_t k) { return at + k <= in.size(); };
  auto bad = [&](const char* what) {
    std::fprintf(stderr, "terrain_probe: %s: %s\n", argv[2], what);
    return 2;
  };
  if (!have(1)) return bad("empty");
  const long n_maps = (long)in[at++];
  if (n_maps < 0 || n_maps > 64) return bad("map count");
  std::vector<Map> maps;
  std::vector<size_t> map_at;
  for (long m = 0; m < n_maps; ++m) {
    if (!have(7)) return bad("truncated map header");
    Map mp = {(int)in[at], (int)in[at + 1], (int)in[at + 2], in[at + 3], in[at + 4], in[at + 5], in[at + 6], nullptr};
    at += 7;
    if ((mp.kind != 7 && mp.kind != 8) || mp.rows < 1 || mp.cols < 1 || mp.rows > 4096 || mp.cols > 4096 || !(mp.res > 0) || !(mp.eps > 0))
      return bad("map header");
    if (!have((size_t)mp.rows * mp.cols)) return bad("truncated map");
    map_at.push_back(at);
    at += (size_t)mp.rows * mp.cols;
    maps.push_back(mp);
  }
  struct Group {
    int terrain_id, map;
    double mu, flat_height;
    long n;
    size_t at;
  };
  const long per_in = m_eval ? 2 : 5, per_out = m_eval ? 4 : m_force ? FORCE_OUT : 5;
  if (!have(1)) return bad("no groups");
  const long n_groups = (long)in[at++];
  if (n_groups < 1 || n_groups > 4096) return bad("group count");
  std::vector<Group> groups;
  long total = 0;
  for (long g = 0; g < n_groups; ++g) {
    if (!have(5)) return bad("truncated group header");
    Group gr = {(int)in[at], (int)in[at + 1], in[at + 2], in[at + 3], (long)in[at + 4], at + 5};
    at += 5;
    if (gr.terrain_id < 0 || gr.terrain_id > 8 || gr.n < 1 || gr.n > (1L << 24)) return bad("group header");
    if ((gr.terrain_id >= 7) != (gr.map >= 0) || gr.map >= n_maps) return bad("group map index");
    if (gr.map >= 0 && maps[gr.map].kind != gr.terrain_id) return bad("group map kind");
    if (!have((size_t)gr.n * per_in)) return bad("truncated group");
    at += (size_t)gr.n * per_in;
    total += gr.n;
    groups.push_back(gr);
  }
  if (at != in.size()) return bad("trailing data");

  int devices = 0;
  if (hipGetDeviceCount(&devices) != hipSuccess || devices == 0) {
    std::fprintf(stderr, "terrain_probe: no HIP device\n");
    return 3;
  }
  for (size_t m = 0; m < maps.size(); ++m) {
    Map& mp = maps[m];
    const size_t cells = (size_t)mp.rows * mp.cols;
    if (mp.kind == 7) {
      if (!ok(hipMalloc(&mp.dev, cells * sizeof(double)), "hipMalloc") ||
          !ok(hipMemcpy(mp.dev, in.data() + map_at[m], cells * sizeof(double), hipMemcpyHostToDevice), "copy map"))
        return 4;
    } else {
      std::vector<float> el(cells);
      for (size_t k = 0; k < cells; ++k) el[k] = (float)in[map_at[m] + k];
      if (!ok(hipMalloc(&mp.dev, cells * sizeof(float)), "hipMalloc") ||
          !ok(hipMemcpy(mp.dev, el.data(), cells * sizeof(float), hipMemcpyHostToDevice), "copy map"))
        return 4;
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
    twr::DevStruct* d_S = nullptr;
    double *d_in = nullptr, *d_out = nullptr;
    const size_t n_in = (size_t)gr.n * per_in, n_out = (size_t)gr.n * per_out;
    if (!ok(hipMalloc(&d_S, sizeof S), "hipMalloc") || !ok(hipMalloc(&d_in, n_in * sizeof(double)), "hipMalloc") ||
        !ok(hipMalloc(&d_out, n_out * sizeof(double)), "hipMalloc"))
      return 4;
    if (!ok(hipMemcpy(d_S, &S, sizeof S, hipMemcpyHostToDevice), "copy header") ||
        !ok(hipMemcpy(d_in, in.data() + gr.at, n_in * sizeof(double), hipMemcpyHostToDevice), "copy in") ||
        !ok(hipMemset(d_out, 0xFF, n_out * sizeof(double)), "hipMemset"))   // unwritten results read back as NaN
      return 4;
    const unsigned blocks = (unsigned)((gr.n + BLOCK - 1) / BLOCK);
    if (m_eval) eval_probe<<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    else if (m_force) force_probe<true><<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    else force_probe<false><<<blocks, BLOCK>>>(d_S, d_in, gr.n, d_out);
    if (!ok(hipGetLastError(), "launch") || !ok(hipDeviceSynchronize(), "kernel")) return 4;
    if (!ok(hipMemcpy(out.data() + out_at, d_out, n_out * sizeof(double), hipMemcpyDeviceToHost), "copy out")) return 4;
    out_at += n_out;
    if (!ok(hipFree(d_S), "hipFree") || !ok(hipFree(d_in), "hipFree") || !ok(hipFree(d_out), "hipFree")) return 4;
  }
  for (Map& mp : maps)
    if (!ok(hipFree(mp.dev), "hipFree")) return 4;
  std::FILE* f = std::fopen(argv[3], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, "terrain_probe: cannot write %s\n", argv[3]);
    return 2;
  }
  return 0;
}
