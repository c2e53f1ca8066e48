// Test program (nothing in the product links it): runs locate_segment and hermite_all of kernels/spline_math.h and
// phase_poly_durations_wave of kernels/phase_durations.h on a file of points and writes the raw results, so that
// tests/test_segment_probe.py can hold them to the reference's recorded answers.
//
//   segment_probe locate       IN OUT   OUT: per point the id (as a double) and t_local of locate_segment
//   segment_probe durations64  IN OUT   OUT: per case ph[32], md[64], fd[64] of phase_poly_durations_wave called by 64 threads
//   segment_probe durations256 IN OUT   the same called by 256 threads (unwritten entries read back as NaN)
//   segment_probe hermite      IN OUT   OUT: per point wp[4], wv[4], wa[4] of hermite_all
//
// IN (raw doubles)
//   locate     the number of lists; per list its length n (1 .. 64) and n durations; the number of points; per point the index
//              of its list and t, the points ordered by list.  A workgroup stages one list in LDS, as phase_locate_kernel
//              does, and each of its lanes looks up one time.
//   durations* the number of cases; per case the number of phases n (1 .. 32), whether the foot starts in contact, the
//              polynomials per swing phase and per stance phase of the force, t_total, then the n - 1 schedule variables.
//              Each case runs on a blob of its own, filled by hand with the fields the function reads: a PhaseTables whose
//              slot e = case mod 4 describes the ee-motion polynomials and whose slot (e + 1) mod 4 the ee-force polynomials.
//   hermite    the number of points; per point t and iT.
//
// Exit status: see probe_host.h.
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels/phase_durations.h"
#include "kernels/spline_math.h"

#define PROBE_NAME "segment_probe"
#include "probe_host.h"

namespace {
constexpr int BLOCK = 256;
constexpr int DUR_OUT = twr::TWR_MAX_PHASES_DEV + 2 * twr::kMaxPhasePolys;
constexpr int X_PAD = 3;   // the schedule variables of a case start at this x offset

struct LocateWork {
  int32_t d_at, n, p_at, count;   // the list: durations[d_at .. d_at + n); the points [p_at, p_at + count), count <= BLOCK
};

__global__ __launch_bounds__(BLOCK) void locate_probe(const LocateWork* __restrict__ work, const double* __restrict__ durations,
                                                      const double* __restrict__ t, double* __restrict__ out) {
  __shared__ double s_d[twr::kMaxPhasePolys];
  const LocateWork w = work[blockIdx.x];
  const int lane = threadIdx.x;
  if (lane < w.n) s_d[lane] = durations[w.d_at + lane];
  __syncthreads();
  if (lane >= w.count) return;
  double tl;
  const int id = twr::locate_segment(s_d, w.n, t[w.p_at + lane], tl);
  out[2 * (size_t)(w.p_at + lane)] = (double)id;
  out[2 * (size_t)(w.p_at + lane) + 1] = tl;
}

struct DurWork {
  uint64_t blob, x;
  int32_t e, pad;
};

__global__ __launch_bounds__(BLOCK) void durations_probe(const DurWork* __restrict__ work, double* __restrict__ out, int nthreads) {
  __shared__ double s_ph[twr::TWR_MAX_PHASES_DEV], s_md[twr::kMaxPhasePolys];
  const DurWork w = work[blockIdx.x];
  const char* blob = reinterpret_cast<const char*>(w.blob);
  const twr::PhaseTables* PT = twr::tbl<twr::PhaseTables>(blob, 0);
  const double* x = reinterpret_cast<const double*>(w.x);
  const int lane = threadIdx.x;
  double* __restrict__ o = out + (size_t)DUR_OUT * blockIdx.x;
  twr::phase_poly_durations_wave(PT, blob, x, w.e, s_ph, s_md, lane, nthreads);
  for (int i = lane; i < PT->n_phases[w.e]; i += nthreads) o[i] = s_ph[i];
  for (int q = lane; q < PT->n_mpoly[w.e]; q += nthreads) o[twr::TWR_MAX_PHASES_DEV + q] = s_md[q];
  __syncthreads();
  const int f = (w.e + 1) % twr::kMaxEE;
  twr::phase_poly_durations_wave(PT, blob, x, f, s_ph, s_md, lane, nthreads);
  for (int q = lane; q < PT->n_mpoly[f]; q += nthreads) o[twr::TWR_MAX_PHASES_DEV + twr::kMaxPhasePolys + q] = s_md[q];
}

__global__ __launch_bounds__(BLOCK) void hermite_probe(const double* __restrict__ p, long n, double* __restrict__ out) {
  const long i = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= n) return;
  double wp[4], wv[4], wa[4];
  twr::hermite_all(p[2 * i], p[2 * i + 1], wp, wv, wa);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[12 * i + j] = wp[j];
    out[12 * i + 4 + j] = wv[j];
    out[12 * i + 8 + j] = wa[j];
  }
}

// ee-motion (constant = contact) or ee-force (constant = !contact) polynomials of n phases: BuildPolyInfos
// (nodes_variables_phase_based.cc:38-58)
std::vector<twr::PhasePoly> poly_infos(int n, bool first_constant, int n_changing) {
  std::vector<twr::PhasePoly> v;
  bool constant = first_constant;
  for (int i = 0; i < n; ++i) {
    const int k = constant ? 1 : n_changing;
    for (int j = 0; j < k; ++j) {
      twr::PhasePoly p;
      std::memset(&p, 0, sizeof p);
      p.phase = i;
      p.n_in_phase = k;
      p.poly_in_phase = j;
      v.push_back(p);
    }
    constant = !constant;
  }
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: segment_probe locate|durations64|durations256|hermite IN OUT\n");
    return probe::REFUSED;
  }
  const bool m_locate = !std::strcmp(argv[1], "locate"), m_d64 = !std::strcmp(argv[1], "durations64"),
             m_d256 = !std::strcmp(argv[1], "durations256"), m_hermite = !std::strcmp(argv[1], "hermite");
  if (!m_locate && !m_d64 && !m_d256 && !m_hermite) {
    std::fprintf(stderr, "segment_probe: unknown mode %s\n", argv[1]);
    return probe::REFUSED;
  }
  probe::Input in;
  if (!in.read(argv[2])) return probe::REFUSED;
  // parse on the host first: every count and index is checked against what the file holds before anything reaches the device
  if (!in.have(1)) return in.bad("empty");
  // every mode parses, asks for a device, uploads, sizes `out` and launches; the results of all three are collected below
  std::vector<double> out;
  probe::Device dev;
  double* d_out = nullptr;

  if (m_locate) {
    const long n_lists = (long)in.next();
    if (n_lists < 1 || n_lists > (1L << 20)) return in.bad("list count");
    std::vector<double> durations;
    std::vector<int32_t> d_at, d_n;
    for (long l = 0; l < n_lists; ++l) {
      if (!in.have(1)) return in.bad("truncated list header");
      const long n = (long)in.next();
      if (n < 1 || n > twr::kMaxPhasePolys) return in.bad("list length");
      if (!in.have((size_t)n)) return in.bad("truncated list");
      d_at.push_back((int32_t)durations.size());
      d_n.push_back((int32_t)n);
      durations.insert(durations.end(), in.here(), in.here() + n);
      in.at += (size_t)n;
    }
    if (!in.have(1)) return in.bad("no points");
    const long n_points = (long)in.next();
    if (n_points < 1 || n_points > (1L << 24)) return in.bad("point count");
    if (!in.have(2 * (size_t)n_points)) return in.bad("truncated points");
    if (in.at + 2 * (size_t)n_points != in.v.size()) return in.bad("trailing data");
    std::vector<double> t((size_t)n_points);
    std::vector<LocateWork> work;
    long prev = -1;
    for (long k = 0; k < n_points; ++k) {
      const long l = (long)in[2 * k];
      if (l < 0 || l >= n_lists || l < prev) return in.bad("list index (the points are ordered by list)");
      t[k] = in[2 * k + 1];
      if (l != prev || work.back().count == BLOCK) work.push_back({d_at[l], d_n[l], (int32_t)k, 0});
      ++work.back().count;
      prev = l;
    }
    if (!probe::have_device()) return probe::NO_DEVICE;
    LocateWork* d_work = nullptr;
    double *d_dur = nullptr, *d_t = nullptr;
    out.resize(2 * (size_t)n_points);
    if (!dev.upload(&d_work, work) || !dev.upload(&d_dur, durations) || !dev.upload(&d_t, t) || !dev.results(&d_out, out.size()))
      return probe::HIP_FAILED;
    locate_probe<<<(unsigned)work.size(), BLOCK>>>(d_work, d_dur, d_t, d_out);
  } else if (m_hermite) {
    const long n = (long)in.next();
    if (n < 1 || n > (1L << 24)) return in.bad("point count");
    if (!in.have(2 * (size_t)n)) return in.bad("truncated points");
    if (in.at + 2 * (size_t)n != in.v.size()) return in.bad("trailing data");
    if (!probe::have_device()) return probe::NO_DEVICE;
    double* d_p = nullptr;
    out.resize(12 * (size_t)n);
    if (!dev.upload(&d_p, in.here(), 2 * (size_t)n) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
    hermite_probe<<<(unsigned)((n + BLOCK - 1) / BLOCK), BLOCK>>>(d_p, n, d_out);
  } else {
    const long n_cases = (long)in.next();
    if (n_cases < 1 || n_cases > 4096) return in.bad("case count");
    // one blob per case: PhaseTables, then the ee-motion PhasePoly array, then the ee-force one; one x per case
    std::vector<std::vector<char>> blobs;
    std::vector<std::vector<double>> xs;
    std::vector<int> ee;
    for (long c = 0; c < n_cases; ++c) {
      if (!in.have(5)) return in.bad("truncated case header");
      const long n = (long)in[0];
      const bool contact = in[1] != 0.0;
      const long pps = (long)in[2], ppf = (long)in[3];
      const double t_total = in[4];
      in.at += 5;
      if (n < 1 || n > twr::TWR_MAX_PHASES_DEV || pps < 1 || pps > 16 || ppf < 1 || ppf > 16) return in.bad("case header");
      if (!in.have((size_t)(n - 1))) return in.bad("truncated case");
      const std::vector<twr::PhasePoly> mp = poly_infos((int)n, contact, (int)pps), fp = poly_infos((int)n, !contact, (int)ppf);
      if (mp.size() > (size_t)twr::kMaxPhasePolys || fp.size() > (size_t)twr::kMaxPhasePolys) return in.bad("more than 64 polynomials");
      const int e = (int)(c % twr::kMaxEE), f = (e + 1) % twr::kMaxEE;
      twr::PhaseTables PT;
      std::memset(&PT, 0, sizeof PT);
      for (int s : {e, f}) {
        PT.off_sched[s] = X_PAD;
        PT.n_phases[s] = (int32_t)n;
        PT.t_total[s] = t_total;
      }
      PT.n_mpoly[e] = (int32_t)mp.size();
      PT.o_mpoly[e] = (uint32_t)sizeof PT;
      PT.n_mpoly[f] = (int32_t)fp.size();
      PT.o_mpoly[f] = (uint32_t)(sizeof PT + mp.size() * sizeof(twr::PhasePoly));
      std::vector<char> blob(sizeof PT + (mp.size() + fp.size()) * sizeof(twr::PhasePoly));
      std::memcpy(blob.data(), &PT, sizeof PT);
      std::memcpy(blob.data() + PT.o_mpoly[e], mp.data(), mp.size() * sizeof(twr::PhasePoly));
      std::memcpy(blob.data() + PT.o_mpoly[f], fp.data(), fp.size() * sizeof(twr::PhasePoly));
      std::vector<double> x((size_t)X_PAD, -1.0);
      x.insert(x.end(), in.here(), in.here() + (n - 1));
      in.at += (size_t)(n - 1);
      blobs.push_back(blob), xs.push_back(x), ee.push_back(e);
    }
    if (!in.at_end()) return in.bad("trailing data");
    if (!probe::have_device()) return probe::NO_DEVICE;
    std::vector<DurWork> work;
    for (long c = 0; c < n_cases; ++c) {
      char* d_blob = nullptr;
      double* d_x = nullptr;
      if (!dev.upload(&d_blob, blobs[c]) || !dev.upload(&d_x, xs[c])) return probe::HIP_FAILED;
      work.push_back({(uint64_t)(uintptr_t)d_blob, (uint64_t)(uintptr_t)d_x, ee[c], 0});
    }
    DurWork* d_work = nullptr;
    out.resize((size_t)DUR_OUT * n_cases);
    if (!dev.upload(&d_work, work) || !dev.results(&d_out, out.size())) return probe::HIP_FAILED;
    const int nthreads = m_d64 ? 64 : 256;
    durations_probe<<<(unsigned)n_cases, nthreads>>>(d_work, d_out, nthreads);
  }
  if (!probe::collect(out.data(), d_out, out.size()) || !dev.release()) return probe::HIP_FAILED;
  return probe::write_out(argv[3], out);
}
