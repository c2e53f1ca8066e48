// The host side that the stand-alone device probes tests/*_probe.hip share (nothing in the product includes it): reading
// IN, a cursor over its doubles, HIP error reporting, owned device buffers, the result buffer and writing OUT.  A probe
// defines PROBE_NAME ("trig_probe", ...) before it includes this file; every message starts with that name.  Host code
// only: no kernel and no __device__ function lives here.
//
// Exit status of every probe: 0 done, 2 usage / file error, 3 no HIP device, 4 a HIP call failed.  Status 2 is decided
// on the host before anything reaches a device; tests/probe.py starts no further probe after a 3 or a 4.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#ifndef PROBE_NAME
#error "define PROBE_NAME before including probe_host.h"
#endif

namespace probe {
enum : int { DONE = 0, REFUSED = 2, NO_DEVICE = 3, HIP_FAILED = 4 };

inline bool ok(hipError_t err, const char* what) {
  if (err == hipSuccess) return true;
  std::fprintf(stderr, PROBE_NAME ": %s: %s\n", what, hipGetErrorString(err));
  return false;
}

// the doubles of IN and a cursor over them: in[k] is the k-th double from the cursor on
struct Input {
  std::vector<double> v;
  const char* file = "";
  size_t at = 0;

  bool read(const char* path) {
    file = path;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) {
      std::fprintf(stderr, PROBE_NAME ": cannot read %s\n", path);
      return false;
    }
    double buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(double), 4096, f)) > 0) v.insert(v.end(), buf, buf + got);
    std::fclose(f);
    return true;
  }
  bool have(size_t k) const { return at + k <= v.size(); }
  bool at_end() const { return at == v.size(); }
  double operator[](size_t k) const { return v[at + k]; }
  double next() { return v[at++]; }
  const double* here() const { return v.data() + at; }
  int bad(const char* what) const {
    std::fprintf(stderr, PROBE_NAME ": %s: %s\n", file, what);
    return REFUSED;
  }
};

inline bool have_device() {
  int devices = 0;
  if (hipGetDeviceCount(&devices) == hipSuccess && devices > 0) return true;
  std::fprintf(stderr, PROBE_NAME ": no HIP device\n");
  return false;
}

// Device buffers of one owner, freed together by release().  A probe that meets a HIP failure returns HIP_FAILED at once
// and frees nothing more.
struct Device {
  std::vector<void*> owned;

  template <class T>
  bool alloc(T** dev, size_t n) {   // an empty buffer still holds one element
    void* p = nullptr;
    if (!ok(hipMalloc(&p, (n ? n : 1) * sizeof(T)), "hipMalloc")) return false;
    owned.push_back(p);
    *dev = static_cast<T*>(p);
    return true;
  }
  template <class T>
  bool upload(T** dev, const T* host, size_t n) {
    return alloc(dev, n) && (n == 0 || ok(hipMemcpy(*dev, host, n * sizeof(T), hipMemcpyHostToDevice), "copy in"));
  }
  template <class T>
  bool upload(T** dev, const std::vector<T>& host) {
    return upload(dev, host.data(), host.size());
  }
  // n doubles for a kernel's results, every byte 0xFF: what the kernel leaves unwritten reads back as NaN
  bool results(double** dev, size_t n) { return alloc(dev, n) && ok(hipMemset(*dev, 0xFF, n * sizeof(double)), "hipMemset"); }
  bool release() {
    for (void* p : owned)
      if (!ok(hipFree(p), "hipFree")) return false;
    owned.clear();
    return true;
  }
};

// after the caller's launch: the launch and the kernel succeeded, and the n results are in host[0 .. n)
inline bool collect(double* host, const double* dev, size_t n) {
  return ok(hipGetLastError(), "launch") && ok(hipDeviceSynchronize(), "kernel") &&
         ok(hipMemcpy(host, dev, n * sizeof(double), hipMemcpyDeviceToHost), "copy out");
}

// the last statement of a probe's main: its exit status
inline int write_out(const char* path, const std::vector<double>& out) {
  std::FILE* f = std::fopen(path, "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size() || std::fclose(f) != 0) {
    std::fprintf(stderr, PROBE_NAME ": cannot write %s\n", path);
    return REFUSED;
  }
  return DONE;
}
}  // namespace probe
