#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace twr {
#define TWR_DEV __device__ __forceinline__
#ifdef TWR_DIAG_NOCONFLICT
// DIAGNOSTIC BUILD ONLY (make DIAG=-DTWR_DIAG_NOCONFLICT; wrong results on purpose): every scattered 8-byte store into the LDS
// image of dyn_kernel / rom_kernel goes to `8 * lane + a constant of the call site` instead of its CSR position -- the sixteen
// lanes of a ds_write_b64 group then hit sixteen different bank pairs (MI355X_MICROARCH.md: 4 x 16 contiguous lanes, bank =
// (a / 4) mod 32), with the same number of stores and no address arithmetic at all: an UPPER bound of what removing the bank
// conflicts of the image scatter can buy.
template <int N>
TWR_DEV void diag_put(double v) {
  const uint32_t a = (threadIdx.x & 63u) << 3;
  asm volatile("ds_write_b64 %0, %1 offset:%2" ::"v"(a), "v"(v), "n"((N % 30) * 512));
}
#define lds_put(l, o, ...) diag_put<__COUNTER__>(__VA_ARGS__)
#define TWR_ROM_PUT(idx, ...) diag_put<__COUNTER__>(__VA_ARGS__)
#else
#define TWR_ROM_PUT(idx, ...) stage[idx] = (__VA_ARGS__)
TWR_DEV void lds_put(char* __restrict__ lds, uint32_t byte_off, double v) { *reinterpret_cast<double*>(lds + byte_off) = v; }
#endif
TWR_DEV double lds_f64(const char* __restrict__ lds, uint32_t byte_off) {
  return *reinterpret_cast<const double*>(lds + byte_off);
}
// NaN-propagating max of two violations (score_kernel, eval_scores_kernel): a NaN operand wins
TWR_DEV double nan_max(double a, double b) { return (a != a || b != b) ? (a != a ? a : b) : fmax(a, b); }
constexpr int TWR_MAX_PHASES_DEV = 32;  // = TWR_MAX_PHASES of include/towr_amd.h

template <typename T>
TWR_DEV const T* tbl(const char* blob, uint32_t off) {
  return reinterpret_cast<const T*>(blob + off);
}
// Device addresses stored as integers in the work items: tell the compiler they are global memory
// (a plain reinterpret_cast yields a generic pointer -> flat_load, which also ties up lgkmcnt).
#if defined(__HIP_DEVICE_COMPILE__)
#define TWR_GLOBAL __attribute__((address_space(1)))
#else
#define TWR_GLOBAL
#endif
template <typename T>
TWR_DEV const TWR_GLOBAL T* gptr(uint64_t addr) {
  return reinterpret_cast<const TWR_GLOBAL T*>(addr);
}
// Read-only tables reached through a wave-uniform address: the constant address space makes their loads
// scalar (s_load into SGPRs) instead of one vector load per lane.
#if defined(__HIP_DEVICE_COMPILE__)
#define TWR_CONST __attribute__((address_space(4)))
#else
#define TWR_CONST
#endif
template <typename T>
TWR_DEV const TWR_CONST T* cptr(uint64_t addr) {
  return reinterpret_cast<const TWR_CONST T*>(addr);
}
}  // namespace twr
