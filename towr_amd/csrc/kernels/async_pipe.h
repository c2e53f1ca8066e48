#pragma once
#include <stdint.h>

#include "common.h"
#include "spline_math.h"

namespace twr {
// --- asynchronous loads.  The software pipeline of dyn_phase_kernel is scheduled by hand: its vector loads are issued
// as asm into AGPRs (free at one wave per SIMD) and waited for with explicit counted s_waitcnt, always inside the
// iteration that issued them.  Left to the compiler the prefetched values are shuffled between register files right
// after the loads are issued (which waits for them on the spot), and every wait behind the copy-out drains its stores.
// The compiler sees none of these loads; a value is used only through the wait that follows its load (`+a` operands),
// and the compiler's own waits (scalar loads, LDS) are unaffected.
typedef float twr_v4f __attribute__((ext_vector_type(4)));
TWR_DEV void aload(double& d, const void* p) { asm volatile("global_load_dwordx2 %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
TWR_DEV void aload(twr_v4f& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
TWR_DEV void aload(uint32_t& d, const void* p) { asm volatile("global_load_dword %0, %1, off" : "=a"(d) : "v"(p) : "memory"); }
// s_waitcnt vmcnt(N) only (gfx9 encoding: vmcnt in bits 3:0 and 15:14, expcnt / lgkmcnt fields left at "no wait")
constexpr int vmcnt_imm(int n) { return (n & 0xF) | (0x7 << 4) | (0xF << 8) | ((n >> 4) << 14); }
TWR_DEV double pdyn_f64(float lo, float hi) { return __hiloint2double((int)__float_as_uint(hi), (int)__float_as_uint(lo)); }
TWR_DEV double sel4(int i, const double v[4]) { return i == 0 ? v[0] : (i == 1 ? v[1] : (i == 2 ? v[2] : v[3])); }
// sum over the four quads of a 16-lane row (lanes l, l-4, l-8, l-12 mod 16): DPP row_ror
TWR_DEV double row4_sum(double v) {
  v += quad_perm<0x124>(v);  // row_ror:4
  v += quad_perm<0x128>(v);  // row_ror:8
  return v;
}
// zero [0, n) doubles of an LDS image (n rounded up to a pair): eight 16-byte stores per lane and round, lanes past the
// end re-clear the last pair
TWR_DEV void lds_clear(double* __restrict__ img, int n, int lane) {
  const double2 z = {0.0, 0.0};
  const int npairs = (n + 1) >> 1, nit = (npairs + 63) >> 6;
  for (int it0 = 0; it0 < nit; it0 += 8) {
#pragma unroll
    for (int b = 0; b < 8; ++b) reinterpret_cast<double2*>(img)[min(lane + 64 * (it0 + b), npairs - 1)] = z;
  }
}
// image -> HBM for a run-time length: batches of eight 16-byte LDS reads, then their eight stores; iterations past the
// end re-store the last complete pair (idempotent).  The image is NOT shifted by the parity of the destination (it fills
// the workgroup's LDS to the last byte): a 16-byte aligned global pair is read from an 8-byte aligned LDS address with
// ds_read2_b64.  The batch is staged in AGPRs (DS and vector-memory instructions take them as data operands; the kernel
// runs few waves per SIMD, so they are free), which leaves the arch VGPRs to the math -- left to the register
// allocator the eight reads end up serialised through one VGPR quad.  Written as asm for that reason; the waits are
// explicit (the compiler's own s_waitcnt counts stay conservative: unknown younger operations only make them stricter).
// NIT > 0: compile-time number of store instructions (the wait for the loads issued before them can then be counted);
// NIT = 0: run-time length (images larger than 40 KB).  At most two more stores follow (odd head / tail).
template <int NIT>
TWR_DEV void stream_out(double* __restrict__ dst, const double* __restrict__ stage, int n, int par, int lane) {
  char* al = reinterpret_cast<char*>(dst - par);  // 16-byte aligned; global pair t = image values 2t - par, 2t + 1 - par
  const int total = n + par;
  const uint32_t last = (uint32_t)((total >> 1) - 1) * 16u;
  const uint32_t first = (uint32_t)(par + lane) * 16u;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)stage - 8u * (uint32_t)par;
  constexpr int kB = 8;
  auto batch = [&](int it0) {
    uint32_t off[kB];
    twr_v4f v[kB];
#pragma unroll
    for (int b = 0; b < kB; ++b) {
      off[b] = min(first + 1024u * (uint32_t)(it0 + b), last);
      asm volatile("ds_read2_b64 %0, %1 offset1:1" : "=a"(v[b]) : "v"(lds0 + off[b]) : "memory");
    }
#pragma unroll
    for (int b = 0; b < kB; ++b) {
      switch (kB - 1 - b) {   // the b-th read has landed once at most kB-1-b younger ones are outstanding
        case 7: asm volatile("s_waitcnt lgkmcnt(7)" : "+a"(v[b])); break;
        case 6: asm volatile("s_waitcnt lgkmcnt(6)" : "+a"(v[b])); break;
        case 5: asm volatile("s_waitcnt lgkmcnt(5)" : "+a"(v[b])); break;
        case 4: asm volatile("s_waitcnt lgkmcnt(4)" : "+a"(v[b])); break;
        case 3: asm volatile("s_waitcnt lgkmcnt(3)" : "+a"(v[b])); break;
        case 2: asm volatile("s_waitcnt lgkmcnt(2)" : "+a"(v[b])); break;
        case 1: asm volatile("s_waitcnt lgkmcnt(1)" : "+a"(v[b])); break;
        default: asm volatile("s_waitcnt lgkmcnt(0)" : "+a"(v[b])); break;
      }
      asm volatile("global_store_dwordx4 %0, %1, %2" : : "v"(off[b]), "a"(v[b]), "s"(al) : "memory");
    }
  };
  if constexpr (NIT > 0) {
    static_assert(NIT % kB == 0, "whole batches");
#pragma unroll
    for (int it0 = 0; it0 < NIT; it0 += kB) batch(it0);
  } else {
    const int nit = ((total >> 1) - par + 63) >> 6;
    for (int it0 = 0; it0 < nit; it0 += kB) batch(it0);
  }
  if (par && lane == 0 && n > 0) dst[0] = stage[0];
  if ((total & 1) && lane == 0 && total - 1 > par) dst[n - 1] = stage[n - 1];
}
}  // namespace twr
