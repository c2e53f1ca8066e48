#pragma once
#include <stdint.h>

#include "common.h"

namespace twr {
// ---------------------------------------------------------------- LDS image -> global
// The image is placed at stage[par + i] with par = parity of the destination's 8-byte index,
// so that 16-byte aligned global pairs are 16-byte aligned LDS pairs.
TWR_DEV void copy_out(double* __restrict__ dst, const double* __restrict__ stage, int n, int par, int lane) {
  double* al = dst - par;  // 16-byte aligned
  const int total = n + par;
  const int npairs = total >> 1;
  for (int t = lane; t < npairs; t += 64) {
    if (t == 0 && par) {
      al[1] = stage[1];
    } else {
      const double2 v = *reinterpret_cast<const double2*>(stage + 2 * t);
      *reinterpret_cast<double2*>(al + 2 * t) = v;
    }
  }
  if ((total & 1) && lane == 0 && total - 1 >= par) al[total - 1] = stage[total - 1];
}
// Same, with a compile-time number of store instructions: iterations past the end re-store the
// last pair (idempotent).  A fixed count lets the compiler keep the stores in flight behind a
// counted s_waitcnt vmcnt(N) when the persistent loop next touches its prefetched loads (on gfx9
// loads and stores retire through one in-order counter; an unknown store count would force
// vmcnt(0), i.e. a full store drain per slice).
// NT: the 16-byte stores carry the non-temporal hint (global_store_dwordx4 ... nt): the values stream to HBM without
// displacing what the kernels RE-READ -- a sweep's per-candidate tables and x -- from the XCD's L2 and the Infinity Cache.
// Chosen per batch (twr_batch_create): worth 5-15 % of a step whose candidates all bring their own tables and
// whose output exceeds the Infinity Cache; it COSTS rom_kernel 10-15 % when one structure serves thousands of problems.
template <int NIT, int kBatch, bool NT = false>
TWR_DEV void copy_out_fixed(double* __restrict__ dst, const double* __restrict__ stage, int n, int par, int lane) {
  // byte offsets as unsigned 32-bit values: one VGPR addresses both the LDS read and the global store (wave-uniform
  // base + 32-bit offset), two VALU instructions per store instead of a 64-bit address computation
  char* al = reinterpret_cast<char*>(dst - par);  // 16-byte aligned
  const char* st = reinterpret_cast<const char*>(stage);
  const int total = n + par;
  const uint32_t last = (uint32_t)((total >> 1) - 1) * 16u;  // last complete pair; pairs [par, npairs) are complete
  const uint32_t first = (uint32_t)(par + lane) * 16u;
  // Branch-free on purpose: lanes past the end of the slice re-store its last pair (idempotent; predicating them off
  // makes the compiler sink every LDS read into its own `if`), and the count of vector-memory instructions stays a
  // compile-time constant (counted s_waitcnt for the prefetched loads).
  // kBatch = LDS reads in flight before the first store needs its data.  (In dyn_kernel, which sits at the VGPR limit,
  // the register allocator leaves the copy-out one quad of registers and the reads end up serialised with their stores
  // anyway; moving the copy-out ahead of the front half or pipelining it by hand changed nothing measurable.)
#pragma unroll
  for (int it0 = 0; it0 < NIT; it0 += kBatch) {
    double2 v[kBatch];
    uint32_t off[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; ++b)
      if (it0 + b < NIT) {
        off[b] = min(first + 1024u * (uint32_t)(it0 + b), last);
        v[b] = *reinterpret_cast<const double2*>(st + off[b]);
      }
#pragma unroll
    for (int b = 0; b < kBatch; ++b)
      if (it0 + b < NIT) {
        if (NT) {
          typedef double twr_d2 __attribute__((ext_vector_type(2)));
          const twr_d2 vv = {v[b].x, v[b].y};
          __builtin_nontemporal_store(vv, reinterpret_cast<twr_d2*>(al + off[b]));
        } else {
          *reinterpret_cast<double2*>(al + off[b]) = v[b];
        }
      }
  }
  // first and last value of the slice (they sit in half pairs when the slice starts / ends on an odd index): stored by
  // every lane, whatever the parity -- two more store instructions that are ALWAYS issued.  A store inside a divergent
  // `if` is a branch the compiler must assume not taken when it counts the stores behind a prefetched load, and one
  // uncounted store is enough to turn the next counted wait into a drain of the whole copy-out.
  // (A/B on one box, rom_kernel: these two as `if (lane == 0)` stores cost 4 %: 0.876 -> 0.914 ms)
  dst[0] = stage[par];
  dst[n - 1] = stage[total - 1];
}

// dynamic / range of motion: persistent workgroups, software pipelined over the strided work list.
// Loop body for slice i (its record -- and for rom its x values -- were prefetched):
//   C  compute slice i into the LDS image          (the ONLY call site of the math: every slice of a
//      batch goes through the same instruction sequence, so equal x give bit-identical results
//      wherever they sit in the batch)
//   A  issue the record loads of slice i+2 and (rom) the x loads of slice i+1
//   B  stream the image of slice i to HBM with a fixed number of store instructions
// One wave per workgroup: its LDS accesses are ordered, no barriers.
}  // namespace twr
