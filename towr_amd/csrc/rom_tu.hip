// Second translation unit of the kernels: only twr::rom_kernel and its lookup, compiled with
// -mllvm -amdgpu-sched-strategy=max-memory-clause (see Makefile and kernels/rom.h).
#include <hip/hip_runtime.h>

#include "eval_plan.h"

#include "kernels/common.h"
#include "kernels/host_launch.h"
#include "kernels/spline_math.h"
#include "kernels/rom_item.h"
#include "kernels/copy_out.h"
#include "kernels/rom.h"

namespace twr {

template <int NIT, bool WANT_G, bool WANT_J, bool NT>
__global__ __launch_bounds__(64, 1) void rom_kernel(const RomWork* __restrict__ work, int n_work, const double* __restrict__ x,
                                                    double* __restrict__ g, double* __restrict__ jac) {
  __shared__ __attribute__((aligned(16))) double stage[kRomLds];
  rom_body<NIT, WANT_G, WANT_J, NT>(work, n_work, x, g, jac, stage, threadIdx.x, blockIdx.x, gridDim.x);
}
RomFn rom_kernel_fn(const LaunchStep& p) {
  return pick<kRomNits>(p.nit, [&](auto nit) {
    return pick<kStoresNT>(p.store, [&](auto st) -> RomFn { return rom_kernel<nit, StoreG(st), StoreJ(st), StoreNT(st)>; });
  });
}

}  // namespace twr
