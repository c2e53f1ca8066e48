#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <tuple>
#include <utility>

namespace twr {
// Kernel launch that RETURNS its status (hipLaunchKernel) instead of leaving it in the thread's sticky error slot: the
// library neither reads nor clears an error the host application may have pending.
template <typename T, size_t... I>
static inline hipError_t twr_launch_impl(const void* k, dim3 g, dim3 b, size_t lds, hipStream_t s, T& vals, std::index_sequence<I...>) {
  void* ptrs[] = {static_cast<void*>(&std::get<I>(vals))...};
  return hipLaunchKernel(k, g, b, ptrs, lds, s);
}
template <typename... P, typename... A>
static inline hipError_t twr_launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A... args) {
  static_assert(sizeof...(P) == sizeof...(A), "kernel argument count");
  std::tuple<P...> vals{static_cast<P>(args)...};
  return twr_launch_impl(reinterpret_cast<const void*>(kern), grid, block, lds, stream, vals, std::index_sequence_for<P...>{});
}
static inline hipError_t twr_first(hipError_t a, hipError_t b) { return a != hipSuccess ? a : b; }
// The instantiation a planned launch names (eval_plan.h: the key lists kStoresNT ... kValuesNx): pick<L>(v, f) returns
// f(std::integral_constant<int, v>) if v is an entry of the list L, else a null kernel.  Every templated kernel has one
// lookup built from these, the one place its instantiations are listed.
template <const auto& L, class F, size_t... I>
static inline auto pick(int v, F f, std::index_sequence<I...>) {
  decltype(f(std::integral_constant<int, L[0]>{})) r = nullptr;
  (void)(... || (L[I] == v && (r = f(std::integral_constant<int, L[I]>{}), true)));
  return r;
}
template <const auto& L, class F>
static inline auto pick(int v, F f) {
  return pick<L>(v, f, std::make_index_sequence<sizeof(L) / sizeof(L[0])>{});
}
}  // namespace twr
