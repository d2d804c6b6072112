// tmac_select.h — run-time values to template arguments, and the launch behind them.  The one idiom of every kernel launcher:
//     plan (tmac_launch_plan.h, plain C++)  ->  select (here)  ->  launch (here).
// A selector hands the value to a generic lambda as a compile-time constant; the lambda nests the next selector or, innermost, guards the
// instantiation with the kernel's policy predicate (`if constexpr (!..._inst_exists(...)) return hipErrorInvalidValue;`) and launches.
// Only what passes the predicate is instantiated: the predicate IS the list of kernels a translation unit emits.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace tmac {

// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline hipError_t sel_bool(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }

// f(std::integral_constant<int, V>{}) for the V of Vs... that equals v; none: hipErrorInvalidValue
template <int... Vs, class F>
inline hipError_t sel_int(int v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs ? (e = f(std::integral_constant<int, Vs>{}), true) : false) || ...);
    return e;
}

// Launch with `lds_bytes` of dynamic LDS.  Above 64 KB the size must be allowed per kernel first (hipFuncAttributeMaxDynamicSharedMemorySize):
// allow_lds does, and launch_lds allows it on every such launch.  launch_lds_once keeps the launcher's per-instantiation cache (`allowed`: a function-local
// static of the selecting lambda, the bytes allowed so far) and raises it to `allow_bytes`, the kernel's largest footprint, by one call.
template <class... KA>
inline hipError_t allow_lds(void (*kern)(KA...), size_t lds_bytes) {
    if (lds_bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}
template <class... KA, class... A>
inline hipError_t launch_lds(void (*kern)(KA...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const A&... args) {
    const hipError_t e = allow_lds(kern, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, args...);
    return hipGetLastError();
}
template <class... KA, class... A>
inline hipError_t launch_lds_once(size_t& allowed, size_t allow_bytes, void (*kern)(KA...), dim3 grid, dim3 block, size_t lds_bytes,
                                  hipStream_t st, const A&... args) {
    if (lds_bytes > allowed) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)allow_bytes);
        if (e != hipSuccess) return e;
        allowed = allow_bytes;
    }
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, st, args...);
    return hipGetLastError();
}

}  // namespace tmac
