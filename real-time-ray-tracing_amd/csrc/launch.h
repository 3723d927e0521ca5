// Host-side launch helpers: run-time flags as template arguments, and a checked kernel launch.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace rtl {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for run-time bools b0, b1, ...: inside a
// generic lambda each argument converts to a constant, so a kernel template is named once,
//   with_flags([&](auto rcp, auto pk) { return launch(k_filter<rcp, pk>, g, b, s, args...); }, rcp, pk);
// instantiates k_filter for every combination and launches the chosen one.  A combination that must
// not exist is folded into one that does with a constant in the lambda
// (constexpr bool kPk = list && pk;), not dispatched on.
template <class F>
auto with_flags(F&& f) {
    return f();
}
template <class F, class... Bools>
auto with_flags(F&& f, bool b, Bools... rest) {
    auto bind = [&](auto k) { return with_flags([&](auto... ks) { return f(k, ks...); }, rest...); };
    return b ? bind(std::true_type{}) : bind(std::false_type{});
}

// kernel<<<grid, block, 0, stream>>>(args...) with the arguments converted to the kernel's parameter
// types (a uint2* for a const uint2* parameter needs no cast); the launch's error
template <class... Params, class... Args>
hipError_t launch(void (*kernel)(Params...), dim3 grid, dim3 block, hipStream_t stream, Args&&... args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, static_cast<Params>(args)...);
    return hipGetLastError();
}

}  // namespace rtl
