// variant.h — how host code picks one instantiation of a kernel template and launches it.
//
//   variant_dispatch(f, a, b, ...)   a, b, ...: bool, or OneOf<V0, V1, ...>{v} for a small int.  Calls
//                                    f(std::bool_constant<a>{}, std::integral_constant<int, v>{}, ...) and returns what it
//                                    returns (every instantiation of f the same type, void included; that type's
//                                    default when a OneOf value is none of its Vs).
//   launch_kernel(ctx, stage, kernel, grid, block, args...)   one launch on the context's stream, with an event pair
//                                    attached when the stage is being timed.
//
// A call site names its kernel once, in a generic lambda, and states which combinations exist once, as an `if constexpr`
// around the launch: only those are instantiated.  The lambda returns whether it launched, so that a combination the guard
// leaves out is an error at the call site, not a frame that silently was not drawn:
//
//   const bool ok = variant_dispatch([&](auto eo, auto aov) {
//       if constexpr (!(eo.value && aov.value)) { launch_kernel(ctx, NO_STAGE, k<eo.value, aov.value>, grid, block, p); return true; }
//       else return false;
//   }, early_out, want_aov);
#pragma once
#include <hip/hip_ext.h>
#include <type_traits>

#include "common.h"

template <int... Vs> struct OneOf { int v; };

template <class F> auto variant_dispatch(F &&f) { return f(); }
template <class F, class... Rest> auto variant_dispatch(F &&f, bool b, Rest... rest);
template <class F, int V0, int... Vs, class... Rest> auto variant_dispatch(F &&f, OneOf<V0, Vs...> c, Rest... rest) {
    // (the choice made so far is bound as a value: the constants reach f as parameters, usable in constant expressions)
    auto with = [&](auto k) { return variant_dispatch([&](auto... ks) { return f(k, ks...); }, rest...); };
    if (c.v == V0) return with(std::integral_constant<int, V0>{});
    if constexpr (sizeof...(Vs) != 0) return variant_dispatch(f, OneOf<Vs...>{c.v}, rest...);
    else return decltype(with(std::integral_constant<int, V0>{}))();
}
template <class F, class... Rest> auto variant_dispatch(F &&f, bool b, Rest... rest) {
    auto with = [&](auto k) { return variant_dispatch([&](auto... ks) { return f(k, ks...); }, rest...); };
    return b ? with(std::true_type{}) : with(std::false_type{});
}

constexpr int NO_STAGE = -1; // launch_kernel: a launch no stage times

// Timed runs attach the event pair to the launch itself (no marker packets around the kernel).  The pair is taken here,
// immediately before the launch: call this after everything that can fail — a pair that was handed out and never recorded
// would be read by splat_stage_time_stats.
template <class... Params, class... Args>
void launch_kernel(splat_ctx *ctx, int stage, void (*kernel)(Params...), dim3 grid, dim3 block, const Args &...args) {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (stage != NO_STAGE && stage_event_pair(ctx, stage, &ev0, &ev1))
        hipExtLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ev0, ev1, 0, static_cast<Params>(args)...);
    else hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, static_cast<Params>(args)...);
}

// LAUNCH_CHECK where the launch's name is chosen at run time (what: "launch k_...")
inline int launch_check(splat_ctx *ctx, const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SPLAT_OK : ctx_fail(ctx, SPLAT_ERR_HIP, what, e);
}
