// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two permutations around the expert products of a mixture-of-experts layer
// (qs_mx_moe_dispatch.h): rows quantized once and written to the k rows the routing gave them, and the k expert rows of every token
// weighted by its gates and summed.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_moe_dispatch.h"

namespace {

// T, D, k of either call: 0 for an empty problem, 1 to go on, QS_ERR_ARG
int moe_shape(int64_t T, int64_t D, int k) {
    if (T < 0 || D < 0 || k < 1 || k > 32 || T > INT32_MAX || T * k > INT32_MAX || D > INT32_MAX) return QS_ERR_ARG;
    if ((T + kMoeDTokens - 1) / kMoeDTokens > kMaxGrid) return QS_ERR_ARG;
    return T == 0 || D == 0 ? 0 : 1;
}

int mx_moe_dispatch_route(const qs_mx_moe_dispatch_args& a) {
    if (!a.inv || !a.codes || !a.scales || (!a.x && (!a.x_codes || !a.x_scales))) return QS_ERR_ARG;
    if (!mx_format_ok(a.format)) return QS_ERR_ARG;
    const int shape = moe_shape(a.T, a.D, a.k);
    if (shape < 0 || (a.x && a.stride < a.D)) return QS_ERR_ARG;
    if (a.x && !dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if (!aligned4(a.inv) || (a.x && (((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0)) return QS_ERR_ALIGN;
    if (shape == 0) return 0;
    if (!a.x) return a.D % 16 == 0 && aligned16(a.x_codes) && aligned16(a.codes) ? QS_MX_MOE_DISPATCH_ROUTE_VEC : QS_MX_MOE_DISPATCH_ROUTE_PLAIN;
    return a.D % 8 == 0 && a.stride % 8 == 0 && aligned16(a.x) && aligned8(a.codes) ? QS_MX_MOE_DISPATCH_ROUTE_VEC
                                                                                    : QS_MX_MOE_DISPATCH_ROUTE_PLAIN;
}

int mx_moe_dispatch_launch(const qs_mx_moe_dispatch_args& a, int route) {
    MoeDispatchArgs k;
    k.x = a.x, k.xc = a.x_codes, k.xs = a.x_scales, k.inv = a.inv, k.codes = a.codes, k.scales = a.scales;
    k.stride = a.stride, k.rows = a.T * a.k;
    k.T = (int)a.T, k.D = (int)a.D, k.k = a.k, k.nb = (int)((a.D + QS_MX_BLOCK - 1) / QS_MX_BLOCK);
    const dim3 grid((unsigned)((a.T + kMoeDTokens - 1) / kMoeDTokens)), block(kMoeDThreads);
    const bool vec = route == QS_MX_MOE_DISPATCH_ROUTE_VEC;
    hipStream_t s = (hipStream_t)a.stream;
    if (!a.x) {
        if (vec) hipLaunchKernelGGL((mx_moe_dispatch_copy_kernel<true>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((mx_moe_dispatch_copy_kernel<false>), grid, block, 0, s, k);
        return launch_status();
    }
    const MxFormat f = mx_format(a.format);
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        if (vec) hipLaunchKernelGGL((mx_moe_dispatch_kernel<XD, true>), grid, block, 0, s, f, k);
        else hipLaunchKernelGGL((mx_moe_dispatch_kernel<XD, false>), grid, block, 0, s, f, k);
        return launch_status();
    });
}

int mx_moe_combine_route(const qs_mx_moe_combine_args& a) {
    if (!a.y || !a.inv || !a.gates || !a.out) return QS_ERR_ARG;
    const int shape = moe_shape(a.T, a.D, a.k);
    if (shape < 0) return QS_ERR_ARG;
    if (!dt_ok(a.ydt) || !dt_ok(a.odt)) return QS_ERR_DTYPE;
    if (!aligned4(a.inv) || !aligned4(a.gates) || (((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 ||
        (((uintptr_t)a.out) & (dt_size(a.odt) - 1)) != 0)
        return QS_ERR_ALIGN;
    if (shape == 0) return 0;
    const bool vec = a.D % 4 == 0 && (((uintptr_t)a.y) & (4 * dt_size(a.ydt) - 1)) == 0 && (((uintptr_t)a.out) & (4 * dt_size(a.odt) - 1)) == 0;
    return vec ? QS_MX_MOE_DISPATCH_ROUTE_VEC : QS_MX_MOE_DISPATCH_ROUTE_PLAIN;
}

int mx_moe_combine_launch(const qs_mx_moe_combine_args& a, int route) {
    MoeCombineArgs k;
    k.y = a.y, k.inv = a.inv, k.gates = a.gates, k.out = a.out, k.rows = a.T * a.k;
    k.T = (int)a.T, k.D = (int)a.D, k.k = a.k, k.odt = a.odt;
    const dim3 grid((unsigned)((a.T + kMoeDTokens - 1) / kMoeDTokens)), block(kMoeDThreads);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.ydt, [&](auto Y) {
        constexpr int YD = decltype(Y)::value;
        if (route == QS_MX_MOE_DISPATCH_ROUTE_VEC) hipLaunchKernelGGL((mx_moe_combine_kernel<YD, true>), grid, block, 0, s, k);
        else hipLaunchKernelGGL((mx_moe_combine_kernel<YD, false>), grid, block, 0, s, k);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_moe_dispatch_route(const qs_mx_moe_dispatch_args* args) {
    qs_mx_moe_dispatch_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_moe_dispatch_route(a);
}

int qs_mx_moe_dispatch_v(const qs_mx_moe_dispatch_args* args) {
    qs_mx_moe_dispatch_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_moe_dispatch_route(a);
    if (route <= 0) return route;
    return mx_moe_dispatch_launch(a, route);
}

int qs_mx_moe_combine_route(const qs_mx_moe_combine_args* args) {
    qs_mx_moe_combine_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_moe_combine_route(a);
}

int qs_mx_moe_combine_v(const qs_mx_moe_combine_args* args) {
    qs_mx_moe_combine_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_moe_combine_route(a);
    if (route <= 0) return route;
    return mx_moe_combine_launch(a, route);
}

}  // extern "C"
