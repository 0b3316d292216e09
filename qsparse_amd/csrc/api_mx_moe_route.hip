// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), top-k routing of a mixture-of-experts layer (qs_mx_moe_route.h): selection, gates
// and the deterministic counting sort of the flat ids by expert, in one launch for one tile of tokens and in three for more.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_moe_route.h"

namespace {

int64_t moe_tiles(int64_t T) { return (T + kMoeTile - 1) / kMoeTile; }

// the checks of qs_mx_moe_route_v, in the header's order, and the route: QS_MX_MOE_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_moe_route_route(const qs_mx_moe_route_args& a) {
    if (!a.logits || !a.gates || !a.experts || !a.offs || !a.order || !a.inv) return QS_ERR_ARG;
    if (a.E < 1 || a.E > kMoeMaxE || a.k < 1 || a.k > kMoeMaxK || a.k > a.E || a.T < 0 || a.stride < 0) return QS_ERR_ARG;
    if (a.T > INT32_MAX || a.T * a.k > INT32_MAX) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.logits) & (dt_size(a.xdt) - 1)) != 0 || !aligned4(a.gates) || !aligned4(a.experts) || !aligned4(a.offs) ||
        !aligned4(a.order) || !aligned4(a.inv) || !aligned4(a.workspace))
        return QS_ERR_ALIGN;
    if (a.T == 0) return 0;
    if (a.T <= kMoeTile) return QS_MX_MOE_ROUTE_ONE;
    if (!a.workspace || a.workspace_bytes < 4 * (moe_tiles(a.T) + 1) * a.E) return QS_ERR_ARG;
    return QS_MX_MOE_ROUTE_TILED;
}

template <int XDT>
int select_launch(const MoeRouteArgs& k, int one, hipStream_t s) {
    const dim3 grid((unsigned)k.ntiles), block(kMoeThreads);
    if (k.E <= 64) hipLaunchKernelGGL((mx_moe_route_select_kernel<XDT, 1>), grid, block, 0, s, k, one);
    else if (k.E <= 256) hipLaunchKernelGGL((mx_moe_route_select_kernel<XDT, 4>), grid, block, 0, s, k, one);
    else hipLaunchKernelGGL((mx_moe_route_select_kernel<XDT, 16>), grid, block, 0, s, k, one);
    return launch_status();
}

int mx_moe_route_launch(const qs_mx_moe_route_args& a, int route) {
    MoeRouteArgs k;
    k.logits = a.logits, k.stride = a.stride, k.gates = a.gates, k.experts = a.experts, k.offs = a.offs, k.order = a.order, k.inv = a.inv;
    k.hist = (int32_t*)a.workspace;
    k.T = (int)a.T, k.E = (int)a.E, k.k = a.k, k.ntiles = (int)moe_tiles(a.T);
    hipStream_t s = (hipStream_t)a.stream;
    const int one = route == QS_MX_MOE_ROUTE_ONE;
    const int st = with_dtype(a.xdt, [&](auto X) { return select_launch<decltype(X)::value>(k, one, s); });
    if (st != 0 || one) return st;
    hipLaunchKernelGGL(mx_moe_route_scan_kernel, dim3(1), dim3(kMoeScanThreads), 0, s, k);
    const int64_t n = a.T * a.k;
    hipLaunchKernelGGL(mx_moe_route_place_kernel, dim3((unsigned)((n + kMoeThreads - 1) / kMoeThreads)), dim3(kMoeThreads), 0, s, k);
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_moe_route_route(const qs_mx_moe_route_args* args) {
    qs_mx_moe_route_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_moe_route_route(a);
}

int qs_mx_moe_route_v(const qs_mx_moe_route_args* args) {
    qs_mx_moe_route_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_moe_route_route(a);
    if (route <= 0) return route;
    return mx_moe_route_launch(a, route);
}

}  // extern "C"
