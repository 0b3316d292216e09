// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the 2-d convolution on MX codes (qs_mx_conv.h): implicit GEMM through the
// block-scaled MFMA, all 5 x 5 pairs of element formats.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_conv.h"

namespace {

// the checks of qs_mx_conv2d_v and the route it takes for these operands: QS_MX_CONV_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_conv_route(const qs_mx_conv2d_args& a, MxConvPlan* plan) {
    const int st = mx_conv_check_args(a, true);
    if (st != QS_OK) return st;
    return mx_conv2d_route_of(a, plan);
}

}  // namespace

extern "C" {

int qs_mx_conv2d_route(const qs_mx_conv2d_args* args) {
    qs_mx_conv2d_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_conv_route(a, nullptr);
}

int qs_mx_conv2d_v(const qs_mx_conv2d_args* args) {
    qs_mx_conv2d_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    MxConvPlan p;
    const int route = mx_conv_route(a, &p);
    if (route <= 0) return route;
    if (route == QS_MX_CONV_ROUTE_GEMM) return mx_conv_as_matmul(a, p.M);
    const int tiles_n = (int)mx_tiles(a.Cout);
    const int64_t grid = mx_tiles(p.M) * tiles_n;
    const MxcShape g = mxc_shape(a, p.OH, p.OW);
    return mx_dispatch(a.x_format, a.w_format, route == QS_MX_CONV_ROUTE_VEC, [&](auto FX, auto FW, auto VEC) {
        hipLaunchKernelGGL((mx_conv_kernel<decltype(FX)::value, decltype(FW)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.bias, a.y, a.ydt, p.M,
                           a.Cout, g, tiles_n, mx_y_vec(a.y, a.ydt, a.Cout));
        return launch_status();
    });
}

}  // extern "C"
