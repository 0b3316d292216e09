// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the 2-d convolution on MX codes that writes MX codes (qs_mx_conv_q.h): the
// implicit GEMM of qs_mx_conv2d_v with bias, optional ReLU and the MX quantizer of the output in its epilogue, all 5 x 5 pairs of
// input formats; the output format is a kernel argument.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_conv_q.h"

namespace {

// the checks of qs_mx_conv2d_q_v and the route it takes for these operands: QS_MX_CONV_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_conv_q_route(const qs_mx_conv2d_q_args& a, MxConvPlan* plan) {
    int st = mx_conv_check_operands(a, mx_q_args_ok(a));
    if (st != QS_OK) return st;
    if (a.bias && (((uintptr_t)a.bias) & 3u) != 0) return QS_ERR_ALIGN;
    if ((st = mx_conv_check_limits(a)) != QS_OK) return st;
    MxConvPlan p;
    const int route = mx_conv2d_route_of(a, &p);
    if (route <= 0) return route;
    const int64_t out = p.M * a.Cout;      // (every product below was bounded by mx_conv_plan)
    if (mx_overlap(a.out_codes, out, a.x_codes, a.B * a.H * a.W * a.C) ||
        mx_overlap(a.out_codes, out, a.w_codes, a.Cout * a.KH * a.KW * a.C))
        return QS_ERR_ARG;
    if (plan) *plan = p;
    return route;
}

}  // namespace

extern "C" {

int qs_mx_conv2d_q_route(const qs_mx_conv2d_q_args* args) {
    qs_mx_conv2d_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_conv_q_route(a, nullptr);
}

int qs_mx_conv2d_q_v(const qs_mx_conv2d_q_args* args) {
    qs_mx_conv2d_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    MxConvPlan p;
    const int route = mx_conv_q_route(a, &p);
    if (route <= 0) return route;
    if (route == QS_MX_CONV_ROUTE_GEMM) {  // x IS A [B H W, C] and w IS B [Cout, C] as they lie
        qs_mx_matmul_q_args m = {};
        m.struct_size = sizeof(m);
        m.a_format = a.x_format, m.b_format = a.w_format;
        m.a_codes = a.x_codes, m.a_scales = a.x_scales, m.b_codes = a.w_codes, m.b_scales = a.w_scales;
        m.bias = a.bias, m.out_format = a.out_format, m.act = a.act, m.out_codes = a.out_codes, m.out_scales = a.out_scales;
        m.M = p.M, m.N = a.Cout, m.K = a.C;
        m.stream = a.stream;
        return qs_mx_matmul_q_v(&m);
    }
    const int tiles_n = (int)mx_tiles(a.Cout);
    const int64_t grid = mx_tiles(p.M) * tiles_n;
    const MxcShape g = mxc_shape(a, p.OH, p.OW);
    const MxFormat f = mx_format(a.out_format);
    return mx_dispatch(a.x_format, a.w_format, route == QS_MX_CONV_ROUTE_VEC, [&](auto FX, auto FW, auto VEC) {
        hipLaunchKernelGGL((mx_conv_q_kernel<decltype(FX)::value, decltype(FW)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.bias,
                           (int)(a.act == QS_MX_ACT_RELU), f, a.out_codes, a.out_scales, p.M, a.Cout, g, tiles_n, mx_c_vec(a.out_codes, a.Cout));
        return launch_status();
    });
}

}  // extern "C"
