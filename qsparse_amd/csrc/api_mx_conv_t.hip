// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the transposed 2-d convolution on MX codes (qs_mx_conv_t.h): the
// fractionally-strided implicit GEMM through the block-scaled MFMA, all 5 x 5 pairs of element formats.  Also the input gradient of
// qs_mx_conv2d_v's convolution (qsparse_amd/mx_conv_transpose.py).
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_conv_t.h"

namespace {

// the checks of qs_mx_conv_transpose2d_v and the route it takes for these operands: QS_MX_CONV_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_conv_t_route(const qs_mx_conv_transpose2d_args& a, MxConvPlan* plan) {
    // the output padding must be smaller than the stride or the dilation (torch's rule)
    const bool out_pad_ok = a.out_pad_h >= 0 && a.out_pad_w >= 0 && a.out_pad_h < (a.stride_h > a.dil_h ? a.stride_h : a.dil_h) &&
                            a.out_pad_w < (a.stride_w > a.dil_w ? a.stride_w : a.dil_w);
    const int st = mx_conv_check_args(a, out_pad_ok);
    if (st != QS_OK) return st;
    if (a.H > INT32_MAX || a.W > INT32_MAX) return QS_ERR_ARG;
    // every term below is a product of two values below 2^31: no overflow in 64 bits
    const int64_t EH = (int64_t)a.dil_h * (a.KH - 1), EW = (int64_t)a.dil_w * (a.KW - 1);             // reach of the dilated kernel
    const int64_t OH = (a.H - 1) * a.stride_h - 2 * (int64_t)a.pad_h + EH + a.out_pad_h + 1;
    const int64_t OW = (a.W - 1) * a.stride_w - 2 * (int64_t)a.pad_w + EW + a.out_pad_w + 1;
    if (OH < 1 || OW < 1) return QS_ERR_ARG;
    // the kernel keeps oh + ph, ow + pw and kh dh, kw dw in 31 bits (addresses: 64)
    if (OH + a.pad_h > INT32_MAX || OW + a.pad_w > INT32_MAX || EH > INT32_MAX || EW > INT32_MAX) return QS_ERR_ARG;
    const int route = mx_conv_plan(a, OH, OW, plan);
    // without output padding either, OH == H and OW == W
    return route > 0 && mx_conv_is_gemm(a) && a.out_pad_h == 0 && a.out_pad_w == 0 ? QS_MX_CONV_ROUTE_GEMM : route;
}

}  // namespace

extern "C" {

int qs_mx_conv_transpose2d_route(const qs_mx_conv_transpose2d_args* args) {
    qs_mx_conv_transpose2d_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_conv_t_route(a, nullptr);
}

int qs_mx_conv_transpose2d_v(const qs_mx_conv_transpose2d_args* args) {
    qs_mx_conv_transpose2d_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    MxConvPlan p;
    const int route = mx_conv_t_route(a, &p);
    if (route <= 0) return route;
    if (route == QS_MX_CONV_ROUTE_GEMM) return mx_conv_as_matmul(a, p.M);
    const int tiles_n = (int)mx_tiles(a.Cout);
    const int64_t grid = mx_tiles(p.M) * tiles_n;
    const MxctShape g = {mxc_shape(a, p.OH, p.OW), UINT32_MAX / (uint32_t)a.stride_h, UINT32_MAX / (uint32_t)a.stride_w};
    return mx_dispatch(a.x_format, a.w_format, route == QS_MX_CONV_ROUTE_VEC, [&](auto FX, auto FW, auto VEC) {
        hipLaunchKernelGGL((mx_conv_t_kernel<decltype(FX)::value, decltype(FW)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.bias, a.y, a.ydt, p.M,
                           a.Cout, g, tiles_n, mx_y_vec(a.y, a.ydt, a.Cout));
        return launch_status();
    });
}

}  // extern "C"
