// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the transposed 2-d convolution on MX codes (qs_mx_conv_t.h): the
// fractionally-strided implicit GEMM through the block-scaled MFMA, all 5 x 5 pairs of element formats.  Also the input gradient of
// qs_mx_conv2d_v's convolution (qsparse_amd/mx_conv_transpose.py).
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_conv_t.h"

namespace {

struct ConvTPlan {
    int64_t OH, OW, M;
};

// the checks of qs_mx_conv_transpose2d_v and the route it takes for these operands: QS_MX_CONV_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_conv_t_route(const qs_mx_conv_transpose2d_args& a, ConvTPlan* plan) {
    if (!a.x_codes || !a.x_scales || !a.w_codes || !a.w_scales || !a.y) return QS_ERR_ARG;
    if (!mx_format_ok(a.x_format) || !mx_format_ok(a.w_format)) return QS_ERR_ARG;
    if (a.B < 0 || a.Cout < 0 || a.H < 1 || a.W < 1 || a.C < 1 || a.KH < 1 || a.KW < 1) return QS_ERR_ARG;
    if (a.stride_h < 1 || a.stride_w < 1 || a.dil_h < 1 || a.dil_w < 1 || a.pad_h < 0 || a.pad_w < 0) return QS_ERR_ARG;
    // the output padding must be smaller than the stride or the dilation (torch's rule)
    if (a.out_pad_h < 0 || a.out_pad_w < 0) return QS_ERR_ARG;
    if (a.out_pad_h >= (a.stride_h > a.dil_h ? a.stride_h : a.dil_h) || a.out_pad_w >= (a.stride_w > a.dil_w ? a.stride_w : a.dil_w)) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (a.bias && (((uintptr_t)a.bias) & 3u) != 0)) return QS_ERR_ALIGN;
    if (a.H > INT32_MAX || a.W > INT32_MAX || a.C > INT32_MAX - QS_MX_BLOCK || a.B > INT32_MAX || a.Cout > INT32_MAX) return QS_ERR_ARG;
    // every term below is a product of two values below 2^31: no overflow in 64 bits
    const int64_t EH = (int64_t)a.dil_h * (a.KH - 1), EW = (int64_t)a.dil_w * (a.KW - 1);             // reach of the dilated kernel
    const int64_t OH = (a.H - 1) * a.stride_h - 2 * (int64_t)a.pad_h + EH + a.out_pad_h + 1;
    const int64_t OW = (a.W - 1) * a.stride_w - 2 * (int64_t)a.pad_w + EW + a.out_pad_w + 1;
    if (OH < 1 || OW < 1) return QS_ERR_ARG;
    // the kernel keeps oh + ph, ow + pw and kh dh, kw dw in 31 bits (addresses: 64)
    if (OH + a.pad_h > INT32_MAX || OW + a.pad_w > INT32_MAX || EH > INT32_MAX || EW > INT32_MAX) return QS_ERR_ARG;
    const int64_t taps = (int64_t)a.KH * a.KW, Cp = (a.C + QS_MX_BLOCK - 1) / QS_MX_BLOCK * QS_MX_BLOCK;
    if (taps > INT32_MAX || taps > INT64_MAX / Cp) return QS_ERR_ARG;
    if (a.B == 0 || a.Cout == 0) return 0;
    const int64_t Kp = taps * Cp;
    if (OH > INT64_MAX / OW || a.B > INT64_MAX / (OH * OW)) return QS_ERR_ARG;
    const int64_t M = a.B * OH * OW;
    if (a.H > INT64_MAX / a.W || a.B > INT64_MAX / (a.H * a.W) || a.B * a.H * a.W > INT64_MAX / a.C) return QS_ERR_ARG;
    if (M > INT64_MAX / a.Cout || M > INT64_MAX / Kp || a.Cout > INT64_MAX / Kp) return QS_ERR_ARG;
    const int64_t tiles = ((M + kMxgTile - 1) / kMxgTile) * ((a.Cout + kMxgTile - 1) / kMxgTile);
    if (tiles > kMaxGrid) return QS_ERR_ARG;
    if (plan) *plan = ConvTPlan{OH, OW, M};
    if (taps == 1 && a.stride_h == 1 && a.stride_w == 1 && a.pad_h == 0 && a.pad_w == 0 && a.out_pad_h == 0 && a.out_pad_w == 0 &&
        a.C % QS_MX_BLOCK == 0)
        return QS_MX_CONV_ROUTE_GEMM;                   // OH == H, OW == W: x is A [B H W, C] and w is B [Cout, C] as they lie
    return (a.C % 16 == 0 && aligned16(a.x_codes) && aligned16(a.w_codes)) ? QS_MX_CONV_ROUTE_VEC : QS_MX_CONV_ROUTE_PLAIN;
}

template <int FX, int FW>
int launch_pair(const qs_mx_conv_transpose2d_args& a, const ConvTPlan& p, int route) {
    const int tiles_n = (int)((a.Cout + kMxgTile - 1) / kMxgTile);
    const int64_t grid = ((p.M + kMxgTile - 1) / kMxgTile) * tiles_n;
    // four consecutive n per lane in one store: every row of y must keep the store's alignment
    const int y_vec = a.Cout % 4 == 0 && (((uintptr_t)a.y) & (4 * dt_size(a.ydt) - 1)) == 0;
    MxctShape g;
    g.s.H = (int)a.H, g.s.W = (int)a.W, g.s.C = (int)a.C, g.s.nb = (int)((a.C + QS_MX_BLOCK - 1) / QS_MX_BLOCK);
    g.s.KH = a.KH, g.s.KW = a.KW, g.s.sh = a.stride_h, g.s.sw = a.stride_w, g.s.ph = a.pad_h, g.s.pw = a.pad_w, g.s.dh = a.dil_h, g.s.dw = a.dil_w;
    g.s.OW = (int)p.OW, g.s.OHW = p.OH * p.OW;
    g.mh = UINT32_MAX / (uint32_t)a.stride_h, g.mw = UINT32_MAX / (uint32_t)a.stride_w;
    hipStream_t s = (hipStream_t)a.stream;
    if (route == QS_MX_CONV_ROUTE_VEC)
        hipLaunchKernelGGL((mx_conv_t_kernel<FX, FW, true>), dim3((unsigned)grid), dim3(kMxgThreads), 0, s, a.x_codes, a.x_scales, a.w_codes,
                           a.w_scales, a.bias, a.y, a.ydt, p.M, a.Cout, g, tiles_n, y_vec);
    else
        hipLaunchKernelGGL((mx_conv_t_kernel<FX, FW, false>), dim3((unsigned)grid), dim3(kMxgThreads), 0, s, a.x_codes, a.x_scales, a.w_codes,
                           a.w_scales, a.bias, a.y, a.ydt, p.M, a.Cout, g, tiles_n, y_vec);
    return launch_status();
}

template <int FX>
int launch_x(const qs_mx_conv_transpose2d_args& a, const ConvTPlan& p, int route) {
    switch (a.w_format) {
        case QS_MX_FP8_E4M3: return launch_pair<FX, QS_MX_FP8_E4M3>(a, p, route);
        case QS_MX_FP8_E5M2: return launch_pair<FX, QS_MX_FP8_E5M2>(a, p, route);
        case QS_MX_FP6_E2M3: return launch_pair<FX, QS_MX_FP6_E2M3>(a, p, route);
        case QS_MX_FP6_E3M2: return launch_pair<FX, QS_MX_FP6_E3M2>(a, p, route);
        default: return launch_pair<FX, QS_MX_FP4_E2M1>(a, p, route);
    }
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
    ConvTPlan p;
    const int route = mx_conv_t_route(a, &p);
    if (route <= 0) return route;
    if (route == QS_MX_CONV_ROUTE_GEMM) {
        qs_mx_matmul_args m = {};
        m.struct_size = sizeof(m);
        m.a_format = a.x_format, m.b_format = a.w_format;
        m.a_codes = a.x_codes, m.a_scales = a.x_scales, m.b_codes = a.w_codes, m.b_scales = a.w_scales;
        m.bias = a.bias, m.y = a.y, m.ydt = a.ydt;
        m.M = p.M, m.N = a.Cout, m.K = a.C;
        m.stream = a.stream;
        return qs_mx_matmul_v(&m);
    }
    switch (a.x_format) {
        case QS_MX_FP8_E4M3: return launch_x<QS_MX_FP8_E4M3>(a, p, route);
        case QS_MX_FP8_E5M2: return launch_x<QS_MX_FP8_E5M2>(a, p, route);
        case QS_MX_FP6_E2M3: return launch_x<QS_MX_FP6_E2M3>(a, p, route);
        case QS_MX_FP6_E3M2: return launch_x<QS_MX_FP6_E3M2>(a, p, route);
        default: return launch_x<QS_MX_FP4_E2M1>(a, p, route);
    }
}

}  // extern "C"
