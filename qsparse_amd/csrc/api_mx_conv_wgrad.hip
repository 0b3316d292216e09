// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the weight gradient of the 2-d convolution on MX codes (qs_mx_conv_wgrad.h):
// the batch-blocked implicit GEMM through the block-scaled MFMA, all 5 x 5 pairs of element formats, split along K' into slices whose
// partial sums mx_gemm_reduce_kernel (qs_mx_gemm_splitk.h) adds in order.  A translation unit of its own: its 50 instantiations
// compile next to those of the other products, not after them.
// Host side: argument checks, the slicing and the automatic slice count, route, launch configuration.  No allocation, no
// synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_conv_wgrad.h"
#include "qs_mx_gemm_splitk.h"

namespace {

// the most slices the automatic rule asks for.  3f's 16 suits a linear layer's wgrad (tens of tiles); this product has as few as 5
// tiles and thousands of steps, and 512 work-groups then need about 100 slices (measured: DESIGN.md 3h)
constexpr int64_t kWgradSplitMax = 128;

struct WgradPlan {
    int64_t N, steps;     // KH KW C; K-steps of the whole product
    SplitPlan split;
};

// the checks of qs_mx_conv2d_wgrad_v and the route it takes for these operands: QS_MX_CONV_ROUTE_VEC / _PLAIN, 0 for an empty
// problem, QS_ERR_*
int wgrad_route(const qs_mx_conv2d_wgrad_args& a, WgradPlan* plan) {
    if (!a.dyt_codes || !a.dyt_scales || !a.xt_codes || !a.xt_scales || !a.dw) return QS_ERR_ARG;
    if (!mx_format_ok(a.dy_format) || !mx_format_ok(a.x_format)) return QS_ERR_ARG;
    if (a.B < 1 || a.Cout < 0 || a.C < 0 || a.H < 1 || a.W < 1 || a.KH < 1 || a.KW < 1 || a.split_k < 0) return QS_ERR_ARG;
    if (a.stride_h < 1 || a.stride_w < 1 || a.dil_h < 1 || a.dil_w < 1 || a.pad_h < 0 || a.pad_w < 0) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.dw) & (dt_size(a.ydt) - 1)) != 0) return QS_ERR_ALIGN;
    // the kernel keeps coordinates inside one image, b, c and n in 32 bits (addresses: 64)
    if (a.B > INT32_MAX - QS_MX_BLOCK || a.C > INT32_MAX || a.Cout > INT32_MAX) return QS_ERR_ARG;
    const int64_t HP = a.H + 2 * (int64_t)a.pad_h, WP = a.W + 2 * (int64_t)a.pad_w;
    if (a.H > INT32_MAX || a.W > INT32_MAX || HP > INT32_MAX || WP > INT32_MAX) return QS_ERR_ARG;
    const int64_t EH = (int64_t)a.dil_h * (a.KH - 1) + 1, EW = (int64_t)a.dil_w * (a.KW - 1) + 1;      // extent of the dilated kernel
    if (EH > HP || EW > WP) return QS_ERR_ARG;                                                        // OH < 1 or OW < 1
    if (a.OH != (HP - EH) / a.stride_h + 1 || a.OW != (WP - EW) / a.stride_w + 1) return QS_ERR_ARG;
    const int64_t taps = (int64_t)a.KH * a.KW, Bp = (a.B + QS_MX_BLOCK - 1) / QS_MX_BLOCK * QS_MX_BLOCK;
    if (taps > INT32_MAX) return QS_ERR_ARG;
    if (a.Cout == 0 || a.C == 0) return 0;
    // every product of extents in 64 bits: the operands, the result, the gathered operands
    const int64_t N = taps * a.C, pixels = a.OH * a.OW;                   // each a product of two values below 2^31
    if (pixels > INT64_MAX / Bp) return QS_ERR_ARG;
    const int64_t Kp = pixels * Bp;
    if (a.Cout > INT64_MAX / Kp || N > INT64_MAX / Kp || a.Cout > INT64_MAX / N) return QS_ERR_ARG;
    if (a.H * a.W > INT64_MAX / a.C || a.H * a.W * a.C > INT64_MAX / Bp) return QS_ERR_ARG;
    const int64_t tiles = mx_tiles(a.Cout) * mx_tiles(N);
    if (tiles > kMaxGrid) return QS_ERR_ARG;
    SplitPlan sp;
    const int st = split_plan(a.Cout, N, Kp, a.split_k, kWgradSplitMax, &sp);
    if (st != QS_OK) return st;
    if (sp.slices > 1) {
        const int ws = split_workspace_status(sp, a.workspace, a.workspace_bytes, tiles);
        if (ws != QS_OK) return ws;
    }
    if (plan) *plan = WgradPlan{N, cdiv(Kp, kMxgK), sp};
    return (a.B % 16 == 0 && aligned16(a.dyt_codes) && aligned16(a.xt_codes)) ? QS_MX_CONV_ROUTE_VEC : QS_MX_CONV_ROUTE_PLAIN;
}

}  // namespace

extern "C" {

int qs_mx_conv2d_wgrad_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int32_t* slices, uint64_t* workspace_bytes) {
    return split_plan_out(M, N, K, split_k, kWgradSplitMax, slices, workspace_bytes);
}

int qs_mx_conv2d_wgrad_route(const qs_mx_conv2d_wgrad_args* args) {
    qs_mx_conv2d_wgrad_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return wgrad_route(a, nullptr);
}

int qs_mx_conv2d_wgrad_v(const qs_mx_conv2d_wgrad_args* args) {
    qs_mx_conv2d_wgrad_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    WgradPlan p;
    const int route = wgrad_route(a, &p);
    if (route <= 0) return route;
    const int64_t M = a.Cout, N = p.N;
    const int tiles_n = (int)mx_tiles(N), tiles = (int)mx_tiles(M) * tiles_n, slices = p.split.slices;
    const int64_t grid = (int64_t)tiles * slices;
    MxwShape g;
    g.H = (int)a.H, g.W = (int)a.W, g.C = (int)a.C, g.B = (int)a.B, g.nb = (int)((a.B + QS_MX_BLOCK - 1) / QS_MX_BLOCK);
    g.OH = (int)a.OH, g.OW = (int)a.OW, g.Cout = (int)a.Cout;
    g.KH = a.KH, g.KW = a.KW, g.sh = a.stride_h, g.sw = a.stride_w, g.ph = a.pad_h, g.pw = a.pad_w, g.dh = a.dil_h, g.dw = a.dil_w;
    const int ws_vec = N % 4 == 0;                 // every row of every slice then keeps the workspace's 16-byte alignment
    const int y_vec = mx_y_vec(a.dw, a.ydt, N);
    float* ws = slices > 1 ? (float*)a.workspace : nullptr;
    hipStream_t s = (hipStream_t)a.stream;
    const int st = mx_dispatch(a.dy_format, a.x_format, route == QS_MX_CONV_ROUTE_VEC, [&](auto FG, auto FX, auto VEC) {
        hipLaunchKernelGGL((mx_conv_wgrad_kernel<decltype(FG)::value, decltype(FX)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, s, a.dyt_codes, a.dyt_scales, a.xt_codes, a.xt_scales, ws, a.dw, a.ydt, M, N, g, tiles_n,
                           tiles, p.split.per, p.steps, slices, y_vec, ws_vec);
        return launch_status();
    });
    if (st != 0 || slices == 1) return st;
    return mx_launch_reduce(ws, nullptr, a.dw, a.ydt, M, N, slices, s);
}

}  // extern "C"
