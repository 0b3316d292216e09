// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the weight gradient of the grouped matrix product on MX codes
// (qs_mx_gmm_wgrad.h): dw[e] = dy_e^T x_e for E groups of tokens whose boundaries lie in device memory, the contraction along the
// ragged axis, through the block-scaled MFMA, all 5 x 5 pairs of element formats, one launch.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation, no read of offs.
#include "qs_mx_gmm_wgrad.h"

namespace {

// the checks of qs_mx_grouped_wgrad_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty result,
// QS_ERR_*
int mx_gmm_wgrad_route(const qs_mx_grouped_wgrad_args& a) {
    if (!a.dw || !a.offs) return QS_ERR_ARG;
    if (!mx_format_ok(a.g_format) || !mx_format_ok(a.x_format)) return QS_ERR_ARG;
    if (a.T < 0 || a.N < 0 || a.K < 0 || a.E < 0 || a.E > QS_MX_GROUPED_MAX_GROUPS) return QS_ERR_ARG;
    if (a.T > 0 && (!a.gt_codes || !a.gt_scales || !a.xt_codes || !a.xt_scales)) return QS_ERR_ARG;    // (no token: nothing to read)
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.dw) & (dt_size(a.ydt) - 1)) != 0 || (((uintptr_t)a.offs) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.E == 0 || a.N == 0 || a.K == 0) return 0;
    if (a.N > INT64_MAX / a.K || a.E > INT64_MAX / (a.N * a.K)) return QS_ERR_ARG;
    if (a.T > 0 && (a.N > INT64_MAX / a.T || a.K > INT64_MAX / a.T)) return QS_ERR_ARG;
    if (a.E > kMaxGrid / mx_tiles(a.N) || a.E * mx_tiles(a.N) > kMaxGrid / mx_tiles(a.K)) return QS_ERR_ARG;
    // T % 16 == 0 makes every row of gt and xt a multiple of 16 bytes, so aligned bases align every piece
    return (a.T % 16 == 0 && aligned16(a.gt_codes) && aligned16(a.xt_codes)) ? QS_MX_GEMM_ROUTE_VEC : QS_MX_GEMM_ROUTE_PLAIN;
}

}  // namespace

extern "C" {

int qs_mx_grouped_wgrad_route(const qs_mx_grouped_wgrad_args* args) {
    qs_mx_grouped_wgrad_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gmm_wgrad_route(a);
}

int qs_mx_grouped_wgrad_v(const qs_mx_grouped_wgrad_args* args) {
    qs_mx_grouped_wgrad_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gmm_wgrad_route(a);
    if (route <= 0) return route;
    const int tiles_m = (int)mx_tiles(a.N), tiles_n = (int)mx_tiles(a.K);
    const int64_t grid = a.E * tiles_m * tiles_n;
    return mx_dispatch(a.g_format, a.x_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FG, auto FX, auto VEC) {
        hipLaunchKernelGGL((mx_gmm_wgrad_kernel<decltype(FG)::value, decltype(FX)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.gt_codes, a.gt_scales, a.xt_codes, a.xt_scales, a.offs, a.dw, a.ydt,
                           a.T, (int)a.E, a.N, a.K, tiles_m, tiles_n, mx_y_vec(a.dw, a.ydt, a.K));
        return launch_status();
    });
}

}  // extern "C"
