// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), RMSNorm / LayerNorm in front of the MX quantizer (qs_mx_norm.h): the row
// statistics of x [R, C] in one launch, then the codes and E8M0 scales of y = norm(x) * w (+ b) with blocks along C and -- stored
// transposed, when asked for -- with blocks along R in a second one.  y is never written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_norm.h"

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// the checks of qs_mx_norm_quant_v and the kernels it launches for these operands: QS_MX_NORM_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_norm_route(const qs_mx_norm_quant_args& a) {
    const bool layer = a.mode == QS_MX_NORM_LAYER, col = a.col_format != -1;
    if (a.mode != QS_MX_NORM_RMS && !layer) return QS_ERR_ARG;
    if (!a.x || !a.row_codes || !a.row_scales || !a.rstd || (layer && !a.mean)) return QS_ERR_ARG;
    if (!mx_format_ok(a.row_format) || (col && (!mx_format_ok(a.col_format) || !a.col_codes || !a.col_scales))) return QS_ERR_ARG;
    if (!(a.eps >= 0.0f) || a.eps > 3.0e38f) return QS_ERR_ARG;                  // (also refuses a NaN)
    if (a.R < 0 || a.C < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0 || !aligned4(a.weight) || !aligned4(a.bias) || !aligned4(a.rstd) ||
        (layer && !aligned4(a.mean)))
        return QS_ERR_ALIGN;
    if (a.R == 0 || a.C == 0) return 0;
    if (a.R > INT64_MAX / a.C) return QS_ERR_ARG;
    const int64_t tiles = ((a.R + kMxq2Rows - 1) / kMxq2Rows) * ((a.C + kMxq2Cols - 1) / kMxq2Cols);
    if ((a.C + kMxq2Cols - 1) / kMxq2Cols > kMaxGrid || tiles > kMaxGrid) return QS_ERR_ARG;
    const bool vec = a.C % QS_MX_BLOCK == 0 && aligned16(a.x) && aligned16(a.weight) && aligned16(a.bias);
    return vec ? QS_MX_NORM_ROUTE_VEC : QS_MX_NORM_ROUTE_PLAIN;
}

int mx_norm_launch(const qs_mx_norm_quant_args& a, int route) {
    const bool layer = a.mode == QS_MX_NORM_LAYER, col = a.col_format != -1;
    // a col pair that is not asked for keeps a valid descriptor the kernel never reads, and null pointers whatever the caller left there
    const MxFormat fr = mx_format(a.row_format), fc = mx_format(col ? a.col_format : 0);
    uint8_t *cc = col ? a.col_codes : nullptr, *cs = col ? a.col_scales : nullptr;
    float* mean = layer ? a.mean : nullptr;
    const int tiles_c = (int)((a.C + kMxq2Cols - 1) / kMxq2Cols);
    const int64_t grid = ((a.R + kMxq2Rows - 1) / kMxq2Rows) * tiles_c;
    const int64_t sgrid = (a.R + kMxnStatRows - 1) / kMxnStatRows;
    const int row_vec = aligned4(a.row_codes), col_vec = col && a.R % 16 == 0 && aligned16(cc);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        if (route == QS_MX_NORM_ROUTE_VEC) {
            hipLaunchKernelGGL((mx_norm_stats_kernel<XD, true>), dim3((unsigned)sgrid), dim3(kMxq2Threads), 0, s, a.x, a.rstd, mean, a.R,
                               a.C, a.eps);
            hipLaunchKernelGGL((mx_norm_apply_kernel<XD, true>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.weight,
                               a.bias, (const float*)a.rstd, (const float*)mean, a.row_codes, a.row_scales, cc, cs, a.R, a.C, tiles_c,
                               row_vec, col_vec);
        } else {
            hipLaunchKernelGGL((mx_norm_stats_kernel<XD, false>), dim3((unsigned)sgrid), dim3(kMxq2Threads), 0, s, a.x, a.rstd, mean, a.R,
                               a.C, a.eps);
            hipLaunchKernelGGL((mx_norm_apply_kernel<XD, false>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.weight,
                               a.bias, (const float*)a.rstd, (const float*)mean, a.row_codes, a.row_scales, cc, cs, a.R, a.C, tiles_c, 0,
                               0);
        }
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_norm_quant_route(const qs_mx_norm_quant_args* args) {
    qs_mx_norm_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_norm_route(a);
}

int qs_mx_norm_quant_v(const qs_mx_norm_quant_args* args) {
    qs_mx_norm_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_norm_route(a);
    if (route <= 0) return route;
    return mx_norm_launch(a, route);
}

}  // extern "C"
