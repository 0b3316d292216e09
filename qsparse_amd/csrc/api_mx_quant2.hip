// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two-way, codes-only MX quantizer (qs_mx_quant2.h): one read of x [R, C],
// codes and E8M0 scales with blocks along C and -- stored transposed -- with blocks along R, rounded to nearest-even or stochastically
// (the descriptor's `rounding`: the kernel instantiated with SR = true).
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_quant2.h"

namespace {

// the checks of qs_mx_quant2_v and the kernel it launches for these operands: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_quant2_route(const qs_mx_quant2_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const bool row = a.row_codes && a.row_scales, col = a.col_codes && a.col_scales;
    if (!a.x || (!row && !col)) return QS_ERR_ARG;
    if ((!a.row_codes) != (!a.row_scales) || (!a.col_codes) != (!a.col_scales)) return QS_ERR_ARG;      // half a pair
    if ((row && !mx_format_ok(a.row_format)) || (col && !mx_format_ok(a.col_format))) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0) return QS_ERR_ALIGN;
    if (a.R == 0 || a.C == 0) return 0;
    if (a.R > INT64_MAX / a.C) return QS_ERR_ARG;
    const int64_t tiles = ((a.R + kMxq2Rows - 1) / kMxq2Rows) * ((a.C + kMxq2Cols - 1) / kMxq2Cols);
    if ((a.C + kMxq2Cols - 1) / kMxq2Cols > kMaxGrid || tiles > kMaxGrid) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    const bool vec = a.C % v == 0 && aligned16(a.x) && (!col || (a.R % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_Q2_ROUTE_TILE_VEC : QS_MX_Q2_ROUTE_TILE_PLAIN;
}

template <bool SR>
int mx_quant2_launch(const qs_mx_quant2_args& a, int route) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    // a pair that is not asked for keeps a valid descriptor the kernel never reads
    const MxFormat fr = mx_format(a.row_codes ? a.row_format : 0), fc = mx_format(a.col_codes ? a.col_format : 0);
    const int tiles_c = (int)((a.C + kMxq2Cols - 1) / kMxq2Cols);
    const int64_t grid = ((a.R + kMxq2Rows - 1) / kMxq2Rows) * tiles_c;
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        // a lane stores 8 (two-byte inputs) or 4 (float32) row codes at once where row_codes keeps that alignment in every row
        const int row_vec = a.row_codes && (((uintptr_t)a.row_codes) & (XD == QS_F32 ? 3u : 7u)) == 0;
        if (route == QS_MX_Q2_ROUTE_TILE_VEC)
            hipLaunchKernelGGL((mx_quant2_kernel<XD, true, SR>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.row_codes,
                               a.row_scales, a.col_codes, a.col_scales, a.R, a.C, tiles_c, row_vec, sr);
        else
            hipLaunchKernelGGL((mx_quant2_kernel<XD, false, SR>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.row_codes,
                               a.row_scales, a.col_codes, a.col_scales, a.R, a.C, tiles_c, 0, sr);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_quant2_route(const qs_mx_quant2_args* args) {
    qs_mx_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_quant2_route(a);
}

int qs_mx_quant2_v(const qs_mx_quant2_args* args) {
    qs_mx_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_quant2_route(a);
    if (route <= 0) return route;
    return a.rounding == QS_MX_ROUND_STOCHASTIC ? mx_quant2_launch<true>(a, route) : mx_quant2_launch<false>(a, route);
}

// the v27 names of the two entry points above
int qs_mx_quant2_sr_route(const qs_mx_quant2_sr_args* args) { return qs_mx_quant2_route(args); }
int qs_mx_quant2_sr_v(const qs_mx_quant2_sr_args* args) { return qs_mx_quant2_v(args); }

}  // extern "C"
