// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the batched, strided two-way MX quantizer (qs_mx_quant2.h,
// mx_quant2_batched_kernel): G0 x G1 slices [R, C] of x, each read once where it lies, leave as dense row pairs [G, R, C] and col pairs
// [G, C, R] -- slice by slice the bits of qs_mx_quant2_v -- from one launch.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"

namespace {

// the checks of qs_mx_quant2_batched_v, in qs_mx_quant2_v's order, and the kernel it launches for these operands: QS_MX_Q2_ROUTE_*, 0 for
// an empty tensor, QS_ERR_*
int mx_quant2_batched_route(const qs_mx_quant2_batched_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const Mxq2Pairs pairs = mxq2_pairs_by_pointer(a);
    if (!a.x || !pairs.ok) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0 || a.G0 < 0 || a.G1 < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0) return QS_ERR_ALIGN;
    if (a.G0 == 0 || a.G1 == 0 || a.R == 0 || a.C == 0) return 0;
    int64_t G, n;
    if (!mxq2_slices_ok(a, &G, &n) || !mxq2_grid_ok(a.R, a.C, G)) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    const bool vec = a.C % v == 0 && aligned16(a.x) && a.x_stride_r % v == 0 && a.x_stride_g0 % v == 0 && a.x_stride_g1 % v == 0 &&
                     (!pairs.col || (a.R % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_Q2_ROUTE_TILE_VEC : QS_MX_Q2_ROUTE_TILE_PLAIN;
}

template <bool SR>
int mx_quant2_batched_launch(const qs_mx_quant2_batched_args& a, int route) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    const Mxq2Launch l = mxq2_launch(a, a.row_codes != nullptr, a.col_codes != nullptr, a.R, a.C);
    const dim3 grid((unsigned)(a.G0 * a.G1 * l.tiles));
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        const int row_vec = mxq2_row_vec(l, XD == QS_F32 ? 4 : 8);             // (as qs_mx_quant2_v)
        if (route == QS_MX_Q2_ROUTE_TILE_VEC)
            hipLaunchKernelGGL((mx_quant2_batched_kernel<XD, true, SR>), grid, dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.x, a.G1,
                               a.x_stride_g0, a.x_stride_g1, a.x_stride_r, l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.R, a.C,
                               l.tiles, l.tiles_c, row_vec, sr);
        else
            hipLaunchKernelGGL((mx_quant2_batched_kernel<XD, false, SR>), grid, dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.x, a.G1,
                               a.x_stride_g0, a.x_stride_g1, a.x_stride_r, l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.R, a.C,
                               l.tiles, l.tiles_c, 0, sr);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_quant2_batched_route(const qs_mx_quant2_batched_args* args) {
    qs_mx_quant2_batched_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_quant2_batched_route(a);
}

int qs_mx_quant2_batched_v(const qs_mx_quant2_batched_args* args) {
    qs_mx_quant2_batched_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_quant2_batched_route(a);
    if (route <= 0) return route;
    return a.rounding == QS_MX_ROUND_STOCHASTIC ? mx_quant2_batched_launch<true>(a, route) : mx_quant2_batched_launch<false>(a, route);
}

}  // extern "C"
