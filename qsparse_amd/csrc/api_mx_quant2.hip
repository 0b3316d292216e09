// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two-way, codes-only MX quantizer (qs_mx_quant2.h): one read of x [R, C],
// codes and E8M0 scales with blocks along C and -- stored transposed -- with blocks along R, rounded to nearest-even or stochastically
// (the descriptor's `rounding`: the kernel instantiated with SR = true).
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"

namespace {

// the checks of qs_mx_quant2_v and the kernel it launches for these operands: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_quant2_route(const qs_mx_quant2_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const Mxq2Pairs pairs = mxq2_pairs_by_pointer(a);
    if (!a.x || !pairs.ok) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0) return QS_ERR_ALIGN;
    if (a.R == 0 || a.C == 0) return 0;
    if (a.R > INT64_MAX / a.C || !mxq2_grid_ok(a.R, a.C)) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    const bool vec = a.C % v == 0 && aligned16(a.x) && (!pairs.col || (a.R % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_Q2_ROUTE_TILE_VEC : QS_MX_Q2_ROUTE_TILE_PLAIN;
}

template <bool SR>
int mx_quant2_launch(const qs_mx_quant2_args& a, int route) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    const Mxq2Launch l = mxq2_launch(a, a.row_codes != nullptr, a.col_codes != nullptr, a.R, a.C);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        // a lane stores 8 (two-byte inputs) or 4 (float32) row codes at once
        const int row_vec = mxq2_row_vec(l, XD == QS_F32 ? 4 : 8);
        if (route == QS_MX_Q2_ROUTE_TILE_VEC)
            hipLaunchKernelGGL((mx_quant2_kernel<XD, true, SR>), dim3((unsigned)l.tiles), dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.x,
                               l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.R, a.C, l.tiles_c, row_vec, sr);
        else
            hipLaunchKernelGGL((mx_quant2_kernel<XD, false, SR>), dim3((unsigned)l.tiles), dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.x,
                               l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.R, a.C, l.tiles_c, 0, sr);
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
