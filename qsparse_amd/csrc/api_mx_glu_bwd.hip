// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two-way MX quantizer with the GLU derivative in front (qs_mx_glu_bwd.h): one
// read of dh [T, H] and of the interleaved pre-activations v [T, 2 H], then the codes and E8M0 scales of dv [T, 2 H] with blocks along
// 2 H and -- stored transposed -- with blocks along T, rounded to nearest-even or stochastically.  dv is never written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"
#include "qs_mx_glu_bwd.h"

namespace {

// the checks of qs_mx_glu_bwd_quant2_v and the kernel it launches for these operands: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_glu_bwd_route(const qs_mx_glu_bwd_quant2_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const Mxq2Pairs pairs = mxq2_pairs_by_format(a);
    if (!a.dh || !a.v || !pairs.ok) return QS_ERR_ARG;
    if (a.T < 0 || a.H < 0 || a.H % QS_MX_BLOCK != 0 || a.H > INT64_MAX / 2) return QS_ERR_ARG;
    if (a.act != QS_MX_GLU_RELU && a.act != QS_MX_GLU_SILU && a.act != QS_MX_GLU_GELU) return QS_ERR_ARG;
    if (!dt_ok(a.dhdt) || !dt_ok(a.vdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.dh) & (dt_size(a.dhdt) - 1)) != 0 || (((uintptr_t)a.v) & (dt_size(a.vdt) - 1)) != 0) return QS_ERR_ALIGN;
    if (a.T == 0 || a.H == 0) return 0;
    const int64_t C = 2 * a.H;
    if (a.T > INT64_MAX / C || !mxq2_grid_ok(a.T, C)) return QS_ERR_ARG;
    const bool vec = aligned16(a.dh) && aligned16(a.v) && (!pairs.col || (a.T % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_Q2_ROUTE_TILE_VEC : QS_MX_Q2_ROUTE_TILE_PLAIN;
}

template <bool SR>
int mx_glu_bwd_launch(const qs_mx_glu_bwd_quant2_args& a, int route) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    const Mxq2Launch l = mxq2_launch(a, a.row_format != -1, a.col_format != -1, a.T, 2 * a.H);
    const dim3 grid((unsigned)l.tiles);
    const int row_vec = mxq2_row_vec(l, 4);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.dhdt, [&](auto D) {
        return with_dtype(a.vdt, [&](auto V) {
            constexpr int DD = decltype(D)::value, VD = decltype(V)::value;
            if (route == QS_MX_Q2_ROUTE_TILE_VEC)
                hipLaunchKernelGGL((mx_glu_bwd_quant2_kernel<DD, VD, true, SR>), grid, dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.dh, a.v,
                                   (int)a.act, l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.T, a.H, l.tiles_c, row_vec, sr);
            else
                hipLaunchKernelGGL((mx_glu_bwd_quant2_kernel<DD, VD, false, SR>), grid, dim3(kMxq2Threads), 0, s, l.fr, l.fc, a.dh, a.v,
                                   (int)a.act, l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.T, a.H, l.tiles_c, 0, sr);
            return launch_status();
        });
    });
}

}  // namespace

extern "C" {

int qs_mx_glu_bwd_quant2_route(const qs_mx_glu_bwd_quant2_args* args) {
    qs_mx_glu_bwd_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_glu_bwd_route(a);
}

int qs_mx_glu_bwd_quant2_v(const qs_mx_glu_bwd_quant2_args* args) {
    qs_mx_glu_bwd_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_glu_bwd_route(a);
    if (route <= 0) return route;
    return a.rounding == QS_MX_ROUND_STOCHASTIC ? mx_glu_bwd_launch<true>(a, route) : mx_glu_bwd_launch<false>(a, route);
}

}  // extern "C"
