// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the softmax backward in front of the two-way MX quantizer
// (qs_mx_softmax_train.h): the row sums D of p * dp in one launch, then the codes and E8M0 scales of ds = (p * (dp - D)) * scale with
// blocks along S and -- stored transposed -- with blocks along T in a second one, rounded to nearest-even or stochastically.  p is
// formed again from s, m and Z; neither p nor ds is ever written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"
#include "qs_mx_softmax_train.h"

namespace {

// the checks of qs_mx_softmax_bwd_quant_v and the kernels it launches for these operands: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty
// tensor, QS_ERR_*
int mx_softmax_bwd_route(const qs_mx_softmax_bwd_quant_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const Mxq2Pairs pairs = mxq2_pairs_by_format(a);
    if (!a.dp || !a.s || !a.m || !a.Z || !a.D || !pairs.ok) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0) return QS_ERR_ARG;
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.sdt) || !dt_ok(a.ddt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.s) & (dt_size(a.sdt) - 1)) != 0 || (((uintptr_t)a.dp) & (dt_size(a.ddt) - 1)) != 0 || !aligned4(a.mask) ||
        !aligned4(a.m) || !aligned4(a.Z) || !aligned4(a.D))
        return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0) return 0;
    if (a.G > INT64_MAX / a.T || a.G * a.T > INT64_MAX / a.S) return QS_ERR_ARG;
    if ((a.G * a.T + kMsxRows - 1) / kMsxRows > kMaxGrid) return QS_ERR_ARG;
    if (!mxq2_grid_ok(a.T, a.S, a.G)) return QS_ERR_ARG;
    const bool vec = a.S % QS_MX_BLOCK == 0 && aligned16(a.s) && aligned16(a.dp) && aligned16(a.mask) &&
                     (!pairs.col || (a.T % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_SOFTMAX_ROUTE_VEC : QS_MX_SOFTMAX_ROUTE_PLAIN;
}

template <bool VEC, bool SR>
int mx_softmax_bwd_enqueue(const qs_mx_softmax_bwd_quant_args& a) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    const int64_t R = a.G * a.T;
    const int64_t mask_rows = (a.mask && a.mask_slices != 1) ? R : a.T;
    const Mxq2Launch l = mxq2_launch(a, a.row_format != -1, a.col_format != -1, a.T, a.S);
    const int row_vec = VEC && mxq2_row_vec(l, 4);              // (S % 32 == 0 keeps it in every row of every slice)
    hipStream_t st = (hipStream_t)a.stream;
    return with_dtype(a.sdt, [&](auto X) {
        return with_dtype(a.ddt, [&](auto Dt) {
            constexpr int XD = decltype(X)::value, DD = decltype(Dt)::value;
            hipLaunchKernelGGL((mx_softmax_bwd_rows_kernel<XD, DD, VEC>), dim3((unsigned)((R + kMsxRows - 1) / kMsxRows)),
                               dim3(kMxq2Threads), 0, st, a.dp, a.s, a.mask, a.m, a.Z, a.D, R, a.T, a.S, mask_rows, a.scale, a.causal);
            hipLaunchKernelGGL((mx_softmax_bwd_quant2_kernel<XD, DD, VEC, SR>), dim3((unsigned)(a.G * l.tiles)), dim3(kMxq2Threads), 0, st,
                               l.fr, l.fc, a.dp, a.s, a.mask, a.m, a.Z, (const float*)a.D, l.row_codes, l.row_scales, l.col_codes,
                               l.col_scales, a.T, a.S, mask_rows, a.scale, a.causal, l.tiles, l.tiles_c, row_vec, sr);
            return launch_status();
        });
    });
}

}  // namespace

extern "C" {

int qs_mx_softmax_bwd_quant_route(const qs_mx_softmax_bwd_quant_args* args) {
    qs_mx_softmax_bwd_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_softmax_bwd_route(a);
}

int qs_mx_softmax_bwd_quant_v(const qs_mx_softmax_bwd_quant_args* args) {
    qs_mx_softmax_bwd_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_softmax_bwd_route(a);
    if (route <= 0) return route;
    const bool sr = a.rounding == QS_MX_ROUND_STOCHASTIC;
    if (route == QS_MX_SOFTMAX_ROUTE_VEC) return sr ? mx_softmax_bwd_enqueue<true, true>(a) : mx_softmax_bwd_enqueue<true, false>(a);
    return sr ? mx_softmax_bwd_enqueue<false, true>(a) : mx_softmax_bwd_enqueue<false, false>(a);
}

}  // extern "C"
