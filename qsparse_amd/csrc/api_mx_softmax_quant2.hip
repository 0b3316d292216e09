// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two-way form of the MX softmax quantizer (qs_mx_softmax_train.h): the row
// statistics m and Z of s [G, T, S] in one launch, then the codes and E8M0 scales of p = softmax(s * scale (+ mask)) with blocks along
// S and -- stored transposed, when asked for -- with blocks along T in a second one.  p is never written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"
#include "qs_mx_softmax_train.h"

namespace {

// the checks of qs_mx_softmax_quant2_v and the kernels it launches for these operands: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor,
// QS_ERR_*
int mx_softmax_quant2_route(const qs_mx_softmax_quant2_args& a) {
    if (!a.s || !a.m || !a.Z || !mxq2_pairs_by_format(a, true).ok) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0) return QS_ERR_ARG;
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.sdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.s) & (dt_size(a.sdt) - 1)) != 0 || !aligned4(a.mask) || !aligned4(a.m) || !aligned4(a.Z)) return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0) return 0;
    if (a.G > INT64_MAX / a.T || a.G * a.T > INT64_MAX / a.S) return QS_ERR_ARG;
    if ((a.G * a.T + kMsxRows - 1) / kMsxRows > kMaxGrid) return QS_ERR_ARG;
    if (!mxq2_grid_ok(a.T, a.S, a.G)) return QS_ERR_ARG;
    const bool vec = a.S % QS_MX_BLOCK == 0 && aligned16(a.s) && aligned16(a.mask) && aligned8(a.row_codes);
    return vec ? QS_MX_SOFTMAX_ROUTE_VEC : QS_MX_SOFTMAX_ROUTE_PLAIN;
}

template <bool VEC>
int mx_softmax_quant2_enqueue(const qs_mx_softmax_quant2_args& a) {
    const bool col = a.col_format != -1;
    const int64_t R = a.G * a.T;
    const int64_t mask_rows = (a.mask && a.mask_slices != 1) ? R : a.T;
    const Mxq2Launch l = mxq2_launch(a, true, col, a.T, a.S);
    const int row_vec = VEC, col_vec = VEC && col && a.T % 16 == 0 && aligned16(l.col_codes);      // (VEC: row_codes is 8-byte aligned)
    hipStream_t st = (hipStream_t)a.stream;
    with_dtype(a.sdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        hipLaunchKernelGGL((mx_softmax_stats_kernel<XD, VEC>), dim3((unsigned)((R + kMsxRows - 1) / kMsxRows)), dim3(kMxq2Threads), 0, st,
                           a.s, a.mask, a.m, a.Z, R, a.T, a.S, mask_rows, a.scale, a.causal);
        hipLaunchKernelGGL((mx_softmax_quant2_kernel<XD, VEC>), dim3((unsigned)(a.G * l.tiles)), dim3(kMxq2Threads), 0, st, l.fr, l.fc, a.s,
                           a.mask, (const float*)a.m, (const float*)a.Z, l.row_codes, l.row_scales, l.col_codes, l.col_scales, a.T, a.S,
                           mask_rows, a.scale, a.causal, l.tiles, l.tiles_c, row_vec, col_vec);
        return 0;
    });
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_softmax_quant2_route(const qs_mx_softmax_quant2_args* args) {
    qs_mx_softmax_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_softmax_quant2_route(a);
}

int qs_mx_softmax_quant2_v(const qs_mx_softmax_quant2_args* args) {
    qs_mx_softmax_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_softmax_quant2_route(a);
    if (route <= 0) return route;
    return route == QS_MX_SOFTMAX_ROUTE_VEC ? mx_softmax_quant2_enqueue<true>(a) : mx_softmax_quant2_enqueue<false>(a);
}

}  // extern "C"
