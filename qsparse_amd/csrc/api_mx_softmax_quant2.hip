// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the two-way form of the MX softmax quantizer (qs_mx_softmax_train.h): the row
// statistics m and Z of s [G, T, S] in one launch, then the codes and E8M0 scales of p = softmax(s * scale (+ mask)) with blocks along
// S and -- stored transposed, when asked for -- with blocks along T in a second one.  p is never written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_softmax_train.h"

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// the checks of qs_mx_softmax_quant2_v and the kernels it launches for these operands: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor,
// QS_ERR_*
int mx_softmax_quant2_route(const qs_mx_softmax_quant2_args& a) {
    const bool col = a.col_format != -1;
    if (!a.s || !a.row_codes || !a.row_scales || !a.m || !a.Z) return QS_ERR_ARG;
    if (!mx_format_ok(a.row_format) || (col && (!mx_format_ok(a.col_format) || !a.col_codes || !a.col_scales))) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0) return QS_ERR_ARG;
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.sdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.s) & (dt_size(a.sdt) - 1)) != 0 || !aligned4(a.mask) || !aligned4(a.m) || !aligned4(a.Z)) return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0) return 0;
    if (a.G > INT64_MAX / a.T || a.G * a.T > INT64_MAX / a.S) return QS_ERR_ARG;
    if ((a.G * a.T + kMsxRows - 1) / kMsxRows > kMaxGrid) return QS_ERR_ARG;
    const int64_t tiles_c = (a.S + kMxq2Cols - 1) / kMxq2Cols, tiles_r = (a.T + kMxq2Rows - 1) / kMxq2Rows;
    if (tiles_c > kMaxGrid || tiles_r > kMaxGrid / tiles_c || a.G > kMaxGrid / (tiles_r * tiles_c)) return QS_ERR_ARG;
    const bool vec = a.S % QS_MX_BLOCK == 0 && aligned16(a.s) && aligned16(a.mask) && aligned8(a.row_codes);
    return vec ? QS_MX_SOFTMAX_ROUTE_VEC : QS_MX_SOFTMAX_ROUTE_PLAIN;
}

template <bool VEC>
int mx_softmax_quant2_enqueue(const qs_mx_softmax_quant2_args& a) {
    const bool col = a.col_format != -1;
    const int64_t R = a.G * a.T;
    const int64_t mask_rows = (a.mask && a.mask_slices != 1) ? R : a.T;
    // a col pair that is not asked for keeps a valid descriptor the kernel never reads, and null pointers whatever the caller left there
    const MxFormat fr = mx_format(a.row_format), fc = mx_format(col ? a.col_format : 0);
    uint8_t *cc = col ? a.col_codes : nullptr, *cs = col ? a.col_scales : nullptr;
    const int tiles_c = (int)((a.S + kMxq2Cols - 1) / kMxq2Cols);
    const int tiles = (int)(((a.T + kMxq2Rows - 1) / kMxq2Rows) * tiles_c);
    const int row_vec = VEC, col_vec = VEC && col && a.T % 16 == 0 && aligned16(cc);      // (VEC: row_codes is 8-byte aligned)
    hipStream_t st = (hipStream_t)a.stream;
    with_dtype(a.sdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        hipLaunchKernelGGL((mx_softmax_stats_kernel<XD, VEC>), dim3((unsigned)((R + kMsxRows - 1) / kMsxRows)), dim3(kMxq2Threads), 0, st,
                           a.s, a.mask, a.m, a.Z, R, a.T, a.S, mask_rows, a.scale, a.causal);
        hipLaunchKernelGGL((mx_softmax_quant2_kernel<XD, VEC>), dim3((unsigned)(a.G * tiles)), dim3(kMxq2Threads), 0, st, fr, fc, a.s,
                           a.mask, (const float*)a.m, (const float*)a.Z, a.row_codes, a.row_scales, cc, cs, a.T, a.S, mask_rows, a.scale,
                           a.causal, tiles, tiles_c, row_vec, col_vec);
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
