// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the softmax backward in front of the two-way MX quantizer
// (qs_mx_softmax_train.h): the row sums D of p * dp in one launch, then the codes and E8M0 scales of ds = (p * (dp - D)) * scale with
// blocks along S and -- stored transposed -- with blocks along T in a second one, rounded to nearest-even or stochastically.  p is
// formed again from s, m and Z; neither p nor ds is ever written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_softmax_train.h"

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3u) == 0; }

// the checks of qs_mx_softmax_bwd_quant_v and the kernels it launches for these operands: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty
// tensor, QS_ERR_*
int mx_softmax_bwd_route(const qs_mx_softmax_bwd_quant_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    const bool row = a.row_format != -1, col = a.col_format != -1;
    if (!a.dp || !a.s || !a.m || !a.Z || !a.D || (!row && !col)) return QS_ERR_ARG;
    if ((row && (!mx_format_ok(a.row_format) || !a.row_codes || !a.row_scales)) ||
        (col && (!mx_format_ok(a.col_format) || !a.col_codes || !a.col_scales)))
        return QS_ERR_ARG;
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
    const int64_t tiles_c = (a.S + kMxq2Cols - 1) / kMxq2Cols, tiles_r = (a.T + kMxq2Rows - 1) / kMxq2Rows;
    if (tiles_c > kMaxGrid || tiles_r > kMaxGrid / tiles_c || a.G > kMaxGrid / (tiles_r * tiles_c)) return QS_ERR_ARG;
    const bool vec = a.S % QS_MX_BLOCK == 0 && aligned16(a.s) && aligned16(a.dp) && aligned16(a.mask) &&
                     (!col || (a.T % 16 == 0 && aligned16(a.col_codes)));
    return vec ? QS_MX_SOFTMAX_ROUTE_VEC : QS_MX_SOFTMAX_ROUTE_PLAIN;
}

template <bool VEC, bool SR>
int mx_softmax_bwd_enqueue(const qs_mx_softmax_bwd_quant_args& a) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, 0u} : MxSr{};      // (the kernel sets the stream per phase)
    const bool row = a.row_format != -1, col = a.col_format != -1;
    const int64_t R = a.G * a.T;
    const int64_t mask_rows = (a.mask && a.mask_slices != 1) ? R : a.T;
    // a pair that is not asked for keeps a valid descriptor the kernel never reads, and null pointers whatever the caller left there
    const MxFormat fr = mx_format(row ? a.row_format : 0), fc = mx_format(col ? a.col_format : 0);
    uint8_t *rc = row ? a.row_codes : nullptr, *rs = row ? a.row_scales : nullptr;
    uint8_t *cc = col ? a.col_codes : nullptr, *cs = col ? a.col_scales : nullptr;
    const int tiles_c = (int)((a.S + kMxq2Cols - 1) / kMxq2Cols);
    const int tiles = (int)(((a.T + kMxq2Rows - 1) / kMxq2Rows) * tiles_c);
    const int row_vec = VEC && rc && aligned4(rc);              // (S % 32 == 0 keeps it in every row of every slice)
    hipStream_t st = (hipStream_t)a.stream;
    return with_dtype(a.sdt, [&](auto X) {
        return with_dtype(a.ddt, [&](auto Dt) {
            constexpr int XD = decltype(X)::value, DD = decltype(Dt)::value;
            hipLaunchKernelGGL((mx_softmax_bwd_rows_kernel<XD, DD, VEC>), dim3((unsigned)((R + kMsxRows - 1) / kMsxRows)),
                               dim3(kMxq2Threads), 0, st, a.dp, a.s, a.mask, a.m, a.Z, a.D, R, a.T, a.S, mask_rows, a.scale, a.causal);
            hipLaunchKernelGGL((mx_softmax_bwd_quant2_kernel<XD, DD, VEC, SR>), dim3((unsigned)(a.G * tiles)), dim3(kMxq2Threads), 0, st, fr,
                               fc, a.dp, a.s, a.mask, a.m, a.Z, (const float*)a.D, rc, rs, cc, cs, a.T, a.S, mask_rows, a.scale, a.causal,
                               tiles, tiles_c, row_vec, sr);
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
