// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), scale, mask and softmax in front of the MX quantizer (qs_mx_softmax.h): the
// codes and E8M0 scales of p = softmax(s * scale (+ mask)) over the last axis of s [G, T, S], blocks along S, in one launch.  Neither
// the masked scores nor p is ever written.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_softmax.h"

namespace {

// the checks of qs_mx_softmax_quant_v and the kernel it launches for these operands: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor,
// QS_ERR_*
int mx_softmax_route(const qs_mx_softmax_quant_args& a) {
    if (!a.s || !a.codes || !a.scales) return QS_ERR_ARG;
    if (!mx_format_ok(a.format) || (a.causal != 0 && a.causal != 1)) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0) return QS_ERR_ARG;
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.sdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.s) & (dt_size(a.sdt) - 1)) != 0 || (((uintptr_t)a.mask) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0) return 0;
    if (a.G > INT64_MAX / a.T || a.G * a.T > INT64_MAX / a.S) return QS_ERR_ARG;
    if ((a.G * a.T + kMsxRows - 1) / kMsxRows > kMaxGrid) return QS_ERR_ARG;
    const bool vec = a.S % QS_MX_BLOCK == 0 && aligned16(a.s) && aligned16(a.mask) && aligned8(a.codes);
    return vec ? QS_MX_SOFTMAX_ROUTE_VEC : QS_MX_SOFTMAX_ROUTE_PLAIN;
}

template <bool VEC, bool RES>
int mx_softmax_enqueue(const qs_mx_softmax_quant_args& a) {
    const int64_t R = a.G * a.T;
    const int64_t mask_rows = (a.mask && a.mask_slices != 1) ? R : a.T;
    with_dtype(a.sdt, [&](auto X) {
        hipLaunchKernelGGL((mx_softmax_quant_kernel<decltype(X)::value, VEC, RES>), dim3((unsigned)((R + kMsxRows - 1) / kMsxRows)),
                           dim3(kMxq2Threads), 0, (hipStream_t)a.stream, mx_format(a.format), a.s, a.mask, a.codes, a.scales, R, a.T,
                           a.S, mask_rows, a.scale, a.causal);
        return 0;
    });
    return launch_status();
}

int mx_softmax_launch(const qs_mx_softmax_quant_args& a, int route) {
    const bool res = a.S <= (int64_t)kMsxResPasses * kMxnPass;  // the row fits the wave's registers: s is read once
    if (route == QS_MX_SOFTMAX_ROUTE_VEC) return res ? mx_softmax_enqueue<true, true>(a) : mx_softmax_enqueue<true, false>(a);
    return res ? mx_softmax_enqueue<false, true>(a) : mx_softmax_enqueue<false, false>(a);
}

}  // namespace

extern "C" {

int qs_mx_softmax_quant_route(const qs_mx_softmax_quant_args* args) {
    qs_mx_softmax_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_softmax_route(a);
}

int qs_mx_softmax_quant_v(const qs_mx_softmax_quant_args* args) {
    qs_mx_softmax_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_softmax_route(a);
    if (route <= 0) return route;
    return mx_softmax_launch(a, route);
}

}  // extern "C"
