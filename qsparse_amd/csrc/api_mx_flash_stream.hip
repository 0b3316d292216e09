// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), attention on MX codes in one launch for any key length (qs_mx_flash_stream.h):
// the key axis walked in chunks of 128 with a running maximum, a running sum and a rescaled accumulator -- the header's chunk
// recurrence, whose scores and attention weights never reach memory.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_flash_stream.h"

namespace {

// the checks of qs_mx_flash_attention_streamed_v -- qs_mx_flash_attention_v's, in its order, without the bound on S -- and the kernel
// it launches for these operands: QS_MX_FLASH_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_flash_stream_route(const qs_mx_flash_attention_args& a) {
    if (!a.q_codes || !a.q_scales || !a.k_codes || !a.k_scales || !a.vt_codes || !a.vt_scales || !a.y) return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.p_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0 || a.d < 0 || a.dv < 0) return QS_ERR_ARG;
    if (a.d > kMxfMaxD || a.dv > kMxfMaxD) return QS_ERR_ARG;
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (((uintptr_t)a.mask) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0 || a.dv == 0) return 0;
    if (a.d == 0) return QS_ERR_ARG;
    // G T S elements of the mask, G S 128 codes of k and vt, G T 128 elements of y: every byte count fits 64 bits
    if (a.G > INT64_MAX / 4 / kMxfMaxD / a.T || a.G > INT64_MAX / 4 / kMxfMaxD / a.S || a.G * a.T > INT64_MAX / 4 / a.S) return QS_ERR_ARG;
    if (a.G > kMaxGrid / ((a.T + kMxfRows - 1) / kMxfRows)) return QS_ERR_ARG;
    const bool vec = a.d % 16 == 0 && a.S % 16 == 0 && aligned16(a.q_codes) && aligned16(a.k_codes) && aligned16(a.vt_codes) &&
                     aligned16(a.mask);
    return vec ? QS_MX_FLASH_ROUTE_VEC : QS_MX_FLASH_ROUTE_PLAIN;
}

int mx_flash_stream_launch(const qs_mx_flash_attention_args& a, int route) {
    MxfArgs k;
    k.q = a.q_codes, k.qs = a.q_scales, k.k = a.k_codes, k.ks = a.k_scales, k.vt = a.vt_codes, k.vts = a.vt_scales;
    k.mask = a.mask, k.y = a.y;
    k.T = a.T, k.S = a.S, k.d = a.d, k.dv = a.dv;
    k.mask_rows = (a.mask && a.mask_slices != 1) ? a.G * a.T : a.T;
    k.scale = a.scale;
    k.qk_format = a.qk_format, k.p_format = a.p_format, k.v_format = a.v_format;
    k.ydt = a.ydt, k.causal = a.causal, k.vec = route == QS_MX_FLASH_ROUTE_VEC;
    k.y_vec = mx_y_vec(a.y, a.ydt, a.dv);
    k.tiles = (int)((a.T + kMxfRows - 1) / kMxfRows);
    hipLaunchKernelGGL(mx_flash_stream_kernel, dim3((unsigned)(a.G * k.tiles)), dim3(kMxgThreads), 0, (hipStream_t)a.stream,
                       mx_format(a.p_format), k);
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_flash_attention_streamed_route(const qs_mx_flash_attention_args* args) {
    qs_mx_flash_attention_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_flash_stream_route(a);
}

int qs_mx_flash_attention_streamed_v(const qs_mx_flash_attention_args* args) {
    qs_mx_flash_attention_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_flash_stream_route(a);
    if (route <= 0) return route;
    return mx_flash_stream_launch(a, route);
}

}  // extern "C"
