// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), attention on MX codes in one launch (qs_mx_flash.h): Q . K^T through the
// block-scaled MFMA, the softmax quantizer's definition on the accumulators, P . V through the MFMA again -- bit for bit the chain
// qs_mx_bmm_v -> qs_mx_softmax_quant_v -> qs_mx_bmm_v, whose scores and attention weights never reach memory.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_flash.h"

namespace {

// the checks of qs_mx_flash_attention_v and the kernel it launches for these operands: QS_MX_FLASH_ROUTE_*, 0 for an empty problem,
// QS_ERR_*
int mx_flash_route(const qs_mx_flash_attention_args& a) {
    if (!a.q_codes || !a.q_scales || !a.k_codes || !a.k_scales || !a.vt_codes || !a.vt_scales || !a.y) return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.p_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.G < 0 || a.T < 0 || a.S < 0 || a.d < 0 || a.dv < 0) return QS_ERR_ARG;
    if (a.S > kMxfMaxS || a.d > kMxfMaxD || a.dv > kMxfMaxD) return QS_ERR_ARG;       // the supported range: a row of scores stays on chip
    if (a.mask && a.mask_slices != 1 && a.mask_slices != a.G) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (((uintptr_t)a.mask) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.G == 0 || a.T == 0 || a.S == 0 || a.dv == 0) return 0;
    if (a.d == 0) return QS_ERR_ARG;
    if (a.G > INT64_MAX / a.T || a.G * a.T > INT64_MAX / kMxfMaxS) return QS_ERR_ARG;   // (S, d, dv <= 512: every operand's byte count fits)
    if (a.G > kMaxGrid / ((a.T + kMxfRows - 1) / kMxfRows)) return QS_ERR_ARG;
    // mx_bmm's rule for the three code operands (K is d for q and k, S for vt), and 16-byte loads of the mask
    const bool vec = a.d % 16 == 0 && a.S % 16 == 0 && aligned16(a.q_codes) && aligned16(a.k_codes) && aligned16(a.vt_codes) &&
                     aligned16(a.mask);
    return vec ? QS_MX_FLASH_ROUTE_VEC : QS_MX_FLASH_ROUTE_PLAIN;
}

int mx_flash_launch(const qs_mx_flash_attention_args& a, int route) {
    MxfArgs k;
    k.q = a.q_codes, k.qs = a.q_scales, k.k = a.k_codes, k.ks = a.k_scales, k.vt = a.vt_codes, k.vts = a.vt_scales;
    k.mask = a.mask, k.y = a.y;
    k.T = a.T, k.S = a.S, k.d = a.d, k.dv = a.dv;
    k.mask_rows = (a.mask && a.mask_slices != 1) ? a.G * a.T : a.T;
    k.scale = a.scale;
    k.qk_format = a.qk_format, k.ydt = a.ydt, k.causal = a.causal, k.vec = route == QS_MX_FLASH_ROUTE_VEC;
    k.y_vec = mx_y_vec(a.y, a.ydt, a.dv);
    k.tiles = (int)((a.T + kMxfRows - 1) / kMxfRows);
    const dim3 grid((unsigned)(a.G * k.tiles));
    k.p_format = a.p_format, k.v_format = a.v_format;
    const MxFormat fp = mx_format(a.p_format);
    if (a.S > 256)                                              // 32 fragments of scores per lane instead of 16
        hipLaunchKernelGGL(mx_flash_kernel<32>, grid, dim3(kMxgThreads), 0, (hipStream_t)a.stream, fp, k);
    else
        hipLaunchKernelGGL(mx_flash_kernel<16>, grid, dim3(kMxgThreads), 0, (hipStream_t)a.stream, fp, k);
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_flash_attention_route(const qs_mx_flash_attention_args* args) {
    qs_mx_flash_attention_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_flash_route(a);
}

int qs_mx_flash_attention_v(const qs_mx_flash_attention_args* args) {
    qs_mx_flash_attention_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_flash_route(a);
    if (route <= 0) return route;
    return mx_flash_launch(a, route);
}

}  // extern "C"
