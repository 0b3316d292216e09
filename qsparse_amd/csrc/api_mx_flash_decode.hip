// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), grouped-query attention on MX codes for decoding (qs_mx_flash_decode.h): one wave
// per (sequence, kv head, 16 packed query rows, split of the key axis), the valid length read on the device, the splits combined by a
// second small kernel in a fixed order.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_flash_decode.h"

namespace {

// the checks of qs_mx_flash_decode_v, in the header's order, and the kernel it launches for these operands: QS_MX_FLASH_ROUTE_*, 0 for
// an empty problem, QS_ERR_*
int mx_flash_decode_route(const qs_mx_flash_decode_args& a) {
    if (!a.q_codes || !a.q_scales || !a.k_codes || !a.k_scales || !a.vt_codes || !a.vt_scales || !a.y) return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.p_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.B < 0 || a.Hq < 0 || a.Hkv < 0 || a.T < 0 || a.S < 0 || a.d < 0 || a.dv < 0 || a.kv_splits < 1) return QS_ERR_ARG;
    if (a.d > kMxfMaxD || a.dv > kMxfMaxD) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || !aligned4(a.kv_len) || !aligned4(a.workspace)) return QS_ERR_ALIGN;
    if (a.B == 0 || a.Hq == 0 || a.T == 0 || a.dv == 0) return 0;
    if (a.Hkv == 0 || a.Hq % a.Hkv != 0 || a.Hq / a.Hkv > kMxdMaxRows || a.Hq / a.Hkv * a.T > kMxdMaxRows) return QS_ERR_ARG;
    if (a.S == 0 || a.d == 0 || a.S > INT32_MAX - kMxsChunk) return QS_ERR_ARG;
    // B Hkv S 128 codes of k and vt, B Hq T 128 elements of y, B Hkv R n (dv + 3) floats of workspace: every byte count fits 64 bits
    const int64_t R = a.Hq / a.Hkv * a.T, tiles = (R + 15) / 16;
    int64_t heads, waves, recs;
    if (!mul_ok(a.B, a.Hkv, &heads) || heads > INT64_MAX / 4 / kMxfMaxD / a.S || heads > INT64_MAX / 4 / kMxfMaxD / kMxdMaxRows) return QS_ERR_ARG;
    if (!mul_ok(heads * tiles, a.kv_splits, &waves) || waves > 4 * kMaxGrid || heads * R > 8 * kMaxGrid) return QS_ERR_ARG;
    if (!mul_ok(heads * R, a.kv_splits, &recs) || recs > INT64_MAX / 4 / (kMxfMaxD + 3)) return QS_ERR_ARG;
    if (a.kv_splits > 1 && (!a.workspace || a.workspace_bytes < recs * (a.dv + 3) * 4)) return QS_ERR_ARG;
    const bool vec = a.d % 16 == 0 && a.S % 16 == 0 && aligned16(a.q_codes) && aligned16(a.k_codes) && aligned16(a.vt_codes);
    return vec ? QS_MX_FLASH_ROUTE_VEC : QS_MX_FLASH_ROUTE_PLAIN;
}

int mx_flash_decode_launch(const qs_mx_flash_decode_args& a, int route) {
    MxdArgs k;
    k.q = a.q_codes, k.qs = a.q_scales, k.k = a.k_codes, k.ks = a.k_scales, k.vt = a.vt_codes, k.vts = a.vt_scales;
    k.kv_len = a.kv_len, k.ws = a.workspace, k.y = a.y;
    k.T = (int)a.T, k.S = (int)a.S, k.d = (int)a.d, k.dv = (int)a.dv, k.Hkv = (int)a.Hkv, k.r = (int)(a.Hq / a.Hkv);
    k.R = k.r * k.T, k.tiles = (k.R + 15) / 16, k.n = a.kv_splits;
    const int chunks = (k.S + kMxsChunk - 1) / kMxsChunk;
    k.cps = (chunks + k.n - 1) / k.n;
    k.items = a.B * a.Hkv * k.tiles * k.n;
    k.scale = a.scale;
    k.qk_format = a.qk_format, k.p_format = a.p_format, k.v_format = a.v_format;
    k.ydt = a.ydt, k.causal = a.causal, k.vec = route == QS_MX_FLASH_ROUTE_VEC;
    k.y_vec = mx_y_vec(a.y, a.ydt, a.dv);
    hipLaunchKernelGGL(mx_flash_decode_kernel, dim3((unsigned)((k.items + 3) / 4)), dim3(kMxgThreads), 0, (hipStream_t)a.stream,
                       mx_format(a.p_format), k);
    if (k.n > 1) {
        const int64_t quads = a.B * a.Hq * a.T * ((a.dv + 3) / 4);
        hipLaunchKernelGGL(mx_flash_decode_combine_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)a.stream, k,
                           quads);
    }
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_flash_decode_route(const qs_mx_flash_decode_args* args) {
    qs_mx_flash_decode_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_flash_decode_route(a);
}

int qs_mx_flash_decode_v(const qs_mx_flash_decode_args* args) {
    qs_mx_flash_decode_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_flash_decode_route(a);
    if (route <= 0) return route;
    return mx_flash_decode_launch(a, route);
}

}  // extern "C"
