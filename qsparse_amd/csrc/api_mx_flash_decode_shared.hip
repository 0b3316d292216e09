// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), grouped-query attention on MX codes for decoding from a paged cache whose sequences
// share a prefix (qs_mx_flash_decode_shared.h): one launch of shared items -- 16 rows of the batch against the prefix's keys -- and own
// items, then mx_flash_decode_combine_kernel over the sp + so records of every row.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_flash_decode_shared.h"

namespace {

// log2(page) for a power of two >= 32, else -1
int page_log2(int64_t page) {
    if (page < QS_MX_BLOCK || page > ((int64_t)1 << 30) || (page & (page - 1)) != 0) return -1;
    return __builtin_ctzll((unsigned long long)page);
}

// the chunks of the longest shared part these shapes allow: Csmax
int64_t shared_chunks_max(const qs_mx_flash_decode_shared_paged_args& a) {
    const int64_t u = a.page > kMxsChunk ? a.page : kMxsChunk, cap = (a.NPs < a.NP ? a.NPs : a.NP) * a.page;
    return cap / u * u / kMxsChunk;
}

// the checks of qs_mx_flash_decode_shared_paged_v, in the header's order, and the kernel it launches for these operands:
// QS_MX_FLASH_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_flash_decode_shared_route(const qs_mx_flash_decode_shared_paged_args& a) {
    if (!a.q_codes || !a.q_scales || !a.k_pool || !a.k_pool_scales || !a.vt_pool || !a.vt_pool_scales || !a.block_table || !a.kv_len ||
        !a.shared_table || !a.shared_len || !a.y)
        return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.p_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.B < 0 || a.Hq < 0 || a.Hkv < 0 || a.T < 0 || a.P < 0 || a.NP < 0 || a.NPs < 0 || a.page < 0 || a.d < 0 || a.dv < 0 ||
        a.kv_splits < 1 || a.shared_splits < 1)
        return QS_ERR_ARG;
    if (a.d > kMxfMaxD || a.dv > kMxfMaxD) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || !aligned4(a.block_table) || !aligned4(a.kv_len) || !aligned4(a.shared_table) ||
        !aligned4(a.shared_len) || !aligned4(a.workspace))
        return QS_ERR_ALIGN;
    if (a.B == 0 || a.Hq == 0 || a.T == 0 || a.dv == 0) return 0;
    if (a.Hkv == 0 || a.Hq % a.Hkv != 0 || a.Hq / a.Hkv > kMxdMaxRows || a.Hq / a.Hkv * a.T > kMxdMaxRows) return QS_ERR_ARG;
    if (a.P < 1 || a.P > INT32_MAX || a.NP < 1 || a.NPs < 1 || a.NPs > INT32_MAX || a.d == 0) return QS_ERR_ARG;
    // as qs_mx_flash_decode_paged_v, with n = shared_splits + kv_splits records per row and the shared items' waves
    const int lg = page_log2(a.page);
    int64_t S, heads, pool, rows, waves_o, waves_s, recs, entries;
    if (lg < 0 || !mul_ok(a.NP, a.page, &S) || S > INT32_MAX - kMxsChunk) return QS_ERR_ARG;
    const int64_t R = a.Hq / a.Hkv * a.T, tiles = (R + 15) / 16, n = (int64_t)a.shared_splits + a.kv_splits;
    if (!mul_ok(a.B, a.Hkv, &heads) || heads > INT64_MAX / 4 / kMxfMaxD / kMxdMaxRows || !mul_ok(a.B, a.NP, &entries) ||
        entries > INT64_MAX / 4 || n > INT32_MAX)
        return QS_ERR_ARG;
    if (!mul_ok(a.P, a.Hkv, &pool) || pool > INT64_MAX / 4 / kMxfMaxD / a.page) return QS_ERR_ARG;
    if (!mul_ok(a.B, R, &rows) || rows > INT32_MAX) return QS_ERR_ARG;
    if (!mul_ok(heads * tiles, a.kv_splits, &waves_o) || !mul_ok(a.Hkv * ((rows + 15) / 16), a.shared_splits, &waves_s) ||
        waves_o > 4 * kMaxGrid - waves_s || heads * R > 8 * kMaxGrid)
        return QS_ERR_ARG;
    if (!mul_ok(heads * R, n, &recs) || recs > INT64_MAX / 4 / (kMxfMaxD + 3)) return QS_ERR_ARG;
    if (!a.workspace || a.workspace_bytes < recs * (a.dv + 3) * 4) return QS_ERR_ARG;
    // every page base is 16-byte aligned: page * d % 16 == 0 with d % 16 == 0, vt rows are `page` >= 32 bytes apart
    const bool vec = a.d % 16 == 0 && aligned16(a.q_codes) && aligned16(a.k_pool) && aligned16(a.vt_pool);
    return vec ? QS_MX_FLASH_ROUTE_VEC : QS_MX_FLASH_ROUTE_PLAIN;
}

int mx_flash_decode_shared_launch(const qs_mx_flash_decode_shared_paged_args& a, int route) {
    MxdSharedArgs k;
    k.q = a.q_codes, k.qs = a.q_scales, k.k = a.k_pool, k.ks = a.k_pool_scales, k.vt = a.vt_pool, k.vts = a.vt_pool_scales;
    k.kv_len = a.kv_len, k.ws = a.workspace, k.y = a.y;
    k.table = a.block_table, k.P = (int)a.P, k.NP = (int)a.NP, k.lg = page_log2(a.page);
    k.stable = a.shared_table, k.slen = a.shared_len, k.B = (int)a.B, k.NPs = (int)a.NPs;
    k.cap = (int)((a.NPs < a.NP ? a.NPs : a.NP) * a.page), k.ulg = k.lg > 7 ? k.lg : 7;
    k.T = (int)a.T, k.S = (int)(a.NP * a.page), k.d = (int)a.d, k.dv = (int)a.dv, k.Hkv = (int)a.Hkv, k.r = (int)(a.Hq / a.Hkv);
    k.R = k.r * k.T, k.tiles = (k.R + 15) / 16, k.sp = a.shared_splits, k.n = a.shared_splits + a.kv_splits;
    const int chunks = (k.S + kMxsChunk - 1) / kMxsChunk;
    const int64_t csmax = shared_chunks_max(a);
    k.cps = (chunks + a.kv_splits - 1) / a.kv_splits;
    k.cps_s = (int)(((csmax > 1 ? csmax : 1) + k.sp - 1) / k.sp);
    k.tiles_s = (int)((a.B * k.R + 15) / 16);
    k.items_s = a.Hkv * k.tiles_s * k.sp;
    k.items = k.items_s + a.B * a.Hkv * k.tiles * a.kv_splits;
    k.scale = a.scale;
    k.qk_format = a.qk_format, k.p_format = a.p_format, k.v_format = a.v_format;
    k.ydt = a.ydt, k.causal = a.causal, k.vec = route == QS_MX_FLASH_ROUTE_VEC;
    k.y_vec = mx_y_vec(a.y, a.ydt, a.dv);
    hipLaunchKernelGGL(mx_flash_decode_shared_kernel, dim3((unsigned)((k.items + 3) / 4)), dim3(kMxgThreads), 0, (hipStream_t)a.stream,
                       mx_format(a.p_format), k);
    const int64_t quads = a.B * a.Hq * a.T * ((a.dv + 3) / 4);
    hipLaunchKernelGGL(mx_flash_decode_combine_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)a.stream,
                       (const MxdArgs&)k, quads);
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_flash_decode_shared_paged_route(const qs_mx_flash_decode_shared_paged_args* args) {
    qs_mx_flash_decode_shared_paged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_flash_decode_shared_route(a);
}

int qs_mx_flash_decode_shared_paged_v(const qs_mx_flash_decode_shared_paged_args* args) {
    qs_mx_flash_decode_shared_paged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_flash_decode_shared_route(a);
    if (route <= 0) return route;
    return mx_flash_decode_shared_launch(a, route);
}

}  // extern "C"
