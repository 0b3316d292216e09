// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), grouped-query attention on MX codes for a ragged batch of new tokens against the
// cache they were appended to (qs_mx_flash_ragged.h): a flat token-major q cut into sequences by cu_seqlens, which the kernel reads as it
// reads kv_len and the block table; one work-group per (kv head, item), each finding its (sequence, tile) itself.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_flash_ragged.h"

namespace {

// log2(page) for a power of two >= 32, else -1
int page_log2(int64_t page) {
    if (page < QS_MX_BLOCK || page > ((int64_t)1 << 30) || (page & (page - 1)) != 0) return -1;
    return __builtin_ctzll((unsigned long long)page);
}

// work-groups per kv head: ceil(r Ttot / 64) + B, at least the tiles of every cu_seqlens
int64_t ragged_items(int64_t r, int64_t Ttot, int64_t B) { return (r * Ttot + kMxfRows - 1) / kMxfRows + B; }

// the checks of qs_mx_flash_ragged_v, in the header's order, and the kernel it launches for these operands: QS_MX_FLASH_ROUTE_*, 0 for an
// empty problem, QS_ERR_*
int mx_flash_ragged_route(const qs_mx_flash_ragged_args& a) {
    const bool paged = a.block_table != nullptr;
    if (!a.q_codes || !a.q_scales || !a.k_codes || !a.k_scales || !a.vt_codes || !a.vt_scales || !a.y || !a.kv_len || !a.cu_seqlens)
        return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.p_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.causal != 0 && a.causal != 1) return QS_ERR_ARG;
    if (a.B < 0 || a.Hq < 0 || a.Hkv < 0 || a.Ttot < 0 || a.S < 0 || a.d < 0 || a.dv < 0 || a.P < 0 || a.NP < 0 || a.page < 0)
        return QS_ERR_ARG;
    if (a.d > kMxfMaxD || a.dv > kMxfMaxD) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || !aligned4(a.kv_len) || !aligned4(a.block_table) || !aligned4(a.cu_seqlens))
        return QS_ERR_ALIGN;
    if (a.B == 0 || a.Hq == 0 || a.Ttot == 0 || a.dv == 0) return 0;
    if (a.Hkv == 0 || a.Hq % a.Hkv != 0 || a.d == 0) return QS_ERR_ARG;
    int64_t S = a.S;
    if (paged && (a.P < 1 || a.P > INT32_MAX || a.NP < 1 || page_log2(a.page) < 0 || !mul_ok(a.NP, a.page, &S))) return QS_ERR_ARG;
    if (S == 0 || S > INT32_MAX - kMxsChunk) return QS_ERR_ARG;
    // r Ttot packed rows in an int; B Hkv S 128 codes of the cache (P Hkv page 128 of the pool), B NP entries, Ttot Hq 128 elements of y:
    // every byte count fits 64 bits; `items` work-groups per kv head
    int64_t R, heads, rows, pool, entries, blocks;
    if (a.Ttot > INT32_MAX || !mul_ok(a.Hq / a.Hkv, a.Ttot, &R) || R > INT32_MAX - kMxfRows) return QS_ERR_ARG;
    if (!mul_ok(a.B, a.Hkv, &heads) || heads > INT32_MAX || !mul_ok(a.Ttot, a.Hq, &rows) || rows > INT64_MAX / 4 / kMxfMaxD) return QS_ERR_ARG;
    if (paged) {
        if (!mul_ok(a.P, a.Hkv, &pool) || pool > INT64_MAX / 4 / kMxfMaxD / a.page || !mul_ok(a.B, a.NP, &entries) || entries > INT64_MAX / 4)
            return QS_ERR_ARG;
    } else if (heads > INT64_MAX / 4 / kMxfMaxD / S) {
        return QS_ERR_ARG;
    }
    if (!mul_ok(a.Hkv, ragged_items(a.Hq / a.Hkv, a.Ttot, a.B), &blocks) || blocks > kMaxGrid) return QS_ERR_ARG;
    // paged: every page base is 16-byte aligned (page * d % 16 == 0 with d % 16 == 0, vt rows are `page` >= 32 bytes apart)
    const bool vec = a.d % 16 == 0 && (paged || S % 16 == 0) && aligned16(a.q_codes) && aligned16(a.k_codes) && aligned16(a.vt_codes);
    return vec ? QS_MX_FLASH_ROUTE_VEC : QS_MX_FLASH_ROUTE_PLAIN;
}

int mx_flash_ragged_launch(const qs_mx_flash_ragged_args& a, int route) {
    const bool paged = a.block_table != nullptr;
    MxgArgs k;
    k.q = a.q_codes, k.qs = a.q_scales, k.k = a.k_codes, k.ks = a.k_scales, k.vt = a.vt_codes, k.vts = a.vt_scales;
    k.kv_len = a.kv_len, k.table = a.block_table, k.cu = a.cu_seqlens, k.y = a.y;
    k.P = paged ? (int)a.P : 0, k.NP = paged ? (int)a.NP : 0, k.lg = paged ? page_log2(a.page) : 30;
    k.S = (int)(paged ? a.NP * a.page : a.S), k.d = (int)a.d, k.dv = (int)a.dv, k.Hkv = (int)a.Hkv, k.r = (int)(a.Hq / a.Hkv);
    k.T = 0, k.R = 0, k.tiles = 0, k.heads = 0;
    k.B = (int)a.B, k.Hq = (int)a.Hq, k.Ttot = (int)a.Ttot, k.items = (int)ragged_items(k.r, a.Ttot, a.B);
    k.scale = a.scale;
    k.qk_format = a.qk_format, k.p_format = a.p_format, k.v_format = a.v_format;
    k.ydt = a.ydt, k.causal = a.causal, k.vec = route == QS_MX_FLASH_ROUTE_VEC;
    k.y_vec = mx_y_vec(a.y, a.ydt, a.dv);
    const dim3 grid((unsigned)((int64_t)k.items * k.Hkv));
    if (paged)
        hipLaunchKernelGGL(mx_flash_ragged_kernel<true>, grid, dim3(kMxgThreads), 0, (hipStream_t)a.stream, mx_format(a.p_format), k);
    else
        hipLaunchKernelGGL(mx_flash_ragged_kernel<false>, grid, dim3(kMxgThreads), 0, (hipStream_t)a.stream, mx_format(a.p_format), k);
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_flash_ragged_route(const qs_mx_flash_ragged_args* args) {
    qs_mx_flash_ragged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_flash_ragged_route(a);
}

int qs_mx_flash_ragged_v(const qs_mx_flash_ragged_args* args) {
    qs_mx_flash_ragged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_flash_ragged_route(a);
    if (route <= 0) return route;
    return mx_flash_ragged_launch(a, route);
}

}  // extern "C"
