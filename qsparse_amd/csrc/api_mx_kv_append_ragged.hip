// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), appending a RAGGED batch of tokens to the paged MX KV cache
// (qs_mx_kv_append_ragged.h): mx_kv_append_paged's one launch with the new tokens flat and token-major and the sequences' extents in
// cu_seqlens, which the kernel reads.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_kv_append_ragged.h"

namespace {

constexpr int64_t kKvaMaxExtent = (int64_t)1 << 30;             // S and Ttot: L_b + t stays inside 32 bits

// log2(page) for a power of two >= 32, else -1
int page_log2(int64_t page) {
    if (page < QS_MX_BLOCK || page > kKvaMaxExtent || (page & (page - 1)) != 0) return -1;
    return __builtin_ctzll((unsigned long long)page);
}

struct RaggedGrid {
    int64_t lpr, rpg, n_row, n_edge, n_mid;
};
RaggedGrid ragged_grid(const qs_mx_kv_append_ragged_args& a, int64_t Hq) {
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    RaggedGrid g;
    g.lpr = (a.d + QS_MX_BLOCK - 1) / QS_MX_BLOCK * (QS_MX_BLOCK / v), g.rpg = qs::kKvaThreads / g.lpr;
    g.n_row = ((a.Hkv + Hq) * a.Ttot + g.rpg - 1) / g.rpg;
    g.n_edge = a.B * a.Hkv, g.n_mid = a.Ttot / QS_MX_BLOCK * a.Hkv;     // whole middle blocks: at most floor(Ttot / 32) per kv head
    return g;
}

// the checks of qs_mx_kv_append_ragged_v, in the header's order, and the kernel it launches for these operands:
// QS_MX_KV_APPEND_ROUTE_*, 0 for an empty problem, QS_ERR_*
int mx_kv_append_ragged_route(const qs_mx_kv_append_ragged_args& a) {
    if (!a.k_pool || !a.k_pool_scales || !a.vt_pool || !a.vt_pool_scales || !a.v_tail || !a.block_table || !a.kv_len || !a.cu_seqlens ||
        !a.k_new || !a.v_new)
        return QS_ERR_ARG;
    if (!mx_format_ok(a.qk_format) || !mx_format_ok(a.v_format)) return QS_ERR_ARG;
    if (a.interleaved != 0 && a.interleaved != 1) return QS_ERR_ARG;
    if ((a.cos == nullptr) != (a.sin == nullptr)) return QS_ERR_ARG;
    if (a.q_new && (!a.q_codes || !a.q_scales)) return QS_ERR_ARG;
    if (a.B < 0 || a.Hq < 0 || a.Hkv < 0 || a.Ttot < 0 || a.P_pool < 0 || a.NP < 0 || a.page < 0 || a.d < 0 || a.dv < 0 || a.P < 0)
        return QS_ERR_ARG;
    if (a.d > kKvaMaxD || a.dv > kKvaMaxD) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    const uintptr_t em = dt_size(a.xdt) - 1;
    if ((((uintptr_t)a.k_new) & em) != 0 || (((uintptr_t)a.v_new) & em) != 0 || (((uintptr_t)a.q_new) & em) != 0 || !aligned4(a.v_tail) ||
        !aligned4(a.block_table) || !aligned4(a.kv_len) || !aligned4(a.cu_seqlens) || !aligned4(a.cos) || !aligned4(a.sin))
        return QS_ERR_ALIGN;
    if (a.B == 0 || a.Ttot == 0) return 0;
    const int64_t Hq = a.q_new ? a.Hq : 0;
    if (a.Hkv == 0 || Hq % a.Hkv != 0 || a.d == 0 || a.dv == 0) return QS_ERR_ARG;
    int64_t S, pool, entries;
    if (a.P_pool < 1 || a.P_pool > INT32_MAX || a.NP < 1 || page_log2(a.page) < 0 || !mul_ok(a.NP, a.page, &S) || S > kKvaMaxExtent)
        return QS_ERR_ARG;
    if (a.Ttot > kKvaMaxExtent || a.B > INT32_MAX - 1 || a.Hkv > INT32_MAX || Hq > INT32_MAX) return QS_ERR_ARG;
    if (a.cos && ((a.d & 1) || a.P < S || a.P > INT32_MAX)) return QS_ERR_ARG;
    // Ttot (Hkv + Hq) 128 elements, P_pool Hkv page 128 codes, B NP entries, B Hkv 128 32 floats of v_tail: every index fits 64 bits
    int64_t rows, heads;
    if (!mul_ok(a.Ttot, a.Hkv + Hq, &rows) || rows > INT64_MAX / 4 / kKvaMaxD) return QS_ERR_ARG;
    if (!mul_ok(a.B, a.Hkv, &heads) || heads > INT64_MAX / 4 / kKvaMaxD / QS_MX_BLOCK) return QS_ERR_ARG;
    if (!mul_ok(a.P_pool, a.Hkv, &pool) || pool > INT64_MAX / 4 / kKvaMaxD / a.page || !mul_ok(a.B, a.NP, &entries) || entries > INT64_MAX / 4)
        return QS_ERR_ARG;
    const RaggedGrid g = ragged_grid(a, Hq);
    if (g.n_row + g.n_edge + g.n_mid > kMaxGrid) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    const bool rows_vec = a.d % v == 0 && aligned16(a.k_new) && aligned16(a.q_new) && (((uintptr_t)a.k_pool) & (v - 1)) == 0 &&
                          (((uintptr_t)a.q_codes) & (v - 1)) == 0 &&
                          (!a.cos || (aligned16(a.cos) && aligned16(a.sin) && (a.interleaved || (a.d / 2) % v == 0)));
    const bool vt_vec = a.dv % v == 0 && aligned16(a.v_new) && aligned16(a.vt_pool);      // (page % 16 == 0)
    return rows_vec && vt_vec ? QS_MX_KV_APPEND_ROUTE_VEC : QS_MX_KV_APPEND_ROUTE_PLAIN;
}

int mx_kv_append_ragged_launch(const qs_mx_kv_append_ragged_args& a, int route) {
    KvgArgs k;
    k.k_new = a.k_new, k.v_new = a.v_new, k.q_new = a.q_new, k.cs = a.cos, k.sn = a.sin, k.kv_len = a.kv_len, k.cu = a.cu_seqlens;
    k.k_codes = a.k_pool, k.k_scales = a.k_pool_scales, k.vt_codes = a.vt_pool, k.vt_scales = a.vt_pool_scales;
    k.q_codes = a.q_codes, k.q_scales = a.q_scales, k.v_tail = a.v_tail;
    k.table = a.block_table, k.pool = (int)a.P_pool, k.NP = (int)a.NP, k.lg = page_log2(a.page);
    k.B = (int)a.B, k.Hkv = (int)a.Hkv, k.Hq = a.q_new ? (int)a.Hq : 0, k.Ttot = (int)a.Ttot, k.S = (int)(a.NP * a.page), k.d = (int)a.d;
    k.dv = (int)a.dv, k.P = (int)a.P;
    k.T = 0, k.row_groups = 0, k.mid = 0;
    k.mode = !a.cos ? kKvaPlainRows : (a.interleaved ? kKvaInterleaved : kKvaHalf);
    const RaggedGrid g = ragged_grid(a, k.Hq);
    k.lpr = (int)g.lpr, k.rpg = (int)g.rpg;
    k.n_row = (unsigned)g.n_row, k.n_edge = (unsigned)g.n_edge;
    const unsigned grid = (unsigned)(g.n_row + g.n_edge + g.n_mid);
    const MxFormat fq = mx_format(a.qk_format), fv = mx_format(a.v_format);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        if (route == QS_MX_KV_APPEND_ROUTE_VEC)
            hipLaunchKernelGGL((mx_kv_append_ragged_kernel<XD, true>), dim3(grid), dim3(kKvaThreads), 0, s, fq, fv, k);
        else
            hipLaunchKernelGGL((mx_kv_append_ragged_kernel<XD, false>), dim3(grid), dim3(kKvaThreads), 0, s, fq, fv, k);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_kv_append_ragged_route(const qs_mx_kv_append_ragged_args* args) {
    qs_mx_kv_append_ragged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_kv_append_ragged_route(a);
}

int qs_mx_kv_append_ragged_v(const qs_mx_kv_append_ragged_args* args) {
    qs_mx_kv_append_ragged_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_kv_append_ragged_route(a);
    if (route <= 0) return route;
    return mx_kv_append_ragged_launch(a, route);
}

}  // extern "C"
