// Host-side helpers shared by the seven translation units of the products on MX codes (api_mx_gemm.hip, api_mx_gemm_splitk.hip,
// api_mx_conv.hip, api_mx_conv_t.hip, api_mx_conv_wgrad.hip, api_mx_gemm_q.hip, api_mx_conv_q.hip): the dispatch over the 5 x 5 format pairs, the tile count and the store
// rule of y, the descriptor of a product forwarded to qs_mx_matmul_v, what the two split products (mx_matmul's split-K, the
// convolution's weight gradient) share -- the slicing, the body of their `_plan` exports, the checks of their workspace; the launch of
// their reduction is mx_launch_reduce of qs_mx_gemm_splitk.h, next to its kernel -- and the checks the two convolutions share.
// Internal linkage, as qs_host.h.
#pragma once
#include "qs_host.h"
#include "qs_mx_gemm.h"

namespace {

template <typename F>
int mx_with_format(int format, F&& f) {
    switch (format) {
        case QS_MX_FP8_E4M3: return f(IC<QS_MX_FP8_E4M3>{});
        case QS_MX_FP8_E5M2: return f(IC<QS_MX_FP8_E5M2>{});
        case QS_MX_FP6_E2M3: return f(IC<QS_MX_FP6_E2M3>{});
        case QS_MX_FP6_E3M2: return f(IC<QS_MX_FP6_E3M2>{});
        default: return f(IC<QS_MX_FP4_E2M1>{});
    }
}

// f(FA, FB, VEC) with the two formats (checked by the caller: mx_format_ok) and `vec` as integral constants
template <typename F>
int mx_dispatch(int fa, int fb, bool vec, F&& f) {
    return mx_with_format(fa, [&](auto FA) {
        return mx_with_format(fb, [&](auto FB) { return vec ? f(FA, FB, std::true_type{}) : f(FA, FB, std::false_type{}); });
    });
}

inline int64_t mx_tiles(int64_t n) { return (n + kMxgTile - 1) / kMxgTile; }

// four consecutive n per lane in one store: every row of y [., N] must keep the store's alignment
inline int mx_y_vec(const void* y, int ydt, int64_t N) { return N % 4 == 0 && (((uintptr_t)y) & (4 * dt_size(ydt) - 1)) == 0; }

// y = A [M, K] . B [N, K]^T as qs_mx_matmul_v takes it
inline qs_mx_matmul_args mx_matmul_args(int fa, int fb, const uint8_t* a_codes, const uint8_t* a_scales, const uint8_t* b_codes,
                                        const uint8_t* b_scales, const float* bias, void* y, int ydt, int64_t M, int64_t N, int64_t K,
                                        qs_stream_t stream) {
    qs_mx_matmul_args m = {};
    m.struct_size = sizeof(m);
    m.a_format = fa, m.b_format = fb;
    m.a_codes = a_codes, m.a_scales = a_scales, m.b_codes = b_codes, m.b_scales = b_scales;
    m.bias = bias, m.y = y, m.ydt = ydt;
    m.M = M, m.N = N, m.K = K;
    m.stream = stream;
    return m;
}

// ---- what qs_mx_matmul_v and qs_mx_matmul_q_v (codes out) check alike (Args: either descriptor) -----------------------------------
// the operands and extents, all QS_ERR_ARG: they come before the checks of the output's dtype and alignment
template <class Args>
int mx_gemm_check_operands(const Args& a) {
    if (!a.a_codes || !a.a_scales || !a.b_codes || !a.b_scales) return QS_ERR_ARG;
    if (!mx_format_ok(a.a_format) || !mx_format_ok(a.b_format)) return QS_ERR_ARG;
    if (a.M < 0 || a.N < 0 || a.K < 0) return QS_ERR_ARG;
    return QS_OK;
}

// after them, for a product that is not empty: QS_MX_GEMM_ROUTE_VEC or _PLAIN, or QS_ERR_ARG
template <class Args>
int mx_gemm_sized_route(const Args& a) {
    if (a.K == 0 || a.M > INT64_MAX / a.N || a.M > INT64_MAX / a.K || a.N > INT64_MAX / a.K) return QS_ERR_ARG;
    if (mx_tiles(a.M) * mx_tiles(a.N) > kMaxGrid) return QS_ERR_ARG;
    return (a.K % 16 == 0 && aligned16(a.a_codes) && aligned16(a.b_codes)) ? QS_MX_GEMM_ROUTE_VEC : QS_MX_GEMM_ROUTE_PLAIN;
}

// ---- the outputs of the products that write MX codes (qs_mx_matmul_q_v, qs_mx_conv2d_q_v) ---------------------------------------------
// their own arguments, all QS_ERR_ARG
template <class Args>
bool mx_q_args_ok(const Args& a) {
    return a.out_codes && a.out_scales && mx_format_ok(a.out_format) && (a.act == QS_MX_ACT_NONE || a.act == QS_MX_ACT_RELU);
}

// four consecutive codes per lane in one store: every row of out_codes [., N] must keep the store's alignment
inline int mx_c_vec(const void* codes, int64_t N) { return N % 4 == 0 && (((uintptr_t)codes) & 3u) == 0; }

// do the `bytes` (> 0) bytes at `out` and the `in_bytes` (> 0) at `in` share a byte
inline bool mx_overlap(const void* out, int64_t bytes, const void* in, int64_t in_bytes) {
    const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in;
    return o < i + (uint64_t)in_bytes && i < o + (uint64_t)bytes;
}

// ---- the slicing of a product split along K and the automatic slice count (qs_mx_matmul_splitk_plan, qs_mx_conv2d_wgrad_plan;
// split_k == 0): a pure function of (M, N, K) and the caller's cap ----------------------------------------------------------------
constexpr int64_t kSplitMinSteps = 32;     // fewer K-steps than this: never split
constexpr int64_t kSplitFullTiles = 256;   // this many output tiles (one per CU) or more: never split
constexpr int64_t kSplitGroups = 512;      // work-groups aimed at: two co-resident per CU at 64 KiB of LDS each
constexpr int64_t kSplitStepsPerSlice = 8; // a slice keeps at least this many K-steps

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline int64_t auto_split(int64_t M, int64_t N, int64_t K, int64_t cap) {
    const int64_t tiles = mx_tiles(M) * mx_tiles(N), steps = cdiv(K, kMxgK);
    if (steps < kSplitMinSteps || tiles >= kSplitFullTiles) return 1;
    return std::max<int64_t>(1, std::min({kSplitGroups / tiles, steps / kSplitStepsPerSlice, cap}));
}

struct SplitPlan {
    int64_t per;          // K-steps per slice
    int32_t slices;       // S': no slice is empty
    uint64_t bytes;       // of the workspace; 0 when slices == 1
};

// QS_OK and the plan, or QS_ERR_ARG (a negative extent or request, K == 0 of a non-empty product, a byte count beyond 64 bits).
// `cap`: the most slices the automatic rule asks for
inline int split_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int64_t cap, SplitPlan* p) {
    if (M < 0 || N < 0 || K < 0 || split_k < 0) return QS_ERR_ARG;
    *p = SplitPlan{0, 1, 0};
    if (M == 0 || N == 0) return QS_OK;
    if (K == 0 || M > INT64_MAX / N) return QS_ERR_ARG;
    const int64_t steps = cdiv(K, kMxgK);
    const int64_t S = split_k == 0 ? auto_split(M, N, K, cap) : split_k;
    p->per = cdiv(steps, S);
    p->slices = (int32_t)cdiv(steps, p->per);      // <= S <= INT32_MAX
    if (p->slices > 1) {
        if ((uint64_t)(M * N) > UINT64_MAX / 4 / (uint64_t)p->slices) return QS_ERR_ARG;
        p->bytes = (uint64_t)(M * N) * 4u * (uint64_t)p->slices;
    }
    return QS_OK;
}

// the body of qs_mx_matmul_splitk_plan and qs_mx_conv2d_wgrad_plan, which differ in `cap`
inline int split_plan_out(int64_t M, int64_t N, int64_t K, int32_t split_k, int64_t cap, int32_t* slices, uint64_t* workspace_bytes) {
    SplitPlan p;
    const int st = split_plan(M, N, K, split_k, cap, &p);
    if (st != QS_OK) return st;
    if (slices) *slices = p.slices;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return QS_OK;
}

// the workspace of a product that `p` splits (p.slices > 1) over `tiles` output tiles: QS_OK or the error, in this order
inline int split_workspace_status(const SplitPlan& p, const void* workspace, uint64_t workspace_bytes, int64_t tiles) {
    if (!workspace) return QS_ERR_ARG;
    if (!aligned16(workspace)) return QS_ERR_ALIGN;
    if (workspace_bytes < p.bytes) return QS_ERR_WORKSPACE;
    if (tiles * p.slices > kMaxGrid) return QS_ERR_ARG;
    return QS_OK;
}

// ---- what qs_mx_conv2d_v and qs_mx_conv_transpose2d_v check alike (Args: either descriptor) -----------------------------------------
struct MxConvPlan {
    int64_t OH, OW, M;
};

// the operands and the geometry, all QS_ERR_ARG.  `own_ok`: the caller's own conditions on the arguments, which fail before the dtype's
template <class Args>
int mx_conv_check_operands(const Args& a, bool own_ok) {
    if (!a.x_codes || !a.x_scales || !a.w_codes || !a.w_scales) return QS_ERR_ARG;
    if (!mx_format_ok(a.x_format) || !mx_format_ok(a.w_format)) return QS_ERR_ARG;
    if (a.B < 0 || a.Cout < 0 || a.H < 1 || a.W < 1 || a.C < 1 || a.KH < 1 || a.KW < 1) return QS_ERR_ARG;
    if (a.stride_h < 1 || a.stride_w < 1 || a.dil_h < 1 || a.dil_w < 1 || a.pad_h < 0 || a.pad_w < 0) return QS_ERR_ARG;
    return own_ok ? QS_OK : QS_ERR_ARG;
}

// the kernels keep coordinates inside one image in 32 bits (addresses: 64); H and W are the caller's to bound
template <class Args>
int mx_conv_check_limits(const Args& a) {
    return a.C > INT32_MAX - QS_MX_BLOCK || a.B > INT32_MAX || a.Cout > INT32_MAX ? QS_ERR_ARG : QS_OK;
}

// before the output size, for the products that write y: QS_OK or the error
template <class Args>
int mx_conv_check_args(const Args& a, bool own_ok) {
    const int st = mx_conv_check_operands(a, own_ok && a.y);
    if (st != QS_OK) return st;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (a.bias && (((uintptr_t)a.bias) & 3u) != 0)) return QS_ERR_ALIGN;
    return mx_conv_check_limits(a);
}

// after it (1 <= OH, OW; H, W <= INT32_MAX): the sizes, the plan and the kernel -- QS_MX_CONV_ROUTE_VEC or _PLAIN, 0 for an empty
// problem, QS_ERR_ARG
template <class Args>
int mx_conv_plan(const Args& a, int64_t OH, int64_t OW, MxConvPlan* plan) {
    const int64_t taps = (int64_t)a.KH * a.KW, Cp = (a.C + QS_MX_BLOCK - 1) / QS_MX_BLOCK * QS_MX_BLOCK;
    if (taps > INT32_MAX || taps > INT64_MAX / Cp) return QS_ERR_ARG;
    if (a.B == 0 || a.Cout == 0) return 0;
    const int64_t Kp = taps * Cp;
    if (OH > INT64_MAX / OW || a.B > INT64_MAX / (OH * OW)) return QS_ERR_ARG;
    const int64_t M = a.B * OH * OW;
    if (a.H > INT64_MAX / a.W || a.B > INT64_MAX / (a.H * a.W) || a.B * a.H * a.W > INT64_MAX / a.C) return QS_ERR_ARG;
    if (M > INT64_MAX / a.Cout || M > INT64_MAX / Kp || a.Cout > INT64_MAX / Kp) return QS_ERR_ARG;
    if (mx_tiles(M) * mx_tiles(a.Cout) > kMaxGrid) return QS_ERR_ARG;
    if (plan) *plan = MxConvPlan{OH, OW, M};
    return (a.C % 16 == 0 && aligned16(a.x_codes) && aligned16(a.w_codes)) ? QS_MX_CONV_ROUTE_VEC : QS_MX_CONV_ROUTE_PLAIN;
}

// a 1 x 1 kernel at stride 1 without padding over whole blocks: x IS A [B H W, C] and w IS B [Cout, C] as they lie
template <class Args>
bool mx_conv_is_gemm(const Args& a) {
    return a.KH == 1 && a.KW == 1 && a.stride_h == 1 && a.stride_w == 1 && a.pad_h == 0 && a.pad_w == 0 && a.C % QS_MX_BLOCK == 0;
}

// after the argument checks of qs_mx_conv2d_v's convolution (Args: its descriptor or the codes-out one): the output size, then
// mx_conv_plan -- QS_MX_CONV_ROUTE_*, 0 for an empty problem, QS_ERR_ARG
template <class Args>
int mx_conv2d_route_of(const Args& a, MxConvPlan* plan) {
    const int64_t HP = a.H + 2 * (int64_t)a.pad_h, WP = a.W + 2 * (int64_t)a.pad_w;
    if (HP > INT32_MAX || WP > INT32_MAX) return QS_ERR_ARG;
    const int64_t EH = (int64_t)a.dil_h * (a.KH - 1) + 1, EW = (int64_t)a.dil_w * (a.KW - 1) + 1;      // extent of the dilated kernel
    if (EH > HP || EW > WP) return QS_ERR_ARG;                                                        // OH < 1 or OW < 1
    const int route = mx_conv_plan(a, (HP - EH) / a.stride_h + 1, (WP - EW) / a.stride_w + 1, plan);
    return route > 0 && mx_conv_is_gemm(a) ? QS_MX_CONV_ROUTE_GEMM : route;
}

// QS_MX_CONV_ROUTE_GEMM: the call forwarded to qs_mx_matmul_v on the same bytes
template <class Args>
int mx_conv_as_matmul(const Args& a, int64_t M) {
    const qs_mx_matmul_args m = mx_matmul_args(a.x_format, a.w_format, a.x_codes, a.x_scales, a.w_codes, a.w_scales, a.bias, a.y, a.ydt, M,
                                               a.Cout, a.C, a.stream);
    return qs_mx_matmul_v(&m);
}

}  // namespace
