// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the backward of the normalisation in front of the MX quantizer
// (qs_mx_norm_bwd.h): the row statistics c1 / c2 of dxhat [R, C] and x in one launch, dx and the row tiles' column sums in a second,
// dweight / dbias from those partial sums in a third -- each launch only when an output that needs it is asked for.  With the
// residual stream's gradient (qs_mx_norm_bwd_res_v) the second launch adds it to dx in front of dx's one rounding.
// Host side: argument checks, workspace layout, route, launch configuration.  No allocation, no synchronisation.
#include <stddef.h>

#include "qs_mx_quant2_host.h"
#include "qs_mx_norm_bwd.h"

namespace {

inline uint64_t up16(uint64_t n) { return (n + 15u) & ~(uint64_t)15u; }

// the workspace: c1 [R] and, in layer mode, c2 [R] when dx is asked for; the partials of dweight and of dbias, [ceil(R / 128), C]
// each, when either is -- float32, every part at a multiple of 16 bytes
struct NormBwdPlan {
    uint64_t c1, c2, pw, pb, bytes;
};

// QS_ERR_ARG for extents the launches cannot take (checked before any byte count is formed)
int norm_bwd_plan(int64_t R, int64_t C, bool layer, bool need_dx, bool need_cols, NormBwdPlan* out) {
    *out = NormBwdPlan{};
    if (R < 0 || C < 0) return QS_ERR_ARG;
    if (R == 0 || C == 0) return 0;
    if (R > INT64_MAX / C) return QS_ERR_ARG;
    const int64_t tiles_r = mxq2_tiles_r(R);
    if (!mxq2_grid_ok(R, C) || (R + kMxnStatRows - 1) / kMxnStatRows > kMaxGrid) return QS_ERR_ARG;
    uint64_t at = 0;
    if (need_dx) {
        out->c1 = at;
        at += up16((uint64_t)R * 4);
        if (layer) {
            out->c2 = at;
            at += up16((uint64_t)R * 4);
        }
    }
    if (need_cols) {
        const uint64_t part = up16((uint64_t)tiles_r * (uint64_t)C * 4);
        out->pw = at;
        out->pb = at + part;
        at += 2 * part;
    }
    out->bytes = at;
    return 0;
}

// qs_mx_norm_bwd_args as the descriptor with the residual stream's gradient, which it has not: the two agree field for field up to
// `stream` (static_assert below), and both entry points run the one set of checks and launches on the longer one
qs_mx_norm_bwd_res_args with_no_residual(const qs_mx_norm_bwd_args& b) {
    static_assert(offsetof(qs_mx_norm_bwd_res_args, dresidual) == sizeof(qs_mx_norm_bwd_args), "the shared fields are a prefix");
    qs_mx_norm_bwd_res_args a{};
    memcpy(&a, &b, sizeof(b));
    a.struct_size = sizeof(a);
    return a;
}

// the checks of qs_mx_norm_bwd_v / qs_mx_norm_bwd_res_v and the kernels it launches for these operands: QS_MX_NORM_BWD_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int norm_bwd_route(const qs_mx_norm_bwd_res_args& a, NormBwdPlan* plan) {
    const bool layer = a.mode == QS_MX_NORM_LAYER;
    if (a.mode != QS_MX_NORM_RMS && !layer) return QS_ERR_ARG;
    if (!a.dxhat || !a.x || !a.rstd || (layer && !a.mean)) return QS_ERR_ARG;
    if (!a.dx && !a.dweight && !a.dbias) return QS_ERR_ARG;
    if (a.dresidual && !a.dx) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt) || !dt_ok(a.gdt)) return QS_ERR_DTYPE;
    const uintptr_t xm = dt_size(a.xdt) - 1, gm = dt_size(a.gdt) - 1;
    if ((((uintptr_t)a.x) & xm) != 0 || (((uintptr_t)a.dx) & xm) != 0 || (((uintptr_t)a.dresidual) & xm) != 0 ||
        (((uintptr_t)a.dxhat) & gm) != 0 || !aligned4(a.weight) ||
        !aligned4(a.rstd) || (layer && !aligned4(a.mean)) || !aligned4(a.dweight) || !aligned4(a.dbias) || !aligned16(a.workspace))
        return QS_ERR_ALIGN;
    const int st = norm_bwd_plan(a.R, a.C, layer, a.dx != nullptr, a.dweight || a.dbias, plan);
    if (st != 0 || a.R == 0 || a.C == 0) return st;
    if (!a.workspace || a.workspace_bytes < plan->bytes) return QS_ERR_WORKSPACE;
    const bool vec = a.C % QS_MX_BLOCK == 0 && aligned16(a.dxhat) && aligned16(a.x) && aligned16(a.weight) && aligned16(a.dx) &&
                     aligned16(a.dresidual);
    return vec ? QS_MX_NORM_BWD_ROUTE_VEC : QS_MX_NORM_BWD_ROUTE_PLAIN;
}

template <int XD, int GD, bool VEC>
void norm_bwd_enqueue(const qs_mx_norm_bwd_res_args& a, const NormBwdPlan& plan) {
    const bool layer = a.mode == QS_MX_NORM_LAYER, cols = a.dweight || a.dbias;
    char* ws = (char*)a.workspace;
    const float* mean = layer ? a.mean : nullptr;
    float* c1 = a.dx ? (float*)(ws + plan.c1) : nullptr;
    float* c2 = (a.dx && layer) ? (float*)(ws + plan.c2) : nullptr;
    float* pw = a.dweight ? (float*)(ws + plan.pw) : nullptr;
    float* pb = a.dbias ? (float*)(ws + plan.pb) : nullptr;
    const int64_t tiles_r = mxq2_tiles_r(a.R);
    const int tiles_c = (int)mxq2_tiles_c(a.C);
    hipStream_t s = (hipStream_t)a.stream;
    if (a.dx)
        hipLaunchKernelGGL((mx_norm_bwd_stats_kernel<XD, GD, VEC>), dim3((unsigned)((a.R + kMxnStatRows - 1) / kMxnStatRows)),
                           dim3(kMxq2Threads), 0, s, a.dxhat, a.x, a.weight, a.rstd, mean, c1, c2, a.R, a.C);
    const dim3 grid((unsigned)(tiles_r * tiles_c));
    if (a.dresidual)
        hipLaunchKernelGGL((mx_norm_bwd_apply_kernel<XD, GD, VEC, true>), grid, dim3(kMxq2Threads), 0, s, a.dxhat, a.x, a.weight, a.rstd,
                           mean, (const float*)c1, (const float*)c2, a.dx, pw, pb, a.R, a.C, tiles_c, a.dresidual);
    else
        hipLaunchKernelGGL((mx_norm_bwd_apply_kernel<XD, GD, VEC>), grid, dim3(kMxq2Threads), 0, s, a.dxhat, a.x, a.weight, a.rstd, mean,
                           (const float*)c1, (const float*)c2, a.dx, pw, pb, a.R, a.C, tiles_c);
    if (cols)
        hipLaunchKernelGGL(mx_norm_bwd_fold_kernel, dim3((unsigned)((a.C + kMxnbFoldCols - 1) / kMxnbFoldCols), 2), dim3(kMxq2Threads),
                           0, s, (const float*)pw, (const float*)pb, a.dweight, a.dbias, tiles_r, a.C);
}

int norm_bwd_launch(const qs_mx_norm_bwd_res_args& a, const NormBwdPlan& plan, int route) {
    return with_dtype(a.xdt, [&](auto X) {
        return with_dtype(a.gdt, [&](auto G) {
            constexpr int XD = decltype(X)::value, GD = decltype(G)::value;
            if (route == QS_MX_NORM_BWD_ROUTE_VEC) norm_bwd_enqueue<XD, GD, true>(a, plan);
            else norm_bwd_enqueue<XD, GD, false>(a, plan);
            return launch_status();
        });
    });
}

}  // namespace

extern "C" {

int qs_mx_norm_bwd_plan(int64_t R, int64_t C, int32_t mode, int32_t need_dx, int32_t need_cols, uint64_t* workspace_bytes) {
    if (!workspace_bytes || (mode != QS_MX_NORM_RMS && mode != QS_MX_NORM_LAYER)) return QS_ERR_ARG;
    NormBwdPlan plan;
    const int st = norm_bwd_plan(R, C, mode == QS_MX_NORM_LAYER, need_dx != 0, need_cols != 0, &plan);
    *workspace_bytes = plan.bytes;
    return st;
}

int qs_mx_norm_bwd_route(const qs_mx_norm_bwd_args* args) {
    qs_mx_norm_bwd_args a;
    NormBwdPlan plan;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return norm_bwd_route(with_no_residual(a), &plan);
}

int qs_mx_norm_bwd_v(const qs_mx_norm_bwd_args* args) {
    qs_mx_norm_bwd_args a;
    NormBwdPlan plan;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const qs_mx_norm_bwd_res_args r = with_no_residual(a);
    const int route = norm_bwd_route(r, &plan);
    if (route <= 0) return route;
    return norm_bwd_launch(r, plan, route);
}

int qs_mx_norm_bwd_res_route(const qs_mx_norm_bwd_res_args* args) {
    qs_mx_norm_bwd_res_args a;
    NormBwdPlan plan;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return norm_bwd_route(a, &plan);
}

int qs_mx_norm_bwd_res_v(const qs_mx_norm_bwd_res_args* args) {
    qs_mx_norm_bwd_res_args a;
    NormBwdPlan plan;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = norm_bwd_route(a, &plan);
    if (route <= 0) return route;
    return norm_bwd_launch(a, plan, route);
}

}  // extern "C"
