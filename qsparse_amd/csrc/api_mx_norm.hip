// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), RMSNorm / LayerNorm in front of the MX quantizer (qs_mx_norm.h): the row
// statistics of x [R, C] in one launch, then the codes and E8M0 scales of y = norm(x) * w (+ b) with blocks along C and -- stored
// transposed, when asked for -- with blocks along R in a second one.  y is never written.  The add-norm quantizer is the same two
// launches with a statistics kernel that forms and stores h = x + residual first, and the quantizing launch on h.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"
#include "qs_mx_norm.h"

namespace {

// what qs_mx_add_norm_quant_args has beyond qs_mx_norm_quant_args
struct NormAdd {
    const void* residual;
    void* h;
    int rdt;
};

// the checks of qs_mx_norm_quant_v -- with `add`, of qs_mx_add_norm_quant_v -- and the kernels it launches for these operands:
// QS_MX_NORM_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_norm_route(const qs_mx_norm_quant_args& a, const NormAdd* add = nullptr) {
    const bool layer = a.mode == QS_MX_NORM_LAYER;
    if (a.mode != QS_MX_NORM_RMS && !layer) return QS_ERR_ARG;
    if (!a.x || (add && (!add->residual || !add->h)) || !a.rstd || (layer && !a.mean) || !mxq2_pairs_by_format(a, true).ok) return QS_ERR_ARG;
    if (!(a.eps >= 0.0f) || a.eps > 3.0e38f) return QS_ERR_ARG;                  // (also refuses a NaN)
    if (a.R < 0 || a.C < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt) || (add && !dt_ok(add->rdt))) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0 || !aligned4(a.weight) || !aligned4(a.bias) || !aligned4(a.rstd) ||
        (layer && !aligned4(a.mean)))
        return QS_ERR_ALIGN;
    if (add && (((uintptr_t)add->residual | (uintptr_t)add->h) & (dt_size(add->rdt) - 1)) != 0) return QS_ERR_ALIGN;
    if (a.R == 0 || a.C == 0) return 0;
    if (a.R > INT64_MAX / a.C || !mxq2_grid_ok(a.R, a.C)) return QS_ERR_ARG;
    if (add && (a.R + kMxnStatRows - 1) / kMxnStatRows > kMaxGrid) return QS_ERR_ARG;
    const bool vec = a.C % QS_MX_BLOCK == 0 && aligned16(a.x) && aligned16(a.weight) && aligned16(a.bias) &&
                     (!add || (aligned16(add->residual) && aligned16(add->h)));
    return vec ? QS_MX_NORM_ROUTE_VEC : QS_MX_NORM_ROUTE_PLAIN;
}

// the quantizing launch on `x` of dtype `xdt` ([R, C] of `a`; the add-norm quantizer's h)
template <bool VEC>
void mx_norm_apply_enqueue(const qs_mx_norm_quant_args& a, const void* x, int xdt) {
    const bool layer = a.mode == QS_MX_NORM_LAYER, col = a.col_format != -1;
    const Mxq2Launch l = mxq2_launch(a, true, col, a.R, a.C);
    const float* mean = layer ? a.mean : nullptr;
    const int row_vec = VEC && mxq2_row_vec(l, 4), col_vec = VEC && col && a.R % 16 == 0 && aligned16(l.col_codes);
    with_dtype(xdt, [&](auto X) {
        hipLaunchKernelGGL((mx_norm_apply_kernel<decltype(X)::value, VEC>), dim3((unsigned)l.tiles), dim3(kMxq2Threads), 0,
                           (hipStream_t)a.stream, l.fr, l.fc, x, a.weight, a.bias, (const float*)a.rstd, mean, l.row_codes, l.row_scales,
                           l.col_codes, l.col_scales, a.R, a.C, l.tiles_c, row_vec, col_vec);
        return 0;
    });
}

template <bool VEC>
int mx_norm_enqueue(const qs_mx_norm_quant_args& a, const NormAdd* add) {
    float* mean = a.mode == QS_MX_NORM_LAYER ? a.mean : nullptr;
    const dim3 sgrid((unsigned)((a.R + kMxnStatRows - 1) / kMxnStatRows));
    hipStream_t s = (hipStream_t)a.stream;
    with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        if (!add) {
            hipLaunchKernelGGL((mx_norm_stats_kernel<XD, VEC>), sgrid, dim3(kMxq2Threads), 0, s, a.x, a.rstd, mean, a.R, a.C, a.eps);
            return 0;
        }
        return with_dtype(add->rdt, [&](auto Rd) {
            hipLaunchKernelGGL((mx_add_norm_stats_kernel<XD, decltype(Rd)::value, VEC>), sgrid, dim3(kMxq2Threads), 0, s, a.x,
                               add->residual, add->h, a.rstd, mean, a.R, a.C, a.eps);
            return 0;
        });
    });
    if (add) mx_norm_apply_enqueue<VEC>(a, add->h, add->rdt);
    else mx_norm_apply_enqueue<VEC>(a, a.x, a.xdt);
    return launch_status();
}

int mx_norm_launch(const qs_mx_norm_quant_args& a, int route, const NormAdd* add = nullptr) {
    return route == QS_MX_NORM_ROUTE_VEC ? mx_norm_enqueue<true>(a, add) : mx_norm_enqueue<false>(a, add);
}

// the fields qs_mx_add_norm_quant_args shares with qs_mx_norm_quant_args, and the rest
qs_mx_norm_quant_args norm_part(const qs_mx_add_norm_quant_args& q, NormAdd* add) {
    qs_mx_norm_quant_args a{};
    a.struct_size = sizeof(a);
    a.mode = q.mode, a.row_format = q.row_format, a.col_format = q.col_format, a.xdt = q.xdt, a.eps = q.eps;
    a.x = q.x, a.weight = q.weight, a.bias = q.bias;
    a.row_codes = q.row_codes, a.row_scales = q.row_scales, a.col_codes = q.col_codes, a.col_scales = q.col_scales;
    a.rstd = q.rstd, a.mean = q.mean, a.R = q.R, a.C = q.C, a.stream = q.stream;
    *add = NormAdd{q.residual, q.h, q.rdt};
    return a;
}

}  // namespace

extern "C" {

int qs_mx_norm_quant_route(const qs_mx_norm_quant_args* args) {
    qs_mx_norm_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_norm_route(a);
}

int qs_mx_norm_quant_v(const qs_mx_norm_quant_args* args) {
    qs_mx_norm_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_norm_route(a);
    if (route <= 0) return route;
    return mx_norm_launch(a, route);
}

int qs_mx_add_norm_quant_route(const qs_mx_add_norm_quant_args* args) {
    qs_mx_add_norm_quant_args q;
    NormAdd add;
    if (!take_args(args, &q)) return QS_ERR_ARG;
    return mx_norm_route(norm_part(q, &add), &add);
}

int qs_mx_add_norm_quant_v(const qs_mx_add_norm_quant_args* args) {
    qs_mx_add_norm_quant_args q;
    NormAdd add;
    if (!take_args(args, &q)) return QS_ERR_ARG;
    const qs_mx_norm_quant_args a = norm_part(q, &add);
    const int route = mx_norm_route(a, &add);
    if (route <= 0) return route;
    return mx_norm_launch(a, route, &add);
}

}  // extern "C"
