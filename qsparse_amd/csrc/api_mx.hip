// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the MX block-scaled quantizer forward (qs_mx.h): FP8 / FP6 / FP4 elements
// with one E8M0 scale per block of 32 (OCP Microscaling Formats v1.0), rounded to nearest-even or stochastically (the descriptor's
// `rounding`: the same routes and kernels, instantiated with SR = true).
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx.h"

namespace {

inline bool aligned_to(const void* p, size_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// the checks of qs_mx_quant_fwd_v and the kernel it launches for these operands: QS_MX_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_route(const qs_mx_quant_args& a) {
    if (const int st = mx_sr_check(a.rounding, a.step, a.index_base)) return st;
    if (!a.x || !a.y || !mx_format_ok(a.format)) return QS_ERR_ARG;
    if (a.outer < 0 || a.n < 0 || a.inner < 0) return QS_ERR_ARG;
    if (!dt_ok(a.xdt) || !dt_ok(a.ydt) || !(a.ydt == QS_F32 || a.ydt == a.xdt)) return QS_ERR_DTYPE;
    if (!aligned_to(a.x, dt_size(a.xdt)) || !aligned_to(a.y, dt_size(a.ydt))) return QS_ERR_ALIGN;
    if (a.outer == 0 || a.n == 0 || a.inner == 0) return 0;
    if (a.outer > INT64_MAX / a.n || a.outer * a.n > INT64_MAX / a.inner) return QS_ERR_ARG;
    if (a.inner > 1) return QS_MX_ROUTE_STRIDED;
    if (a.n % QS_MX_BLOCK == 0 && aligned16(a.x) && aligned16(a.y) && (!a.codes || aligned16(a.codes))) return QS_MX_ROUTE_INNER_VEC;
    return QS_MX_ROUTE_INNER_PLAIN;
}

template <bool SR>
int mx_launch(const qs_mx_quant_args& a, int route) {
    const MxSr sr = SR ? MxSr{a.seed, a.step, a.index_base, (uint32_t)a.rng_stream} : MxSr{};
    const int64_t numel = a.outer * a.n * a.inner;
    const int64_t nb = (a.n + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
    const MxFormat f = mx_format(a.format);
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        if (route == QS_MX_ROUTE_INNER_VEC) {
            constexpr int64_t per_wg = (int64_t)kMxBlock * (XD == QS_F32 ? 4 : 8);
            const int64_t grid = (numel + per_wg - 1) / per_wg;
            if (grid > kMaxGrid) return (int)QS_ERR_ARG;
            hipLaunchKernelGGL((mx_inner_vec_kernel<XD, SR>), dim3((unsigned)grid), dim3(kMxBlock), 0, s, f, a.x, a.y, a.codes, a.scales,
                               numel, a.ydt, sr);
            return launch_status();
        }
        if (route == QS_MX_ROUTE_INNER_PLAIN) {
            const int64_t nblocks = a.outer * nb;
            const int64_t grid = (nblocks + kMxBlock / 32 - 1) / (kMxBlock / 32);
            if (grid > kMaxGrid) return (int)QS_ERR_ARG;
            hipLaunchKernelGGL((mx_inner_plain_kernel<XD, SR>), dim3((unsigned)grid), dim3(kMxBlock), 0, s, f, a.x, a.y, a.codes, a.scales,
                               nblocks, a.n, nb, a.ydt, sr);
            return launch_status();
        }
        const int64_t total = a.outer * nb * a.inner;
        const int64_t grid = (total + kMxBlock - 1) / kMxBlock;
        if (grid > kMaxGrid) return (int)QS_ERR_ARG;
        hipLaunchKernelGGL((mx_strided_kernel<XD, SR>), dim3((unsigned)grid), dim3(kMxBlock), 0, s, f, a.x, a.y, a.codes, a.scales, total, a.n,
                           a.inner, nb, a.ydt, sr);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_quant_route(const qs_mx_quant_args* args) {
    qs_mx_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_route(a);
}

int qs_mx_quant_fwd_v(const qs_mx_quant_args* args) {
    qs_mx_quant_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_route(a);
    if (route <= 0) return route;
    return a.rounding == QS_MX_ROUND_STOCHASTIC ? mx_launch<true>(a, route) : mx_launch<false>(a, route);
}

// the v27 names of the two entry points above
int qs_mx_quant_sr_route(const qs_mx_quant_sr_args* args) { return qs_mx_quant_route(args); }
int qs_mx_quant_sr_v(const qs_mx_quant_sr_args* args) { return qs_mx_quant_fwd_v(args); }

}  // extern "C"
