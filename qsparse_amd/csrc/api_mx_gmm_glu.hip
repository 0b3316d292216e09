// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the grouped gated matrix product on MX codes (qs_mx_glu.h): group e of A times
// B[e]^T on weights of 2 H interleaved rows through the block-scaled MFMA, bias, act(gate) * up on the accumulators, then H columns as
// a float tensor or as MX codes, all 5 x 5 pairs of input formats; act and the output are kernel arguments.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation, no read of offs.
#include "qs_mx_glu.h"

namespace {

// the product [T, 2 H] as the checks the grouped products share (qs_mx_gmm.h) read it
struct GluGroupedProduct {
    int32_t a_format, b_format;
    const uint8_t *a_codes, *a_scales, *b_codes, *b_scales;
    int64_t bias_batch_stride;
    const int32_t* offs;
    int64_t T, E, N, K;
};

GluGroupedProduct mx_gmm_glu_product(const qs_mx_grouped_glu_matmul_args& a) {
    return {a.a_format, a.b_format, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias_batch_stride, a.offs, a.T, a.E, 2 * a.H, a.K};
}

// the checks of qs_mx_grouped_glu_matmul_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product,
// QS_ERR_*
int mx_gmm_glu_route(const qs_mx_grouped_glu_matmul_args& a) {
    if (!mx_glu_args_ok(a)) return QS_ERR_ARG;
    const GluGroupedProduct p = mx_gmm_glu_product(a);
    if (mx_gmm_check_operands(p) != QS_OK) return QS_ERR_ARG;
    const int st = mx_glu_check_y(a);
    if (st != QS_OK) return st;
    if ((a.bias && (((uintptr_t)a.bias) & 3u) != 0) || (((uintptr_t)a.offs) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.T == 0 || a.H == 0) return 0;
    const int route = mx_gmm_sized_route(p);
    if (route < 0) return route;
    return mx_glu_overlap(a, a.T, a.T * a.K, a.E * p.N * a.K) ? QS_ERR_ARG : route;
}

}  // namespace

extern "C" {

int qs_mx_grouped_glu_matmul_route(const qs_mx_grouped_glu_matmul_args* args) {
    qs_mx_grouped_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gmm_glu_route(a);
}

int qs_mx_grouped_glu_matmul_v(const qs_mx_grouped_glu_matmul_args* args) {
    qs_mx_grouped_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gmm_glu_route(a);
    if (route <= 0) return route;
    const int tiles_n = (int)mx_tiles(2 * a.H);
    const int64_t grid = mx_gmm_mt_max(mx_gmm_glu_product(a)) * tiles_n;
    const MxGluOut out = mx_glu_out(a);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_grouped_glu_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias,
                           a.bias_batch_stride, a.offs, (int)a.act, out, a.T, (int)a.E, a.H, a.K, tiles_n);
        return launch_status();
    });
}

}  // extern "C"
