// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the gated matrix product on MX codes (qs_mx_glu.h): A . B^T on a weight of 2 H
// interleaved rows through the block-scaled MFMA, bias, act(gate) * up on the accumulators, then H columns as a float tensor or as MX
// codes, all 5 x 5 pairs of input formats; act and the output are kernel arguments.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_glu.h"

namespace {

// the product [M, 2 H] as the checks qs_mx_matmul_v and qs_mx_matmul_q_v share (qs_mx_host.h) read it
struct GluProduct {
    int32_t a_format, b_format;
    const uint8_t *a_codes, *a_scales, *b_codes, *b_scales;
    int64_t M, N, K;
};

// the checks of qs_mx_glu_matmul_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
int mx_glu_route(const qs_mx_glu_matmul_args& a) {
    if (!mx_glu_args_ok(a)) return QS_ERR_ARG;
    const GluProduct p = {a.a_format, a.b_format, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.M, 2 * a.H, a.K};
    if (mx_gemm_check_operands(p) != QS_OK) return QS_ERR_ARG;
    const int st = mx_glu_check_y(a);
    if (st != QS_OK) return st;
    if (a.bias && (((uintptr_t)a.bias) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.M == 0 || a.H == 0) return 0;
    const int route = mx_gemm_sized_route(p);
    if (route < 0) return route;
    return mx_glu_overlap(a, a.M, a.M * a.K, p.N * a.K) ? QS_ERR_ARG : route;
}

}  // namespace

extern "C" {

int qs_mx_glu_matmul_route(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_glu_route(a);
}

int qs_mx_glu_matmul_v(const qs_mx_glu_matmul_args* args) {
    qs_mx_glu_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_glu_route(a);
    if (route <= 0) return route;
    const int tiles_n = (int)mx_tiles(2 * a.H);
    const int64_t grid = mx_tiles(a.M) * tiles_n;
    const MxGluOut out = mx_glu_out(a);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_glu_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias, (int)a.act, out,
                           a.M, a.H, a.K, tiles_n);
        return launch_status();
    });
}

}  // extern "C"
