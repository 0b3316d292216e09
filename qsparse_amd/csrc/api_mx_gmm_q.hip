// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the grouped matrix product on MX codes that writes MX codes (qs_mx_gmm.h):
// group e of A times B[e]^T through the block-scaled MFMA, bias, optional ReLU and the MX quantizer of the output in one kernel, all
// 5 x 5 pairs of input formats; the output format is a kernel argument.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation, no read of offs.
#include "qs_mx_gmm.h"

namespace {

// the checks of qs_mx_grouped_matmul_q_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product,
// QS_ERR_*
int mx_gmm_q_route(const qs_mx_grouped_matmul_q_args& a) {
    if (mx_gmm_check_operands(a) != QS_OK || !mx_q_args_ok(a)) return QS_ERR_ARG;
    if ((a.bias && (((uintptr_t)a.bias) & 3u) != 0) || (((uintptr_t)a.offs) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.T == 0 || a.N == 0) return 0;
    const int route = mx_gmm_sized_route(a);
    if (route < 0) return route;
    const int64_t out = a.T * a.N;                  // byte counts over all rows and all weights
    if (mx_overlap(a.out_codes, out, a.a_codes, a.T * a.K)) return QS_ERR_ARG;
    if (a.E > 0 && mx_overlap(a.out_codes, out, a.b_codes, a.E * a.N * a.K)) return QS_ERR_ARG;
    return route;
}

}  // namespace

extern "C" {

int qs_mx_grouped_matmul_q_route(const qs_mx_grouped_matmul_q_args* args) {
    qs_mx_grouped_matmul_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gmm_q_route(a);
}

int qs_mx_grouped_matmul_q_v(const qs_mx_grouped_matmul_q_args* args) {
    qs_mx_grouped_matmul_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gmm_q_route(a);
    if (route <= 0) return route;
    const int tiles_n = (int)mx_tiles(a.N);
    const int64_t grid = mx_gmm_mt_max(a) * tiles_n;
    const MxFormat f = mx_format(a.out_format);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_gmm_q_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias,
                           a.bias_batch_stride, a.offs, (int)(a.act == QS_MX_ACT_RELU), f, a.out_codes, a.out_scales, a.T, (int)a.E, a.N,
                           a.K, tiles_n, mx_c_vec(a.out_codes, a.N));
        return launch_status();
    });
}

}  // extern "C"
