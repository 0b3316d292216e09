// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the grouped matrix product on MX codes (qs_mx_gmm.h): the rows of A [T, K] in
// E consecutive groups whose boundaries lie in device memory, group e times its own weight B[e]^T, through the block-scaled MFMA,
// all 5 x 5 pairs of element formats, one launch.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation, no read of offs.
#include "qs_mx_gmm.h"

namespace {

// the checks of qs_mx_grouped_matmul_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product,
// QS_ERR_*
int mx_gmm_route(const qs_mx_grouped_matmul_args& a) {
    if (!a.y || mx_gmm_check_operands(a) != QS_OK) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (a.bias && (((uintptr_t)a.bias) & 3u) != 0) || (((uintptr_t)a.offs) & 3u) != 0)
        return QS_ERR_ALIGN;
    if (a.T == 0 || a.N == 0) return 0;
    return mx_gmm_sized_route(a);
}

}  // namespace

extern "C" {

int qs_mx_grouped_matmul_route(const qs_mx_grouped_matmul_args* args) {
    qs_mx_grouped_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gmm_route(a);
}

int qs_mx_grouped_matmul_v(const qs_mx_grouped_matmul_args* args) {
    qs_mx_grouped_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gmm_route(a);
    if (route <= 0) return route;
    const int tiles_n = (int)mx_tiles(a.N);
    const int64_t grid = mx_gmm_mt_max(a) * tiles_n;
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_gmm_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias,
                           a.bias_batch_stride, a.offs, a.y, a.ydt, a.T, (int)a.E, a.N, a.K, tiles_n, mx_y_vec(a.y, a.ydt, a.N));
        return launch_status();
    });
}

}  // extern "C"
