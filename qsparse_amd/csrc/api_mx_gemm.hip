// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the matrix product on MX codes (qs_mx_gemm.h): y = A . B^T through the
// block-scaled MFMA, all 5 x 5 pairs of element formats.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_gemm.h"

namespace {

// the checks of qs_mx_matmul_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
int mx_gemm_route(const qs_mx_matmul_args& a) {
    if (!a.a_codes || !a.a_scales || !a.b_codes || !a.b_scales || !a.y) return QS_ERR_ARG;
    if (!mx_format_ok(a.a_format) || !mx_format_ok(a.b_format)) return QS_ERR_ARG;
    if (a.M < 0 || a.N < 0 || a.K < 0) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (a.bias && (((uintptr_t)a.bias) & 3u) != 0)) return QS_ERR_ALIGN;
    if (a.M == 0 || a.N == 0) return 0;
    if (a.K == 0 || a.M > INT64_MAX / a.N || a.M > INT64_MAX / a.K || a.N > INT64_MAX / a.K) return QS_ERR_ARG;
    const int64_t tiles = ((a.M + kMxgTile - 1) / kMxgTile) * ((a.N + kMxgTile - 1) / kMxgTile);
    if (tiles > kMaxGrid) return QS_ERR_ARG;
    return (a.K % 16 == 0 && aligned16(a.a_codes) && aligned16(a.b_codes)) ? QS_MX_GEMM_ROUTE_VEC : QS_MX_GEMM_ROUTE_PLAIN;
}

template <int FA, int FB>
int launch_pair(const qs_mx_matmul_args& a, int route) {
    const int tiles_n = (int)((a.N + kMxgTile - 1) / kMxgTile);
    const int64_t grid = ((a.M + kMxgTile - 1) / kMxgTile) * tiles_n;
    // four consecutive n per lane in one store: every row of y must keep the store's alignment
    const int y_vec = a.N % 4 == 0 && (((uintptr_t)a.y) & (4 * dt_size(a.ydt) - 1)) == 0;
    hipStream_t s = (hipStream_t)a.stream;
    if (route == QS_MX_GEMM_ROUTE_VEC)
        hipLaunchKernelGGL((mx_gemm_kernel<FA, FB, true>), dim3((unsigned)grid), dim3(kMxgThreads), 0, s, a.a_codes, a.a_scales, a.b_codes,
                           a.b_scales, a.bias, a.y, a.ydt, a.M, a.N, a.K, tiles_n, y_vec);
    else
        hipLaunchKernelGGL((mx_gemm_kernel<FA, FB, false>), dim3((unsigned)grid), dim3(kMxgThreads), 0, s, a.a_codes, a.a_scales, a.b_codes,
                           a.b_scales, a.bias, a.y, a.ydt, a.M, a.N, a.K, tiles_n, y_vec);
    return launch_status();
}

template <int FA>
int launch_a(const qs_mx_matmul_args& a, int route) {
    switch (a.b_format) {
        case QS_MX_FP8_E4M3: return launch_pair<FA, QS_MX_FP8_E4M3>(a, route);
        case QS_MX_FP8_E5M2: return launch_pair<FA, QS_MX_FP8_E5M2>(a, route);
        case QS_MX_FP6_E2M3: return launch_pair<FA, QS_MX_FP6_E2M3>(a, route);
        case QS_MX_FP6_E3M2: return launch_pair<FA, QS_MX_FP6_E3M2>(a, route);
        default: return launch_pair<FA, QS_MX_FP4_E2M1>(a, route);
    }
}

}  // namespace

extern "C" {

int qs_mx_matmul_route(const qs_mx_matmul_args* args) {
    qs_mx_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_gemm_route(a);
}

int qs_mx_matmul_v(const qs_mx_matmul_args* args) {
    qs_mx_matmul_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_gemm_route(a);
    if (route <= 0) return route;
    switch (a.a_format) {
        case QS_MX_FP8_E4M3: return launch_a<QS_MX_FP8_E4M3>(a, route);
        case QS_MX_FP8_E5M2: return launch_a<QS_MX_FP8_E5M2>(a, route);
        case QS_MX_FP6_E2M3: return launch_a<QS_MX_FP6_E2M3>(a, route);
        case QS_MX_FP6_E3M2: return launch_a<QS_MX_FP6_E3M2>(a, route);
        default: return launch_a<QS_MX_FP4_E2M1>(a, route);
    }
}

}  // extern "C"
