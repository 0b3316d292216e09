// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the batched matrix product on MX codes (qs_mx_bmm.h): y[g] = A[g] . B[g]^T
// for G dense slices through the block-scaled MFMA, all 5 x 5 pairs of element formats, one launch.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_bmm.h"

namespace {

// the checks of qs_mx_bmm_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
int mx_bmm_route(const qs_mx_bmm_args& a) {
    if (!a.y || mx_bmm_check_operands(a) != QS_OK) return QS_ERR_ARG;
    if (!dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 || (a.bias && (((uintptr_t)a.bias) & 3u) != 0)) return QS_ERR_ALIGN;
    if (a.G == 0 || a.M == 0 || a.N == 0) return 0;
    return mx_bmm_sized_route(a);
}

}  // namespace

extern "C" {

int qs_mx_bmm_route(const qs_mx_bmm_args* args) {
    qs_mx_bmm_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_bmm_route(a);
}

int qs_mx_bmm_v(const qs_mx_bmm_args* args) {
    qs_mx_bmm_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_bmm_route(a);
    if (route <= 0) return route;
    if (mx_bmm_forwards(a)) {                       // (qs_mx_bmm.h, kMxbForwardTiles; the route is the one each launch takes)
        const int64_t nkb = (a.K + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
        for (int64_t g = 0; g < a.G; ++g) {
            const qs_mx_matmul_args m = mx_matmul_args(a.a_format, a.b_format, a.a_codes + g * a.M * a.K, a.a_scales + g * a.M * nkb,
                                                       a.b_codes + g * a.N * a.K, a.b_scales + g * a.N * nkb,
                                                       a.bias ? a.bias + g * a.bias_batch_stride : nullptr,
                                                       (uint8_t*)a.y + g * a.M * a.N * (int64_t)dt_size(a.ydt), a.ydt, a.M, a.N, a.K, a.stream);
            const int st = qs_mx_matmul_v(&m);
            if (st != QS_OK) return st;
        }
        return QS_OK;
    }
    const int tiles_n = (int)mx_tiles(a.N), tiles = (int)(mx_tiles(a.M) * tiles_n);
    const int64_t grid = a.G * tiles;
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_bmm_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias,
                           a.bias_batch_stride, a.y, a.ydt, a.M, a.N, a.K, tiles, tiles_n, mx_y_vec(a.y, a.ydt, a.N));
        return launch_status();
    });
}

}  // extern "C"
