// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the batched matrix product on MX codes that writes MX codes (qs_mx_bmm.h):
// A[g] . B[g]^T through the block-scaled MFMA, bias, optional ReLU and the MX quantizer of the output in one kernel, all 5 x 5 pairs
// of input formats; the output format is a kernel argument.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_bmm.h"

namespace {

// the checks of qs_mx_bmm_q_v and the kernel it launches for these operands: QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
int mx_bmm_q_route(const qs_mx_bmm_q_args& a) {
    if (mx_bmm_check_operands(a) != QS_OK || !mx_q_args_ok(a)) return QS_ERR_ARG;
    if (a.bias && (((uintptr_t)a.bias) & 3u) != 0) return QS_ERR_ALIGN;
    if (a.G == 0 || a.M == 0 || a.N == 0) return 0;
    const int route = mx_bmm_sized_route(a);
    if (route < 0) return route;
    const int64_t out = a.G * a.M * a.N;            // byte counts over all slices
    if (mx_overlap(a.out_codes, out, a.a_codes, a.G * a.M * a.K) || mx_overlap(a.out_codes, out, a.b_codes, a.G * a.N * a.K)) return QS_ERR_ARG;
    return route;
}

}  // namespace

extern "C" {

int qs_mx_bmm_q_route(const qs_mx_bmm_q_args* args) {
    qs_mx_bmm_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_bmm_q_route(a);
}

int qs_mx_bmm_q_v(const qs_mx_bmm_q_args* args) {
    qs_mx_bmm_q_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_bmm_q_route(a);
    if (route <= 0) return route;
    if (mx_bmm_forwards(a)) {                       // (qs_mx_bmm.h, kMxbForwardTiles; the route is the one each launch takes)
        const int64_t nkb = (a.K + QS_MX_BLOCK - 1) / QS_MX_BLOCK, nnb = (a.N + QS_MX_BLOCK - 1) / QS_MX_BLOCK;
        for (int64_t g = 0; g < a.G; ++g) {
            qs_mx_matmul_q_args m = {};
            m.struct_size = sizeof(m);
            m.a_format = a.a_format, m.b_format = a.b_format;
            m.a_codes = a.a_codes + g * a.M * a.K, m.a_scales = a.a_scales + g * a.M * nkb;
            m.b_codes = a.b_codes + g * a.N * a.K, m.b_scales = a.b_scales + g * a.N * nkb;
            m.bias = a.bias ? a.bias + g * a.bias_batch_stride : nullptr;
            m.out_format = a.out_format, m.act = a.act;
            m.out_codes = a.out_codes + g * a.M * a.N, m.out_scales = a.out_scales + g * a.M * nnb;
            m.M = a.M, m.N = a.N, m.K = a.K;
            m.stream = a.stream;
            const int st = qs_mx_matmul_q_v(&m);
            if (st != QS_OK) return st;
        }
        return QS_OK;
    }
    const int tiles_n = (int)mx_tiles(a.N), tiles = (int)(mx_tiles(a.M) * tiles_n);
    const int64_t grid = a.G * tiles;
    const MxFormat f = mx_format(a.out_format);
    return mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_bmm_q_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, (hipStream_t)a.stream, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias,
                           a.bias_batch_stride, (int)(a.act == QS_MX_ACT_RELU), f, a.out_codes, a.out_scales, a.M, a.N, a.K, tiles, tiles_n,
                           mx_c_vec(a.out_codes, a.N));
        return launch_status();
    });
}

}  // extern "C"
