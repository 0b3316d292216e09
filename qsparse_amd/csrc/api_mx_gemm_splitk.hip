// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the matrix product on MX codes split along K (qs_mx_gemm_splitk.h): partial
// products of slices of K into a caller-provided workspace, then an ordered float32 reduction.  A translation unit of its own: the
// 50 instantiations of the partial kernel compile next to the 50 of api_mx_gemm.hip, not after them.
// Host side: argument checks, the slicing and the automatic slice count, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_gemm_splitk.h"

namespace {

constexpr int64_t kSplitMax = 16;    // the most slices the automatic rule asks for

qs_mx_matmul_args unsplit_args(const qs_mx_matmul_splitk_args& a) {
    return mx_matmul_args(a.a_format, a.b_format, a.a_codes, a.a_scales, a.b_codes, a.b_scales, a.bias, a.y, a.ydt, a.M, a.N, a.K, a.stream);
}

// the checks of qs_mx_matmul_splitk_v and the kernel its first launch runs: every check of qs_mx_matmul_v (by asking it), then the
// request and the workspace.  QS_MX_GEMM_ROUTE_*, 0 for an empty product, QS_ERR_*
int splitk_route(const qs_mx_matmul_splitk_args& a, SplitPlan* p) {
    const qs_mx_matmul_args m = unsplit_args(a);
    const int route = qs_mx_matmul_route(&m);
    if (route < 0) return route;
    if (a.split_k < 1) return QS_ERR_ARG;
    if (route == 0) return 0;
    const int st = split_plan(a.M, a.N, a.K, a.split_k, kSplitMax, p);
    if (st != QS_OK) return st;
    if (p->slices == 1) return route;              // forwarded to qs_mx_matmul_v: no workspace
    const int64_t tiles = mx_tiles(a.M) * mx_tiles(a.N);       // <= kMaxGrid (qs_mx_matmul_route)
    const int ws = split_workspace_status(*p, a.workspace, a.workspace_bytes, tiles);
    return ws != QS_OK ? ws : route;
}

// the two launches: the partial products of every slice, then their ordered sum
int launch_split(const qs_mx_matmul_splitk_args& a, const SplitPlan& p, int route) {
    const int tiles_n = (int)mx_tiles(a.N);
    const int tiles = (int)mx_tiles(a.M) * tiles_n;
    const int64_t grid = (int64_t)tiles * p.slices;
    const int ws_vec = a.N % 4 == 0;               // every row of every slice then keeps the workspace's 16-byte alignment
    float* ws = (float*)a.workspace;
    hipStream_t s = (hipStream_t)a.stream;
    const int st = mx_dispatch(a.a_format, a.b_format, route == QS_MX_GEMM_ROUTE_VEC, [&](auto FA, auto FB, auto VEC) {
        hipLaunchKernelGGL((mx_gemm_partial_kernel<decltype(FA)::value, decltype(FB)::value, decltype(VEC)::value>), dim3((unsigned)grid),
                           dim3(kMxgThreads), 0, s, a.a_codes, a.a_scales, a.b_codes, a.b_scales, ws, a.M, a.N, a.K, tiles_n, tiles, p.per,
                           ws_vec);
        return launch_status();
    });
    if (st != 0) return st;
    return mx_launch_reduce(ws, a.bias, a.y, a.ydt, a.M, a.N, p.slices, s);
}

}  // namespace

extern "C" {

int qs_mx_matmul_splitk_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int32_t* slices, uint64_t* workspace_bytes) {
    return split_plan_out(M, N, K, split_k, kSplitMax, slices, workspace_bytes);
}

int qs_mx_matmul_splitk_route(const qs_mx_matmul_splitk_args* args) {
    qs_mx_matmul_splitk_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    SplitPlan p;
    return splitk_route(a, &p);
}

int qs_mx_matmul_splitk_v(const qs_mx_matmul_splitk_args* args) {
    qs_mx_matmul_splitk_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    SplitPlan p;
    const int route = splitk_route(a, &p);
    if (route <= 0) return route;
    if (p.slices == 1) {
        const qs_mx_matmul_args m = unsplit_args(a);
        return qs_mx_matmul_v(&m);
    }
    return launch_split(a, p, route);
}

}  // extern "C"
