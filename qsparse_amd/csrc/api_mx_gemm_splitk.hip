// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the matrix product on MX codes split along K (qs_mx_gemm_splitk.h): partial
// products of slices of K into a caller-provided workspace, then an ordered float32 reduction.  A translation unit of its own: the
// 50 instantiations of the partial kernel compile next to the 50 of api_mx_gemm.hip, not after them.
// Host side: argument checks, the slicing and the automatic slice count, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_host.h"
#include "qs_mx_gemm_splitk.h"

namespace {

// ---- the automatic slice count (qs_mx_matmul_splitk_plan, split_k == 0): a pure function of (M, N, K) --------------------------------
constexpr int64_t kSplitMinSteps = 32;     // fewer K-steps than this: never split
constexpr int64_t kSplitFullTiles = 256;   // this many output tiles (one per CU) or more: never split
constexpr int64_t kSplitGroups = 512;      // work-groups aimed at: two co-resident per CU at 64 KiB of LDS each
constexpr int64_t kSplitStepsPerSlice = 8; // a slice keeps at least this many K-steps
constexpr int64_t kSplitMax = 16;

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

int64_t auto_split(int64_t M, int64_t N, int64_t K) {
    const int64_t tiles = cdiv(M, kMxgTile) * cdiv(N, kMxgTile), steps = cdiv(K, kMxgK);
    if (steps < kSplitMinSteps || tiles >= kSplitFullTiles) return 1;
    return std::max<int64_t>(1, std::min({kSplitGroups / tiles, steps / kSplitStepsPerSlice, kSplitMax}));
}

struct SplitPlan {
    int64_t per;          // K-steps per slice
    int32_t slices;       // S': no slice is empty
    uint64_t bytes;       // of the workspace; 0 when slices == 1
};

// QS_OK and the plan, or QS_ERR_ARG (a negative extent or request, K == 0 of a non-empty product, a byte count beyond 64 bits)
int split_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, SplitPlan* p) {
    if (M < 0 || N < 0 || K < 0 || split_k < 0) return QS_ERR_ARG;
    *p = SplitPlan{0, 1, 0};
    if (M == 0 || N == 0) return QS_OK;
    if (K == 0 || M > INT64_MAX / N) return QS_ERR_ARG;
    const int64_t steps = cdiv(K, kMxgK);
    const int64_t S = split_k == 0 ? auto_split(M, N, K) : split_k;
    p->per = cdiv(steps, S);
    p->slices = (int32_t)cdiv(steps, p->per);      // <= S <= INT32_MAX
    if (p->slices > 1) {
        if ((uint64_t)(M * N) > UINT64_MAX / 4 / (uint64_t)p->slices) return QS_ERR_ARG;
        p->bytes = (uint64_t)(M * N) * 4u * (uint64_t)p->slices;
    }
    return QS_OK;
}

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
    const int st = split_plan(a.M, a.N, a.K, a.split_k, p);
    if (st != QS_OK) return st;
    if (p->slices == 1) return route;              // forwarded to qs_mx_matmul_v: no workspace
    if (!a.workspace) return QS_ERR_ARG;
    if (!aligned16(a.workspace)) return QS_ERR_ALIGN;
    if (a.workspace_bytes < p->bytes) return QS_ERR_WORKSPACE;
    const int64_t tiles = cdiv(a.M, kMxgTile) * cdiv(a.N, kMxgTile);       // <= kMaxGrid (qs_mx_matmul_route)
    if (tiles * p->slices > kMaxGrid) return QS_ERR_ARG;
    return route;
}

// the two launches: the partial products of every slice, then their ordered sum
int launch_split(const qs_mx_matmul_splitk_args& a, const SplitPlan& p, int route) {
    const int tiles_n = (int)cdiv(a.N, kMxgTile);
    const int tiles = (int)cdiv(a.M, kMxgTile) * tiles_n;
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
    const int64_t groups_n = cdiv(a.N, 4), groups = a.M * groups_n;
    const int64_t blocks = std::min<int64_t>(cdiv(groups, kBlock), kMaxGrid);       // the kernel strides over the rest
    hipLaunchKernelGGL(mx_gemm_reduce_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, ws, a.bias, a.y, a.ydt, a.M, a.N, (int)p.slices,
                       groups_n, ws_vec, mx_y_vec(a.y, a.ydt, a.N));
    return launch_status();
}

}  // namespace

extern "C" {

int qs_mx_matmul_splitk_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int32_t* slices, uint64_t* workspace_bytes) {
    SplitPlan p;
    const int st = split_plan(M, N, K, split_k, &p);
    if (st != QS_OK) return st;
    if (slices) *slices = p.slices;
    if (workspace_bytes) *workspace_bytes = p.bytes;
    return QS_OK;
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
