// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the rotary embedding as a dense call (qs_mx_rope.h, mx_rope_kernel): G0 x G1
// strided slices [R, C] of x are rotated by the [R, C / 2] tables in float32 and written, rounded once, to a dense y [G, R, C] in any
// of the three dtypes -- one element-wise launch.  Its inverse flag makes it its own backward.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_mx_quant2_host.h"
#include "qs_mx_rope.h"

namespace {

// the checks of qs_mx_rope_v, in qs_mx_quant2_batched_v's order, and the kernel it launches for these operands: QS_MX_ROPE_ROUTE_*, 0
// for an empty tensor, QS_ERR_*
int mx_rope_route(const qs_mx_rope_args& a) {
    if (!a.x || !a.y || !a.cos || !a.sin) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0 || a.G0 < 0 || a.G1 < 0 || (a.C & 1)) return QS_ERR_ARG;
    if (!dt_ok(a.xdt) || !dt_ok(a.ydt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0 || (((uintptr_t)a.y) & (dt_size(a.ydt) - 1)) != 0 ||
        (((uintptr_t)a.cos) & 3u) != 0 || (((uintptr_t)a.sin) & 3u) != 0)
        return QS_ERR_ALIGN;
    if (a.G0 == 0 || a.G1 == 0 || a.R == 0 || a.C == 0) return 0;
    int64_t G, n;
    if (!mxq2_slices_ok(a, &G, &n)) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    // one lane per group of v columns: G R ceil(C / v) lanes in work-groups of kBlock
    if ((n + v - 1) / v + a.R * G > kMaxGrid * (int64_t)kBlock) return QS_ERR_ARG;
    const bool vec = a.C % v == 0 && aligned16(a.x) && a.x_stride_r % v == 0 && a.x_stride_g0 % v == 0 && a.x_stride_g1 % v == 0 &&
                     aligned16(a.y) && aligned16(a.cos) && aligned16(a.sin) && (a.interleaved || (a.C / 2) % v == 0);
    return vec ? QS_MX_ROPE_ROUTE_VEC : QS_MX_ROPE_ROUTE_PLAIN;
}

template <bool IL>
int mx_rope_launch(const qs_mx_rope_args& a, int route) {
    const int inverse = a.inverse != 0;
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        const int64_t cg = (a.C + (XD == QS_F32 ? 3 : 7)) / (XD == QS_F32 ? 4 : 8);
        const int64_t total = a.G0 * a.G1 * a.R * cg;
        const unsigned grid = (unsigned)((total + kBlock - 1) / kBlock);
        return with_dtype(a.ydt, [&](auto Y) {
            constexpr int YD = decltype(Y)::value;
            if (route == QS_MX_ROPE_ROUTE_VEC)
                hipLaunchKernelGGL((mx_rope_kernel<XD, YD, true, IL>), dim3(grid), dim3(kBlock), 0, s, a.x, a.y, a.cos, a.sin, a.G1,
                                   a.x_stride_g0, a.x_stride_g1, a.x_stride_r, a.R, a.C, cg, total, inverse);
            else
                hipLaunchKernelGGL((mx_rope_kernel<XD, YD, false, IL>), dim3(grid), dim3(kBlock), 0, s, a.x, a.y, a.cos, a.sin, a.G1,
                                   a.x_stride_g0, a.x_stride_g1, a.x_stride_r, a.R, a.C, cg, total, inverse);
            return launch_status();
        });
    });
}

}  // namespace

extern "C" {

int qs_mx_rope_route(const qs_mx_rope_args* args) {
    qs_mx_rope_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_rope_route(a);
}

int qs_mx_rope_v(const qs_mx_rope_args* args) {
    qs_mx_rope_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_rope_route(a);
    if (route <= 0) return route;
    return a.interleaved ? mx_rope_launch<true>(a, route) : mx_rope_launch<false>(a, route);
}

}  // extern "C"
