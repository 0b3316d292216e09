// libqsparse_hip.so -- C ABI (include/qsparse_hip.h), the rotary embedding in front of the batched two-way MX quantizer (qs_mx_rope.h,
// mx_rope_quant2_kernel): G0 x G1 strided slices [R, C] of x are rotated by the [R, C / 2] tables in float32 and leave as dense row
// pairs [G, R, C] and col pairs [G, C, R] -- the bits of qs_mx_quant2_batched_v on the rotated float32 tensor, which is never written
// -- from one launch.
// Host side: argument checks, route, launch configuration.  No allocation, no synchronisation.
#include "qs_host.h"
#include "qs_mx_rope.h"

namespace {

// a * b into *out unless it passes INT64_MAX (a, b >= 0)
bool mul_ok(int64_t a, int64_t b, int64_t* out) {
    if (a != 0 && b > INT64_MAX / a) return false;
    *out = a * b;
    return true;
}

// the checks of qs_mx_rope_quant2_v, in qs_mx_quant2_batched_v's order, and the kernel it launches for these operands:
// QS_MX_ROPE_ROUTE_*, 0 for an empty tensor, QS_ERR_*
int mx_rope_quant2_route(const qs_mx_rope_quant2_args& a) {
    const bool row = a.row_codes && a.row_scales, col = a.col_codes && a.col_scales;
    if (!a.x || !a.cos || !a.sin || (!row && !col)) return QS_ERR_ARG;
    if ((!a.row_codes) != (!a.row_scales) || (!a.col_codes) != (!a.col_scales)) return QS_ERR_ARG;      // half a pair
    if ((row && !mx_format_ok(a.row_format)) || (col && !mx_format_ok(a.col_format))) return QS_ERR_ARG;
    if (a.R < 0 || a.C < 0 || a.G0 < 0 || a.G1 < 0 || (a.C & 1)) return QS_ERR_ARG;
    if (!dt_ok(a.xdt)) return QS_ERR_DTYPE;
    if ((((uintptr_t)a.x) & (dt_size(a.xdt) - 1)) != 0 || (((uintptr_t)a.cos) & 3u) != 0 || (((uintptr_t)a.sin) & 3u) != 0)
        return QS_ERR_ALIGN;
    if (a.G0 == 0 || a.G1 == 0 || a.R == 0 || a.C == 0) return 0;
    if (a.x_stride_r < a.C || a.x_stride_g0 < 0 || a.x_stride_g1 < 0) return QS_ERR_ARG;
    // the outputs' G R C and the last element of x, both within int64
    int64_t G, n, e0, e1, er;
    if (!mul_ok(a.G0, a.G1, &G) || !mul_ok(a.R, a.C, &n) || !mul_ok(G, n, &n)) return QS_ERR_ARG;
    if (!mul_ok(a.G0 - 1, a.x_stride_g0, &e0) || !mul_ok(a.G1 - 1, a.x_stride_g1, &e1) || !mul_ok(a.R - 1, a.x_stride_r, &er))
        return QS_ERR_ARG;
    if (e0 > INT64_MAX - e1 || e0 + e1 > INT64_MAX - er || e0 + e1 + er > INT64_MAX - a.C) return QS_ERR_ARG;
    const int64_t tiles_c = (a.C + kMxq2Cols - 1) / kMxq2Cols, tiles_r = (a.R + kMxq2Rows - 1) / kMxq2Rows;
    if (tiles_c > kMaxGrid || tiles_r > kMaxGrid / tiles_c || G > kMaxGrid / (tiles_r * tiles_c)) return QS_ERR_ARG;
    const int64_t v = a.xdt == QS_F32 ? 4 : 8;
    const bool vec = a.C % v == 0 && aligned16(a.x) && a.x_stride_r % v == 0 && a.x_stride_g0 % v == 0 && a.x_stride_g1 % v == 0 &&
                     (!col || (a.R % 16 == 0 && aligned16(a.col_codes))) && aligned16(a.cos) && aligned16(a.sin) &&
                     (a.interleaved || (a.C / 2) % v == 0);
    return vec ? QS_MX_ROPE_ROUTE_VEC : QS_MX_ROPE_ROUTE_PLAIN;
}

template <bool IL>
int mx_rope_quant2_launch(const qs_mx_rope_quant2_args& a, int route) {
    // a pair that is not asked for keeps a valid descriptor the kernel never reads
    const MxFormat fr = mx_format(a.row_codes ? a.row_format : 0), fc = mx_format(a.col_codes ? a.col_format : 0);
    const int tiles_c = (int)((a.C + kMxq2Cols - 1) / kMxq2Cols);
    const int tiles = (int)(((a.R + kMxq2Rows - 1) / kMxq2Rows) * tiles_c);
    const int64_t grid = a.G0 * a.G1 * tiles;
    const int inverse = a.inverse != 0;
    hipStream_t s = (hipStream_t)a.stream;
    return with_dtype(a.xdt, [&](auto X) {
        constexpr int XD = decltype(X)::value;
        // as qs_mx_quant2_v: C % V == 0 on the VEC route keeps the alignment of row_codes in every row of every slice
        const int row_vec = a.row_codes && (((uintptr_t)a.row_codes) & (XD == QS_F32 ? 3u : 7u)) == 0;
        if (route == QS_MX_ROPE_ROUTE_VEC)
            hipLaunchKernelGGL((mx_rope_quant2_kernel<XD, true, IL>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.cos,
                               a.sin, a.G1, a.x_stride_g0, a.x_stride_g1, a.x_stride_r, a.row_codes, a.row_scales, a.col_codes,
                               a.col_scales, a.R, a.C, tiles, tiles_c, row_vec, inverse);
        else
            hipLaunchKernelGGL((mx_rope_quant2_kernel<XD, false, IL>), dim3((unsigned)grid), dim3(kMxq2Threads), 0, s, fr, fc, a.x, a.cos,
                               a.sin, a.G1, a.x_stride_g0, a.x_stride_g1, a.x_stride_r, a.row_codes, a.row_scales, a.col_codes,
                               a.col_scales, a.R, a.C, tiles, tiles_c, 0, inverse);
        return launch_status();
    });
}

}  // namespace

extern "C" {

int qs_mx_rope_quant2_route(const qs_mx_rope_quant2_args* args) {
    qs_mx_rope_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    return mx_rope_quant2_route(a);
}

int qs_mx_rope_quant2_v(const qs_mx_rope_quant2_args* args) {
    qs_mx_rope_quant2_args a;
    if (!take_args(args, &a)) return QS_ERR_ARG;
    const int route = mx_rope_quant2_route(a);
    if (route <= 0) return route;
    return a.interleaved ? mx_rope_quant2_launch<true>(a, route) : mx_rope_quant2_launch<false>(a, route);
}

}  // extern "C"
