// Host-side helpers shared by the translation units whose kernels run on the two-way MX quantizer's tile (qs_mx_quant2.h: 128 rows x
// 64 columns): api_mx_quant2.hip, api_mx_quant2_batched.hip, api_mx_rope_quant2.hip, api_mx_softmax_quant2.hip, api_mx_softmax_bwd.hip,
// api_mx_glu_bwd.hip, api_mx_norm.hip, api_mx_norm_bwd.hip -- and api_mx_rope.hip, for the strided slices alone.  The checks return
// what the units returned in the order they returned it: every failure in here is QS_ERR_ARG, and a unit calls them where its own
// copy stood.  Internal linkage, as qs_host.h.
#pragma once
#include "qs_host.h"
#include "qs_mx_quant2.h"

namespace {

// which pairs the caller asks for and whether they are whole.  Two spellings (Args: any descriptor with the four pair pointers and the
// two formats): a pair is there when BOTH its pointers are (half a pair is an error), or when its format is not -1 (then both pointers
// must be); `need_row`: the call has no form without a row pair
struct Mxq2Pairs {
    bool row, col, ok;                                          // ok: at least one pair, each whole, each format known
};

template <class Args>
Mxq2Pairs mxq2_pairs_by_pointer(const Args& a) {
    const bool row = a.row_codes && a.row_scales, col = a.col_codes && a.col_scales;
    const bool half = (!a.row_codes) != (!a.row_scales) || (!a.col_codes) != (!a.col_scales);
    return Mxq2Pairs{row, col, (row || col) && !half && (!row || mx_format_ok(a.row_format)) && (!col || mx_format_ok(a.col_format))};
}

template <class Args>
Mxq2Pairs mxq2_pairs_by_format(const Args& a, bool need_row = false) {
    const bool row = need_row || a.row_format != -1, col = a.col_format != -1;
    return Mxq2Pairs{row, col, (row || col) && (!row || (mx_format_ok(a.row_format) && a.row_codes && a.row_scales)) &&
                                   (!col || (mx_format_ok(a.col_format) && a.col_codes && a.col_scales))};
}

// G0 x G1 strided slices [R, C] of x, none empty (Args: x_stride_*, G0, G1, R, C): the strides' signs, then G = G0 G1, n = G R C and
// the last element of x, all within int64
template <class Args>
bool mxq2_slices_ok(const Args& a, int64_t* G, int64_t* n) {
    if (a.x_stride_r < a.C || a.x_stride_g0 < 0 || a.x_stride_g1 < 0) return false;
    int64_t e0, e1, er;
    if (!mul_ok(a.G0, a.G1, G) || !mul_ok(a.R, a.C, n) || !mul_ok(*G, *n, n)) return false;
    if (!mul_ok(a.G0 - 1, a.x_stride_g0, &e0) || !mul_ok(a.G1 - 1, a.x_stride_g1, &e1) || !mul_ok(a.R - 1, a.x_stride_r, &er)) return false;
    return !(e0 > INT64_MAX - e1 || e0 + e1 > INT64_MAX - er || e0 + e1 + er > INT64_MAX - a.C);
}

inline int64_t mxq2_tiles_r(int64_t R) { return (R + kMxq2Rows - 1) / kMxq2Rows; }
inline int64_t mxq2_tiles_c(int64_t C) { return (C + kMxq2Cols - 1) / kMxq2Cols; }

// one work-group per tile per slice in a linear grid (R, C, G >= 1)
inline bool mxq2_grid_ok(int64_t R, int64_t C, int64_t G = 1) {
    const int64_t tiles_c = mxq2_tiles_c(C), tiles_r = mxq2_tiles_r(R);
    return !(tiles_c > kMaxGrid || tiles_r > kMaxGrid / tiles_c || G > kMaxGrid / (tiles_r * tiles_c));
}

// what every launch on the tile hands its kernel: a pair that is not asked for keeps a valid descriptor the kernel never reads, and
// null pointers whatever the caller left there
struct Mxq2Launch {
    MxFormat fr, fc;
    uint8_t *row_codes, *row_scales, *col_codes, *col_scales;
    int tiles_c, tiles;                                         // tiles per slice: tiles_r * tiles_c
};

template <class Args>
Mxq2Launch mxq2_launch(const Args& a, bool row, bool col, int64_t R, int64_t C) {
    Mxq2Launch l{mx_format(row ? a.row_format : 0), mx_format(col ? a.col_format : 0), nullptr, nullptr, nullptr, nullptr, 0, 0};
    if (row) l.row_codes = a.row_codes, l.row_scales = a.row_scales;
    if (col) l.col_codes = a.col_codes, l.col_scales = a.col_scales;
    l.tiles_c = (int)mxq2_tiles_c(C);
    l.tiles = (int)(mxq2_tiles_r(R) * l.tiles_c);
    return l;
}

// a lane stores its `v` (4 or 8) row codes at once where row_codes keeps that alignment (the VEC routes' C % v == 0 keeps it in every
// row of every slice)
inline int mxq2_row_vec(const Mxq2Launch& l, unsigned v) { return l.row_codes && (((uintptr_t)l.row_codes) & (v - 1)) == 0; }

}  // namespace
