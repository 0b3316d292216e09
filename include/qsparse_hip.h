/*
 * qsparse_hip.h -- C ABI of libqsparse_hip.so: the MI355X (gfx950) implementation of the tensor math
 * behind mlzxy/qsparse's QuantizeLayer / PruneLayer forward + backward.
 *
 * This is the drop-in boundary.  The reference has no native layer (its "kernels" are chains of eager
 * ATen operators inside qsparse/quantize.py, qsparse/sparse.py and qsparse/util.py); every entry point
 * below names the reference lines whose arithmetic it replaces.  A binding needs nothing but a dlopen:
 * plain pointers, sizes and enums, no torch types.
 *
 * Conventions
 *   - Every tensor is CONTIGUOUS and described as a 3-d view [outer, C, inner]: `C` is the extent of the
 *     reference's `channel_index` dimension, `outer`/`inner` the products of the extents before/after it.
 *     Tensor-wise operation: pass nparam == 1 (C and inner may then be any factorisation of numel).
 *   - Per-channel parameters are DEVICE float arrays of length nparam (1 or C).  A NULL parameter
 *     pointer selects the by-value host scalar that follows it in the argument list.
 *   - dtypes: QS_F32 / QS_BF16 / QS_F16.  Arithmetic is IEEE binary32, one rounding per operator of the
 *     reference chain (built with -ffp-contract=off; division is correctly rounded).
 *   - All work is enqueued on `stream` (a hipStream_t); no call allocates, frees or synchronises, so
 *     every call is hipGraph-capturable.  Scratch memory is caller-provided (qs_workspace_bytes).
 *   - Return value: 0 on success, a positive hipError_t from the runtime, or a negative QS_ERR_* for a
 *     rejected argument (nothing is enqueued in that case).  qs_status_string() explains either kind.
 *   - Data pointers of x / y / g must be 16-byte aligned (QS_ERR_ALIGN otherwise).
 */
#ifndef QSPARSE_HIP_H
#define QSPARSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QS_ABI_VERSION 28
/* ABI compatibility (from v25 on).
 *   - Every positional prototype in this header is FROZEN as of v25: a later version never changes the argument list of an
 *     existing symbol.  qs_abi_floor() returns the oldest version whose prototypes this library still honours (25); a binding
 *     written against version V works with any library with qs_abi_floor() <= V <= qs_version().
 *   - New operands arrive through the DESCRIPTOR entry points (qs_*_v): the operands of a call in a struct whose first field,
 *     `struct_size`, is sizeof(the struct) AS THE CALLER COMPILED IT.  Fields are only ever appended.  The library copies
 *     min(struct_size, its own sizeof) bytes into a zeroed struct: a caller built against an older header leaves the newer fields
 *     0 / NULL (every appended field is optional with that default), a caller built against a newer header is understood up to
 *     what this library knows.  The fields are the positional arguments of the entry point of the same name, one for one, followed
 *     by the appended ones, each marked with the version that introduced it.
 *   - The positional entry points remain: thin wrappers that fill the descriptor.  qs_site_plan / qs_multi_row / qs_multi_stage
 *     are caller-built tables whose layout is likewise append-only from v25 on. */

enum qs_dtype { QS_F32 = 0, QS_BF16 = 1, QS_F16 = 2 };

enum qs_error {
    QS_OK = 0,
    QS_ERR_DTYPE = -1,     /* unsupported dtype combination              */
    QS_ERR_ARG = -2,       /* inconsistent sizes / NULL where not allowed */
    QS_ERR_ALIGN = -3,     /* data pointer not 16-byte aligned           */
    QS_ERR_WORKSPACE = -4, /* workspace too small                        */
    QS_ERR_RANK = -5       /* broadcast pattern needs more than QS_MAX_DIMS collapsed dims */
};

enum qs_workspace_op { QS_WS_KTH_VALUE = 1, QS_WS_REDUCE = 2 /* n = C * inner of a per-channel qs_absmax / qs_minmax */ };

#define QS_MAX_DIMS 6

typedef void* qs_stream_t; /* hipStream_t */

/* Folded activations.  convert() wraps whatever activation modules the user names (qsparse/convert.py:214-218); the entry
 * points below that take `pre_relu` -- and qs_mean_dim / qs_mean_dim_cl through their flags -- absorb the activation in front
 * of an operator: its output is never written, statistics and forward read its input, the forward records the ONE bit per
 * element its backward needs (gate_out) and qs_quant_ste_relu_bwd applies it.  `pre_relu` is 0 (none), 1 (nn.ReLU) or a handle
 * from qs_activation() for the others:
 *   QS_ACT_HARDTANH  clamp(x, a, b): nn.Hardtanh(a, b), nn.ReLU6 (a = 0, b = 6);  backward 0 where x <= a or x >= b
 *   QS_ACT_LEAKY     x > 0 ? x : x*a (product rounded to x's dtype): nn.LeakyReLU(a);  backward g*a where x <= 0
 * Handles are interned descriptors: small positive integers, valid for the life of the process, the same (kind, a, b) always
 * yields the same handle; thread-safe.  Returns a negative QS_ERR_* for an unknown kind or a full table (256 entries). */
enum qs_act_kind { QS_ACT_NONE = 0, QS_ACT_RELU = 1, QS_ACT_HARDTANH = 2, QS_ACT_LEAKY = 3 };
int qs_activation(int kind, float a, float b);

int qs_version(void);
int qs_abi_floor(void);      /* (v25) see "ABI compatibility" above */
const char* qs_status_string(int status);
size_t qs_workspace_bytes(int op, int64_t n);

/* ---- quantizers: forward ------------------------------------------------------------------------ */

/* ScalerQuantization.forward, qsparse/quantize.py:100-117.
 *   q = int32(rint(round_to(qdt, f32(x) / s_c)));  y = f32(q) * s_c
 * qdt is the dtype the reference's quotient tensor has (f32 when the scaler is a >=1-d tensor, the input
 * dtype when it is a Python float / 0-d tensor).  `codes` (nullable) receives q.  `chan_mask` (nullable,
 * nparam-independent, length C, one byte per channel) fuses a preceding channel PruneLayer
 * (x * mask, qsparse/sparse.py:116): masked channels are quantised as x*0.  The reference never
 * saturates (its clamp at :110-116 acts on a temporary, `q.float().clamp_(...)`, and is lost); saturate != 0 is that
 * clamp with the assignment it lacks -- q = clamp(q, code_lo, code_hi) on the int32 codes, i.e. after the float -> int
 * conversion, so a NaN input (INT_MIN) lands on code_lo -- as an explicit opt-in: code_lo / code_hi = -2^(bits-1)+notch /
 * 2^(bits-1)-1+notch, or 0 / 2^bits-1 with use_uint (:111-116).  pre_relu != 0 quantises max(x, 0): the nn.ReLU that convert() finds in front of the pair
 * (qsparse/convert.py:214-218) folded into the same pass.
 * elide_masked != 0 (with chan_mask): the x of a pruned channel is not loaded at all -- it only ever meets `* 0`
 * (sparse.py:116) -- and the quantizer is applied to +0.0 instead: bit-identical to the loading path for every finite
 * x; a NaN / Inf on a pruned channel yields f32(0)*s instead of the reference's f32(INT_MIN)*s.  chan_mask bytes are then
 * read as an ELISION MASK: 1 kept, 0 pruned and skipped, 2 pruned but LOADED (a zero factor like 0, so NaN / Inf come out as in
 * the reference) -- qs_pq_select's elide_mask_out marks 2 the pruned channels whose abs-max of this step is not finite, which
 * makes the eliding call bit-identical to the loading one for every x.
 * gate_out (nullable; needs pre_relu != 0; ceil(numel / 8) bytes): the folded ReLU's gate for the backward, one BIT per
 * element in memory order -- bit (e & 7) of gate_out[e >> 3] = !(x[e] <= 0), ATen's threshold_backward -- so that
 * qs_quant_ste_relu_bwd reads one bit instead of x per element and x need not be kept.  Every element is loaded then;
 * with elide_masked != 0 the x of a pruned channel still counts as +0.0, i.e. the result is the eliding call's. */
int qs_quant_scaler_fwd(const void* x, void* y, int32_t* codes,
                        const float* scale, int64_t nscale, float scale_host,
                        const uint8_t* chan_mask,
                        int64_t outer, int64_t C, int64_t inner,
                        int xdt, int ydt, int qdt,
                        int saturate, int32_t code_lo, int32_t code_hi, int pre_relu, int elide_masked,
                        uint8_t* gate_out, void* image_out, int imgdt, void* xback_out, qs_stream_t stream);

/* DecimalQuantization.forward, qsparse/quantize.py:44-63:  q = int32(trunc(x * 2^d)); y = f32(q) * 2^-d */
int qs_quant_decimal_fwd(const void* x, void* y, int32_t* codes,
                         const float* decimal, int64_t ndecimal, float decimal_host,
                         const uint8_t* chan_mask,
                         int64_t outer, int64_t C, int64_t inner,
                         int xdt, int ydt, int qdt,
                         int saturate, int32_t code_lo, int32_t code_hi, int pre_relu, int elide_masked,
                         uint8_t* gate_out, void* image_out, int imgdt, void* xback_out, qs_stream_t stream);

/* (ABI v25) qs_quant_scaler_fwd / qs_quant_decimal_fwd as ONE descriptor entry point; `kind` selects the quantizer, `param` /
 * `nparam` / `param_host` are scale / nscale / scale_host or decimal / ndecimal / decimal_host. */
enum qs_quant_kind { QS_QUANT_SCALER = 0, QS_QUANT_DECIMAL = 1 };
typedef struct qs_quant_fwd_args {
    uint32_t struct_size;        /* sizeof(qs_quant_fwd_args) as the caller compiled it */
    int32_t kind;                /* enum qs_quant_kind */
    const void* x;
    void* y;
    int32_t* codes;
    const float* param;
    int64_t nparam;
    float param_host;
    int32_t xdt, ydt, qdt;
    const uint8_t* chan_mask;
    int64_t outer, C, inner;
    int32_t saturate, code_lo, code_hi, pre_relu, elide_masked, imgdt;
    uint8_t* gate_out;
    void* image_out;
    void* xback_out;
    qs_stream_t stream;
} qs_quant_fwd_args;
int qs_quant_fwd_v(const qs_quant_fwd_args* args);

/* image_out (nullable; qs_quant_scaler_fwd / qs_quant_decimal_fwd, with gate_out, ydt == QS_F32 and codes == NULL): the same
 * pass also writes RNE(y) in imgdt (QS_BF16 / QS_F16) -- the low-precision image autocast would make of y in front of a
 * convolution -- at +2 instead of a 6 B/elem cast pass.  Served by the gate-recording widening kernels; qs_quant_image_ok tells
 * whether a geometry is one of theirs (1) or the call would be rejected with QS_ERR_ARG (0). */
int qs_quant_image_ok(int64_t outer, int64_t C, int64_t inner, int per_channel_param, int has_mask, int mask_aligned8, int xdt);

/* xback_out (nullable; same kernels and conditions as image_out -- gate_out, ydt == QS_F32, codes == NULL, a geometry for which
 * qs_quant_image_ok answers 1): the same pass also stores act(x) in xdt at xback_out[e] -- nn.ReLU: ATen's clamp_min(x, 0), NaN
 * and -0.0 pass; any other folded activation likewise.  With xback_out == x this IS the forward of an nn.ReLU(inplace=True) /
 * nn.ReLU6(inplace=True) standing in front of the operator (what
 * torchvision-style networks carry where the reference's convert() puts its operators, qsparse/convert.py:199-229): other
 * holders of x see relu(x) as they must, at the price of one more store (+2 / +4 B/elem) instead of ATen's read + write pass
 * (4 / 8 B/elem).  Every lane reads the elements it rewrites before it rewrites them; no other lane touches them. */

/* LineQuantization.forward, qsparse/quantize.py:148-181.  lines = device float [nlines, 2] = (start, end).
 * float_zero_point != 0: ((clamp(rint((xc-start)/step),0,N-1))*step)+start   (:168-181)
 * float_zero_point == 0: (clamp(rint(xc/step)-rint(start/step),0,N-1)+rint(start/step))*step  (:161-166)
 * `codes` (nullable, int32, x's shape): the level index in [0, N-1] -- the clamp's result, before `* step + start` /
 * `+ rint(start/step)` -- for the integer export (the arithmetic tests/test_quantize.py:73-101 pins for the decimal
 * quantizer); INT32_MIN where x is NaN. */
int qs_quant_line_fwd(const void* x, void* y, int32_t* codes, const float* lines, int64_t nlines, int bits,
                      int float_zero_point, int64_t outer, int64_t C, int64_t inner,
                      int xdt, int ydt, qs_stream_t stream);

/* ---- quantizers: straight-through backward ------------------------------------------------------ */

/* ScalerQuantization.backward / DecimalQuantization.backward, qsparse/quantize.py:66-77,120-131:
 *   gx = cast(gxdt, min(max(g, lo_mul*step_c), hi_mul*step_c))     (passthrough != 0: gx = cast(g))
 * and +0.0 where that clamp is NaN -- a NaN g, or any g once step_c is NaN: the reference's `v[v != grad_output] = 0` (:76,
 * :130) compares the clamped tensor with itself, i.e. zeroes exactly the NaNs (fixture F17).
 * step_c = scale (step_is_decimal == 0) or 2^-d (step_is_decimal != 0);  lo_mul = -2^(bits-1)+notch,
 * hi_mul = 2^(bits-1)-1+notch.  chan_mask (nullable) fuses the PruneLayer backward g*mask
 * (autograd MulBackward0 of qsparse/sparse.py:116).  g and gx may alias.
 * elide_masked != 0 (with chan_mask): the g of a pruned channel is not loaded and gx = +0.0 there; the reference's
 * g*0 carries the sign of clamp(g), so this is numerically equal, not bit-identical (opt-in). */
int qs_quant_ste_bwd(const void* g, void* gx,
                     const float* step, int64_t nstep, float step_host, int step_is_decimal,
                     float lo_mul, float hi_mul, int passthrough,
                     const uint8_t* chan_mask,
                     int64_t outer, int64_t C, int64_t inner,
                     int gdt, int gxdt, int elide_masked, qs_stream_t stream);

/* The same backward with the gate of a folded activation -- `act`: 1 (nn.ReLU, threshold_backward: 0 where x <= 0) or a
 * qs_activation() handle (hardtanh_backward: 0 where x <= a or x >= b; leaky_relu_backward: v * slope where x <= 0, v the
 * clamped, masked gradient rounded to xdt):
 *   gx = cast(xdt, x <= 0 ? 0 : min(max(g, lo_mul*step_c), hi_mul*step_c) * mask_c)                    (nn.ReLU)
 * x is the ReLU's INPUT (dtype xdt); gx has x's dtype.  gate (nullable): the bitmap a forward call recorded through
 * gate_out over the same [outer, C, inner] geometry; when given, x is not read (it may be NULL) and xdt only names the
 * dtype of gx: 4 + 1/8 + sizeof(xdt) bytes per element instead of 4 + 2 * sizeof(xdt).
 * g2 (nullable, dtype g2dt = QS_BF16 / QS_F16, with gate and gdt == QS_F32 and elide_masked == 0): a second gradient of
 * the same geometry that is ADDED to g in float32 before the clamp -- g may then be NULL (g2 alone).  It is autograd's
 * accumulation of the gradients a float32 output receives under autocast (float32 from float32 consumers, bf16 from the
 * convolution that consumed its bf16 image) done inside the kernel: no cast pass, no add pass, 2 instead of 4 bytes read. */
int qs_quant_ste_relu_bwd(const void* g, const void* x, const uint8_t* gate, void* gx,
                          const float* step, int64_t nstep, float step_host, int step_is_decimal,
                          float lo_mul, float hi_mul, const uint8_t* chan_mask,
                          int64_t outer, int64_t C, int64_t inner, int gdt, int xdt, int elide_masked, int act,
                          const void* g2, int g2dt, qs_stream_t stream);

/* (ABI v25) The same entry point with its operands in a size-prefixed descriptor (see "Descriptor entry points" at the top of
 * this header): fields are only ever appended, a caller compiled against an older header sets a smaller struct_size and the
 * fields it does not know read as 0 / NULL.  The fields up to g2dt are the positional arguments above, one for one.
 *   g3      (v25; nullable; dtype g2dt; needs g2, gdt == xdt == QS_F32) a THIRD gradient of the same geometry, added between g
 *           and g2: gx = gate * clamp((g + f32(g3)) + f32(g2)) * mask, each term optional from the left.  Autograd accumulates
 *           the shares of a tensor's consumers in REVERSE order of the consumers' creation: with float32 consumers created
 *           last, the second 2-byte consumer (g3) before them and the first 2-byte consumer (g2) first of all, this is the
 *           reference's grouping bit for bit -- the site in front of a ResNet block whose down-sampling convolution reads the same
 *           activation as the block's first convolution.
 *   gx_image / gx_image_dt  (v25; nullable; QS_BF16 / QS_F16; needs gdt == xdt == QS_F32, 16-byte aligned) RNE(gx), written by the
 *           same pass next to gx (+2 B/elem): the gradient of the 2-byte operand of a type-promoting add in front of the site
 *           (`bn(conv(h)) + identity` under autocast: bf16 + float32 -> float32), which ATen's AddBackward0 produces with a
 *           cast pass of gx of its own (6 B/elem). */
/* (v26) The caller's activation.  convert(..., activation_layers=[nn.GELU]) puts the operators behind an activation the kernels do
 * not fold: its forward value is the caller's (ATen's) pass, the site reads that.  Its BACKWARD needs only the site's input gradient
 * and the activation's input, so the site's backward evaluates it on the way out:
 *   act_x / act_x_kind   (nullable; QS_DACT_GELU: nn.GELU(approximate='none')) the activation's INPUT, of dtype xdt, gx's shape and
 *           layout, 16-byte aligned.  gx = gelu_backward(RNE_xdt(gx_site), act_x) with gx_site the site's own result (clamp(g [+ g3]
 *           [+ g2]) * mask), in ATen's GPU arithmetic bit for bit (float32 opmath, dy * fma(x, pdf, cdf)).  `x` and `gate` are not
 *           read (the site has no folded activation of its own then, or the identity's); `elide_masked` is ignored; g2 is allowed
 *           without a gate. */
enum qs_dact_kind { QS_DACT_NONE = 0, QS_DACT_GELU = 1 };
typedef struct qs_ste_relu_bwd_args {
    uint32_t struct_size;        /* sizeof(qs_ste_relu_bwd_args) as the caller compiled it */
    int32_t gdt, xdt, g2dt;
    const void* g;
    const void* x;
    const uint8_t* gate;
    void* gx;
    const float* step;
    int64_t nstep;
    float step_host;
    int32_t step_is_decimal;
    float lo_mul, hi_mul;
    const uint8_t* chan_mask;
    int64_t outer, C, inner;
    int32_t elide_masked, act;
    const void* g2;
    qs_stream_t stream;
    /* ---- v25 ---- */
    const void* g3;
    void* gx_image;
    int32_t gx_image_dt;
    int32_t reserved0;
    /* ---- v26 ---- */
    const void* act_x;           /* see "the caller's activation" above; NULL: none */
    int32_t act_x_kind;          /* QS_DACT_GELU */
    int32_t reserved1;
} qs_ste_relu_bwd_args;
int qs_quant_ste_relu_bwd_v(const qs_ste_relu_bwd_args* args);

/* ---- statistics ---------------------------------------------------------------------------------- */

/* max |x| over the tensor (per_channel == 0 -> out[1]) or per channel (out[C]);
 * DecimalQuantizer.optimize, qsparse/quantize.py:329-340.  Order-independent, hence bit-exact.
 * accumulate != 0: out is max-accumulated instead of overwritten (the caller keeps it zeroed between steps, e.g.
 * through qs_scale_update's clear_absmax), which saves the initialisation launch.
 * pre_relu != 0: the statistic of max(x, 0) -- a preceding nn.ReLU folded into the quantizer's kernels.
 * out_lines (1 unless per_channel == 0 and accumulate != 0): the tensor-wise maximum is accumulated into `out_lines`
 * partial accumulators, QS_AMAX_LINE_STRIDE floats (one 128-byte line) apart, out[l * QS_AMAX_LINE_STRIDE]; their
 * maximum is the result (qs_scale_update folds them).  Same-address atomics serialise on MI355X (~12 ns each), which
 * caps a one-word reduction at ~256 workgroups; 16 lines lift that cap.
 * ws (nullable): qs_workspace_bytes(QS_WS_REDUCE, C*inner) bytes of scratch; with it a per-channel reduction over few
 * columns and many rows (channels_last activations: inner == 1, C <= 512) runs as two atomics-free stages; 0 bytes means the shape never takes that route. */
int qs_absmax(const void* x, float* out, int per_channel,
              int64_t outer, int64_t C, int64_t inner, int xdt, int accumulate, int pre_relu, int out_lines,
              void* ws, size_t ws_bytes, qs_stream_t stream);

/* min and max of x over the tensor or per channel; AdaptiveQuantizer.optimize, quantize.py:410-418
 * (min over the batch of per-sample minima == global per-channel minimum).
 * accumulate == 0: out_min / out_max receive floats (three launches: key initialisation, reduction, key -> float).
 * accumulate != 0: out_min / out_max are persistent buffers of order-preserving uint32 KEYS, neutral on entry (min keys
 * 0xffffffff, max keys 0), min- / max-accumulated by ONE launch and left as keys: qs_lines_update(from_keys = 1) turns them
 * into floats and makes them neutral again -- two launches per AdaptiveQuantizer step instead of four (ABI v9). */
int qs_minmax(const void* x, float* out_min, float* out_max, int per_channel,
              int64_t outer, int64_t C, int64_t inner, int xdt, int accumulate, void* ws, size_t ws_bytes,
              qs_stream_t stream);

/* Step counters.  The reference keeps them on the host (Python ints / `.item()` reads) and they enter the
 * arithmetic of every running mean.  A by-value kernel argument is frozen when a launch is captured into a
 * hipGraph, so every entry point that takes a counter `t` also takes `t_dev` (nullable): a device-resident
 * int64 holding the same counter, read by the kernel INSTEAD of `t` when non-NULL.  Counters are advanced
 * either by the caller (any stream-ordered increment), by qs_pq_select's bump_* arguments, or -- qs_scale_update,
 * qs_lines_update with advance_t_dev != 0 -- by the kernel itself after every thread has read them (the update then
 * runs as a single workgroup). */

/* weight[i] <- t == 0 ? new : (t*weight[i] + new)/(t+1),  new = absmax[i] / 2^(bits-1) rounded to stat_dt, the
 * dtype of the tensor the abs-max was taken from: the reference divides in that dtype, which matters for fp16,
 * where small maxima underflow into subnormals (quantize.py:340,344-348).  clear_absmax != 0 zeroes absmax[i]
 * after use; bump_i32 (nullable) is a one-element device counter incremented once (QuantizeLayer._n_updates,
 * quantize.py:515).  absmax_lines > 1 (n == 1 only): the tensor-wise abs-max arrives as that many partial accumulators
 * QS_AMAX_LINE_STRIDE floats apart (qs_absmax with out_lines); their maximum is used and all of them are cleared. */
int qs_scale_update(float* absmax, int absmax_lines, float* weight, int64_t n, int64_t t, int64_t* t_dev,
                    int advance_t_dev, int bits, int clear_absmax, int32_t* bump_i32, int stat_dt, qs_stream_t stream);

/* lines[i] <- (lines[i]*(t-1) + (mn[i], mx[i])) / t   with t already incremented (quantize.py:427-430);
 * t_dev holds the counter BEFORE the increment (t = *t_dev + 1).  from_keys != 0: mn / mx hold the keys of
 * qs_minmax(accumulate = 1); they are converted here and reset to the neutral keys. */
int qs_lines_update(float* mn, float* mx, float* lines, int64_t n, int64_t t_after,
                    int64_t* t_dev, int advance_t_dev, int from_keys, qs_stream_t stream);

/* d[i] = rint(log2(nan_to_num(1/scale[i], posinf=1, neginf=1)))  (quantize.py:316) */
int qs_decimal_from_scale(const float* scale, float* decimal, int64_t n, qs_stream_t stream);

/* SUMMATION-ORDER PIN.  The staged-mean entry points below (qs_mean_dim, qs_mean_dim_split, qs_mean_dim_cl, qs_mean_cl_w,
 * qs_mean_strided, qs_mean_last2, qs_multi_stage_mean) restate the summation order of ATen's CPU SumKernel.cpp with ONE intra-op
 * thread as torch 2.10 computes it -- the version the reference ran under when the golden fixtures were recorded
 * (the .npz files under tests/golden: meta["torch"], meta["intra_op_threads"]).  The host package warns once at import under another torch
 * (qsparse_amd.util.PINNED_TORCH / check_torch_pin); tests/test_aten_contract.py (CPU) and tests/test_aten_contract_gpu.py (the
 * same probes in the `-m gpu` set) detect a moved order. */

/* One stage of squeeze_tensor_to_shape (qsparse/util.py:92-99): mean over the middle dim of a contiguous
 * [pre, n, post] tensor -> [pre, 1, post], fp32 accumulation in ATen's CPU summation order (cascade /
 * 4-way interleave), one fp32 division by n, one rounding to odt.
 * flags: QS_MEAN_ABS takes |x| first (sparse.py:87);  QS_MEAN_L0 maps x -> (x != 0) when *l0_flag != 0
 * (sparse.py:85-86; l0_flag is a device int written by qs_l0_flag).
 * absmax_out (nullable, device float[C * absmax_stride]) is additionally max-ACCUMULATED with per-channel
 * max|x| at absmax_out[channel * absmax_stride], where channel = (column / chan_div) % C  -- the statistics of
 * a following tensor-wise QuantizeLayer fused into the same read of x.  The caller provides it zeroed
 * (qs_pq_select re-zeroes it after use).  The accumulation is one device atomic per wave and channel, and
 * MI355X serialises atomics that fall into the same 128-byte line (~10 ns each, exposed at the end of a short
 * kernel): absmax_stride = QS_AMAX_LINE_STRIDE gives every channel its own line (measured, batch-64 ResNet
 * activations: 33.9 -> 10.3 us on 256x14x14 maps, 87.9 -> 18.4 us on 128 x 64x32x32); 1 is a dense float[C]. */
#define QS_AMAX_LINE_STRIDE 32
#define QS_MEAN_ABS 1
#define QS_MEAN_L0 2
#define QS_MEAN_RELU 4 /* statistics of act(x): a folded preceding activation (abs-max included) -- nn.ReLU, or the one whose
                          qs_activation() handle rides in bits 8.. of the flags: QS_MEAN_ACT(handle) */
#define QS_MEAN_ACT(handle) (QS_MEAN_RELU | ((handle) << 8))
int qs_mean_dim(const void* x, void* out, int64_t pre, int64_t n, int64_t post,
                int xdt, int odt, int flags, const int32_t* l0_flag,
                float* absmax_out, int64_t absmax_stride, int64_t chan_div, int64_t C, qs_stream_t stream);

/* qs_mean_dim for a [pre, n, post] tensor that is the MEMORY of a permuted one (post >= 2): ATen decides between cascade and
 * row-sum order per output from the coordinates of the dim its TensorIterator puts innermost, which for such a tensor need not be
 * the flattened post (qsparse_amd/util.py `aten_reduce_plan`).  Where that set is a prefix of the columns -- the usual case, e.g. a
 * [B, T, C] activation seen as [B, C, T] and reduced over B: t < 4 * floor(T / 4) -- the caller names it: columns [0, mr_cols) of
 * every slice in cascade order, the others in row-sum order, through the same kernels as qs_mean_dim (16-byte loads, 8 columns per
 * lane).  No abs-max rider.  (ABI v23) */
int qs_mean_dim_split(const void* x, void* out, int64_t pre, int64_t n, int64_t post, int64_t mr_cols, int xdt, int odt, int flags,
                      const int32_t* l0_flag, qs_stream_t stream);

/* (ABI v25) The statistics of a token-major activation x[N][T][C] whose mask runs along the LAST dim (`prune(dimensions={2})` on a
 * transformer block's hidden activation; qsparse/sparse.py:231-239, util.py:92-99): the two stages of squeeze_tensor_to_shape --
 * stage[T][C] = mean over N (rounded to xdt), stage_mean[C] = mean over T of that (rounded) -- in ATen's order for the contiguous
 * tensor, i.e. exactly two qs_mean_dim calls, plus the per-channel abs-max of the mean's operand (|x|, or |act(x)| with
 * QS_MEAN_RELU / QS_MEAN_ACT) max-accumulated into chan_absmax[c * absmax_stride] (nullable; zero on entry as for qs_mean_dim).
 * Every column of a row is a channel of its own here, so the abs-max cannot ride per wave as in the NCHW stage: the first stage
 * stores one key per COLUMN into amax_part (nullable workspace, float[T * C], 16-byte aligned; no atomics) and a small third
 * launch folds it per channel.  Without amax_part -- or for widths / flags the per-column kernels do not serve -- the abs-max rides
 * in qs_mean_dim's atomic form (same values).  flags: QS_MEAN_ABS [| QS_MEAN_RELU | QS_MEAN_ACT(handle)]. */
int qs_token_stats(const void* x, void* stage, void* stage_mean, float* amax_part, float* chan_absmax, int64_t absmax_stride, int64_t N,
                   int64_t T, int64_t C, int xdt, int flags, qs_stream_t stream);

/* The first stage for a channels_last (NHWC in memory) activation x[n][hw][C]: mean over n ->
 * out[C][hw], NCHW-contiguous like the result of Tensor.mean(0, keepdim=True) on a channels_last tensor, in the
 * summation order ATen uses for that layout (per channel, positions hw < 4*floor(hw/4) in cascade order, the rest
 * 4-way interleaved; the later stages are the NCHW ones: qs_mean_last2 / qs_mean_dim).  flags as for qs_mean_dim
 * (QS_MEAN_L0 reads l0_flag, nullable otherwise).  C % 8 == 0 with flags 0, QS_MEAN_ABS or QS_MEAN_ABS|QS_MEAN_RELU and
 * a 16-byte aligned x take the vector kernels (16-byte loads, 8 channels per lane); every other channel count and flag
 * combination a scalar kernel in the same order.  amax_part (nullable, device float[C*hw]) receives the maximum over
 * n of |x| (or max(x, 0) with QS_MEAN_RELU) per output element; hand it to qs_mean_last2, which reduces it to the
 * per-channel abs-max without atomics. */
int qs_mean_dim_cl(const void* x, void* out, int64_t n, int64_t hw, int64_t C, int xdt, int odt, int flags,
                   const int32_t* l0_flag, float* amax_part, qs_stream_t stream);

/* The ONE stage of squeeze_tensor_to_shape (qsparse/util.py:92-99) for a channels_last activation x[N][H][W][C] whose first --
 * and then only -- reduced dim is W (a mask that keeps N, C and H; `prune(dimensions={0, 1, 2})`, qsparse/sparse.py:228-249):
 * mean over W -> out[N][C][H], NCHW-contiguous like Tensor.mean(3, keepdim=True) of such a tensor, in ATen's summation order
 * for it (scalar inner sum: four interleaved cascade sums over w, then ((p0 + p1) + p2) + p3; NOT the vectorised order of the
 * contiguous NCHW row).  flags / l0_flag as for qs_mean_dim.  (ABI v20) */
int qs_mean_cl_w(const void* x, void* out, int64_t N, int64_t H, int64_t W, int64_t C, int xdt, int odt, int flags,
                 const int32_t* l0_flag, qs_stream_t stream);

/* The FIRST stage of squeeze_tensor_to_shape (qsparse/util.py:92-99) for a dense tensor laid out in any dim order other than the
 * ones above (a transposed weight, a permuted activation, NDHWC with the batch kept ...): the mean over one dim of `n` elements
 * `stride` elements apart, read where the tensor lies (x needs element alignment only), written to the contiguous result
 * Tensor.mean(dim, keepdim=True) returns.  The caller describes the kept dims (nkept <= 6, after merging what merges) by size,
 * input stride and output stride, the one the lane index should run fastest over first, and names the summation order ATen's
 * TensorIterator + SumKernel.cpp arrive at for this layout (host logic, qsparse_amd/util.py `aten_reduce_plan`):
 *   order 0  vectorised inner sum (needs stride == 1, n >= 8): 8 interleaved row-sums, the n % 8 tail, then the 8 lanes in turn
 *   order 1  row-sum for every output (four interleaved cascade sums, ((p0 + p1) + p2) + p3)
 *   order 2  cascade sum for outputs whose coordinate in kept dim `split_dim` is < `split`, row-sum for the rest
 * flags / l0_flag as for qs_mean_dim (no abs-max rider).  (ABI v22) */
int qs_mean_strided(const void* x, void* out, int64_t n, int64_t stride, int nkept, const int64_t* kept_size,
                    const int64_t* kept_in_stride, const int64_t* kept_out_stride, int order, int split_dim, int64_t split,
                    int xdt, int odt, int flags, const int32_t* l0_flag, qs_stream_t stream);

/* The last two stages of squeeze_tensor_to_shape fused for a contiguous [pre, H, W] tensor whose trailing
 * two dims are both reduced: mean over H (rounded to xdt), then mean over W (rounded to odt) -> out[pre].
 * Same summation order and rounding points as two qs_mean_dim calls.  (H*W + W + 8)*4 bytes of LDS <= 63 KiB
 * (112 x 112 maps fit),
 * otherwise QS_ERR_ARG (use two qs_mean_dim calls).
 * amax_part (nullable, [pre, H, W] from qs_mean_dim_cl): absmax_out[p * absmax_stride] is max-accumulated with the
 * maximum of slice p.
 * record (nullable, device float[2 * pre]): this rank's exchange record in qs_stats_pack's layout, written on the way
 * out -- record[p] = float(out[p]), record[pre + p] = absmax_out[p * absmax_stride] (0 when absmax_out is NULL; with
 * amax_part NULL absmax_out is only read) -- which saves the qs_stats_pack launch of a data-parallel step. */
int qs_mean_last2(const void* x, void* out, int64_t pre, int64_t H, int64_t W, int xdt, int odt,
                  const float* amax_part, float* absmax_out, int64_t absmax_stride, float* record, qs_stream_t stream);

/* *flag = (min(x) == 0), qsparse/sparse.py:85 */
int qs_l0_flag(const void* x, int64_t numel, int xdt, int32_t* flag, float* scratch2, qs_stream_t stream);

/* state[i] <- (t*state[i] + f32(new[i])) / (t+1)   (MagnitudePruningCallback.update_magnitude,
 * qsparse/sparse.py:88-89) */
int qs_running_mean(float* state, const void* newv, int newdt, int64_t n, int64_t t, const int64_t* t_dev,
                    qs_stream_t stream);

/* ---- mask construction --------------------------------------------------------------------------- */

/* thr = sort_ascending(imp)[k]  (calculate_mask_given_importance, qsparse/util.py:113-116; the caller
 * computes k = max(int(s*n-1),0)+1 on the host exactly as the reference does).  NaNs order last.
 * ws: qs_workspace_bytes(QS_WS_KTH_VALUE, n) bytes. */
int qs_kth_value(const float* imp, int64_t n, int64_t k, float* thr, void* ws, size_t ws_bytes,
                 qs_stream_t stream);

/* mask[i] = imp[i] >= *thr   (util.py:117) */
int qs_mask_ge(const float* imp, const float* thr, uint8_t* mask, int64_t n, qs_stream_t stream);

/* ---- mask apply ------------------------------------------------------------------------------------ */

/* y = x * mask with a broadcast bool mask (qsparse/sparse.py:66,116,122,263) and, with g in place of x,
 * its backward g * mask.  The tensor is described by `ndim` collapsed extents `sizes`; `mask_strides[d]`
 * is the mask's element stride along d (0 where the mask has extent 1).
 * pre_relu != 0: y = max(x, 0) * mask, a preceding nn.ReLU folded into the prune site; only for masks that
 * vary along one run of dims (channel masks; QS_ERR_ARG otherwise).  Its backward is
 * qs_quant_ste_relu_bwd with step_host = 1 and lo_mul / hi_mul = -inf / +inf.
 * elide_masked != 0 (channel-type masks): pruned channels are not loaded and y = +0.0 there; the reference's x*0
 * carries the sign of x, so this is numerically equal, not bit-identical (opt-in).
 * gate_out (nullable; needs pre_relu != 0): the ReLU's gate bitmap for that backward, as in qs_quant_scaler_fwd. */
int qs_mask_apply(const void* x, const uint8_t* mask, void* y, int ndim, const int64_t* sizes,
                  const int64_t* mask_strides, int dt, int pre_relu, int elide_masked, uint8_t* gate_out,
                  qs_stream_t stream);

/* ---- fused channel-prune -> tensor-wise-quantize statistics (the headline pair) -------------------- */

/* One launch over C-sized state, replacing (per training step of the pair
 * Sequential(PruneLayer(dims={1}), QuantizeLayer(channelwise=-1)) built by convert(), convert.py:214-218):
 *   magnitude  <- (t_mag*magnitude + f32(stage_mean))/(t_mag+1)       if update_magnitude   (sparse.py:89)
 *   mask       <- magnitude >= sort(magnitude)[k]                      if refresh_mask       (util.py:113-117)
 *   absmax_all <- max over channels with mask != 0 of chan_absmax      (== max|x*mask|, quantize.py:329-340; a pruned
 *                 channel whose chan_absmax is Inf / NaN contributes a NaN: its x * 0 is NaN in the product the reference
 *                 takes x.abs().max() of, so the scale turns NaN there too)
 *   scale      <- t_q == 0 ? new : (t_q*scale + new)/(t_q+1), new = absmax_all/2^(bits-1)  if update_scale
 * stage_mean is the last squeeze stage's output ([C] in dtype sdt).  Single workgroup; C <= 65536.
 * chan_absmax[c * chan_absmax_stride] (stride as for qs_mean_dim's absmax_out, >= 1) is zeroed after use when
 * update_scale != 0.  bump_i32_a / bump_i32_b / bump_i64_a / bump_i64_b
 * (each nullable) are one-element device counters incremented by one at the end: the layers' `_n_updates`,
 * the pruning callback's `t` and the quantizer's device-side `t` (sparse.py:117,272; quantize.py:348,515), so
 * that a step needs no separate counter kernels.  t_mag_dev / t_q_dev: see "Step counters" above.  stat_dt: dtype
 * of the activation (the new scale's quotient is rounded to it, as in qs_scale_update).
 * gathered (nullable, device float[world][2*C]): the all-gathered qs_stats_pack records of a data-parallel run.  When
 * given, channel c's importance is (sum over ranks, in rank order, of gathered[r][c]) / world and its abs-max the
 * maximum over ranks of gathered[r][C + c] -- what qs_stats_combine computes -- read INSTEAD of stage_mean and
 * chan_absmax (which, when non-NULL, is still zeroed).
 * elide_mask_out (nullable, with update_scale): [C] bytes for a forward that skips the loads of pruned channels -- 1 for a kept
 * channel, 0 for a pruned channel whose abs-max this step is finite (x * 0 is a zero whatever x is: its loads may be skipped), 2
 * for a pruned channel that holds a NaN / Inf (x * 0 is NaN there and rounds to INT_MIN, quantize.py:109 on CPU: it must be
 * loaded).  Passed as the forward's chan_mask together with elide_masked, elision is bit-identical to the loading path for EVERY
 * input. */
int qs_pq_select(float* magnitude, const void* stage_mean, int sdt, int64_t C,
                 int update_magnitude, int64_t t_mag,
                 int refresh_mask, int64_t k, uint8_t* mask,
                 float* chan_absmax, int64_t chan_absmax_stride, int update_scale, int64_t t_q, int bits, float* scale,
                 int32_t* bump_i32_a, int32_t* bump_i32_b, int64_t* bump_i64_a, int64_t* bump_i64_b,
                 const int64_t* t_mag_dev, const int64_t* t_q_dev, int stat_dt, const float* gathered, int world,
                 uint8_t* elide_mask_out, qs_stream_t stream);

/* (ABI v25) qs_pq_select with its operands in a descriptor */
typedef struct qs_pq_select_args {
    uint32_t struct_size;        /* sizeof(qs_pq_select_args) as the caller compiled it */
    int32_t sdt, stat_dt, bits, world;
    int32_t update_magnitude, refresh_mask, update_scale;
    float* magnitude;
    const void* stage_mean;
    int64_t C, t_mag, k, t_q;
    uint8_t* mask;
    float* chan_absmax;
    int64_t chan_absmax_stride;
    float* scale;
    int32_t* bump_i32_a;
    int32_t* bump_i32_b;
    int64_t* bump_i64_a;
    int64_t* bump_i64_b;
    const int64_t* t_mag_dev;
    const int64_t* t_q_dev;
    const float* gathered;
    uint8_t* elide_mask_out;
    qs_stream_t stream;
} qs_pq_select_args;
int qs_pq_select_v(const qs_pq_select_args* args);

/* ---- data-parallel statistics exchange (no counterpart in the reference, whose masks and scales drift per rank) -- */

/* record[0..C) = f32(stage[i]) (0 when stage == NULL), record[C..2C) = absmax[i * absmax_stride] (0 when NULL):
 * the per-rank record of the fused pair's statistics, to be all-gathered by the caller (RCCL / any transport). */
int qs_stats_pack(const void* stage, int sdt, const float* absmax, int64_t absmax_stride, int64_t C, float* record,
                  qs_stream_t stream);

/* gathered = `world` records of 2C floats in rank order.  stage_out[i] = (sum over ranks, in rank order) / world;
 * absmax_out[i * absmax_stride] = max over ranks.  Either output may be NULL. */
int qs_stats_combine(const float* gathered, int world, int64_t C, float* stage_out, float* absmax_out,
                     int64_t absmax_stride, qs_stream_t stream);

/* ---- one activation site per call ------------------------------------------------------------------- */

/* A convert-built activation site -- Sequential(Sequential(act, PruneLayer{dims={1}}), QuantizeLayer{tensor-wise
 * ScalerQuantizer}), reference convert.py:214-218 -- runs, per training step, the launches
 *     statistics (qs_mean_dim | qs_mean_dim_cl)  ->  qs_mean_last2  ->  qs_pq_select  ->  qs_quant_scaler_fwd
 * and one launch backward.  Issued one by one from the host language each of them costs an FFI transition plus argument
 * marshalling (20-30 us of Python each); these two entry points enqueue the whole sequence from ONE call.  They add no
 * arithmetic: they call the entry points above with the arguments the plan describes, in that order, on `stream`.
 *
 * The plan names what does not change from step to step: the geometry of x as the kernels address it (NCHW-contiguous:
 * layout 0, x = [N][C][H*W]; dense channels_last: layout 1, x = [N][H*W][C]; a 2-d activation [N][C] -- nn.Linear's output:
 * layout 2 with H = W = 1, whose statistics are ONE qs_mean_dim launch, no qs_mean_last2), dtypes, the layer state (running
 * magnitude, mask, running scale, step counters -- all device pointers, the objects PruneLayer / QuantizeLayer /
 * MagnitudePruningCallback hold, reference sparse.py:58-122, quantize.py:327-349, 473-518) and the caller's workspaces
 * (stage: C*H*W elements of xdt; amax_part: C*H*W floats, channels_last only; chan_absmax: C * absmax_stride floats,
 * zero on entry and re-zeroed by the select).  The caller builds it once per site and input signature and rebuilds it
 * when a pointer or a shape changes. */
typedef struct qs_site_plan {
    int64_t N, C, H, W;
    int32_t layout;              /* 0: NCHW-contiguous, 1: channels_last (NHWC in memory), 2: [N][C] (H = W = 1) */
    int32_t xdt, ydt;            /* input dtype; output dtype (QS_F32: the reference's promotion, or xdt) */
    int32_t bits;                /* of the quantizer */
    float* magnitude;            /* [C]  MagnitudePruningCallback.magnitude */
    uint8_t* mask;               /* [C]  PruneLayer.mask */
    float* scale;                /* [1]  QuantizeLayer.weight */
    float* chan_absmax;          /* [C * absmax_stride] scratch accumulator */
    int64_t absmax_stride;
    void* stage;                 /* [C*H*W] xdt scratch: first-stage means (unused, nullable, for layout 2) */
    float* amax_part;            /* [C*H*W] scratch (layout 1; layout 3, nullable there: qs_token_stats' per-column keys), NULL for layout 0 */
    void* stage_mean;            /* [C] xdt scratch: the importance of this step */
    int32_t* prune_n_updates;    /* nullable: PruneLayer._n_updates, incremented by the select */
    int32_t* quant_n_updates;    /* nullable: QuantizeLayer._n_updates, incremented by the select */
    int64_t* callback_t;         /* nullable: MagnitudePruningCallback.t, incremented by the select */
    int64_t* quantizer_t_dev;    /* nullable: device copy of the quantizer callback's t (graph-safe mode): read instead of
                                    t_q and incremented */
    int32_t callback_t_from_device; /* != 0: the running-magnitude counter is read from *callback_t instead of t_mag */
    int32_t saturate;            /* != 0: codes are clamped to [code_lo, code_hi] (qs_quant_scaler_fwd's opt-in saturation) */
    int32_t code_lo, code_hi;
    int32_t act;                 /* the activation QS_SITE_PRE_RELU folds: 0 / 1 nn.ReLU, else a qs_activation() handle */
    uint8_t* elide_mask;         /* nullable: [C] scratch, qs_pq_select's elide_mask_out: the chan_mask of an eliding forward on the
                                    steps that have statistics (QS_SITE_LIVE), exact for every x; without it, and on steps without
                                    statistics, QS_SITE_ELIDE elides through the mask itself (exact for finite x only) */
    float* absmax_dense;         /* nullable: [C] scratch accumulator of QS_SITE_SCALE_ONLY steps (zero on entry, re-zeroed by the select) */
    void* reduce_ws;             /* nullable: qs_absmax's `ws` for this geometry (QS_SITE_SCALE_ONLY steps) */
    int64_t reduce_ws_bytes;
} qs_site_plan;

/* flags of qs_site_fwd */
#define QS_SITE_LIVE 1        /* training step with live statistics: magnitude and scale are updated (else: apply only) */
#define QS_SITE_REFRESH 2     /* rebuild the mask from the running magnitude, threshold rank k */
#define QS_SITE_PRE_RELU 4    /* x is the input of a folded activation (plan->act; nn.ReLU by default) */
#define QS_SITE_ELIDE 8       /* elide_masked of qs_quant_scaler_fwd (through plan->elide_mask on QS_SITE_LIVE steps) */
#define QS_SITE_NO_MASK 16    /* apply without the channel mask (pruning not started) -- only without QS_SITE_LIVE */
#define QS_SITE_STATS_DONE 32 /* with QS_SITE_LIVE: the statistics launches were already enqueued by qs_site_stats (a data-parallel
                                 step: the caller exchanged the record in between); qs_site_fwd starts at the select */
#define QS_SITE_NO_QUANT 128  /* the site is a PruneLayer ALONE (reference sparse.py:215-273 behind an activation, convert.py:214-218;
                                 plan->scale and the quantizer fields are unused): with QS_SITE_LIVE the statistics are the staged
                                 mean alone (no abs-max), with QS_SITE_LIVE or QS_SITE_REFRESH the select updates magnitude / mask /
                                 the prune counters, and the apply is y = act?(x) * mask in x's dtype (qs_mask_apply); qs_site_bwd
                                 with the flag: gx = gate * g * mask (qs_quant_ste_relu_bwd without a clamp) or g * mask */
#define QS_SITE_SCALE_ONLY 64 /* with QS_SITE_LIVE: the mask is frozen (MagnitudePruningCallback.t passed stop_mask_refresh,
                                 sparse.py:107-116 -- the steady state of devise_layerwise_pruning_schedule recipes, :343-359):
                                 magnitude and mask stay, the statistics are qs_absmax per channel into plan->absmax_dense
                                 and the select updates the scale (max over the kept channels) and the counters */

/* y = Q(relu?(x) * mask); with QS_SITE_LIVE preceded by statistics + select exactly as the four calls above.
 * gate_out, image_out / imgdt, xback_out: nullable, see qs_quant_scaler_fwd.  t_mag / t_q: the running-mean counters of this step (reference
 * sparse.py:88, quantize.py:344), k: threshold rank (util.py:115-116).  gathered / world: nullable / 1; the all-gathered
 * records of qs_site_stats (see there and qs_pq_select).
 * decimal: NULL for a ScalerQuantizer; else the site's quantizer is a DecimalQuantizer (reference quantize.py:275-367, same
 * running scale, power-of-two step): device float[1] of THIS call, which receives qs_decimal_from_scale(plan->scale) after the
 * select (one more launch) and is what qs_quant_decimal_fwd applies -- and what qs_site_bwd of this forward must be given. */
int qs_site_fwd(const qs_site_plan* plan, const void* x, void* y, uint8_t* gate_out, int flags, int64_t t_mag, int64_t k,
                int64_t t_q, void* image_out, int imgdt, const float* gathered, int world, void* xback_out, float* decimal,
                qs_stream_t stream);

/* (ABI v25) qs_site_fwd with its per-call operands in a descriptor */
typedef struct qs_site_fwd_args {
    uint32_t struct_size;        /* sizeof(qs_site_fwd_args) as the caller compiled it */
    int32_t flags, imgdt, world;
    const void* x;
    void* y;
    uint8_t* gate_out;
    int64_t t_mag, k, t_q;
    void* image_out;
    const float* gathered;
    void* xback_out;
    float* decimal;
    qs_stream_t stream;
} qs_site_fwd_args;
int qs_site_fwd_v(const qs_site_plan* plan, const qs_site_fwd_args* args);

/* The statistics half of a live qs_site_fwd on its own -- qs_mean_dim | qs_mean_dim_cl, then qs_mean_last2, which also writes
 * this rank's exchange record (record: device float[2*C] = importance | per-channel abs-max, qs_stats_pack's layout) -- for a
 * data-parallel step: the caller all-gathers the records of all ranks (RCCL / any transport) and passes them to
 * qs_site_fwd(flags | QS_SITE_STATS_DONE, gathered, world), whose select combines them in rank order (qs_pq_select's
 * `gathered`).  Two calls and one collective per site instead of five calls; the reference has no counterpart (its masks and
 * scales drift per rank, sparse.py:58-122 / quantize.py:327-349 run on the rank's shard only).  flags: QS_SITE_PRE_RELU. */
int qs_site_stats(const qs_site_plan* plan, const void* x, int flags, float* record, qs_stream_t stream);

/* gx = gate * clamp(g) * mask in xdt (qs_quant_ste_relu_bwd with the bitmap when `gate` is given, qs_quant_ste_bwd
 * otherwise); g has dtype gdt, the geometry of the plan.  lo_mul / hi_mul as there.  g2 / g2dt: the second gradient of
 * qs_quant_ste_relu_bwd (needs `gate`; g may then be NULL).  decimal: NULL (the clamp follows plan->scale) or the float[1] its
 * forward call filled (DecimalQuantizer: the clamp follows 2^-decimal). */
int qs_site_bwd(const qs_site_plan* plan, const void* g, const uint8_t* gate, void* gx, int gdt, int flags, float lo_mul,
                float hi_mul, const void* g2, int g2dt, const float* decimal, qs_stream_t stream);

/* (ABI v25) qs_site_bwd with its operands in a size-prefixed descriptor; g3 / gx_image / gx_image_dt as in
 * qs_ste_relu_bwd_args (they need `gate` and a float32 site: plan->xdt == gdt == QS_F32). */
typedef struct qs_site_bwd_args {
    uint32_t struct_size;        /* sizeof(qs_site_bwd_args) as the caller compiled it */
    int32_t flags;
    int32_t gdt, g2dt;
    const void* g;
    const uint8_t* gate;
    void* gx;
    float lo_mul, hi_mul;
    const void* g2;
    const float* decimal;
    qs_stream_t stream;
    /* ---- v25 ---- */
    const void* g3;
    void* gx_image;
    int32_t gx_image_dt;
    int32_t reserved0;
    /* ---- v26 ---- */
    const void* act_x;           /* the caller's activation, as in qs_ste_relu_bwd_args (needs a quantizing site; `gate` is not read) */
    int32_t act_x_kind;
    int32_t reserved1;
} qs_site_bwd_args;
int qs_site_bwd_v(const qs_site_plan* plan, const qs_site_bwd_args* args);

/* A lone tensor-wise ScalerQuantizer step -- QuantizeLayer.forward in training (reference quantize.py:473-518 with
 * optimize :327-349 and ScalerQuantization.forward :100-117) -- from ONE call: with `update` != 0
 *     qs_absmax(x, amax_lines, tensor-wise, accumulate, pre_relu, lines)  ->  qs_scale_update(amax_lines, lines, scale, 1, t,
 *     t_dev, advance, bits, clear, n_updates, xdt)  ->  qs_quant_scaler_fwd(x, y, scale, pre_relu, gate_out)
 * and with `update` == 0 the last of them alone (evaluation).  amax_lines: [lines][QS_AMAX_LINE_STRIDE] floats, zero on entry,
 * re-zeroed by the update; n_updates (nullable) is incremented; t_dev (nullable) is read instead of t and incremented.
 * image_out / imgdt (ABI v21): the autocast image of qs_quant_scaler_fwd -- RNE(y) in bf16 / fp16 from the same pass, for the
 * convolution behind a quantize-only activation site (needs pre_relu, gate_out and qs_quant_image_ok(1, 1, numel, ...)). */
#define QS_QSTEP_APPLY 0      /* `update` of qs_quantize_step: quantize only (evaluation) */
#define QS_QSTEP_ALL 1        /* abs-max, running scale, quantize */
#define QS_QSTEP_ABSMAX 2     /* the abs-max launch alone (y may be NULL): a data-parallel step all-reduces (MAX) the accumulator
                                 lines between this call and the next */
#define QS_QSTEP_FINISH 3     /* running scale from the (reduced) accumulator lines, then quantize */
int qs_quantize_step(const void* x, void* y, uint8_t* gate_out, float* amax_lines, int lines, float* scale, int64_t numel,
                     int xdt, int ydt, int bits, int64_t t, int64_t* t_dev, int32_t* n_updates, int pre_relu, int update,
                     int saturate, int32_t code_lo, int32_t code_hi, void* xback_out, void* image_out, int imgdt, qs_stream_t stream);

/* (ABI v25) qs_quantize_step with its operands in a descriptor */
typedef struct qs_quantize_step_args {
    uint32_t struct_size;        /* sizeof(qs_quantize_step_args) as the caller compiled it */
    int32_t lines, xdt, ydt, bits, pre_relu, update, saturate, code_lo, code_hi, imgdt;
    const void* x;
    void* y;
    uint8_t* gate_out;
    float* amax_lines;
    float* scale;
    int64_t numel, t;
    int64_t* t_dev;
    int32_t* n_updates;
    void* xback_out;
    void* image_out;
    qs_stream_t stream;
} qs_quantize_step_args;
int qs_quantize_step_v(const qs_quantize_step_args* args);

/* ---- multi-tensor weight path ---------------------------------------------------------------------- */

/* The weight-side operators of a converted network (quantize(conv) / quantize(linear), reference quantize.py:559-571
 * through imitation.py:61-68) are the same three small kernels per layer and step: abs-max, running scale, quantization.
 * These entry points run them for a LIST of float32 tensors in one launch each.  The list is a DEVICE-resident table of
 * qs_multi_row that the caller builds once per set of layers (host copy -> qs_multi_plan fills the derived fields -> upload)
 * and reuses every step; what changes from step to step -- the output buffer, which rows train -- is either an argument
 * (`ybase`) or a field the caller rewrites.  Tensor-wise AND per-channel Scaler / Decimal quantizers: a tensor is the
 * CONTIGUOUS [outer, C, inner] view around the reference's channel dim (C == 1, outer == 1, inner == numel for tensor-wise;
 * the reference's default for weights is channelwise=1, quantize.py:524); parameters have C entries.
 *   qs_multi_absmax        rows with train != 0: amax[c] = max(amax[c], max |x| over channel c)   (quantize.py:329-340; keep
 *                          the accumulators zero between steps -- the update below re-zeroes them)
 *   qs_multi_scale_update  rows with train != 0, every channel c: t = *t_dev + t_offset;
 *                          scale[c] <- t == 0 ? new : (t*scale[c] + new)/(t+1), new = amax[c] / 2^(bits-1) (denom)   (:344-347);
 *                          amax[c] <- 0; decimal[c] <- rint(log2(nan_to_num(1/scale[c]))) where decimal != NULL (:316);
 *                          backup[c] (nullable) <- the scale this update replaces, so that a caller that evaluated a layer
 *                          ahead of time can restore one the forward pass then never reached (imitation.py:61-68 evaluates
 *                          the operator only when the layer's weight is read)
 *   qs_multi_quant_fwd     every row: y[e] = Q(x[e]) with the scale (is_decimal == 0: qs_quant_scaler_fwd's arithmetic) or the
 *                          decimal (qs_quant_decimal_fwd's) of e's channel, y = ybase + y_off; codes clamped to
 *                          [code_lo, code_hi] where code_lo <= code_hi (the opt-in saturation).  advance != 0: the counters of
 *                          the rows that trained -- *t_dev (quantizer callback's t, quantize.py:348) and *bump (the layer's
 *                          `_n_updates`, :515) -- are incremented here, i.e. after every thread of the preceding
 *                          qs_multi_scale_update has read them (stream order).  A callback shared by a layer's weight and
 *                          bias quantizers (:548,559-571) is two rows with the same t_dev and t_offset 0 / 1.
 * A PRUNED weight -- quantize(prune(conv)): the quantizer's input is weight * mask (sparse.py:263 through imitation.py:61-68) --
 * is a row with `mask` set: every x[e] above reads x[e] * mask[.] (the product itself, so that a non-finite weight under a
 * pruned position behaves as in the reference).  mask_C == 0: one mask byte per element; else the mask varies along one run of
 * dims: byte (e / mask_inner) % mask_C.  Steps on which the prune operator only applies its mask take part (before `start`
 * without a mask; after the schedule with a frozen or a still-averaging full-shape magnitude); its counters -- prune_n_updates
 * (PruneLayer._n_updates, sparse.py:272) and prune_t (MagnitudePruningCallback.t, :117) -- are incremented next to the
 * quantizer's where non-NULL.
 *   qs_multi_magnitude     rows with magnitude != NULL (full-shape masks): t = *prune_t;
 *                          mag_backup[e] <- magnitude[e]; magnitude[e] <- (t*magnitude[e] + |x[e]|)/(t+1)   (sparse.py:82-89);
 *                          launched BEFORE qs_multi_quant_fwd (which advances prune_t)
 *   qs_multi_mask_refresh  rows with refresh != 0 (full-shape masks): the mask rebuild of MagnitudePruningCallback
 *                          (sparse.py:58-66 -> util.py:103-117): thr = the select_k-th smallest importance (importance =
 *                          `importance` when non-NULL -- the running magnitude, after qs_multi_magnitude -- else |x|), by the
 *                          4-pass radix select of qs_kth_value run for all rows at once (select_state: 258 uint32 of scratch
 *                          per row, zero before the first use); mask_backup[e] <- mask[e]; mask[e] <- importance[e] >= thr.
 *                          Nine launches for the whole table; BEFORE qs_multi_absmax (the quantizer sees the new mask). */
typedef struct qs_multi_row {
    const float* x;              /* the tensor, 4-byte aligned (16-byte aligned tensors take the vector paths) */
    float* scale;                /* [C] running scale (QuantizeLayer.weight) */
    float* amax;                 /* [C] abs-max accumulator, zero between steps */
    float* decimal;              /* [C] or NULL: decimals of a DecimalQuantizer (written by the update, read by the quantizer) */
    float* backup;               /* [C] or NULL */
    int64_t* t_dev;              /* device copy of the quantizer callback's running-mean count (required when train != 0) */
    int32_t* bump;               /* nullable: the layer's `_n_updates` */
    int64_t numel, y_off;        /* elements; offset of the output in `ybase`, elements */
    int64_t outer, inner;        /* [outer, C, inner] */
    int32_t C;
    int32_t train;               /* != 0: this row updates its statistics this step */
    int32_t is_decimal;
    int32_t t_offset;            /* added to *t_dev (1 for the bias quantizer that shares its weight quantizer's callback) */
    int32_t code_lo, code_hi;    /* code_lo > code_hi: no saturation */
    float denom;                 /* 2^(bits-1) */
    const uint8_t* mask;         /* nullable: the prune operator's mask (bool bytes) */
    int64_t mask_inner;          /* see above (ignored with mask_C == 0) */
    int32_t mask_C;              /* 0: one mask byte per element */
    int32_t kind;                /* 0: a weight / bias row.  1: a MASK-LEVEL row -- the importance of a pruned weight whose mask
                                    varies along a subset of dims (x: [numel] float, the staged mean of |weight| that
                                    qs_multi_stage_mean produced this step; numel = the mask's): it takes part in
                                    qs_multi_magnitude and qs_multi_mask_refresh only (scale may be NULL, nothing is quantized).
                                    2: a weight that is NOT quantized on this read -- prune(conv) without a quantizer, or a
                                    quantizer still in its identity phase (quantize.py:496-517: it only counts): y = x * mask
                                    (x where mask == NULL), `bump` (nullable: the idle quantizer's `_n_updates`) incremented,
                                    scale may be NULL */
    int32_t* prune_n_updates;    /* nullable */
    int64_t* prune_t;            /* nullable (required with magnitude) */
    float* magnitude;            /* nullable: [numel] running magnitude, updated by qs_multi_magnitude */
    float* mag_backup;           /* [numel] with magnitude: what the update replaced */
    int32_t refresh;             /* != 0: qs_multi_mask_refresh rebuilds this row's (full-shape, writable) mask */
    uint32_t select_k;           /* rank of the threshold element, ascending (util.py:115-116) */
    const float* importance;     /* nullable: [numel] importance to rank by (NULL: |x|) */
    uint32_t* select_state;      /* [258] scratch of the radix select */
    uint8_t* mask_backup;        /* [numel]: what the rebuild replaced */
    /* derived by qs_multi_plan: */
    int32_t row_splits, absmax_block0, absmax_blocks, quant_block0, chan0, hist_block0, hist_blocks, reserved1;
} qs_multi_row;

/* fills the derived fields of a HOST table in place and returns the launch totals; QS_ERR_ARG for an inconsistent row */
int qs_multi_plan(qs_multi_row* rows_host, int n, int* absmax_blocks, int* quant_blocks, int* channels, int* hist_blocks_out);
int qs_multi_absmax(const qs_multi_row* rows_dev, int n, int absmax_blocks, qs_stream_t stream);
int qs_multi_scale_update(const qs_multi_row* rows_dev, int n, int channels, qs_stream_t stream);
int qs_multi_quant_fwd(const qs_multi_row* rows_dev, int n, int quant_blocks, float* ybase, int advance, qs_stream_t stream);
int qs_multi_magnitude(const qs_multi_row* rows_dev, int n, int quant_blocks, qs_stream_t stream);
/* The importance of pruned weights whose mask varies along a SUBSET of dims (prune()'s default dimensions={1}: one mask entry
 * per input channel) is squeeze_tensor_to_shape(|weight|, mask.shape) (reference util.py:79-99 via sparse.py:82-89): one mean per
 * reduced dim, ascending, each rounded to float32.  qs_multi_stage_mean runs ONE such stage for a list of tensors: entry i
 * averages the middle dim of the contiguous [pre, n, post] tensor x into out [pre, 1, post] (layout 0; |x| first with take_abs),
 * or -- layout 1, the first stage of a channels_last weight -- the leading dim of x = [n][hw = pre][C = post] in memory into the
 * NCHW-contiguous out [C][hw], in ATen's CPU summation order for that case (the orders of qs_mean_dim / qs_mean_dim_cl, one
 * lane per output element).  The caller launches it once per stage level; qs_multi_stage_plan fills block0 of a HOST table. */
typedef struct qs_multi_stage {
    const float* x;
    float* out;
    int64_t pre, n, post;
    int32_t take_abs, layout;
    int32_t block0, reserved;     /* derived */
} qs_multi_stage;
int qs_multi_stage_plan(qs_multi_stage* stages_host, int n, int* blocks);
int qs_multi_stage_mean(const qs_multi_stage* stages_dev, int n, int blocks, qs_stream_t stream);

/* hist_blocks: the total qs_multi_plan returned through *hist_blocks_out (0: no row refreshes) */
int qs_multi_mask_refresh(const qs_multi_row* rows_dev, int n, int hist_blocks, int quant_blocks, qs_stream_t stream);
/*   qs_multi_ste_bwd:       gx[i][e] = clamp(g[i][e], lo_mul[i] * s, hi_mul[i] * s) with s = step[i][c] (or 2^-step[i][c] with
 *                           step_is_decimal), c the channel of e in the contiguous [*, C[i], inner[i]] view the gradient has
 *                           (C == NULL: tensor-wise, one step per tensor): qs_quant_ste_bwd's arithmetic (quantize.py:66-77,
 *                           120-131) for the gradients of a GROUP of weight quantizers that are handed over together.  The
 *                           gradients are fresh tensors every step: HOST arrays of length n of device pointers / values.
 *                           mask / mask_C / mask_inner (each array nullable, entries nullable / 0): the pruned weight's
 *                           backward, gx = clamp(g) * mask (the product: a signed zero under a pruned position, sparse.py:263). */
int qs_multi_ste_bwd(int n, const float* const* g, float* const* gx, float* const* step, const int64_t* numel,
                     const int32_t* C, const int64_t* inner, const float* lo_mul, const float* hi_mul, int step_is_decimal,
                     const uint8_t* const* mask, const int32_t* mask_C, const int64_t* mask_inner, qs_stream_t stream);

/* ---- data-parallel statistics exchange through peer-mapped mailboxes (prototype, ABI v24) -----------------------------------
 * The collective form of the exchange (qs_stats_pack / the record written by the last statistics launch -> all-gather ->
 * qs_pq_select / qs_site_fwd with `gathered`) costs a host-bound network ~40 us of host time per site and step.  The mailbox form
 * replaces the collective by two launches.  Every rank allocates one mailbox per site (qs_mailbox_bytes / qs_mailbox_alloc:
 * fine-grained device memory, zeroed), exports it (qs_mailbox_export: a 64-byte hipIpcMemHandle_t the caller ships to the peers by
 * whatever means it has) and maps its peers' (qs_mailbox_open).  Per step, after the statistics launches have written this rank's
 * n-float record: qs_mailbox_publish stores the record into slot `rank` of EVERY mailbox in `boxes` (host array of `world` device
 * pointers, this rank's own included; one-sided stores over xGMI), fences system-wide and raises flag `rank` there to `step`;
 * qs_mailbox_wait spins -- at most max_spins polls per rank, never a hang -- until every flag of the local mailbox shows `step`,
 * and returns in *records the [world][n] float records of this step (a device pointer into the mailbox: the `gathered` argument
 * of qs_pq_select / qs_site_fwd, combined in rank order there as after the all-gather).  A rank whose flag did not arrive in time
 * is FATAL FOR THE STEP (ABI v25): *status = 1 + that rank and its record of this step is overwritten with NaNs before anything
 * reads it, so the statistics -- magnitude, scale, output -- of a rank that missed a peer turn NaN at once instead of drifting on a
 * stale record; the caller polls *status (one word; asynchronously is enough) and stops.
 * qs_mailbox_alloc returns fine-grained memory or an error (ABI v25: no coarse-grained fall-back -- a peer's stores would not be
 * guaranteed visible to the local acquire loads); the caller then keeps the collective exchange.
 * qs_records_max (ABI v25): out[i] = max over ranks of records[r][i] as uint32 keys -- the all-reduce (MAX) of a quantize-only
 * site's abs-max accumulator lines (qs_quantize_step, QS_QSTEP_ABSMAX / _FINISH) taken from the mailbox.
 * `step` counts from 1 and alternates between the mailbox's two halves; no rank can be more than one step ahead of the slowest
 * (its next publish is ordered behind its own select), so a half is never written while it is read.  qs_mailbox_alloc / _free /
 * _open / _close are set-up calls: they allocate, map and synchronise like the hip calls they wrap. */
size_t qs_mailbox_bytes(int world, int64_t n);
int qs_mailbox_alloc(size_t bytes, void** ptr);
int qs_mailbox_free(void* ptr);
int qs_mailbox_export(void* ptr, void* handle64);
int qs_mailbox_open(const void* handle64, void** ptr);
int qs_mailbox_close(void* ptr);
int qs_mailbox_publish(const float* rec, int64_t n, void* const* boxes, int world, int rank, uint32_t step, qs_stream_t stream);
int qs_mailbox_wait(void* box, int world, int64_t n, uint32_t step, int32_t* status, uint32_t max_spins, const float** records,
                    qs_stream_t stream);
int qs_records_max(const float* records, int world, int64_t n, float* out, qs_stream_t stream);

/* ---- MX block-scaled quantizer (OCP Microscaling Formats v1.0), ABI v27; rounding modes v28 ------------------------------------
 * The tensor is CONTIGUOUS memory seen as [outer, n, inner]; a block is 32 consecutive elements along `n` (the last block of a
 * line is shorter when n % 32 != 0), nb = ceil(n / 32) blocks per line.  Per block, on the float32 widening of x:
 *   amax = max |x_i|.  NaN or Inf: every y_i of the block is NaN, the scale byte 0xFF, every code 0.
 *   e = clamp(floor(log2(amax)) - emax, -127, 127), -127 for amax == 0 (the exponent is taken from the bits, float32 subnormals
 *   included);  scale byte = e + 127 (E8M0);  X = 2^e
 *   q_i = x_i / X rounded to nearest, ties to even (`rounding` == QS_MX_ROUND_NEAREST, the default; stochastic: below), onto the
 *   element format's value grid (its subnormals included), then clamped to +- the largest normal; a zero keeps its sign; no
 *   format's own NaN / Inf code is ever produced
 *   y_i = q_i * X (exact in float32, subnormals kept), rounded once to ydt
 *   codes[i] (nullable; uint8, x's geometry) = the format's encoding of q_i -- sign, exponent, mantissa -- in the low bits
 *   (QS_MX_FP8_E4M3 / _E5M2: the bytes of OCP e4m3fn / e5m2);  scales (nullable; uint8 [outer, nb, inner]) = the scale bytes.
 * ydt is QS_F32 or xdt.  inner == 1 selects the innermost-axis kernels: with n % 32 == 0 and x, y (and codes: 8 bytes) 16-byte
 * aligned the 16-bytes-per-lane form, otherwise one element per lane; inner > 1 the strided-axis kernel (lanes along `inner`).
 * x, y need the alignment of their element type only (QS_ERR_ALIGN otherwise).  One pass over the data, no workspace.
 *
 * (v28) `rounding` == QS_MX_ROUND_STOCHASTIC changes ONE step of the definition above: how q_i is chosen between the two grid
 * values that enclose v = x_i * 2^-e (float32, as before).  abs-max, scale byte, X, the NaN / Inf block, the clamp and the codes
 * are unchanged.
 *   ab = bits of |v|;  E = max(ab >> 23, 1);  m = (ab & 0x7FFFFF) | (ab >> 23 ? 0x800000 : 0)          (|v| = m 2^(E - 150))
 *   ex = max(E, float32-biased exponent of the format's smallest normal);  sh = (23 - mbits) + (ex - E)   (>= 20)
 *   T  = sh <= 56 ? floor(m 2^32 / 2^sh) : 0  in 64 bits;  n = (T + w) >> 32  with w the element's 32-bit random word
 *   |q| = min(n 2^(ex - 127 - mbits), largest normal), the sign of v kept (a negative value that rounds to zero is -0)
 * A value on the grid is returned unchanged for every w; w = 0 truncates toward zero; E[q] = v for every v that is not clamped.
 * Random words, one per code, a pure function of the operands below (counter-based, no generator state):
 *   j = index_base + the row-major linear index of the code in ITS OWN output tensor (codes / x for qs_mx_quant_fwd_v; row_codes
 *       [R, C] for the row pair, col_codes [C, R] for the col pair), 64 bits
 *   k = seed + (step ? (uint64_t)*step : 0)  mod 2^64 -- *step is read by the KERNEL when it runs, never written: a launch captured
 *       in a graph draws new words on every replay once the owner advances the counter on the stream
 *   (o0, o1, o2, o3) = Philox4x32-10(counter = (lo32(j >> 2), hi32(j >> 2), rng_stream, 0), key = (lo32(k), hi32(k)))
 *       (Random123's constants: multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85);  w = o[j & 3]
 *   rng_stream: the descriptor's for qs_mx_quant_fwd_v; 0 for the row pair and 1 for the col pair of qs_mx_quant2_v -- so the col
 *       pair is what qs_mx_quant_fwd_v writes for the transpose of x with rng_stream = 1, the row pair what it writes for x with 0.
 * Routes and alignment rules do not depend on the mode.  QS_ERR_ARG, checked first and in both modes: a rounding that is neither
 * mode, a step pointer that is not 8-byte aligned, an index_base that is no multiple of 4.  No atomics.  A caller that passes the
 * v27 struct_size leaves the five rounding fields 0 / NULL: nearest. */
#define QS_MX_ROUND_NEAREST 0
#define QS_MX_ROUND_STOCHASTIC 1
enum qs_mx_format { QS_MX_FP8_E4M3 = 0, QS_MX_FP8_E5M2 = 1, QS_MX_FP6_E2M3 = 2, QS_MX_FP6_E3M2 = 3, QS_MX_FP4_E2M1 = 4 };
#define QS_MX_BLOCK 32
typedef struct qs_mx_quant_args {
    uint32_t struct_size;        /* sizeof(qs_mx_quant_args) as the caller compiled it */
    int32_t format;              /* enum qs_mx_format */
    const void* x;
    void* y;
    uint8_t* codes;              /* nullable */
    uint8_t* scales;             /* nullable */
    int32_t xdt, ydt;
    int64_t outer, n, inner;
    qs_stream_t stream;
    int32_t rounding;            /* (v28) QS_MX_ROUND_* */
    int32_t rng_stream;          /* (v28) third counter word (`stream` above is the HIP stream) */
    uint64_t seed;               /* (v28) */
    const int64_t* step;         /* (v28) nullable (= 0); device memory, one int64, read by the kernel */
    uint64_t index_base;         /* (v28) a multiple of 4 */
} qs_mx_quant_args;
int qs_mx_quant_fwd_v(const qs_mx_quant_args* args);
/* the kernel qs_mx_quant_fwd_v launches for these operands, decided by the code that launches it and without enqueuing anything:
 * one of QS_MX_ROUTE_*, 0 for an empty tensor, or the QS_ERR_* the call would return */
#define QS_MX_ROUTE_INNER_VEC 1
#define QS_MX_ROUTE_INNER_PLAIN 2
#define QS_MX_ROUTE_STRIDED 3
int qs_mx_quant_route(const qs_mx_quant_args* args);

/* ---- MX matrix product (block-scaled MFMA) -----------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (27): by the rule above prototypes are frozen and symbols are only ever added, so a
 * binding written against v27 is served unchanged; a binding that needs these two symbols resolves them when it loads the
 * library and fails there against a library that lacks them.
 *
 * y[m, n] = round_once_to_ydt( sum_k val_a(a_codes[m, k]) * 2^(a_scales[m, k / 32] - 127)
 *                                  * val_b(b_codes[n, k]) * 2^(b_scales[n, k / 32] - 127)  +  bias[n] )
 * i.e. A . B^T with B laid out as an nn.Linear weight.  val_*: the value of the element format's code (sign, exponent, mantissa in
 * the low bits of the byte, as qs_mx_quant_fwd_v writes them).  Products are exact, the sum is accumulated in float32 by
 * v_mfma_scale_f32_16x16x128_f8f6f4 in steps of 128 along K (the order inside a step is the instruction's), the bias is added in
 * float32, the result rounded once to ydt.  "Accumulated in float32" is as accurate as the instruction, measured (DESIGN.md 3b,
 * "Accumulation"): inside a group of eight consecutive k a product keeps its bits down to 2^(E - 13), E the largest sum of two
 * operand exponents (exponent fields, scale bytes included; zero codes aside) in the group, and is cut toward zero below; the group
 * sums, the four blocks of a step and the incoming sum are then added with 24 significant bits.  So
 *   |y - exact| <= sum over the groups of (the terms with a bit below the group's quantum) x quantum
 *                  + 18 ceil(K / 128) 2^-23 sum_k |a_k b_k| + ulp_ydt(y) + 2^-23 |bias|
 * at every K (tests/mx_gemm_ref.py, model_bound); the first term is zero when both sides are FP4.  The two formats may differ.
 *   - Any M, N >= 0 (M == 0 or N == 0: nothing is enqueued) and K >= 1.  K % 32 != 0: the last block is short, the missing
 *     elements count as zero.  Nothing outside the five operands and y is read or written.
 *   - A scale byte 0xFF (the quantizer's mark of a block that held NaN / Inf) makes every output whose dot product reads that
 *     block NaN: row m of y for a byte of A's row m, column n for a byte of B's row n.
 *   - Range.  Every scale byte 0..254 is honoured, 0 (2^-127, itself a float32 subnormal) and 254 included: a product whose
 *     exact magnitude lies in [2^-126, 2^128) enters the sum exactly whatever the two bytes are.  Outside that range, as measured
 *     on the MI355X and the same for all 25 format pairs (tests/test_mx_one_term_gpu.py pins it): underflow is GRADUAL -- a
 *     product below 2^-126 is rounded to the nearest float32 subnormal, ties to even, not flushed; a product of magnitude
 *     >= 2^128 gives Inf of its sign.  The float32 sum is +0 both for an exact zero (a -0 product included) and for a product
 *     of either sign that rounds to zero in float32: the sum starts at +0.  So y = round_dt(+0 + bias) there, which is +0 for
 *     a -0 bias too.  The fp16 / bf16 rounding of y is a plain IEEE cast of the float32 acc + bias (nearest even, subnormals
 *     kept, Inf on overflow) and keeps the sign: a negative sum too small for the dtype gives -0.
 *   - Code bytes the quantizer never writes (E5M2 Inf / NaN patterns, E4M3 0x7F / 0xFF, bits above the format's width) give an
 *     unspecified value in the outputs that read them, never a fault.
 *   - a_codes / b_codes / scales: any address.  y: aligned to its element; bias: to 4 bytes (QS_ERR_ALIGN otherwise).
 *     K % 16 == 0 with both code bases 16-byte aligned takes the 16-bytes-per-load kernel (QS_MX_GEMM_ROUTE_VEC), anything else
 *     the same kernel with predicated byte loads (QS_MX_GEMM_ROUTE_PLAIN).  No workspace. */
typedef struct qs_mx_matmul_args {
    uint32_t struct_size;            /* sizeof(qs_mx_matmul_args) as the caller compiled it */
    int32_t a_format, b_format;      /* enum qs_mx_format, may differ */
    const uint8_t* a_codes;          /* [M, K], one code per byte, row-major */
    const uint8_t* a_scales;         /* [M, ceil(K / 32)] E8M0 bytes */
    const uint8_t* b_codes;          /* [N, K] */
    const uint8_t* b_scales;         /* [N, ceil(K / 32)] */
    const float* bias;               /* nullable, [N] float32 */
    void* y;                         /* [M, N] row-major */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t M, N, K;
    qs_stream_t stream;
} qs_mx_matmul_args;
int qs_mx_matmul_v(const qs_mx_matmul_args* args);
/* the kernel qs_mx_matmul_v launches for these operands, nothing enqueued: QS_MX_GEMM_ROUTE_*, 0 for an empty product, or the
 * QS_ERR_* the call would return */
#define QS_MX_GEMM_ROUTE_VEC 1
#define QS_MX_GEMM_ROUTE_PLAIN 2
int qs_mx_matmul_route(const qs_mx_matmul_args* args);

/* ---- MX matrix product, split along K (deterministic split-K) ----------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * For products with a small output and a long contraction (a linear layer's weight gradient): qs_mx_matmul_v has one work-group per
 * 128 x 128 tile of y, each walking all of K; here the walk is cut into slices that run side by side.  With steps = ceil(K / 128)
 * and a requested slice count S >= 1:
 *   per = ceil(steps / S),  S' = ceil(steps / per)  (no slice is empty; S' <= S, and S' requested again gives S' again)
 *   slice s covers the K-steps [s per, min((s + 1) per, steps)), i.e. the codes k in [128 s per, min(128 (s + 1) per, K)): slice
 *   boundaries are multiples of 128, hence of the MX block
 *   p_s[m, n] = the float32 value qs_mx_matmul_v computes for the operands restricted to slice s, without bias, ydt = QS_F32
 *   y[m, n]   = round_once_to_ydt( ((p_0 + p_1) + p_2 + ... + p_{S'-1}) + bias[n] )
 * All adds are float32, in ascending s; the bias is added last.  S' == 1 IS qs_mx_matmul_v: the call is forwarded to it and the
 * result is bit-identical.  The result is a pure function of the operands and S -- the same on every run and every device: there are
 * no atomics of any kind and no synchronisation between work-groups.  0xFF scale bytes keep their meaning: a NaN partial makes the
 * sum NaN.  Two launches (partial products into the workspace: tiles x S' work-groups; the reduction), graph-capturable, no
 * allocation, no synchronisation.
 *   - workspace: caller-provided, S' * M * N * 4 bytes (qs_mx_matmul_splitk_plan tells), 16-byte aligned (QS_ERR_ALIGN otherwise);
 *     too small: QS_ERR_WORKSPACE; NULL with S' > 1: QS_ERR_ARG.  Not needed, and not looked at, when S' == 1.  Its contents on
 *     entry do not matter; on return it holds the partials, and nothing past S' * M * N * 4 bytes was written.
 *   - Every check of qs_mx_matmul_v applies unchanged and comes first; then split_k < 1: QS_ERR_ARG.  M == 0 or N == 0: nothing is
 *     enqueued.  tiles * S' beyond 2^31 - 1 or a byte count beyond 64 bits: QS_ERR_ARG.
 *   - Routes are those of qs_mx_matmul_v, decided by the same conditions (K % 16 == 0, 16-byte aligned code bases). */
typedef struct qs_mx_matmul_splitk_args {
    uint32_t struct_size;            /* sizeof(qs_mx_matmul_splitk_args) as the caller compiled it */
    int32_t a_format, b_format;      /* the fields of qs_mx_matmul_args, with their meaning ... */
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    void* y;
    int32_t ydt;
    int64_t M, N, K;
    qs_stream_t stream;
    int32_t split_k;                 /* ... and: S >= 1, the requested number of slices */
    int32_t reserved0;
    void* workspace;                 /* S' * M * N float32; nullable when S' == 1 */
    uint64_t workspace_bytes;
} qs_mx_matmul_splitk_args;
int qs_mx_matmul_splitk_v(const qs_mx_matmul_splitk_args* args);
/* the kernel the first launch of qs_mx_matmul_splitk_v runs for these operands (S' == 1: the one qs_mx_matmul_v runs), nothing
 * enqueued: QS_MX_GEMM_ROUTE_*, 0 for an empty product, or the QS_ERR_* the call would return */
int qs_mx_matmul_splitk_route(const qs_mx_matmul_splitk_args* args);
/* writes S' and the workspace bytes (0 when S' == 1) of a request; either pointer may be NULL.  split_k == 0 asks for the library's
 * automatic choice, a pure function of (M, N, K) on compile-time constants (no query of the device) and the single place the rule
 * lives.  With tiles = ceil(M / 128) ceil(N / 128) and steps = ceil(K / 128):
 *     S = 1                                                 when steps < 32 or tiles >= 256
 *     S = max(1, min(floor(512 / tiles), floor(steps / 8), 16))   otherwise
 * -- 256 tiles already give every CU a work-group; 512 work-groups are two co-resident ones per CU; a slice keeps at least 8 steps.
 * QS_ERR_ARG: a negative extent or request, K == 0 with M, N > 0, a byte count beyond 64 bits.  M == 0 or N == 0: S' = 1, 0 bytes. */
int qs_mx_matmul_splitk_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int32_t* slices, uint64_t* workspace_bytes);

/* ---- MX two-way quantizer (codes only) -----------------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (27), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * x is CONTIGUOUS [R, C] (float32, bf16 or fp16) and is read once.  Two output pairs, each nullable as a whole, at least one given:
 *   row pair  row_codes uint8 [R, C], row_scales uint8 [R, ceil(C / 32)], format row_format, blocks along C: the codes and scales
 *             qs_mx_quant_fwd_v writes for x seen as [R, C, 1]
 *   col pair  col_codes uint8 [C, R], row-major, col_scales uint8 [C, ceil(R / 32)], format col_format, blocks along R: the codes and
 *             scales qs_mx_quant_fwd_v writes for the transpose of x, stored as that transpose
 * bit for bit by the definition of the MX block-scaled quantizer above (short last blocks, zero blocks, float32 subnormals, the sign
 * of a zero, a NaN / Inf block: scale 0xFF, codes 0).  The two formats may differ; the format of a pair that is not given is ignored.
 * No de-quantized tensor is written, nothing but the four outputs is written, no workspace.  (v28) `rounding`, `seed`, `step` and
 * `index_base` are the rounding operands of qs_mx_quant_fwd_v above; the row pair draws its words with rng_stream 0, the col pair with 1.
 *   - x needs the alignment of its element (QS_ERR_ALIGN otherwise); codes and scales: any address.
 *   - R == 0 or C == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_Q2_ROUTE_TILE_VEC (16-byte loads of x, 16-byte stores of col_codes): C % 8 == 0 (two-byte x) or C % 4 == 0 (float32), x
 *     16-byte aligned and, when the col pair is written, R % 16 == 0 and col_codes 16-byte aligned.  Anything else takes
 *     QS_MX_Q2_ROUTE_TILE_PLAIN, the same tiling with element accesses: any R, C >= 1.
 *   - QS_ERR_ARG: a null or too short descriptor, x null, both pairs null, codes without scales or the reverse, a format outside
 *     enum qs_mx_format, a negative extent; the rounding operands as for qs_mx_quant_fwd_v, checked before the others.
 *     QS_ERR_DTYPE: xdt is none of the three. */
typedef struct qs_mx_quant2_args {
    uint32_t struct_size;            /* sizeof(qs_mx_quant2_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ */
    const void* x;                   /* [R, C] row-major */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    uint8_t* row_codes;              /* nullable with row_scales; [R, C] */
    uint8_t* row_scales;             /* [R, ceil(C / 32)] */
    uint8_t* col_codes;              /* nullable with col_scales; [C, R] */
    uint8_t* col_scales;             /* [C, ceil(R / 32)] */
    int64_t R, C;
    qs_stream_t stream;
    int32_t rounding;                /* (v28) QS_MX_ROUND_*, as for qs_mx_quant_fwd_v */
    int32_t reserved0;               /* (v28) */
    uint64_t seed;                   /* (v28) */
    const int64_t* step;             /* (v28) nullable (= 0); device memory, one int64, read by the kernel */
    uint64_t index_base;             /* (v28) a multiple of 4; added to the indices of both pairs */
} qs_mx_quant2_args;
int qs_mx_quant2_v(const qs_mx_quant2_args* args);
/* the kernel qs_mx_quant2_v launches for these operands, nothing enqueued: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, or the QS_ERR_*
 * the call would return */
#define QS_MX_Q2_ROUTE_TILE_VEC 1
#define QS_MX_Q2_ROUTE_TILE_PLAIN 2
int qs_mx_quant2_route(const qs_mx_quant2_args* args);

/* ---- MX batched two-way quantizer (codes only) ---------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * qs_mx_quant2_v for G = G0 G1 slices [R, C] of x in ONE launch, each slice read once WHERE IT LIES.  The element stride of x along
 * C is 1; slice g = g0 G1 + g1 (0 <= g0 < G0, 0 <= g1 < G1) begins at x + g0 x_stride_g0 + g1 x_stride_g1 and its row r begins
 * r x_stride_r further on, all three strides in elements -- a dense [G, R, C] tensor is G0 = 1 (or G1 = 1) with x_stride_r = C, the
 * heads of a [B, T, h, d] projection output seen as [B, h, T, d] are G0 = B, G1 = h with the strides (T h d, d, h d).  The four
 * outputs are DENSE, each pair nullable as a whole, at least one given:
 *   row pair  row_codes uint8 [G, R, C], row_scales uint8 [G, R, ceil(C / 32)], format row_format, blocks along C
 *   col pair  col_codes uint8 [G, C, R], col_scales uint8 [G, C, ceil(R / 32)], format col_format, blocks along R
 * Slice g of the four outputs is, bit for bit, what qs_mx_quant2_v writes for slice g of x made contiguous: short last blocks, zero
 * blocks, a NaN / Inf block (scale 0xFF, codes 0) and the sign of a zero included.  A block never spans two slices: the short last
 * block of slice g along R reads nothing of slice g + 1, and nothing outside the G R C addressed elements of x is read at all.
 * Nothing but the four outputs is written; no atomics, no workspace.
 * Stochastic rounding (`rounding`, `seed`, `step`, `index_base` as for qs_mx_quant2_v): the random word of a code is indexed by its
 * row-major index in the WHOLE dense output plus index_base -- (g R + r) C + c with rng_stream 0 for the row pair, (g C + c) R + r
 * with rng_stream 1 for the col pair -- so both pairs are exactly the stochastic qs_mx_quant_fwd_v on the [G, R, C] tensor and on
 * its [G, C, R] transpose.
 *   - checks in qs_mx_quant2_v's order and with its status codes (the rounding operands first; x needs the alignment of its element,
 *     QS_ERR_ALIGN; QS_ERR_DTYPE).  QS_ERR_ARG in addition: G0 < 0 or G1 < 0; for a tensor that is not empty x_stride_r < C (rows
 *     would overlap) or a negative x_stride_g0 / x_stride_g1 (0 is allowed: x is only read), G R C or the offset of the last
 *     addressed element of x beyond INT64_MAX, more than 2^31 - 1 work-groups (G tiles of 128 x 64 per slice).
 *   - G0, G1, R or C equal to 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_Q2_ROUTE_TILE_VEC: qs_mx_quant2_v's conditions (C % 8 == 0 for two-byte x, C % 4 == 0 for float32, x 16-byte aligned and,
 *     when the col pair is written, R % 16 == 0 and col_codes 16-byte aligned -- which keeps every output slice's base aligned) and
 *     all three strides multiples of the 16-byte vector (8 two-byte elements, 4 float32).  Anything else takes
 *     QS_MX_Q2_ROUTE_TILE_PLAIN: the same bits. */
typedef struct qs_mx_quant2_batched_args {
    uint32_t struct_size;            /* sizeof(qs_mx_quant2_batched_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ */
    const void* x;                   /* slice (g0, g1), row r, column c at x[g0 x_stride_g0 + g1 x_stride_g1 + r x_stride_r + c] */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    uint8_t* row_codes;              /* nullable with row_scales; [G, R, C] */
    uint8_t* row_scales;             /* [G, R, ceil(C / 32)] */
    uint8_t* col_codes;              /* nullable with col_scales; [G, C, R] */
    uint8_t* col_scales;             /* [G, C, ceil(R / 32)] */
    int64_t R, C;
    qs_stream_t stream;
    int32_t rounding;                /* QS_MX_ROUND_* */
    int32_t reserved0;
    uint64_t seed;
    const int64_t* step;             /* nullable (= 0); device memory, one int64, read by the kernel */
    uint64_t index_base;             /* a multiple of 4; added to the indices of both pairs */
    int64_t G0, G1;                  /* G = G0 G1 slices */
    int64_t x_stride_g0, x_stride_g1, x_stride_r;   /* in elements */
} qs_mx_quant2_batched_args;
int qs_mx_quant2_batched_v(const qs_mx_quant2_batched_args* args);
/* the kernel qs_mx_quant2_batched_v launches for these operands, nothing enqueued: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
int qs_mx_quant2_batched_route(const qs_mx_quant2_batched_args* args);

/* ---- MX convolution (implicit GEMM on the block-scaled MFMA) -------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * Channels-last operands, MX blocks of 32 along the input channels C (the innermost axis):
 *   x_codes [B, H, W, C], x_scales [B, H, W, ceil(C / 32)];  w_codes [Cout, KH, KW, C], w_scales [Cout, KH, KW, ceil(C / 32)]
 *   y[b, oh, ow, n] = round_once_to_ydt( sum over (kh, kw, c) of
 *                         val_x(x[b, ih, iw, c]) * 2^(x_scales[b, ih, iw, c / 32] - 127)
 *                       * val_w(w[n, kh, kw, c]) * 2^(w_scales[n, kh, kw, c / 32] - 127)  +  bias[n] )
 *   ih = oh * stride_h - pad_h + kh * dil_h,  iw = ow * stride_w - pad_w + kw * dil_w;  a tap outside the image contributes zero
 *   (zero codes, scale byte 127);  OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1, OW likewise;  y is [B, OH, OW, Cout].
 * Order of the sum: with Cp = 32 ceil(C / 32) and k' = (kh * KW + kw) * Cp + c (codes with c >= C are zero codes) the sum is
 * accumulated in float32 from zero along k' in steps of 128, one v_mfma_scale_f32_16x16x128_f8f6f4 per step -- the order of
 * qs_mx_matmul_v on the im2col operands A [B OH OW, KH KW Cp] and Wp [Cout, KH KW Cp], whose result it equals bit for bit.  The
 * bias is added in float32 at the end.  No im2col matrix is written; no workspace; groups == 1.
 *   - A scale byte 0xFF makes NaN every output whose window reads that block: every (b, oh, ow) of channel n for a byte of w's
 *     row n; for a byte of x every output pixel whose window covers that input pixel, in every channel.
 *   - Code bytes the quantizer never writes give an unspecified value in the outputs that read them, never a fault.
 *   - Codes and scales: any address.  y: aligned to its element; bias: to 4 bytes (QS_ERR_ALIGN otherwise).
 *   - B == 0 or Cout == 0: nothing is enqueued, 0 is returned.
 *   - QS_ERR_ARG: a null or too short descriptor, a null operand, a format outside enum qs_mx_format, B or Cout < 0, H, W, C, KH,
 *     KW, a stride or a dilation < 1, a negative padding, OH < 1 or OW < 1, H + 2 pad_h, W + 2 pad_w, B, Cout or C + 32 beyond
 *     INT32_MAX.  QS_ERR_DTYPE: ydt is none of the three.
 * Routes:
 *   QS_MX_CONV_ROUTE_GEMM   KH == KW == 1, strides 1, paddings 0 and C % 32 == 0: the operands ARE [B H W, C] and [Cout, C]; the call
 *                           is forwarded to qs_mx_matmul_v on the same bytes
 *   QS_MX_CONV_ROUTE_VEC    C % 16 == 0 and both code bases 16-byte aligned: 16 bytes per load
 *   QS_MX_CONV_ROUTE_PLAIN  anything else (any C >= 1, any base): the same kernel with predicated byte loads.  Correct, not tuned:
 *                           every tap is padded to 32 channels, so a stem with C = 3 spends 29 / 32 of its products on zeros */
typedef struct qs_mx_conv2d_args {
    uint32_t struct_size;            /* sizeof(qs_mx_conv2d_args) as the caller compiled it */
    int32_t x_format, w_format;      /* enum qs_mx_format, may differ */
    const uint8_t* x_codes;          /* [B, H, W, C], one code per byte */
    const uint8_t* x_scales;         /* [B, H, W, ceil(C / 32)] E8M0 bytes */
    const uint8_t* w_codes;          /* [Cout, KH, KW, C] */
    const uint8_t* w_scales;         /* [Cout, KH, KW, ceil(C / 32)] */
    const float* bias;               /* nullable, [Cout] float32 */
    void* y;                         /* [B, OH, OW, Cout] */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t B, H, W, C, Cout;
    int32_t KH, KW;
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    qs_stream_t stream;
} qs_mx_conv2d_args;
int qs_mx_conv2d_v(const qs_mx_conv2d_args* args);
/* the route qs_mx_conv2d_v takes for these operands, nothing enqueued: QS_MX_CONV_ROUTE_*, 0 for an empty problem, or the QS_ERR_*
 * the call would return */
#define QS_MX_CONV_ROUTE_GEMM 1
#define QS_MX_CONV_ROUTE_VEC 2
#define QS_MX_CONV_ROUTE_PLAIN 3
int qs_mx_conv2d_route(const qs_mx_conv2d_args* args);

/* ---- MX transposed convolution (fractionally-strided implicit GEMM) ----------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28): symbols are only added.  Also the input gradient (dgrad) of qs_mx_conv2d_v's
 * convolution: dx is the transposed convolution of dy with the same weight, contracted over (kh, kw, cout).
 *
 * Channels-last operands, MX blocks of 32 along the contraction channels C (the innermost axis):
 *   x_codes [B, H, W, C], x_scales [B, H, W, ceil(C / 32)];  w_codes [Cout, KH, KW, C], w_scales [Cout, KH, KW, ceil(C / 32)]
 *   (w is nn.ConvTranspose2d.weight [C, Cout, KH, KW] permuted (1, 2, 3, 0); for dgrad conv.weight [Cout_fwd, Cin, KH, KW] permuted
 *   (1, 2, 3, 0), so Cout := Cin and C := Cout_fwd.  The kernel indices are the weight's own, un-flipped.)
 *   OH = (H - 1) stride_h - 2 pad_h + dil_h (KH - 1) + out_pad_h + 1, OW likewise;  y is [B, OH, OW, Cout]
 *   y[b, oh, ow, n] = round_once_to_ydt( sum over (kh, kw, c) of
 *                         val_x(x[b, ih, iw, c]) * 2^(x_scales[b, ih, iw, c / 32] - 127)
 *                       * val_w(w[n, kh, kw, c]) * 2^(w_scales[n, kh, kw, c / 32] - 127)  +  bias[n] )
 *   ih = (oh + pad_h - kh * dil_h) / stride_h,  iw = (ow + pad_w - kw * dil_w) / stride_w;  a tap exists only where both divisions
 *   are exact and 0 <= ih < H, 0 <= iw < W.  A tap that does not exist contributes zero codes with scale byte 127, as do codes
 *   with c >= C.
 * Order of the sum: with Cp = 32 ceil(C / 32) and k' = (kh * KW + kw) * Cp + c the sum is accumulated in float32 from zero along k'
 * in steps of 128, one v_mfma_scale_f32_16x16x128_f8f6f4 per step -- the order of qs_mx_matmul_v on the gathered operands
 * A [B OH OW, KH KW Cp] and Wp [Cout, KH KW Cp], whose result it equals bit for bit.  The bias is added in float32 at the end.  No
 * gathered matrix is written; no workspace; groups == 1.
 *   - No tap is skipped.  A scale byte 0xFF in w's row n makes channel n NaN at every (b, oh, ow), also where no tap exists (the
 *     block meets zero codes there); a byte 0xFF of x makes NaN exactly the outputs that have an existing tap on that pixel.
 *   - An output that no tap reaches (a stride larger than the kernel's reach) is bias[n], or +0.0 without a bias.
 *   - A stride s spends stride_h stride_w - 1 of every stride_h stride_w products on zero codes: correct, not tuned -- there is no
 *     sub-pixel (per-phase) decomposition.
 *   - Code bytes the quantizer never writes give an unspecified value in the outputs that read them, never a fault.
 *   - Codes and scales: any address.  y: aligned to its element; bias: to 4 bytes (QS_ERR_ALIGN otherwise).
 *   - B == 0 or Cout == 0: nothing is enqueued, 0 is returned.
 *   - QS_ERR_ARG: a null or too short descriptor, a null operand, a format outside enum qs_mx_format, B or Cout < 0, H, W, C, KH,
 *     KW, a stride or a dilation < 1, a negative padding, an output padding < 0 or >= max(stride, dilation) of its axis, OH < 1 or
 *     OW < 1, OH + pad_h, OW + pad_w or dil (K - 1) beyond INT32_MAX, B, Cout or C + 32 beyond INT32_MAX.  QS_ERR_DTYPE: ydt is
 *     none of the three.
 * Routes (the values of qs_mx_conv2d_route):
 *   QS_MX_CONV_ROUTE_GEMM   KH == KW == 1, strides 1, paddings 0, output paddings 0 and C % 32 == 0: the operands ARE [B H W, C] and
 *                           [Cout, C]; the call is forwarded to qs_mx_matmul_v on the same bytes
 *   QS_MX_CONV_ROUTE_VEC    C % 16 == 0 and both code bases 16-byte aligned: 16 bytes per load
 *   QS_MX_CONV_ROUTE_PLAIN  anything else (any C >= 1, any base): the same kernel with predicated byte loads */
typedef struct qs_mx_conv_transpose2d_args {
    uint32_t struct_size;            /* sizeof(qs_mx_conv_transpose2d_args) as the caller compiled it */
    int32_t x_format, w_format;      /* enum qs_mx_format, may differ */
    const uint8_t* x_codes;          /* [B, H, W, C], one code per byte */
    const uint8_t* x_scales;         /* [B, H, W, ceil(C / 32)] E8M0 bytes */
    const uint8_t* w_codes;          /* [Cout, KH, KW, C] */
    const uint8_t* w_scales;         /* [Cout, KH, KW, ceil(C / 32)] */
    const float* bias;               /* nullable, [Cout] float32 */
    void* y;                         /* [B, OH, OW, Cout] */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t B, H, W, C, Cout;
    int32_t KH, KW;
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int32_t out_pad_h, out_pad_w;    /* 0 <= out_pad < max(stride, dil) of the axis */
    qs_stream_t stream;
} qs_mx_conv_transpose2d_args;
int qs_mx_conv_transpose2d_v(const qs_mx_conv_transpose2d_args* args);
/* the route qs_mx_conv_transpose2d_v takes for these operands, nothing enqueued: QS_MX_CONV_ROUTE_*, 0 for an empty problem, or the
 * QS_ERR_* the call would return */
int qs_mx_conv_transpose2d_route(const qs_mx_conv_transpose2d_args* args);

/* ---- MX convolution, weight gradient (batch-blocked implicit GEMM, deterministic split-K) ---------------------------------------
 * Added without raising QS_ABI_VERSION (28): symbols are only added.  The weight gradient (wgrad) of qs_mx_conv2d_v's convolution,
 * whose contraction runs over (b, oh, ow).
 *
 * Operands with MX blocks of 32 along the BATCH B, the innermost axis -- a block of 32 images at one pixel and channel is the same 32
 * numbers under every tap (kh, kw), so one quantization of x serves all taps:
 *   dyt_codes [OH, OW, Cout, B], dyt_scales [OH, OW, Cout, ceil(B / 32)];  xt_codes [H, W, C, B], xt_scales [H, W, C, ceil(B / 32)]
 *   (the column pair qs_mx_quant2_v writes for the channels-last tensor seen as [B, OH OW Cout] / [B, H W C])
 *   OH = (H + 2 pad_h - dil_h (KH - 1) - 1) / stride_h + 1, OW likewise (qs_mx_conv2d_v's; any other OH, OW: QS_ERR_ARG)
 *   dw[n, kh, kw, c] = round_once_to_ydt( sum over (oh, ow, b) of
 *                          val_g(dyt[oh, ow, n, b]) * 2^(dyt_scales[oh, ow, n, b / 32] - 127)
 *                        * val_x(xt[ih, iw, c, b])  * 2^(xt_scales[ih, iw, c, b / 32] - 127) )
 *   ih = oh * stride_h - pad_h + kh * dil_h,  iw = ow * stride_w - pad_w + kw * dil_w;  dw is [Cout, KH, KW, C], contiguous.
 * Order of the sum: with Bp = 32 ceil(B / 32), k' = (oh * OW + ow) * Bp + b and K' = OH OW Bp the result equals, bit for bit, that of
 * qs_mx_matmul_splitk_v (qs_mx_matmul_v when S' == 1) on the gathered operands G [Cout, K'] = dyt[oh, ow, n, b] and
 * X' [KH KW C, K'] = xt[ih, iw, c, b] with the same S.  A code with b >= B, or an x tap outside the image, is the zero code; the
 * scale byte of a block that does not exist at all (a tap outside the image) is 127.  No gathered matrix is written; groups == 1.
 *   - Slicing: steps = ceil(K' / 128), per = ceil(steps / S), S' = ceil(steps / per); slice s covers the steps [s per, (s + 1) per);
 *     the float32 partial sums are added in ascending s.  No atomics: the result is a pure function of the operands and S.
 *     split_k == 0 asks for the automatic S of qs_mx_conv2d_wgrad_plan.
 *   - No tap and no pixel is skipped.  A scale byte 0xFF of dyt at channel n makes dw[n] NaN everywhere; a byte 0xFF of xt at
 *     (ih, iw, c) makes dw[:, kh, kw, c] NaN for exactly the taps (kh, kw) through which some output pixel reads (ih, iw).
 *   - A batch below 32 pads its block with zero codes: B = 8 spends 3 / 4 of the products on zeros.
 *   - workspace: caller-provided, S' * Cout * KH KW C * 4 bytes (qs_mx_conv2d_wgrad_plan tells), 16-byte aligned (QS_ERR_ALIGN
 *     otherwise); too small: QS_ERR_WORKSPACE; NULL with S' > 1: QS_ERR_ARG.  Not looked at when S' == 1.  Nothing past those bytes
 *     is written.  One launch, or two when S' > 1 (partials; their ordered sum); graph-capturable, no allocation, no synchronisation.
 *   - Codes and scales: any address.  dw: aligned to its element (QS_ERR_ALIGN otherwise).
 *   - Cout == 0 or C == 0: nothing is enqueued, 0 is returned.
 *   - QS_ERR_ARG: a null or too short descriptor, a null operand, a format outside enum qs_mx_format, B < 1, Cout or C < 0, H, W, KH,
 *     KW, a stride or a dilation < 1, a negative padding or split_k, OH or OW not the convolution's, H + 2 pad_h, W + 2 pad_w, B + 32,
 *     Cout or C beyond INT32_MAX, a product of extents beyond 64 bits, tiles * S' beyond 2^31 - 1.  QS_ERR_DTYPE: ydt is none of the
 *     three.
 * Routes (the values of qs_mx_conv2d_route; there is no GEMM route: even a 1 x 1 operand is not row-major in k'):
 *   QS_MX_CONV_ROUTE_VEC    B % 16 == 0 and both code bases 16-byte aligned: 16 bytes per load
 *   QS_MX_CONV_ROUTE_PLAIN  anything else (any B >= 1, any base): the same kernel with predicated byte loads */
typedef struct qs_mx_conv2d_wgrad_args {
    uint32_t struct_size;            /* sizeof(qs_mx_conv2d_wgrad_args) as the caller compiled it */
    int32_t dy_format, x_format;     /* enum qs_mx_format, may differ */
    const uint8_t* dyt_codes;        /* [OH, OW, Cout, B], one code per byte */
    const uint8_t* dyt_scales;       /* [OH, OW, Cout, ceil(B / 32)] E8M0 bytes */
    const uint8_t* xt_codes;         /* [H, W, C, B] */
    const uint8_t* xt_scales;        /* [H, W, C, ceil(B / 32)] */
    void* dw;                        /* [Cout, KH, KW, C] */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int32_t split_k;                 /* S >= 1, the requested number of slices; 0: the library's choice */
    int64_t B, H, W, C, Cout, OH, OW;
    int32_t KH, KW;
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    qs_stream_t stream;
    void* workspace;                 /* S' * Cout * KH KW C float32; nullable when S' == 1 */
    uint64_t workspace_bytes;
} qs_mx_conv2d_wgrad_args;
int qs_mx_conv2d_wgrad_v(const qs_mx_conv2d_wgrad_args* args);
/* the route qs_mx_conv2d_wgrad_v takes for these operands, nothing enqueued: QS_MX_CONV_ROUTE_VEC or _PLAIN, 0 for an empty
 * problem, or the QS_ERR_* the call would return */
int qs_mx_conv2d_wgrad_route(const qs_mx_conv2d_wgrad_args* args);
/* writes S' and the workspace bytes (0 when S' == 1) of a request on the product M = Cout, N = KH KW C, K = OH OW Bp; either pointer
 * may be NULL.  split_k == 0 asks for the automatic choice, a pure function of (M, N, K): the rule of qs_mx_matmul_splitk_plan with a
 * cap of 128 slices instead of 16 --
 *     S = 1                                                        when steps < 32 or tiles >= 256
 *     S = max(1, min(floor(512 / tiles), floor(steps / 8), 128))   otherwise
 * -- because this product has few tiles (64 -> 64 channels, 3 x 3: 5) and thousands of steps.  Errors as
 * qs_mx_matmul_splitk_plan. */
int qs_mx_conv2d_wgrad_plan(int64_t M, int64_t N, int64_t K, int32_t split_k, int32_t* slices, uint64_t* workspace_bytes);

/* ---- MX products that write MX codes (fused quantizing epilogue) ---------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28): symbols are only added.
 *
 * The matrix product and the convolution above with the NEXT layer's quantizer in their epilogue: instead of y they write the MX
 * codes and E8M0 scale bytes of y, with blocks of 32 along the last axis of y (N / Cout: the next product's K / C).  Definition
 * (normative).  With v[m, n] the float32 value qs_mx_matmul_v / qs_mx_conv2d_v produce for the same operands with ydt = QS_F32
 * (float32 accumulation in their order, bias added in float32, no further rounding; m runs over the rows of y seen as [M, N]):
 *   u = v                                 act == QS_MX_ACT_NONE
 *   u = v > 0 ? v : (v != v ? v : +0)     act == QS_MX_ACT_RELU: NaN stays NaN, everything else that is not positive becomes +0
 *   out_codes [M, N], out_scales [M, ceil(N / 32)] = the codes and scales qs_mx_quant_fwd_v writes for u seen as [M, N, 1] in the
 *   format out_format with QS_MX_ROUND_NEAREST
 * bit for bit: the last block of a row is short when N % 32 != 0; a block that holds NaN / Inf gets the byte 0xFF and codes 0, an
 * all-zero block the byte 0.  No y exists in memory; one launch, no workspace, no atomics.  Stochastic rounding of the output is
 * not offered.
 *   - Every check of qs_mx_matmul_v / qs_mx_conv2d_v that does not concern y applies, with the same precedence; with the
 *     QS_ERR_ARG checks of the operands come: out_codes or out_scales NULL, out_format outside enum qs_mx_format, act outside
 *     QS_MX_ACT_*.  bias: aligned to 4 bytes (QS_ERR_ALIGN).  out_codes, out_scales: any address (N % 4 == 0 with out_codes 4-byte
 *     aligned stores four codes at once, anything else single bytes).  After the size checks: out_codes sharing a byte with a_codes
 *     / b_codes (x_codes / w_codes) is QS_ERR_ARG -- a work-group writes its tile while others still read the operands.
 *   - M == 0 or N == 0 (B == 0 or Cout == 0): nothing is enqueued, 0 is returned.
 *   - Nothing outside out_codes [M, N] and out_scales [M, ceil(N / 32)] is written.
 *   - Routes: those of qs_mx_matmul_route / qs_mx_conv2d_route, by the same conditions on the inputs.  QS_MX_CONV_ROUTE_GEMM forwards
 *     to qs_mx_matmul_q_v on the same bytes.  There is no split-K form. */
#define QS_MX_ACT_NONE 0
#define QS_MX_ACT_RELU 1
typedef struct qs_mx_matmul_q_args {
    uint32_t struct_size;            /* sizeof(qs_mx_matmul_q_args) as the caller compiled it */
    int32_t a_format, b_format;      /* the operands of qs_mx_matmul_args, with their meaning ... */
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    int32_t out_format;              /* ... and: enum qs_mx_format of the output */
    int32_t act;                     /* QS_MX_ACT_* */
    uint8_t* out_codes;              /* [M, N], one code per byte */
    uint8_t* out_scales;             /* [M, ceil(N / 32)] E8M0 bytes */
    int64_t M, N, K;
    qs_stream_t stream;
} qs_mx_matmul_q_args;
int qs_mx_matmul_q_v(const qs_mx_matmul_q_args* args);
/* the kernel qs_mx_matmul_q_v launches for these operands, nothing enqueued: QS_MX_GEMM_ROUTE_*, 0 for an empty product, or the
 * QS_ERR_* the call would return */
int qs_mx_matmul_q_route(const qs_mx_matmul_q_args* args);

typedef struct qs_mx_conv2d_q_args {
    uint32_t struct_size;            /* sizeof(qs_mx_conv2d_q_args) as the caller compiled it */
    int32_t x_format, w_format;      /* the operands of qs_mx_conv2d_args, with their meaning ... */
    const uint8_t* x_codes;
    const uint8_t* x_scales;
    const uint8_t* w_codes;
    const uint8_t* w_scales;
    const float* bias;
    int32_t out_format;              /* ... and: enum qs_mx_format of the output */
    int32_t act;                     /* QS_MX_ACT_* */
    uint8_t* out_codes;              /* [B, OH, OW, Cout], one code per byte */
    uint8_t* out_scales;             /* [B, OH, OW, ceil(Cout / 32)] E8M0 bytes */
    int64_t B, H, W, C, Cout;
    int32_t KH, KW;
    int32_t stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    qs_stream_t stream;
} qs_mx_conv2d_q_args;
int qs_mx_conv2d_q_v(const qs_mx_conv2d_q_args* args);
/* the route qs_mx_conv2d_q_v takes for these operands, nothing enqueued: QS_MX_CONV_ROUTE_*, 0 for an empty problem, or the QS_ERR_*
 * the call would return */
int qs_mx_conv2d_q_route(const qs_mx_conv2d_q_args* args);

/* ---- MX batched matrix product -----------------------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * G independent products in one launch, neither operand shared between them (attention's Q . K^T and P . V per image and head, a
 * linear layer per expert):
 *   y[g, m, n] = round_once_to_ydt( sum_k val_a(a_codes[g, m, k]) * 2^(a_scales[g, m, k / 32] - 127)
 *                                       * val_b(b_codes[g, n, k]) * 2^(b_scales[g, n, k / 32] - 127)  +  bias[g or -, n] )
 * Definition (normative): slice g of y equals, bit for bit, what qs_mx_matmul_v writes for slice g of the operands -- the same
 * tile, the same walk along K in steps of 128, the same order of the 16 MFMAs of a step -- so everything said there about range,
 * short last blocks and unspecified code bytes holds per slice.  A scale byte 0xFF makes every output that reads it NaN, in that
 * slice only.
 *   - All four operands and y are dense: slice g lies g whole slices (M K, M ceil(K / 32), N K, N ceil(K / 32), M N elements) past
 *     its base.  bias is NULL, [N] shared by the slices (bias_batch_stride == 0) or [G, N] (bias_batch_stride == N, in elements);
 *     any other stride is QS_ERR_ARG.
 *   - Checks in the order and with the status codes of qs_mx_matmul_v: a NULL operand, a format outside enum qs_mx_format, a
 *     negative extent or a bad bias stride is QS_ERR_ARG; then ydt (QS_ERR_DTYPE); then y aligned to its element and bias to 4
 *     bytes (QS_ERR_ALIGN).  G == 0, M == 0 or N == 0: nothing is enqueued, 0 is returned.  K == 0 of a non-empty product, any of
 *     G M K, G N K, G M N beyond INT64_MAX, or G ceil(M / 128) ceil(N / 128) beyond 2^31 - 1 work-groups: QS_ERR_ARG.
 *   - One launch, one work-group per 128 x 128 tile of one slice -- unless a slice has 512 tiles or more and fills the GPU by itself:
 *     the slices are then launched one by one, as qs_mx_matmul_v launches them (G launches, the same bits).  Nothing outside the five
 *     operands and y is read or written.
 *   - Routes: K % 16 == 0 with both code bases 16-byte aligned (every slice base then is) takes QS_MX_GEMM_ROUTE_VEC, anything else
 *     QS_MX_GEMM_ROUTE_PLAIN, with the same bits.  No workspace, no split-K form. */
typedef struct qs_mx_bmm_args {
    uint32_t struct_size;            /* sizeof(qs_mx_bmm_args) as the caller compiled it */
    int32_t a_format, b_format;      /* enum qs_mx_format, may differ */
    const uint8_t* a_codes;          /* [G, M, K], one code per byte, dense */
    const uint8_t* a_scales;         /* [G, M, ceil(K / 32)] E8M0 bytes */
    const uint8_t* b_codes;          /* [G, N, K] */
    const uint8_t* b_scales;         /* [G, N, ceil(K / 32)] */
    const float* bias;               /* nullable, float32 [N] or [G, N] */
    int64_t bias_batch_stride;       /* elements from one slice's bias to the next: 0 or N */
    void* y;                         /* [G, M, N] dense */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t G, M, N, K;
    qs_stream_t stream;
} qs_mx_bmm_args;
int qs_mx_bmm_v(const qs_mx_bmm_args* args);
/* the kernel qs_mx_bmm_v launches for these operands, nothing enqueued: QS_MX_GEMM_ROUTE_*, 0 for an empty product, or the
 * QS_ERR_* the call would return */
int qs_mx_bmm_route(const qs_mx_bmm_args* args);

/* The batched product with the quantizing epilogue ("MX products that write MX codes" above): out_codes [G, M, N] and out_scales
 * [G, M, ceil(N / 32)] instead of y, slice g bit for bit what qs_mx_matmul_q_v writes for slice g of the operands.  Checks and their
 * precedence are those of qs_mx_matmul_q_v with the additions of qs_mx_bmm_v; out_codes sharing a byte with a_codes or b_codes --
 * byte counts over all G slices -- is QS_ERR_ARG.  Routes as qs_mx_bmm_route. */
typedef struct qs_mx_bmm_q_args {
    uint32_t struct_size;            /* sizeof(qs_mx_bmm_q_args) as the caller compiled it */
    int32_t a_format, b_format;      /* the operands of qs_mx_bmm_args, with their meaning ... */
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    int64_t bias_batch_stride;
    int32_t out_format;              /* ... and: enum qs_mx_format of the output */
    int32_t act;                     /* QS_MX_ACT_* */
    uint8_t* out_codes;              /* [G, M, N], one code per byte */
    uint8_t* out_scales;             /* [G, M, ceil(N / 32)] E8M0 bytes */
    int64_t G, M, N, K;
    qs_stream_t stream;
} qs_mx_bmm_q_args;
int qs_mx_bmm_q_v(const qs_mx_bmm_q_args* args);
int qs_mx_bmm_q_route(const qs_mx_bmm_q_args* args);

/* ---- MX grouped matrix product ----------------------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The ragged product of a mixture-of-experts layer after routing: the T rows of a are E consecutive groups of DIFFERENT sizes, some
 * of them empty, and group e is multiplied by its own weight b[e].  The sizes are known only on the device: `offs` [E] int32 in
 * DEVICE memory holds the cumulative END row of every group (the convention of torch's grouped mm).  The host side does no
 * allocation, no synchronisation and no read of offs; it is one launch, always.
 * Definition (normative).  Let c_-1 = 0 and c_e = min(max(offs[e], c_{e-1}), T).  Group e is the rows [c_{e-1}, c_e).
 *   - Rows of a group: for r in group e, y[r, :] is what qs_mx_matmul_v writes for that row with the weight b[e] and the bias of e,
 *     bit for bit -- the same walk along K, the same MFMA order, one rounding -- so everything said there about range, short last
 *     blocks and unspecified code bytes holds per row.
 *   - Tail rows: rows r >= c_{E-1} belong to no group.  They get +0, and no bias is added; in the codes-out form they get code 0 and
 *     scale byte 0, what the quantizer writes for an all-zero block.  This is what a capacity-padded token buffer needs.
 *   - Clamped boundaries: with the running maximum and the clamp the groups partition [0, c_{E-1}) for ANY content of offs.  Every
 *     row of the output is stored exactly once and no address outside the operands is formed.  A non-monotone or out-of-range offs
 *     gives the results for the clamped boundaries, never a fault.  The clamp is part of the definition, not an optimisation.
 *   - bias is NULL, [N] shared by the groups (bias_batch_stride == 0) or [E, N] (bias_batch_stride == N, in elements); any other
 *     stride is QS_ERR_ARG.
 *   - Checks in the order and with the status codes of qs_mx_bmm_v: a NULL a_codes / a_scales / y, with E > 0 a NULL b_codes /
 *     b_scales / offs, a format outside enum qs_mx_format, a negative extent, E beyond QS_MX_GROUPED_MAX_GROUPS or a bad bias stride is
 *     QS_ERR_ARG; then ydt (QS_ERR_DTYPE); then y aligned to its element, bias and offs to 4 bytes (QS_ERR_ALIGN).  T == 0 or N == 0:
 *     nothing is enqueued, 0 is returned.  E == 0 is legal: every row is then a tail row.  K == 0 of a non-empty product, any of T K,
 *     E N K, T N beyond INT64_MAX, or a grid beyond 2^31 - 1 work-groups: QS_ERR_ARG.
 *   - One work-group per 128 x 128 tile; the M-tiles are group-relative, so no tile holds rows of two groups.  The host cannot know
 *     their number: the grid is the bound floor((T + 127 (E + 1)) / 128) ceil(N / 128), and a work-group beyond the real total returns
 *     at once.
 *   - Routes: K % 16 == 0 with both code bases 16-byte aligned (every group's rows and every weight then are) takes
 *     QS_MX_GEMM_ROUTE_VEC, anything else QS_MX_GEMM_ROUTE_PLAIN, with the same bits.  No workspace, no split-K form. */
/* The most groups of one call.  Every work-group finds its group by walking offs from the front, so its start-up cost grows with E,
 * and the grid carries up to E + 1 work-groups per column of tiles that walk all of offs, find no tile and leave.  A full walk
 * measured 2.7 us at 64 groups and 41 us at 1024, which is already several times the 128 x 128 x 1024 tile it
 * precedes: the kernel is meant for the expert counts in use (8 .. 256 a layer), and the cap bounds what a call can waste on the
 * walk (0.16 ms a work-group at 4096) rather than promise speed there.  More groups than this want another decode, not this one. */
#define QS_MX_GROUPED_MAX_GROUPS 4096
typedef struct qs_mx_grouped_matmul_args {
    uint32_t struct_size;            /* sizeof(qs_mx_grouped_matmul_args) as the caller compiled it */
    int32_t a_format, b_format;      /* enum qs_mx_format, may differ */
    const uint8_t* a_codes;          /* [T, K], one code per byte, dense: the rows of all groups, group after group */
    const uint8_t* a_scales;         /* [T, ceil(K / 32)] E8M0 bytes */
    const uint8_t* b_codes;          /* [E, N, K]: one weight per group */
    const uint8_t* b_scales;         /* [E, N, ceil(K / 32)] */
    const float* bias;               /* nullable, float32 [N] or [E, N] */
    int64_t bias_batch_stride;       /* elements from one group's bias to the next: 0 or N */
    const int32_t* offs;             /* [E] in DEVICE memory: the cumulative end row of every group; never read by the host */
    void* y;                         /* [T, N] dense */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t T, E, N, K;
    qs_stream_t stream;
} qs_mx_grouped_matmul_args;
int qs_mx_grouped_matmul_v(const qs_mx_grouped_matmul_args* args);
/* the kernel qs_mx_grouped_matmul_v launches for these operands, nothing enqueued and offs not read: QS_MX_GEMM_ROUTE_*, 0 for an
 * empty product, or the QS_ERR_* the call would return */
int qs_mx_grouped_matmul_route(const qs_mx_grouped_matmul_args* args);

/* The grouped product with the quantizing epilogue ("MX products that write MX codes" above): out_codes [T, N] and out_scales
 * [T, ceil(N / 32)] instead of y, the rows of group e bit for bit what qs_mx_matmul_q_v writes for them with the weight b[e], the tail
 * rows code 0 and scale byte 0 whatever `act` is.  Checks and their precedence are those of qs_mx_matmul_q_v with the additions of
 * qs_mx_grouped_matmul_v; out_codes sharing a byte with a_codes or b_codes is QS_ERR_ARG.  Routes as qs_mx_grouped_matmul_route. */
typedef struct qs_mx_grouped_matmul_q_args {
    uint32_t struct_size;            /* sizeof(qs_mx_grouped_matmul_q_args) as the caller compiled it */
    int32_t a_format, b_format;      /* the operands of qs_mx_grouped_matmul_args, with their meaning ... */
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    int64_t bias_batch_stride;
    const int32_t* offs;
    int32_t out_format;              /* ... and: enum qs_mx_format of the output */
    int32_t act;                     /* QS_MX_ACT_* */
    uint8_t* out_codes;              /* [T, N], one code per byte */
    uint8_t* out_scales;             /* [T, ceil(N / 32)] E8M0 bytes */
    int64_t T, E, N, K;
    qs_stream_t stream;
} qs_mx_grouped_matmul_q_args;
int qs_mx_grouped_matmul_q_v(const qs_mx_grouped_matmul_q_args* args);
int qs_mx_grouped_matmul_q_route(const qs_mx_grouped_matmul_q_args* args);

/* ---- MX grouped weight gradient ---------------------------------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The third product of a grouped linear layer's training step: dw[e] [N, K] = dy_e^T x_e, the contraction over the tokens of group e
 * -- the RAGGED axis.  Both operands carry their blocks of 32 along the token axis: gt_codes [N, T] / gt_scales [N, ceil(T / 32)] and
 * xt_codes [K, T] / xt_scales [K, ceil(T / 32)] are the col pairs of qs_mx_quant2_v on dy [T, N] and x [T, K].  `offs` [E] int32 in
 * DEVICE memory is qs_mx_grouped_matmul_v's, with its boundaries for ANY content: c_-1 = 0, c_e = min(max(offs[e], c_{e-1}), T),
 * group e owns the tokens [lo, hi) = [c_{e-1}, c_e).  The host side does no allocation, no synchronisation and no read of offs; it is
 * one launch, always.
 * Definition (normative).  If hi == lo, dw[e] is +0.  Otherwise let s0 = 128 floor(lo / 128), s1 = min(T, 128 ceil(hi / 128)), and
 *     G_e   = gt_codes[:, s0 : s1] with every column t outside [lo, hi) set to byte 0
 *     GS_e  = gt_scales[:, s0 / 32 : ceil(s1 / 32)] with every block that does not intersect [lo, hi) set to 127
 *     X_e, XS_e  likewise from xt
 *   dw[e] is, bit for bit, what qs_mx_matmul_v writes for A = G_e / GS_e [N, s1 - s0] and B = X_e / XS_e [K, s1 - s0] without a bias.
 *   - The 128-alignment of s0 is part of the definition: the kernel walks the global steps of 128 tokens, so each MFMA sees exactly
 *     the 128 codes qs_mx_matmul_v sees.
 *   - A block that straddles a boundary keeps its shared scale byte for both groups; a 0xFF byte there is NaN in both.
 *   - A block wholly outside the group contributes nothing, whatever its bytes are: a NaN row of another group does not leak.
 *   - Tokens t >= c_{E-1} belong to no group and reach nothing.
 *   - Checks: a NULL dw / offs, with T > 0 a NULL gt_codes / gt_scales / xt_codes / xt_scales, a format outside enum qs_mx_format, a
 *     negative extent or E beyond QS_MX_GROUPED_MAX_GROUPS is QS_ERR_ARG; then ydt (QS_ERR_DTYPE); then dw aligned to its element and
 *     offs to 4 bytes (QS_ERR_ALIGN).  E == 0, N == 0 or K == 0: nothing is enqueued, 0 is returned.  T == 0 is legal: every group is
 *     empty and dw is +0.  Any of N T, K T, E N K beyond INT64_MAX or a grid beyond 2^31 - 1 work-groups: QS_ERR_ARG.
 *   - One work-group per (group, 128 x 128 tile of [N, K]): the grid is E ceil(N / 128) ceil(K / 128), the group the slowest index.
 *     No split-K form, no atomics, no workspace: every element of dw is stored exactly once.
 *   - Routes: T % 16 == 0 with both code bases 16-byte aligned takes QS_MX_GEMM_ROUTE_VEC, anything else QS_MX_GEMM_ROUTE_PLAIN, with
 *     the same bits. */
typedef struct qs_mx_grouped_wgrad_args {
    uint32_t struct_size;            /* sizeof(qs_mx_grouped_wgrad_args) as the caller compiled it */
    int32_t g_format, x_format;      /* enum qs_mx_format of gt and xt, may differ */
    const uint8_t* gt_codes;         /* [N, T], one code per byte, dense: dy transposed, blocks along T */
    const uint8_t* gt_scales;        /* [N, ceil(T / 32)] E8M0 bytes */
    const uint8_t* xt_codes;         /* [K, T]: x transposed, blocks along T */
    const uint8_t* xt_scales;        /* [K, ceil(T / 32)] */
    const int32_t* offs;             /* [E] in DEVICE memory: the cumulative end token of every group; never read by the host */
    void* dw;                        /* [E, N, K] dense */
    int32_t ydt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int64_t T, E, N, K;
    qs_stream_t stream;
} qs_mx_grouped_wgrad_args;
int qs_mx_grouped_wgrad_v(const qs_mx_grouped_wgrad_args* args);
/* the kernel qs_mx_grouped_wgrad_v launches for these operands, nothing enqueued and offs not read: QS_MX_GEMM_ROUTE_*, 0 for an empty
 * result, or the QS_ERR_* the call would return */
int qs_mx_grouped_wgrad_route(const qs_mx_grouped_wgrad_args* args);

/* ---- MX gated products (SwiGLU / GeGLU: fused GLU epilogue) -------------------------------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The hidden layer of a gated MLP, h = act(x W_gate^T) * (x W_up^T), as ONE product on a combined weight b of N = 2 H rows whose
 * epilogue multiplies the two halves while they are accumulators and writes H columns: a float tensor, or the MX codes the next
 * product reads.  H % 32 == 0.  The rows of b (and the entries of bias) are INTERLEAVED in runs of 32: for q = 0 .. H / 32 - 1 the
 * rows [64 q, 64 q + 32) are the gate rows of the hidden units [32 q, 32 q + 32), the rows [64 q + 32, 64 q + 64) their up rows.  The
 * interleave is the caller's, done once when the weights are laid down.
 * Definition (normative).  Let v[m, n] be the float32 value qs_mx_matmul_v produces for the same operands (b as [2 H, K]) with ydt
 * = QS_F32, bias included.  For the hidden unit c = 32 q + t, t < 32:
 *   g = v[m, 64 q + t],  u = v[m, 64 q + 32 + t],  z[m, c] = act(g) * u      one float32 multiplication
 *   act(g) = g > 0 ? g : (g != g ? g : +0)                                    QS_MX_GLU_RELU
 *          = g / (1.0f + expf(-g))                                            QS_MX_GLU_SILU
 *          = (g * 0.5f) * (1.0f + erff(g * 0.70710678118654752440f))          QS_MX_GLU_GELU (the erf form; there is no tanh form)
 * all in float32 without contraction, expf / erff the device library's.  The output is
 *   out_format == -1:  y [M, H] = z rounded once to ydt, or
 *   out_format an enum qs_mx_format:  out_codes [M, H], out_scales [M, H / 32] = the codes and scales qs_mx_quant_fwd_v writes for z
 *   seen as [M, H, 1] in that format with QS_MX_ROUND_NEAREST -- a block that holds NaN / Inf gets the byte 0xFF and codes 0, an
 *   all-zero block the byte 0.
 * One launch, no workspace, no atomics, no float v or z in memory.  Stochastic rounding of the output and a split-K form are not
 * offered.
 *   - Checks and their precedence are those of qs_mx_matmul_q_v on N = 2 H; with its QS_ERR_ARG checks of the operands come: H
 *     negative or H % 32 != 0, act outside QS_MX_GLU_*, out_format neither -1 nor an enum qs_mx_format, a NULL y (out_format == -1)
 *     or a NULL out_codes / out_scales (otherwise).  Then, for a float output, ydt (QS_ERR_DTYPE); then y aligned to its element and
 *     bias to 4 bytes (QS_ERR_ALIGN).  M == 0 or H == 0: nothing is enqueued, 0 is returned.  After the size checks: an output (y,
 *     out_codes or out_scales) sharing a byte with a_codes or b_codes is QS_ERR_ARG.
 *   - Nothing outside y [M, H], or out_codes [M, H] and out_scales [M, H / 32], is written.
 *   - Routes: QS_MX_GEMM_ROUTE_*, by the conditions of qs_mx_matmul_route on the inputs. */
#define QS_MX_GLU_RELU 0
#define QS_MX_GLU_SILU 1
#define QS_MX_GLU_GELU 2
typedef struct qs_mx_glu_matmul_args {
    uint32_t struct_size;            /* sizeof(qs_mx_glu_matmul_args) as the caller compiled it */
    int32_t a_format, b_format;      /* enum qs_mx_format, may differ */
    const uint8_t* a_codes;          /* [M, K], one code per byte */
    const uint8_t* a_scales;         /* [M, ceil(K / 32)] E8M0 bytes */
    const uint8_t* b_codes;          /* [2 H, K], rows interleaved as above */
    const uint8_t* b_scales;         /* [2 H, ceil(K / 32)] */
    const float* bias;               /* nullable, float32 [2 H], interleaved as the rows of b */
    int32_t out_format;              /* enum qs_mx_format of the output, or -1 for a float y */
    int32_t act;                     /* QS_MX_GLU_* */
    void* y;                         /* out_format == -1: [M, H] */
    int32_t ydt;                     /* out_format == -1: QS_F32, QS_BF16 or QS_F16 */
    uint8_t* out_codes;              /* otherwise: [M, H], one code per byte */
    uint8_t* out_scales;             /* otherwise: [M, H / 32] E8M0 bytes */
    int64_t M, H, K;
    qs_stream_t stream;
    void* v;                         /* qs_mx_glu_matmul_pre_v only (below): [M, 2 H], columns interleaved as the rows of b */
    int32_t vdt;                     /* ... QS_F32, QS_BF16 or QS_F16 */
    int32_t reserved1;
} qs_mx_glu_matmul_args;
int qs_mx_glu_matmul_v(const qs_mx_glu_matmul_args* args);
/* the kernel qs_mx_glu_matmul_v launches for these operands, nothing enqueued: QS_MX_GEMM_ROUTE_*, 0 for an empty product, or the
 * QS_ERR_* the call would return */
int qs_mx_glu_matmul_route(const qs_mx_glu_matmul_args* args);
/* The same product for a TRAINING forward: one more output, the pre-activations v [M, 2 H] in vdt.  v[m, n] is the accumulator plus
 * bias rounded once to vdt: bit for bit what qs_mx_matmul_v writes for the same operands (b as [2 H, K]) with ydt = vdt.  The first
 * output -- y, or out_codes / out_scales -- is bit for bit qs_mx_glu_matmul_v's.  The kernels are instantiations of their own, so
 * qs_mx_glu_matmul_v, which never looks at v / vdt, launches what it launched before these fields existed.
 * Checks: qs_mx_glu_matmul_v's with v where y is -- a NULL v is QS_ERR_ARG, vdt QS_ERR_DTYPE after ydt, v aligned to its element
 * QS_ERR_ALIGN; after the size checks, v sharing a byte with a_codes, b_codes or the first output is QS_ERR_ARG.  Nothing outside v
 * [M, 2 H] and the first output is written. */
int qs_mx_glu_matmul_pre_v(const qs_mx_glu_matmul_args* args);
int qs_mx_glu_matmul_pre_route(const qs_mx_glu_matmul_args* args);

/* The grouped product ("MX grouped matrix product" above: offs, its boundaries c_e for ANY content, the tail rows) with the gated
 * epilogue: b is [E, 2 H, K], every weight interleaved as above, bias NULL, [2 H] (bias_batch_stride == 0) or [E, 2 H]
 * (bias_batch_stride == 2 H).  A row of group e is bit for bit what qs_mx_glu_matmul_v writes for it with the weight b[e] and the bias
 * of e.  The tail rows r >= c_{E-1} get +0, or code 0 and the scale byte 0, whatever act is.  Checks and their precedence are those of
 * qs_mx_grouped_matmul_q_v on N = 2 H with the additions of qs_mx_glu_matmul_v; offs is never read by the host.  Routes as
 * qs_mx_grouped_matmul_route. */
typedef struct qs_mx_grouped_glu_matmul_args {
    uint32_t struct_size;            /* sizeof(qs_mx_grouped_glu_matmul_args) as the caller compiled it */
    int32_t a_format, b_format;      /* the operands of qs_mx_grouped_matmul_args, with their meaning, b [E, 2 H, K] ... */
    const uint8_t* a_codes;
    const uint8_t* a_scales;
    const uint8_t* b_codes;
    const uint8_t* b_scales;
    const float* bias;
    int64_t bias_batch_stride;       /* 0 or 2 H */
    const int32_t* offs;
    int32_t out_format;              /* ... and the outputs of qs_mx_glu_matmul_args on T rows */
    int32_t act;
    void* y;
    int32_t ydt;
    uint8_t* out_codes;
    uint8_t* out_scales;
    int64_t T, E, H, K;
    qs_stream_t stream;
    void* v;                         /* qs_mx_grouped_glu_matmul_pre_v only: [T, 2 H] */
    int32_t vdt;
    int32_t reserved1;
} qs_mx_grouped_glu_matmul_args;
int qs_mx_grouped_glu_matmul_v(const qs_mx_grouped_glu_matmul_args* args);
int qs_mx_grouped_glu_matmul_route(const qs_mx_grouped_glu_matmul_args* args);
/* qs_mx_glu_matmul_pre_v for the grouped product: v [T, 2 H] is bit for bit what qs_mx_grouped_matmul_v writes for the same operands
 * (b as [E, 2 H, K]) with ydt = vdt, the tail rows +0; the first output is qs_mx_grouped_glu_matmul_v's.  Checks as there, v as above. */
int qs_mx_grouped_glu_matmul_pre_v(const qs_mx_grouped_glu_matmul_args* args);
int qs_mx_grouped_glu_matmul_pre_route(const qs_mx_grouped_glu_matmul_args* args);

/* ---- MX gated backward quantizer (the GLU derivative in front of the two-way quantizer) ----------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The gradient of h = act(g) * u with respect to the interleaved pre-activations, as the MX operands of the two backward products,
 * from ONE read of dh [T, H] and v [T, 2 H] (both CONTIGUOUS; float32, bf16 or fp16, independently).  H % 32 == 0.
 * Definition (normative).  All arithmetic is float32 without contraction on the widened inputs, expf / erff the device library's.
 * For the hidden unit c = 32 q + t, t < 32:  g = v[m, 64 q + t],  u = v[m, 64 q + 32 + t],  d = dh[m, c],
 *   dv[m, 64 q + t]      = (d * u) * act'(g)
 *   dv[m, 64 q + 32 + t] = d * act(g)                       act as for the gated products above
 *   act'(g) = g > 0 ? 1 : (g != g ? g : +0)                                          QS_MX_GLU_RELU
 *           = s * (1.0f + g * (1.0f - s)),  s = 1.0f / (1.0f + expf(-g))             QS_MX_GLU_SILU
 *           = fmaf(g, expf(-0.5f * g * g) * kBeta, 0.5f * (1.0f + erff(g * kAlpha)))  QS_MX_GLU_GELU, kAlpha = (float)sqrt(1/2), kBeta =
 *             (float)(2/sqrt(pi) * sqrt(1/2) * 0.5): the factor ATen's GPU gelu_backward multiplies by (the one fma is part of it)
 * The four outputs are bit for bit what qs_mx_quant2_v writes for the float32 tensor dv [R = T, C = 2 H] with the same row_format,
 * col_format, rounding, seed, step and index_base (the stochastic words: stream 0 at the index of row_codes, stream 1 at that of
 * col_codes): row_codes [T, 2 H], row_scales [T, 2 H / 32], col_codes [2 H, T], col_scales [2 H, ceil(T / 32)].  dv is never rounded
 * to a narrower type and never written; nothing but the outputs is written, no workspace, no atomics.
 * A pair whose format is -1 is skipped and its pointers are ignored; a pair whose format is given needs both its pointers.
 *   - Checks, in order: the rounding operands as for qs_mx_quant2_v; QS_ERR_ARG: a null or too short descriptor, dh or v NULL, both
 *     formats -1, a format neither -1 nor an enum qs_mx_format, a NULL pointer of a given pair, T or H negative, H % 32 != 0, act
 *     outside QS_MX_GLU_*; QS_ERR_DTYPE: dhdt or vdt none of the three; QS_ERR_ALIGN: dh or v not aligned to its element.
 *   - T == 0 or H == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_Q2_ROUTE_TILE_VEC (aligned 16- / 8-byte loads, 16-byte stores of col_codes): dh and v 16-byte aligned and, when the col
 *     pair is written, T % 16 == 0 and col_codes 16-byte aligned.  Anything else takes QS_MX_Q2_ROUTE_TILE_PLAIN: any T >= 1. */
typedef struct qs_mx_glu_bwd_quant2_args {
    uint32_t struct_size;            /* sizeof(qs_mx_glu_bwd_quant2_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ; -1: that pair is skipped */
    int32_t act;                     /* QS_MX_GLU_* */
    const void* dh;                  /* [T, H] row-major */
    const void* v;                   /* [T, 2 H] row-major, columns in the 32-run interleave */
    int32_t dhdt, vdt;               /* QS_F32, QS_BF16 or QS_F16 */
    uint8_t* row_codes;              /* [T, 2 H] */
    uint8_t* row_scales;             /* [T, 2 H / 32] */
    uint8_t* col_codes;              /* [2 H, T] */
    uint8_t* col_scales;             /* [2 H, ceil(T / 32)] */
    int64_t T, H;
    qs_stream_t stream;
    int32_t rounding;                /* QS_MX_ROUND_* */
    int32_t reserved0;
    uint64_t seed;
    const int64_t* step;             /* nullable (= 0); device memory, one int64, read by the kernel */
    uint64_t index_base;             /* a multiple of 4; added to the indices of both pairs */
} qs_mx_glu_bwd_quant2_args;
int qs_mx_glu_bwd_quant2_v(const qs_mx_glu_bwd_quant2_args* args);
/* the kernel qs_mx_glu_bwd_quant2_v launches for these operands, nothing enqueued: QS_MX_Q2_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
int qs_mx_glu_bwd_quant2_route(const qs_mx_glu_bwd_quant2_args* args);

/* ---- MX normalising quantizer (RMSNorm / LayerNorm in front of the one-way / two-way quantizer) -----------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The MX operands of y = norm(x) * weight (+ bias) from x [R, C] (CONTIGUOUS, C innermost; float32, bf16 or fp16) without the float
 * y in memory: the normalisation runs over C, `weight` [C] and `bias` [C] are float32 (NULL: ones / none).
 * Definition (normative).  All arithmetic is float32 without contraction on the widened inputs; `/` and sqrt are the correctly
 * rounded IEEE operations; Cf = (float)C.
 *   sum(t) over a row, t_0 .. t_(C-1) -- a FIXED order that depends on C alone (not on R, the dtype, the route, the launch or mode):
 *     t_i = +0 for C <= i < 512 ceil(C / 512)
 *     quad sums        q_m = (t_4m + t_(4m+1)) + (t_(4m+2) + t_(4m+3))
 *     128 strided partial sums   P_j = (((+0 + q_j) + q_(j+128)) + q_(j+256)) + ...      j < 128, ascending
 *     pairwise tree    for s = 64, 32, 16, 8, 4, 2, 1:  P_j = P_j + P_(j+s), j < s;   sum = P_0
 *     (with tensors: pad to [K, 128, 4]; q = (t[..,0] + t[..,1]) + (t[..,2] + t[..,3]); P = 0; P = P + q[k] for k = 0 .. K-1; then
 *      seven element-wise additions of the upper half of P to the lower)
 *   QS_MX_NORM_RMS     ms   = sum(x_i * x_i) / Cf
 *                      rstd = 1.0f / sqrt(ms + eps)
 *                      y_i  = (x_i * rstd) * w_i (+ b_i)
 *   QS_MX_NORM_LAYER   mean = sum(x_i) / Cf
 *                      d_i  = x_i - mean
 *                      ms   = sum(d_i * d_i) / Cf                (the two-pass variance; the padding terms are +0, not mean^2)
 *                      rstd = 1.0f / sqrt(ms + eps)
 *                      y_i  = (d_i * rstd) * w_i (+ b_i)
 *   rstd is a quiet NaN where ms is not finite: a row that holds a NaN or an Inf (or whose squares overflow) is NaN in EVERY element
 *   of y, so every block that row touches has the scale byte 0xFF and zero codes, in both pairs.  A multiplication by an absent
 *   weight and an addition of an absent bias are not performed.  An all-zero row gives y = b (eps > 0).
 * Outputs: row_codes [R, C] / row_scales [R, ceil(C / 32)] are bit for bit the codes and scales qs_mx_quant_fwd_v writes for y with
 * blocks along C in row_format, col_codes [C, R] / col_scales [C, ceil(R / 32)] the col pair qs_mx_quant2_v writes for y in col_format
 * (col_format -1: skipped, its pointers ignored); both round to nearest-even -- stochastic rounding is not offered.  rstd [R]
 * float32 is always written (it is also the only workspace: the statistics launch writes it, the quantizing launch reads it), mean [R]
 * float32 in layer mode (ignored in rms mode).  Nothing else is written; no atomics; two launches on `stream`, nothing read by the host.
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, an unknown mode, x, row_codes, row_scales or rstd NULL, mean NULL
 *     in layer mode, row_format no enum qs_mx_format, col_format neither -1 nor one, a NULL pointer of a given col pair, eps negative
 *     or not finite, R or C negative; QS_ERR_DTYPE: xdt none of the three; QS_ERR_ALIGN: x not aligned to its element, or weight, bias,
 *     rstd or mean not to 4 bytes.
 *   - R == 0 or C == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_NORM_ROUTE_VEC (16-byte loads of x in the statistics, 16- / 8-byte loads in the quantizing launch, 4-byte stores of
 *     row_codes where it is 4-byte aligned, 16-byte stores of col_codes where R % 16 == 0 and it is 16-byte aligned): C % 32 == 0
 *     and x, weight, bias 16-byte aligned.  Anything else takes QS_MX_NORM_ROUTE_PLAIN, element accesses: any R, C >= 1, same bits. */
#define QS_MX_NORM_RMS 0
#define QS_MX_NORM_LAYER 1
typedef struct qs_mx_norm_quant_args {
    uint32_t struct_size;            /* sizeof(qs_mx_norm_quant_args) as the caller compiled it */
    int32_t mode;                    /* QS_MX_NORM_* */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ; col_format -1: the col pair is skipped */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    float eps;
    const void* x;                   /* [R, C] row-major */
    const float* weight;             /* [C], nullable (ones) */
    const float* bias;               /* [C], nullable (none) */
    uint8_t* row_codes;              /* [R, C] */
    uint8_t* row_scales;             /* [R, ceil(C / 32)] */
    uint8_t* col_codes;              /* [C, R] */
    uint8_t* col_scales;             /* [C, ceil(R / 32)] */
    float* rstd;                     /* [R] */
    float* mean;                     /* [R], layer mode */
    int64_t R, C;
    qs_stream_t stream;
} qs_mx_norm_quant_args;
int qs_mx_norm_quant_v(const qs_mx_norm_quant_args* args);
/* the kernels qs_mx_norm_quant_v launches for these operands, nothing enqueued: QS_MX_NORM_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
#define QS_MX_NORM_ROUTE_VEC 1
#define QS_MX_NORM_ROUTE_PLAIN 2
int qs_mx_norm_quant_route(const qs_mx_norm_quant_args* args);

/* ---- MX norm backward (the backward of the normalisation of the MX normalising quantizer) ------------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * From dxhat [R, C], the gradient with respect to the norm's output y = xhat * weight (+ bias) (float32, bf16 or fp16), x [R, C] in
 * its own dtype, the statistics rstd [R] and (layer mode) mean [R] the forward wrote, and weight [C] (float32; NULL: ones):
 * dx [R, C] in x's dtype, dweight [C] and dbias [C] float32.  All three tensors are CONTIGUOUS, C innermost; each output is nullable
 * and is then neither computed nor written.
 * Definition (normative).  All arithmetic is float32 without contraction on the widened inputs; `/` is the correctly rounded IEEE
 * operation; Cf = (float)C.
 *   xhat_i = (x_i - mean) * rstd     QS_MX_NORM_LAYER           xhat_i = x_i * rstd     QS_MX_NORM_RMS      (as the forward forms it)
 *   g_i    = dxhat_i * w_i           (an absent weight: g_i = dxhat_i, no multiplication)
 *   c1     = rowsum(g_i * xhat_i) / Cf
 *   c2     = rowsum(g_i) / Cf        layer mode only
 *   dx_i   = rstd * (g_i - xhat_i * c1)                  rms
 *   dx_i   = rstd * ((g_i - xhat_i * c1) - c2)           layer           rounded once, to nearest-even, to x's dtype
 *   with `dresidual` [R, C] in x's dtype (qs_mx_norm_bwd_res_v below only): dx_i = (the float32 value above) + f32(dresidual_i), one
 *   more float32 addition in front of that single rounding; without it nothing changes
 *   dweight_c = colsum_r(dxhat[r, c] * xhat[r, c])
 *   dbias_c   = colsum_r(dxhat[r, c])
 *   rowsum is the sum over a row of the MX normalising quantizer above -- a function of C alone; the terms behind the row are +0.
 *   colsum(t) over a column, t_0 .. t_(R-1) -- a FIXED order that depends on R alone (not on C, a dtype, the route, the launch, the
 *   mode or on which outputs are asked for):
 *     t_r = +0 for R <= r < 128 T, T = ceil(R / 128) row tiles
 *     in row tile k, on u_i = t_(128 k + i):
 *       16 strided partial sums   S_l = (((+0 + u_l) + u_(l+16)) + u_(l+32)) + ... + u_(l+112)      l < 16, ascending
 *       pairwise tree             for s = 8, 4, 2, 1:  S_l = S_l + S_(l+s), l < s;   v_k = S_0
 *     over the tiles:
 *       128 strided partial sums  P_j = ((+0 + v_j) + v_(j+128)) + ...                              j < 128, ascending; +0 for j >= T
 *       pairwise tree             for s = 64, 32, 16, 8, 4, 2, 1:  P_j = P_j + P_(j+s), j < s;   colsum = P_0
 *     (with tensors: pad to [T, 8, 16, C]; S = 0; S = S + u[:, m] for m = 0 .. 7; four element-wise additions of the upper half of S
 *      to the lower give v [T, C]; pad v to [K, 128, C]; P = 0; P = P + v[k] for k = 0 .. K-1; seven more halvings)
 *   There are no special cases: NaN and Inf propagate as the arithmetic propagates them -- a row whose rstd is NaN (a row of x the
 *   forward found not finite) has NaN in every element of dx and makes every element of dweight NaN.  No atomics: the same bits on
 *   every run.
 * Workspace: caller-provided, `workspace_bytes` at least what qs_mx_norm_bwd_plan tells for the same R, C, mode and needs, 16-byte
 * aligned.  It holds c1 [R] and c2 [R] (layer mode) when dx is asked for, and the row tiles' column sums, two arrays [T, C], when
 * dweight or dbias is -- float32, each part at the next multiple of 16 bytes.  Its contents on return are unspecified.
 * Up to three launches on `stream`, nothing read by the host: the row statistics (only with dx), the apply launch over 128 x 64
 * tiles (dx and the tiles' column sums), the fold of those sums (only with dweight or dbias).
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, an unknown mode, dxhat, x or rstd NULL, mean NULL in layer mode,
 *     dx, dweight and dbias all NULL, R or C negative; QS_ERR_DTYPE: xdt or gdt none of the three; QS_ERR_ALIGN: x or dx not aligned to
 *     x's element, dxhat not to its own, weight, rstd, mean, dweight or dbias not to 4 bytes, workspace not to 16; QS_ERR_ARG: R * C
 *     beyond 64 bits or more tiles than a launch takes (2^31 - 1); QS_ERR_WORKSPACE: workspace NULL or shorter than the plan.
 *   - R == 0 or C == 0: nothing is enqueued and nothing written, 0 is returned -- the dweight / dbias of a tensor with R == 0 and
 *     C > 0 are sums of no terms, +0, and are the CALLER's to fill (the Python binding does).
 *   - QS_MX_NORM_BWD_ROUTE_VEC (16-byte accesses of float32 tensors, 16- / 8-byte ones of two-byte tensors): C % 32 == 0 and dxhat,
 *     x, weight, dx 16-byte aligned.  Anything else takes QS_MX_NORM_BWD_ROUTE_PLAIN, element accesses: any R, C >= 1, same bits. */
typedef struct qs_mx_norm_bwd_args {
    uint32_t struct_size;            /* sizeof(qs_mx_norm_bwd_args) as the caller compiled it */
    int32_t mode;                    /* QS_MX_NORM_* */
    int32_t xdt;                     /* dtype of x and dx: QS_F32, QS_BF16 or QS_F16 */
    int32_t gdt;                     /* dtype of dxhat, likewise */
    const void* dxhat;               /* [R, C] row-major */
    const void* x;                   /* [R, C] row-major */
    const float* weight;             /* [C], nullable (ones) */
    const float* rstd;               /* [R] */
    const float* mean;               /* [R], layer mode */
    void* dx;                        /* [R, C], nullable */
    float* dweight;                  /* [C], nullable */
    float* dbias;                    /* [C], nullable */
    void* workspace;
    uint64_t workspace_bytes;
    int64_t R, C;
    qs_stream_t stream;
} qs_mx_norm_bwd_args;
int qs_mx_norm_bwd_v(const qs_mx_norm_bwd_args* args);
/* the kernels qs_mx_norm_bwd_v launches for these operands, nothing enqueued: QS_MX_NORM_BWD_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
#define QS_MX_NORM_BWD_ROUTE_VEC 1
#define QS_MX_NORM_BWD_ROUTE_PLAIN 2
int qs_mx_norm_bwd_route(const qs_mx_norm_bwd_args* args);
/* the workspace qs_mx_norm_bwd_v needs for [R, C] in `mode` when dx is asked for (need_dx != 0) and when dweight or dbias is
 * (need_cols != 0): up16(4 R) (twice in layer mode) with need_dx, plus 2 up16(4 ceil(R / 128) C) with need_cols, up16 rounding up to a
 * multiple of 16; 0 for an empty tensor.  QS_ERR_ARG: workspace_bytes NULL, an unknown mode, a negative extent, extents the call refuses. */
int qs_mx_norm_bwd_plan(int64_t R, int64_t C, int32_t mode, int32_t need_dx, int32_t need_cols, uint64_t* workspace_bytes);

/* MX norm backward with the residual stream's gradient.  Added without raising QS_ABI_VERSION (28): symbols are only added;
 * qs_mx_norm_bwd_args and qs_mx_norm_bwd_v above are unchanged.
 *
 * The definition above with one more operand, `dresidual` [R, C] (CONTIGUOUS, the dtype of x and dx; nullable), the gradient that
 * reaches the norm's input by the residual stream:
 *   dx_i   = rstd * (g_i - xhat_i * c1)          + f32(dresidual_i)       rms
 *   dx_i   = rstd * ((g_i - xhat_i * c1) - c2)   + f32(dresidual_i)       layer
 * ONE more float32 addition, in front of the single rounding to x's dtype (not dx rounded and then added).  c1, c2, dweight and
 * dbias do not see it.  With dresidual NULL every output is qs_mx_norm_bwd_v's, bit for bit.  The workspace, its plan
 * (qs_mx_norm_bwd_plan) and the launches are qs_mx_norm_bwd_v's; dresidual is read by the apply launch, with the tile's other loads.
 *   - Checks: qs_mx_norm_bwd_v's, in its order, and with them: QS_ERR_ARG (after "dx, dweight and dbias all NULL"): dresidual given
 *     and dx NULL; QS_ERR_ALIGN: dresidual not aligned to x's element.
 *   - QS_MX_NORM_BWD_ROUTE_VEC: as above and dresidual 16-byte aligned. */
typedef struct qs_mx_norm_bwd_res_args {
    uint32_t struct_size;            /* sizeof(qs_mx_norm_bwd_res_args) as the caller compiled it */
    int32_t mode;                    /* QS_MX_NORM_* */
    int32_t xdt;                     /* dtype of x, dx and dresidual: QS_F32, QS_BF16 or QS_F16 */
    int32_t gdt;                     /* dtype of dxhat, likewise */
    const void* dxhat;               /* [R, C] row-major */
    const void* x;                   /* [R, C] row-major */
    const float* weight;             /* [C], nullable (ones) */
    const float* rstd;               /* [R] */
    const float* mean;               /* [R], layer mode */
    void* dx;                        /* [R, C], nullable */
    float* dweight;                  /* [C], nullable */
    float* dbias;                    /* [C], nullable */
    void* workspace;
    uint64_t workspace_bytes;
    int64_t R, C;
    qs_stream_t stream;
    const void* dresidual;           /* [R, C] row-major, nullable; needs dx */
} qs_mx_norm_bwd_res_args;
int qs_mx_norm_bwd_res_v(const qs_mx_norm_bwd_res_args* args);
/* the kernels qs_mx_norm_bwd_res_v launches for these operands, nothing enqueued: QS_MX_NORM_BWD_ROUTE_*, 0 for an empty tensor, or
 * the QS_ERR_* the call would return */
int qs_mx_norm_bwd_res_route(const qs_mx_norm_bwd_res_args* args);

/* ---- MX add-norm quantizer (the residual add of a pre-norm block in front of the MX normalising quantizer) ----------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * From x [R, C] (the output of the previous branch) and residual [R, C] (the stream), both CONTIGUOUS, C innermost, each float32,
 * bf16 or fp16 and not necessarily alike: the new stream h [R, C] in RESIDUAL's dtype, and the MX operands of norm(h) * weight (+ bias).
 * Definition (normative).
 *   h_i = round_hdt(f32(x_i) + f32(r_i))      ONE float32 addition, without contraction, rounded once to nearest-even to h's dtype
 *                                             (float32: no rounding).  A NaN or an Inf of the sum is kept in h.
 *   Everything else is the MX normalising quantizer above applied to that ROUNDED h: the sums run over the widened h_i, not over the
 *   unrounded float32 sums.  So row_codes, row_scales, col_codes, col_scales, rstd and mean are, bit for bit, what
 *   qs_mx_norm_quant_v writes for x = h, xdt = rdt -- the NaN-row rule included: a row whose h holds a NaN or an Inf is NaN as a whole.
 * h must not overlap x or residual (an in-place update of the stream is not offered); the outputs must not overlap the inputs.
 * Two launches on `stream`, nothing read by the host: a statistics launch that loads x and residual, stores h and forms the row sums
 * from the rounded values (layer mode's second walk forms h again from x and residual; it does not read h back), then the quantizing
 * launch of qs_mx_norm_quant_v on h.  No atomics, no workspace beyond rstd / mean.
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, an unknown mode, x, residual, h, row_codes, row_scales or rstd
 *     NULL, mean NULL in layer mode, row_format no enum qs_mx_format, col_format neither -1 nor one, a NULL pointer of a given col
 *     pair, eps negative or not finite, R or C negative; QS_ERR_DTYPE: xdt or rdt none of the three; QS_ERR_ALIGN: x not aligned to
 *     its element, residual or h not to rdt's, or weight, bias, rstd or mean not to 4 bytes; QS_ERR_ARG: R * C beyond 64 bits or more
 *     tiles than a launch takes.
 *   - R == 0 or C == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_NORM_ROUTE_VEC (16-byte loads of x and residual and 16-byte stores of h in the statistics launch; the quantizing launch
 *     as above): C % 32 == 0 and x, residual, h, weight, bias 16-byte aligned.  Anything else takes QS_MX_NORM_ROUTE_PLAIN, element
 *     accesses: any R, C >= 1, same bits. */
typedef struct qs_mx_add_norm_quant_args {
    uint32_t struct_size;            /* sizeof(qs_mx_add_norm_quant_args) as the caller compiled it */
    int32_t mode;                    /* QS_MX_NORM_* */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ; col_format -1: the col pair is skipped */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    float eps;
    const void* x;                   /* [R, C] row-major */
    const float* weight;             /* [C], nullable (ones) */
    const float* bias;               /* [C], nullable (none) */
    uint8_t* row_codes;              /* [R, C] */
    uint8_t* row_scales;             /* [R, ceil(C / 32)] */
    uint8_t* col_codes;              /* [C, R] */
    uint8_t* col_scales;             /* [C, ceil(R / 32)] */
    float* rstd;                     /* [R] */
    float* mean;                     /* [R], layer mode */
    int64_t R, C;
    qs_stream_t stream;
    const void* residual;            /* [R, C] row-major */
    void* h;                         /* [R, C] row-major, residual's dtype: written */
    int32_t rdt;                     /* dtype of residual and h: QS_F32, QS_BF16 or QS_F16 */
    int32_t reserved0;               /* 0 */
} qs_mx_add_norm_quant_args;
int qs_mx_add_norm_quant_v(const qs_mx_add_norm_quant_args* args);
/* the kernels qs_mx_add_norm_quant_v launches for these operands, nothing enqueued: QS_MX_NORM_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
int qs_mx_add_norm_quant_route(const qs_mx_add_norm_quant_args* args);

/* ---- MX softmax quantizer (scale, additive mask and softmax in front of the one-way quantizer) ---------------------------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * The MX operand of p = softmax(s * scale (+ mask)) over the last axis of s [G, T, S] (CONTIGUOUS, S innermost; float32, bf16 or fp16)
 * without u, e or the float p in memory: the attention weights as the codes the P . V product multiplies.  It is NOT defined through a
 * library's exp: the exponential below is part of the definition, so the bytes are the same on every device.
 * Definition (normative), for the row s_0 .. s_(S-1) at (g, t).  All arithmetic is float32 on the widened inputs, every operation
 * rounded on its own (no contraction, no FMA); `/` is the correctly rounded IEEE division.
 *   L   = S, or with `causal` min(t + 1, S): the lower triangle aligned top-left; T != S is allowed
 *   u_j = s_j * scale              without a mask
 *       = (s_j * scale) + a_j      with one; a is the row (t) of mask [T, S] (mask_slices 1) or the row (g, t) of mask [G, T, S]
 *       = -inf                     for L <= j < S, whatever s_j and a_j hold (they are not read)
 *   m   = max_j u_j
 *   t_j = u_j - m                                                                    (<= 0)
 *   e_j = E(t_j)
 *   Z   = sum(e) in the row-sum order of the MX normalising quantizer above with C = S: a function of S alone
 *   p_j = e_j / Z
 *   E(t):  n = rint(t * 1.44269504f)                            ties to even; 1.44269504f is 0x3fb8aa3b
 *          r = (t - n * 0.693359375f) - n * (-2.12194440e-4f)   Cody-Waite: 0.693359375f is 0x3f318000 (n * it is exact),
 *                                                               -2.12194440e-4f is 0xb95e8083
 *          P = c7; P = P * r + c_k for k = 6 .. 0               Horner, the multiplication and the addition rounded separately;
 *                                                               c_k = 1 / k! rounded to float32: c7 = 0x39500d01 (1 / 5040),
 *                                                               0x3ab60b61, 0x3c088889, 0x3d2aaaab, 0x3e2aaaab, 0.5f, 1.0f, c0 = 1.0f
 *          E = P * 2^n                                          exact: n in [-126, 0], and P > 1 at n = -126
 *          E = +0 where t < -87.0f or t = -inf
 *     E(0) = 1.0f exactly, so the row's maximum contributes exactly 1 and Z >= 1.  Against exp in float64 the largest relative error
 *     found on [-87, 0] is below one float32 ulp (tests/test_mx_softmax.py asserts the bound).
 *   Exceptional rows: a row whose u holds a NaN, or whose m is +inf, or whose m is -inf (every column masked; L = 0 cannot occur) is
 *   NaN in EVERY element of p, the columns behind L included: scale byte 0xFF and zero codes in each of its blocks.  A -inf beside a
 *   finite m is a plain zero.  Rows do not influence each other.
 * Outputs: codes [G, T, S] / scales [G, T, ceil(S / 32)] are bit for bit the codes and scales qs_mx_quant_fwd_v writes for p with
 * blocks along S in `format`, rounding to nearest-even -- stochastic rounding is not offered.  Nothing else is written; no atomics, no
 * workspace; ONE launch on `stream`, nothing read by the host.  A wave owns a row; a row of S <= 1024 is read from memory once, a
 * longer one three times (the bytes do not depend on which).  A causal row reads nothing at or behind L.
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, s, codes or scales NULL, format no enum qs_mx_format, causal neither
 *     0 nor 1, G, T or S negative, mask given with mask_slices neither 1 nor G; QS_ERR_DTYPE: sdt none of the three; QS_ERR_ALIGN: s not
 *     aligned to its element or mask not to 4 bytes; QS_ERR_ARG: G * T * S beyond 64 bits or more rows than a launch takes.
 *     `scale` is any float (a NaN makes every row NaN).  mask and causal may be given together (the definition covers it).
 *   - G == 0, T == 0 or S == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_SOFTMAX_ROUTE_VEC (16-byte loads of s and mask, 8-byte stores of codes): S % 32 == 0, s and mask 16-byte aligned and codes
 *     8-byte aligned.  Anything else takes QS_MX_SOFTMAX_ROUTE_PLAIN, element accesses each predicated on its own index: any T, S >= 1,
 *     any element-aligned base, same bits. */
typedef struct qs_mx_softmax_quant_args {
    uint32_t struct_size;            /* sizeof(qs_mx_softmax_quant_args) as the caller compiled it */
    int32_t format;                  /* enum qs_mx_format */
    int32_t sdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int32_t causal;                  /* 0 or 1 */
    float scale;
    int32_t reserved0;               /* 0 */
    const void* s;                   /* [G, T, S] row-major */
    const float* mask;               /* [T, S] or [G, T, S], additive, nullable (none) */
    int64_t mask_slices;             /* 1: mask is [T, S], shared by the slices; G: it is [G, T, S].  Read only with a mask */
    uint8_t* codes;                  /* [G, T, S] */
    uint8_t* scales;                 /* [G, T, ceil(S / 32)] */
    int64_t G, T, S;
    qs_stream_t stream;
} qs_mx_softmax_quant_args;
int qs_mx_softmax_quant_v(const qs_mx_softmax_quant_args* args);
/* the kernel qs_mx_softmax_quant_v launches for these operands, nothing enqueued: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
#define QS_MX_SOFTMAX_ROUTE_VEC 1
#define QS_MX_SOFTMAX_ROUTE_PLAIN 2
int qs_mx_softmax_quant_route(const qs_mx_softmax_quant_args* args);

/* ---- MX two-way softmax quantizer (the MX softmax quantizer with p's transposed pair and the row statistics) ----------------------------
 * Added without raising QS_ABI_VERSION (28): symbols are only added; qs_mx_softmax_quant_args and qs_mx_softmax_quant_v above are
 * unchanged.
 *
 * The training side's forward.  p [G, T, S] is the p of the MX softmax quantizer above, to the bit (same u, m, E, Z, same exceptional
 * rows).  Outputs:
 *   row_codes [G, T, S] / row_scales [G, T, ceil(S / 32)]   bit for bit what qs_mx_softmax_quant_v writes in `row_format`
 *   col_codes [G, S, T] / col_scales [G, S, ceil(T / 32)]   (col_format != -1) slice by slice the codes and scales of p^T with blocks
 *                                                           along T in `col_format`: the operand of dV = P^T dO.  A row of p that is
 *                                                           NaN as a whole puts 0xFF into every column block it touches.
 *   m [G T], Z [G T]                                        the row maximum (m + 0.0f: a zero maximum of either sign is +0) and the
 *                                                           row sum of the definition, float32; both are the
 *                                                           quiet NaN 0x7fc00000 for a row that is NaN as a whole (its u holds a NaN,
 *                                                           m = +inf, or nothing is admitted).  Always written: the second launch reads
 *                                                           them.
 * Rounding is to nearest-even.  Two launches on `stream`, nothing read by the host, no atomics, no workspace beyond m and Z: a
 * statistics launch (one wave per row) that writes m and Z, then the tile of the MX two-way quantizer (128 rows of T x 64 columns of
 * S) per slice with p_j = E(u_j - m) / Z as its widen step -- E is evaluated in both launches, to the same bits.  A causal row reads
 * nothing at or behind L.  Without a col pair the second launch skips the LDS staging, the barrier and its second phase.
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, s, row_codes, row_scales, m or Z NULL, row_format no enum
 *     qs_mx_format, col_format neither -1 nor one, a NULL pointer of a given col pair, causal neither 0 nor 1, G, T or S negative, mask
 *     given with mask_slices neither 1 nor G; QS_ERR_DTYPE: sdt none of the three; QS_ERR_ALIGN: s not aligned to its element, or mask,
 *     m or Z not to 4 bytes; QS_ERR_ARG: G * T * S beyond 64 bits, more rows or more tiles than a launch takes.
 *   - G == 0, T == 0 or S == 0: nothing is enqueued, 0 is returned.
 *   - The route rule is qs_mx_softmax_quant_v's: QS_MX_SOFTMAX_ROUTE_VEC (16-byte loads of s and mask, 4-byte stores of row codes) with
 *     S % 32 == 0, s and mask 16-byte aligned and row_codes 8-byte aligned; the col pair then leaves in 16-byte stores where
 *     T % 16 == 0 and col_codes is 16-byte aligned, else in byte stores.  Anything else takes QS_MX_SOFTMAX_ROUTE_PLAIN, element
 *     accesses each predicated on its own index: any T, S >= 1, any element-aligned base, same bits. */
typedef struct qs_mx_softmax_quant2_args {
    uint32_t struct_size;            /* sizeof(qs_mx_softmax_quant2_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ; col_format -1: the col pair is skipped */
    int32_t sdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int32_t causal;                  /* 0 or 1 */
    float scale;
    const void* s;                   /* [G, T, S] row-major */
    const float* mask;               /* [T, S] or [G, T, S], additive, nullable (none) */
    int64_t mask_slices;             /* 1: mask is [T, S], shared by the slices; G: it is [G, T, S].  Read only with a mask */
    uint8_t* row_codes;              /* [G, T, S] */
    uint8_t* row_scales;             /* [G, T, ceil(S / 32)] */
    uint8_t* col_codes;              /* [G, S, T] */
    uint8_t* col_scales;             /* [G, S, ceil(T / 32)] */
    float* m;                        /* [G T]: written */
    float* Z;                        /* [G T]: written */
    int64_t G, T, S;
    qs_stream_t stream;
} qs_mx_softmax_quant2_args;
int qs_mx_softmax_quant2_v(const qs_mx_softmax_quant2_args* args);
/* the kernels qs_mx_softmax_quant2_v launches for these operands, nothing enqueued: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor, or
 * the QS_ERR_* the call would return */
int qs_mx_softmax_quant2_route(const qs_mx_softmax_quant2_args* args);

/* ---- MX softmax backward quantizer (the softmax backward in front of the two-way quantizer) ----------------------------------------------
 * Added without raising QS_ABI_VERSION (28): symbols are only added.
 *
 * From dp [G, T, S] (the gradient with respect to p; float32, bf16 or fp16, CONTIGUOUS), the forward's s, mask, scale and causal, and
 * the m and Z qs_mx_softmax_quant2_v wrote: the two MX pairs of ds, the gradient with respect to s.  Definition (normative), for the
 * row (g, t); all arithmetic is float32 on the widened inputs, every operation rounded on its own (no contraction, no FMA):
 *   u_j  as in the MX softmax quantizer;   p_j = E(u_j - m) / Z      the forward's p, to the bit (+0 for L <= j < S)
 *   D    = sum_j (p_j * dp_j)              in the row-sum order of the MX normalising quantizer with C = S: a function of S alone.
 *                                          dp_j is read for every j < S, behind L too
 *   ds_j = (p_j * (dp_j - D)) * scale
 *   a row whose m is NaN is NaN in every element of p, hence of ds.  A NaN or an Inf in dp makes D, hence its row of ds, NaN.
 * Outputs: row_codes [G, T, S] / row_scales and col_codes [G, S, T] / col_scales are bit for bit what qs_mx_quant2_batched_v writes
 * for the float32 ds [G, T, S] with the same formats, rounding, seed, step and index_base -- the same Philox words: stream 0 at index
 * index_base + (g T + t) S + j for the row pair, stream 1 at index_base + (g S + j) T + t for the col pair, `step` read on the device.
 * A pair whose format is -1 is skipped.  Two launches on `stream`, nothing read by the host, no atomics: a row launch (one wave per row)
 * that forms p again from s, m and Z and writes D [G T] -- the caller's float32 workspace --, then the tile of the two-way quantizer
 * per slice with the ds expression as its widen step.  Neither p nor ds is ever written.
 *   - Checks, in order: QS_ERR_ARG: a null or too short descriptor, rounding no QS_MX_ROUND_*, step not 8-byte aligned, index_base no
 *     multiple of 4, dp, s, m, Z or D NULL, both formats -1, a format neither -1 nor an enum qs_mx_format, a NULL pointer of a given
 *     pair, causal neither 0 nor 1, G, T or S negative, mask given with mask_slices neither 1 nor G; QS_ERR_DTYPE: sdt or ddt none of
 *     the three; QS_ERR_ALIGN: s or dp not aligned to its element, or mask, m, Z or D not to 4 bytes; QS_ERR_ARG: G * T * S beyond 64
 *     bits, more rows or more tiles than a launch takes.
 *   - G == 0, T == 0 or S == 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_SOFTMAX_ROUTE_VEC: S % 32 == 0, s, dp and mask 16-byte aligned and, with a col pair, T % 16 == 0 and col_codes 16-byte
 *     aligned (row codes leave in 4-byte stores where row_codes is 4-byte aligned).  Anything else takes QS_MX_SOFTMAX_ROUTE_PLAIN:
 *     any T, S >= 1, any element-aligned base, same bits. */
typedef struct qs_mx_softmax_bwd_quant_args {
    uint32_t struct_size;            /* sizeof(qs_mx_softmax_bwd_quant_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ; -1: that pair is skipped */
    int32_t sdt;                     /* dtype of s: QS_F32, QS_BF16 or QS_F16 */
    int32_t ddt;                     /* dtype of dp, likewise */
    int32_t causal;                  /* 0 or 1 */
    float scale;
    int32_t rounding;                /* QS_MX_ROUND_* */
    const void* dp;                  /* [G, T, S] row-major */
    const void* s;                   /* [G, T, S] row-major */
    const float* mask;               /* [T, S] or [G, T, S], additive, nullable (none) */
    int64_t mask_slices;             /* 1 or G, as above */
    const float* m;                  /* [G T] */
    const float* Z;                  /* [G T] */
    float* D;                        /* [G T]: workspace, written */
    uint8_t* row_codes;              /* [G, T, S] */
    uint8_t* row_scales;             /* [G, T, ceil(S / 32)] */
    uint8_t* col_codes;              /* [G, S, T] */
    uint8_t* col_scales;             /* [G, S, ceil(T / 32)] */
    int64_t G, T, S;
    qs_stream_t stream;
    uint64_t seed;
    const int64_t* step;             /* device pointer, nullable (0) */
    uint64_t index_base;             /* a multiple of 4 */
} qs_mx_softmax_bwd_quant_args;
int qs_mx_softmax_bwd_quant_v(const qs_mx_softmax_bwd_quant_args* args);
/* the kernels qs_mx_softmax_bwd_quant_v launches for these operands, nothing enqueued: QS_MX_SOFTMAX_ROUTE_*, 0 for an empty tensor,
 * or the QS_ERR_* the call would return */
int qs_mx_softmax_bwd_quant_route(const qs_mx_softmax_bwd_quant_args* args);

/* ---- MX rotary embedding (rotary position embedding as a dense call and in front of the batched two-way quantizer) ------------------
 * Added without raising QS_ABI_VERSION (28), by the same rule as qs_mx_matmul_v above: symbols are only added.
 *
 * Operands.  x holds G = G0 G1 slices [R, C] addressed exactly as the MX batched two-way quantizer addresses them (unit stride along
 * C, the three element strides x_stride_g0 / x_stride_g1 / x_stride_r), float32 / bf16 / f16; R is the sequence length T, C the head
 * dimension d, even, h = C / 2.  cos and sin are float32, contiguous, [R, h], shared by every slice.
 * Definition (normative).  Pair j (0 <= j < h) of row t of a slice is
 *   interleaved == 0   (a, b) = (x[t, j], x[t, j + h])    and lands in y[t, j], y[t, j + h]        (rotate-half: Llama / NeoX)
 *   interleaved != 0   (a, b) = (x[t, 2 j], x[t, 2 j + 1]) and lands in y[t, 2 j], y[t, 2 j + 1]  (GPT-J)
 * and, with c = cos[t, j], s = sin[t, j] (inverse != 0: s = -sin[t, j], an exact negation), every operation a float32 operation
 * rounded to nearest on its own, nothing contracted into an FMA:
 *   y_a = (a * c) - (b * s)
 *   y_b = (b * c) + (a * s)
 * x is widened to float32 exactly.  NaN, Inf and signed zeros are whatever these four products, one difference and one sum give;
 * nothing is special-cased.  The inverse call is bit for bit the forward call on -sin, and it is the gradient of the forward with
 * respect to x: there is no other backward formula.
 *
 * qs_mx_rope_v writes y dense, [G, R, C] in ydt, each element rounded once from float32 (round to nearest even), from ONE launch.
 * qs_mx_rope_quant2_v writes, from ONE launch, the four outputs of qs_mx_quant2_batched_v (round to nearest; same shapes, same
 * nullable-pair rule, at least one pair) for the float32 y above: bit for bit qs_mx_quant2_batched_v on that y as a dense float32
 * [G, R, C] tensor.  y is never rounded to x's dtype and never written.
 * Nothing outside the G R C addressed elements of x and the R h elements of each table is read; nothing but the outputs is written;
 * no atomics, no workspace.
 *   - checks in qs_mx_quant2_batched_v's order and with its status codes.  QS_ERR_ARG in addition: cos or sin missing, C odd, y
 *     missing (qs_mx_rope_v).  QS_ERR_DTYPE: xdt, ydt.  QS_ERR_ALIGN: x (y) not aligned to its element, cos or sin not to 4 bytes.
 *   - G0, G1, R or C equal to 0: nothing is enqueued, 0 is returned.
 *   - QS_MX_ROPE_ROUTE_VEC (16-byte loads of x): qs_mx_quant2_batched_v's conditions for QS_MX_Q2_ROUTE_TILE_VEC (for qs_mx_rope_v
 *     those on x, C and the strides, and y 16-byte aligned), cos and sin 16-byte aligned and, with interleaved == 0, h a multiple
 *     of the lane's vector (8 two-byte elements, 4 float32).  Anything else takes QS_MX_ROPE_ROUTE_PLAIN: element accesses predicated
 *     one by one, any even C, any R >= 1, any element-aligned base, the same bits. */
#define QS_MX_ROPE_ROUTE_VEC 1
#define QS_MX_ROPE_ROUTE_PLAIN 2
typedef struct qs_mx_rope_args {
    uint32_t struct_size;            /* sizeof(qs_mx_rope_args) as the caller compiled it */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int32_t ydt;                     /* likewise */
    int32_t interleaved;             /* 0: pairs (j, j + h); else pairs (2 j, 2 j + 1) */
    int32_t inverse;                 /* 0 or 1: -sin in place of sin */
    int32_t reserved0;
    const void* x;                   /* slice (g0, g1), row r, column c at x[g0 x_stride_g0 + g1 x_stride_g1 + r x_stride_r + c] */
    void* y;                         /* [G, R, C], dense */
    const float* cos;                /* [R, C / 2] */
    const float* sin;                /* [R, C / 2] */
    int64_t G0, G1, R, C;            /* G = G0 G1 slices */
    int64_t x_stride_g0, x_stride_g1, x_stride_r;   /* in elements */
    qs_stream_t stream;
} qs_mx_rope_args;
int qs_mx_rope_v(const qs_mx_rope_args* args);
/* the kernel qs_mx_rope_v launches for these operands, nothing enqueued: QS_MX_ROPE_ROUTE_*, 0 for an empty tensor, or the QS_ERR_*
 * the call would return */
int qs_mx_rope_route(const qs_mx_rope_args* args);

typedef struct qs_mx_rope_quant2_args {
    uint32_t struct_size;            /* sizeof(qs_mx_rope_quant2_args) as the caller compiled it */
    int32_t row_format, col_format;  /* enum qs_mx_format, may differ */
    int32_t xdt;                     /* QS_F32, QS_BF16 or QS_F16 */
    int32_t interleaved;             /* as qs_mx_rope_args */
    int32_t inverse;
    const void* x;                   /* as qs_mx_rope_args */
    const float* cos;                /* [R, C / 2] */
    const float* sin;                /* [R, C / 2] */
    uint8_t* row_codes;              /* nullable with row_scales; [G, R, C] */
    uint8_t* row_scales;             /* [G, R, ceil(C / 32)] */
    uint8_t* col_codes;              /* nullable with col_scales; [G, C, R] */
    uint8_t* col_scales;             /* [G, C, ceil(R / 32)] */
    int64_t G0, G1, R, C;            /* G = G0 G1 slices */
    int64_t x_stride_g0, x_stride_g1, x_stride_r;   /* in elements */
    qs_stream_t stream;
} qs_mx_rope_quant2_args;
int qs_mx_rope_quant2_v(const qs_mx_rope_quant2_args* args);
/* the kernel qs_mx_rope_quant2_v launches for these operands, nothing enqueued: QS_MX_ROPE_ROUTE_*, 0 for an empty tensor, or the
 * QS_ERR_* the call would return */
int qs_mx_rope_quant2_route(const qs_mx_rope_quant2_args* args);

/* ---- Aliases kept for v27 callers -------------------------------------------------------------------------------------------
 * v27 had the rounding operands in descriptors and entry points of their own.  Those descriptors were the v28 ones byte for byte, so
 * the type names are typedefs and each function forwards to the entry point above it names: same checks, routes, kernels, bytes. */
typedef qs_mx_quant_args qs_mx_quant_sr_args;
typedef qs_mx_quant2_args qs_mx_quant2_sr_args;
int qs_mx_quant_sr_v(const qs_mx_quant_sr_args* args);          /* qs_mx_quant_fwd_v */
int qs_mx_quant_sr_route(const qs_mx_quant_sr_args* args);      /* qs_mx_quant_route */
int qs_mx_quant2_sr_v(const qs_mx_quant2_sr_args* args);        /* qs_mx_quant2_v */
int qs_mx_quant2_sr_route(const qs_mx_quant2_sr_args* args);    /* qs_mx_quant2_route */

#ifdef __cplusplus
}
#endif
#endif /* QSPARSE_HIP_H */
