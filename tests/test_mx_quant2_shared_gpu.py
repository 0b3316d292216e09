"""What only the parameters of the shared column phase tell apart (qs_mx_quant2.h: mxq2_col_phase / mx_encode_run, called by
mx_quant2_kernel, mx_quant2_batched_kernel, mx_glu_bwd_quant2_kernel and mx_norm_apply_kernel) -- bit for bit against the package's
CPU path, at the smallest shapes that reach each combination:

    norm kernel, [130, 64]        its VEC route with col_vec = 0 -- R % 16 != 0, and again with col_codes one byte off its alignment:
                                  the only caller whose 16-byte store of the col pair hangs on a RUN-TIME flag
    all four kernels, R = 144     VEC route, R % 16 == 0 and R % 32 != 0: the second 16-byte half of the last column block (rows 144 ..
                                  159) is predicated off, its scale bytes come from 16 rows and 16 zeros.  The col pair alone, then both
                                  pairs; nearest, and stochastic on the three kernels that have it.  (The norm kernel has no call
                                  without a row pair.  The GLU kernel runs with act = relu: the CPU path's expf is not the GPU's, relu
                                  is exact on both.)
    batched kernel, 3 x [48, 64]  stochastic, VEC, a non-zero index_base: slice g draws at base + g R C, so the quad index of phase 2
                                  starts at (base + g R C + oc R + orow) / 4.  The descriptor refuses an index_base that is no multiple
                                  of 4 (QS_ERR_ARG, tests/test_mx_quant2_batched_gpu.py), so the base is 12: an odd quad.

test_mx_quant2_gpu.py, test_mx_quant2_batched_gpu.py, test_mx_glu_train_gpu.py and test_mx_norm_gpu.py reach R = 144 too, with other
formats, against other references or with both pairs only; the cases here are the ones named above in one place, per format width
(FP8, FP6, FP4 on each side) and for float32 and bfloat16.

And what only the parameters of the shared PHASE 1 tell apart (mxq2_load4, mxq2_stage, mxq2_emit_row, mxq2_at / mxq2_to_slice, called
by mxq2_tile, the GLU and the RoPE kernel, the load also by the norm kernel; the two softmax kernels and the norm kernel's emit state
the same steps themselves, DESIGN.md 3z, and are pinned here alike), for the six kernels on the tile at shapes the other files do not have:

    all six, PLAIN, [130, 36], [33, 68]  every input one element off its 16 bytes, so that every kernel takes element accesses: a lane
                                  group cut by the edge (36 = 32 + 4: half a two-byte lane's 8; 68 = 64 + 4: a second tile of one
                                  lane) and rows cut inside a pass (130 = 128 + 2, 33).  Row pair alone, col pair alone, both -- the
                                  norm and the forward softmax kernel have no call without a row pair -- nearest and, where the kernel
                                  has it, stochastic; the sliced kernels with G = 3.  The GLU kernel at T = 33 and T = 130, H = 32.
    softmax backward, 3 x [48, 64]  stochastic, VEC, index_base = 12: the row pair's quad index behind a slice offset, as the batched
                                  kernel's above
    causal softmax, T = S = 40    the limit t + 1 cuts inside a lane's four columns in three rows of four, on both softmax kernels"""
import pytest
import torch

import mx_norm_ref as NR
import mx_rope_ref as RR
import mx_softmax_ref as SMR
import qsparse_amd as qs
from qsparse_amd import (_hip, mx_glu_backward_quantize, mx_norm_quantize, mx_quantize_2way, mx_quantize_2way_batched, mx_rope_quantize,
                         mx_softmax_backward_quantize, mx_softmax_quantize)
from qsparse_amd.mx_batched_train import _slice_strides
from qsparse_amd.mx_softmax import _softmax_ds
from qsparse_amd.quantize import _mx_aten, _mx_sr_words

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = [("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp4_e2m1", "mxfp4_e2m1")]      # one per element width
DTYPES = (torch.float32, torch.bfloat16)
NAMES = ("row codes", "row scales", "col codes", "col scales")
SEED, STEP = 2 ** 40 + 9, 3


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def randn(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[:-1] + (1,), generator=g) * 2)).to(dtype)


def agree(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert (g is None) == (w is None), (name, what)
        assert g is None or (g.shape == w.shape and torch.equal(g.cpu(), w)), (name, what)


def last_block_scales(got, want, R, what):
    """every scale byte of the last column block, by itself"""
    assert got[3].shape[-1] == (R + 31) // 32 and torch.equal(got[3][..., -1].cpu(), want[3][..., -1]), what


def rounding(sr, device):
    return dict(rounding="stochastic", seed=SEED, step=torch.tensor([STEP], device=device)) if sr else {}


# ---- the norm kernel: VEC with byte stores of the col pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1], ids=["short R", "short R, col_codes one byte off"])
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_norm_vec_route_without_the_wide_col_store(dtype, row_fmt, col_fmt, offset, monkeypatch):
    R, C = 130, 64
    if offset:
        outs = _hip._mx_quant2_outs

        def carved(*args, **kw):
            o = outs(*args, **kw)
            buf = torch.empty(o[2].numel() + 16, dtype=torch.uint8, device=o[2].device)
            assert buf.data_ptr() % 16 == 0
            return o[:2] + (buf[offset:offset + o[2].numel()].view(o[2].shape),) + o[3:]

        monkeypatch.setattr(_hip, "_mx_quant2_outs", carved)
    for norm in NR.NORMS:
        x, w, b = NR.inputs(17, R, C, dtype)
        want = mx_norm_quantize(x, w, b, norm=norm, eps=NR.EPS, fmt=row_fmt, col_fmt=col_fmt)
        got = mx_norm_quantize(x.to(DEV), w.to(DEV), b.to(DEV), norm=norm, eps=NR.EPS, fmt=row_fmt, col_fmt=col_fmt)
        assert _hip.mx_norm_last_route == _hip.MX_NORM_ROUTE_VEC
        assert got[2].data_ptr() % 16 == offset
        agree(got, want, (norm, offset))
        last_block_scales(got, want, R, (norm, offset))


# ---- R = 144 on the VEC route: the short second half of the last column block ----------------------------------------------------------
def run_quant2(x, rf, cf, sr, device):
    got = mx_quantize_2way(x.to(device), rf, cf, **rounding(sr, device))
    return got, _hip.mx_quant2_last_route


def run_batched(x, rf, cf, sr, device):
    got = mx_quantize_2way_batched(x.to(device), rf, cf, **rounding(sr, device))
    return got, _hip.mx_quant2_batched_last_route


def run_glu(x, rf, cf, sr, device):
    dh, v = x                                         # (dh [T, 32], v [T, 64]: dv is [T, 64], one tile column)
    got = mx_glu_backward_quantize(dh.to(device), v.to(device), act="relu", row_fmt=rf, col_fmt=cf, **rounding(sr, device))
    return got, _hip.mx_glu_bwd_last_route


def run_norm(x, rf, cf, sr, device):
    x, w, b = x
    got = mx_norm_quantize(x.to(device), w.to(device), b.to(device), norm="layer", eps=NR.EPS, fmt=rf, col_fmt=cf)
    return got, _hip.mx_norm_last_route


def inputs_144(kernel, dtype):
    R = 144
    if kernel == "batched":
        return randn((2, R, 64), dtype, 5)
    if kernel == "glu":
        return randn((R, 32), dtype, 6), randn((R, 64), dtype, 7)
    if kernel == "norm":
        return NR.inputs(8, R, 64, dtype)
    return randn((R, 64), dtype, 4)


RUN = {"quant2": run_quant2, "batched": run_batched, "glu": run_glu, "norm": run_norm}
CASES_144 = [(k, sr) for k in RUN for sr in (False, True) if not (k == "norm" and sr)]         # (the norm kernel rounds to nearest only)


@pytest.mark.parametrize("kernel,sr", CASES_144, ids=[f"{k}-{'stochastic' if sr else 'nearest'}" for k, sr in CASES_144])
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_half_a_column_block_on_the_vec_route(dtype, row_fmt, col_fmt, kernel, sr):
    x = inputs_144(kernel, dtype)
    vec = _hip.MX_NORM_ROUTE_VEC if kernel == "norm" else _hip.MX_Q2_ROUTE_TILE_VEC
    for rf in ((row_fmt,) if kernel == "norm" else (None, row_fmt)):       # the col pair alone, then both pairs
        want, _ = RUN[kernel](x, rf, col_fmt, sr, "cpu")
        got, route = RUN[kernel](x, rf, col_fmt, sr, DEV)
        assert route == vec, (kernel, rf)
        agree(got, want, (kernel, rf, col_fmt, sr))
        last_block_scales(got, want, 144, (kernel, rf, col_fmt, sr))


# ---- the batched kernel's quad index behind a slice offset and an index base -------------------------------------------------------------
def cpu_pair(x, fmt, stream, base):
    """codes and scales of the package's one-way CPU path with an index base (which the public call does not take)"""
    return _mx_aten(x, fmt, x.dim() - 1, torch.float32, True, _mx_sr_words(x.shape, SEED, STEP, stream, base))[1:]


@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_batched_stochastic_slices_at_an_index_base(dtype, row_fmt, col_fmt):
    G, R, C, base = 3, 48, 64, 12
    x = randn((G, R, C), dtype, 9)
    xd = x.to(DEV)
    G0, G1, strides = _slice_strides(xd)
    got = _hip.mx_quant2_batched(xd, G0, G1, R, C, strides, row_fmt, col_fmt, "stochastic", SEED, torch.tensor([STEP], device=DEV), base)
    assert _hip.mx_quant2_batched_last_route == _hip.MX_Q2_ROUTE_TILE_VEC
    want = cpu_pair(x, row_fmt, 0, base) + cpu_pair(x.transpose(1, 2).contiguous(), col_fmt, 1, base)
    for g in range(G):                                # slice by slice: a wrong g R C shows in the slices behind the first
        agree([t[g] for t in got], [t[g] for t in want], (g, row_fmt, col_fmt))


# ---- phase 1: every kernel on the PLAIN route, the edge inside a lane group and inside a pass --------------------------------------------
SCALE = 0.37
KINDS = ("row", "col", "both")
PLAIN_SHAPES = ((130, 36), (33, 68))


def off(t):
    """`t` on the device, contiguous, at a base one element off its 16 bytes: no kernel takes a vector load from it"""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    out = flat[1:].view(t.shape).copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (i, what)
        if g is not None:
            assert g.shape == w.shape and torch.equal(g.cpu().contiguous().view(torch.uint8), w.contiguous().view(torch.uint8)), (i, what)


def pair_formats(kind, row_fmt, col_fmt):
    return (None if kind == "col" else row_fmt, None if kind == "row" else col_fmt)


def p1_quant2(x, rf, cf, sr, put, device):
    return mx_quantize_2way(put(x), rf, cf, **rounding(sr, device)), _hip.mx_quant2_last_route


def p1_batched(x, rf, cf, sr, put, device):
    return mx_quantize_2way_batched(put(x), rf, cf, **rounding(sr, device)), _hip.mx_quant2_batched_last_route


def p1_norm(x, rf, cf, sr, put, device):
    x, w, b = x
    return mx_norm_quantize(put(x), w.to(device), b.to(device), norm="layer", eps=NR.EPS, fmt=rf, col_fmt=cf), _hip.mx_norm_last_route


def p1_softmax(x, rf, cf, sr, put, device):
    return mx_softmax_quantize(put(x), scale=SCALE, fmt=rf, col_fmt=cf, return_stats=True), _hip.mx_softmax_quant2_last_route


def p1_softmax_bwd(x, rf, cf, sr, put, device):
    s, dp, m, Z = x
    got = mx_softmax_backward_quantize(put(dp), put(s), m.to(device), Z.to(device), scale=SCALE, row_fmt=rf, col_fmt=cf,
                                       **rounding(sr, device))
    return got, _hip.mx_softmax_bwd_last_route


def p1_rope(x, rf, cf, sr, put, device):
    x, cos, sin = x
    got = ()
    for interleaved, inverse in ((False, False), (True, True)):
        got += mx_rope_quantize(put(x), cos.to(device), sin.to(device), row_fmt=rf, col_fmt=cf, interleaved=interleaved, inverse=inverse)
    return got, _hip.mx_rope_quant2_last_route


def p1_inputs(kernel, R, C, dtype):
    if kernel == "quant2":
        return randn((R, C), dtype, 31)
    if kernel == "batched":
        return randn((3, R, C), dtype, 32)
    if kernel == "norm":
        return NR.inputs(33, R, C, dtype)
    if kernel == "rope":
        return (RR.inputs(34, (3, R, C), dtype),) + tuple(RR.tables(R, C, 35))
    s = SMR.scores(36, (3, R, C), dtype)
    if kernel == "softmax":
        return s
    m, Z = mx_softmax_quantize(s, scale=SCALE, fmt="mxfp8_e4m3", return_stats=True)[-2:]
    return s, randn((3, R, C), dtype, 37), m, Z


# kernel: (run, PLAIN of its route family, has a call without a row pair, rounds stochastically)
P1 = {"quant2": (p1_quant2, _hip.MX_Q2_ROUTE_TILE_PLAIN, True, True), "batched": (p1_batched, _hip.MX_Q2_ROUTE_TILE_PLAIN, True, True),
      "norm": (p1_norm, _hip.MX_NORM_ROUTE_PLAIN, False, False), "softmax": (p1_softmax, _hip.MX_SOFTMAX_ROUTE_PLAIN, False, False),
      "softmax_bwd": (p1_softmax_bwd, _hip.MX_SOFTMAX_ROUTE_PLAIN, True, True), "rope": (p1_rope, _hip.MX_ROPE_ROUTE_PLAIN, True, False)}


@pytest.mark.parametrize("R,C", PLAIN_SHAPES, ids=[f"{r}x{c}" for r, c in PLAIN_SHAPES])
@pytest.mark.parametrize("kernel", list(P1))
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_phase_one_on_the_plain_route(dtype, row_fmt, col_fmt, kernel, R, C):
    run, plain, col_alone, stochastic = P1[kernel]
    x = p1_inputs(kernel, R, C, dtype)
    for kind in KINDS if col_alone else ("row", "both"):
        rf, cf = pair_formats(kind, row_fmt, col_fmt)
        for sr in (False, True) if stochastic else (False,):
            want, _ = run(x, rf, cf, sr, lambda t: t, "cpu")
            got, route = run(x, rf, cf, sr, off, DEV)
            assert route == plain, (kernel, kind, sr)
            same_bytes(got, want, (kernel, kind, sr))


@pytest.mark.parametrize("T", (33, 130))
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_glu_phase_one_on_the_plain_route(dtype, row_fmt, col_fmt, T):
    dh, v = randn((T, 32), dtype, 41), randn((T, 64), dtype, 42)     # (H = 32: dv is [T, 64], one tile column; relu, as above)
    for kind in KINDS:
        rf, cf = pair_formats(kind, row_fmt, col_fmt)
        for sr in (False, True):
            want = mx_glu_backward_quantize(dh, v, act="relu", row_fmt=rf, col_fmt=cf, **rounding(sr, "cpu"))
            got = mx_glu_backward_quantize(off(dh), off(v), act="relu", row_fmt=rf, col_fmt=cf, **rounding(sr, DEV))
            assert _hip.mx_glu_bwd_last_route == _hip.MX_Q2_ROUTE_TILE_PLAIN, (kind, sr)
            same_bytes(got, want, (kind, sr))


# ---- the softmax backward's quad index behind a slice offset and an index base -----------------------------------------------------------
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_softmax_backward_stochastic_slices_at_an_index_base(dtype, row_fmt, col_fmt):
    G, T, S, base = 3, 48, 64, 12
    s, dp = SMR.scores(51, (G, T, S), dtype), randn((G, T, S), dtype, 52)
    m, Z = mx_softmax_quantize(s, scale=SCALE, fmt=row_fmt, return_stats=True)[-2:]
    ds = _softmax_ds(dp, s, m, Z, None, SCALE, False)
    step = torch.tensor([STEP], device=DEV)
    for kind in KINDS:
        rf, cf = pair_formats(kind, row_fmt, col_fmt)
        got = _hip.mx_softmax_bwd_quant(dp.to(DEV), s.to(DEV), m.to(DEV), Z.to(DEV), None, SCALE, False, rf, cf, "stochastic", SEED, step,
                                        base)
        assert _hip.mx_softmax_bwd_last_route == _hip.MX_SOFTMAX_ROUTE_VEC, kind
        want = (tuple(cpu_pair(ds, rf, 0, base)) if rf else (None, None)) + \
               (tuple(cpu_pair(ds.transpose(1, 2).contiguous(), cf, 1, base)) if cf else (None, None))
        for g in range(G):                                # slice by slice: a wrong g T S shows in the slices behind the first
            same_bytes([t if t is None else t[g] for t in got], [t if t is None else t[g] for t in want], (g, kind))


# ---- a causal limit inside a lane's four columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_causal_limit_inside_a_lanes_four(dtype, row_fmt, col_fmt):
    G, T, S = 2, 40, 40
    s, dp = SMR.scores(61, (G, T, S), dtype), randn((G, T, S), dtype, 62)
    for cf in (None, col_fmt):
        want = mx_softmax_quantize(s, scale=SCALE, is_causal=True, fmt=row_fmt, col_fmt=cf, return_stats=True)
        got = mx_softmax_quantize(s.to(DEV), scale=SCALE, is_causal=True, fmt=row_fmt, col_fmt=cf, return_stats=True)
        same_bytes(got, want, ("forward", cf))
    m, Z = want[-2:]
    for kind in KINDS:
        rf, cf = pair_formats(kind, row_fmt, col_fmt)
        for sr in (False, True):
            wantb = mx_softmax_backward_quantize(dp, s, m, Z, scale=SCALE, is_causal=True, row_fmt=rf, col_fmt=cf, **rounding(sr, "cpu"))
            gotb = mx_softmax_backward_quantize(dp.to(DEV), s.to(DEV), m.to(DEV), Z.to(DEV), scale=SCALE, is_causal=True, row_fmt=rf,
                                                col_fmt=cf, **rounding(sr, DEV))
            same_bytes(gotb, wantb, ("backward", kind, sr))
