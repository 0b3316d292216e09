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
(FP8, FP6, FP4 on each side) and for float32 and bfloat16."""
import pytest
import torch

import mx_norm_ref as NR
import qsparse_amd as qs
from qsparse_amd import _hip, mx_glu_backward_quantize, mx_norm_quantize, mx_quantize_2way, mx_quantize_2way_batched
from qsparse_amd.mx_batched_train import _slice_strides
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
