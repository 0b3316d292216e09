"""``mx_flash_attention`` on the GPU: the bytes of qs_mx_flash_attention_v against the composition it is defined as, run on the same
device -- shapes on either side of every tile and chunk bound, the format triples, masks, exceptional rows, the PLAIN route, guard
bytes, ``mx_attention(impl="flash")``, graph capture -- and one check of both against float64 attention."""
import pytest
import torch

import test_mx_flash as TF
from qsparse_amd import _hip, mx_attention, mx_flash_attention, mx_rope_table
from qsparse_amd.quantize import mx_dequantize

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E4, E5, F62, F63, FP4 = _hip.MX_FORMATS[0], _hip.MX_FORMATS[1], _hip.MX_FORMATS[2], _hip.MX_FORMATS[3], _hip.MX_FORMATS[4]
SHAPES = ((1, 1), (5, 31), (17, 33), (64, 128), (65, 129), (197, 197), (16, 256), (33, 257), (9, 512))      # (T, S)
DIMS = ((32, 16), (64, 64), (80, 72), (128, 128))                                                        # (d, dv)
TRIPLES = ((E4, E4, E4), (FP4, FP4, FP4), (E5, F62, FP4), (F63, E4, F62), (FP4, FP4, E4))                  # (qk, p, v)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
G = 3


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def both(ops, trip, mask=None, **kw):
    """(the one launch, the composition on the device) for the format triple `trip`"""
    kw = dict(scale=0.21, p_fmt=trip[1], **kw)
    return TF.flash(ops, trip[0], trip[2], mask, **kw), TF.composition(ops, trip[0], trip[2], mask, **kw)


def masks(seed, T, S):
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(G, T, S, generator=g) > 0.4
    keep[..., 0] = True
    return torch.randn(T, S, generator=g).to(DEV), keep.to(DEV)


def check_all_masks(ops, trip, T, S, dtype):
    fmask, bmask = masks(T + S, T, S)
    for kw in ({}, {"mask": fmask}, {"mask": bmask}, {"is_causal": True}):
        got, want = both(ops, trip, out_dtype=dtype, **kw)
        assert same_bytes(got, want), (T, S, trip, dtype, sorted(kw))
    assert bool(want.float().isfinite().all()) and bool((want != 0).any())


@pytest.mark.parametrize("n,TS", enumerate(SHAPES), ids=lambda v: str(v))
def test_one_launch_equals_the_composition(n, TS):
    """every (T, S) -- causal with T < S, T = S and T > S among them -- with the other axes taken in turn"""
    (T, S), (d, dv), trip = TS, DIMS[n % 4], TRIPLES[n % 5]
    check_all_masks(TF.operands(n, (G,), T, S, d, dv, trip[0], trip[2], DEV), trip, T, S, DTYPES[n % 3])


@pytest.mark.parametrize("trip", TRIPLES, ids=lambda t: "-".join(f[2:] for f in t))
@pytest.mark.parametrize("d,dv", DIMS)
def test_formats_and_head_sizes(d, dv, trip):
    """every head size under every triple at (65, 129) -- two work-groups per slice, a second chunk of one key -- and causal with
    T > S on the wide kernel"""
    check_all_masks(TF.operands(d, (G,), 65, 129, d, dv, trip[0], trip[2], DEV), trip, 65, 129, torch.float32)
    got, want = both(TF.operands(dv, (2,), 300, 260, d, dv, trip[0], trip[2], DEV), trip, is_causal=True, out_dtype=torch.bfloat16)
    assert same_bytes(got, want)


@pytest.mark.parametrize("what", ("q_scale_nan", "masked_row", "inf_mask", "nan_scale"))
def test_exceptional_rows_beside_ordinary_ones(what):
    T, S, row = 21, 70, 6
    qc, qs, kc, ks, vc, vs = TF.operands(7, (G,), T, S, 48, 40, E4, E4, DEV)
    mask = torch.zeros(G, T, S, device=DEV)
    clean, _ = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], mask)
    kw = {}
    if what == "q_scale_nan":
        qs = qs.clone()
        qs[1, row, 0] = 0xFF
    elif what == "masked_row":
        mask[1, row] = float("-inf")
    elif what == "inf_mask":
        mask[1, row, 3] = float("inf")
    else:
        kw["scale"] = float("nan")
    if kw:
        got, want = TF.flash((qc, qs, kc, ks, vc, vs), E4, E4, mask, **kw), TF.composition((qc, qs, kc, ks, vc, vs), E4, E4, mask, **kw)
        assert bool(got.isnan().all())
    else:
        got, want = both((qc, qs, kc, ks, vc, vs), TRIPLES[0], mask)
        assert bool(got[1, row].isnan().all())
        keep = torch.ones(G, T, dtype=torch.bool, device=DEV)
        keep[1, row] = False
        assert same_bytes(got[keep], clean[keep]), "an exceptional row changed its neighbours"
    assert same_bytes(got, want)


@pytest.mark.parametrize("which", ("q", "k", "vt", "mask"))
def test_a_misaligned_base_takes_the_plain_route(which):
    T, S = 20, 64
    ops = list(TF.operands(8, (G,), T, S, 64, 32, E4, E4, DEV))
    mask = masks(9, T, S)[0]
    want = TF.flash(ops, E4, E4, mask, scale=0.21)
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_VEC

    def shifted(t):          # the same values one element off a 16-byte base
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        out = flat[1:].view(t.shape).copy_(t)
        assert out.data_ptr() % 16 != 0 and out.is_contiguous()
        return out

    if which == "mask":
        mask = shifted(mask)
    else:
        ops[{"q": 0, "k": 2, "vt": 4}[which]] = shifted(ops[{"q": 0, "k": 2, "vt": 4}[which]])
    got = TF.flash(ops, E4, E4, mask, scale=0.21)
    assert _hip.mx_flash_last_route == _hip.MX_FLASH_ROUTE_PLAIN and same_bytes(got, want)


@pytest.mark.parametrize("Gs,T,S,dv", ((1, 1, 1, 1), (2, 5, 33, 16), (1, 65, 197, 64)))
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_nothing_outside_the_output_is_written(dtype, Gs, T, S, dv):
    ops = TF.operands(10, (Gs,), T, S, 32, dv, E4, FP4, DEV)
    want = TF.composition(ops, E4, FP4, scale=0.21, out_dtype=dtype)
    n, pad = Gs * T * dv, 256
    flat = torch.full((n + 2 * pad,), -123.0, dtype=dtype, device=DEV)
    got = _hip.mx_flash_attention(*ops[:2], E4, *ops[2:], FP4, None, 0.21, False, E4, dtype, out=flat[pad:pad + n])
    assert same_bytes(got, want)
    assert bool((flat[:pad] == -123.0).all()) and bool((flat[pad + n:] == -123.0).all())


@pytest.mark.parametrize("rope", (False, True))
def test_attention_flash_equals_composed(rope):
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(2, 3, 197, 64, generator=g).bfloat16().to(DEV) for _ in range(3))
    kw = dict(softmax="fused", out_dtype=torch.bfloat16, rope=mx_rope_table(197, 64, device=DEV) if rope else None)
    for extra in ({}, {"is_causal": True}):
        assert same_bytes(mx_attention(q, k, v, impl="flash", **kw, **extra), mx_attention(q, k, v, impl="composed", **kw, **extra))


def test_captured_call_replays_bit_for_bit():
    """one linear capture (no parallel branches), replayed twice on new codes"""
    first, second = TF.operands(12, (G,), 70, 197, 64, 64, E4, E4, DEV), TF.operands(13, (G,), 70, 197, 64, 64, E4, E4, DEV)
    want = TF.composition(second, E4, E4, scale=0.21, is_causal=True)
    static = tuple(t.clone() for t in first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        TF.flash(static, E4, E4, scale=0.21, is_causal=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = TF.flash(static, E4, E4, scale=0.21, is_causal=True)
    for t, s in zip(static, second):
        t.copy_(s)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert same_bytes(out, want)


def test_error_against_float64_attention_is_the_compositions():
    """float64 softmax and products on the de-quantized operands, p unquantized: the one launch is no further from it than the
    composition, in max and in rms -- no margin, the two are defined to be equal"""
    T, S, d, dv = 197, 197, 64, 64
    ops = TF.operands(14, (G,), T, S, d, dv, E4, E4, DEV)
    q, k, vt = (mx_dequantize(ops[i], ops[i + 1], E4, -1, torch.float64) for i in (0, 2, 4))
    ref = torch.softmax(q @ k.transpose(-1, -2) * 0.21, -1) @ vt.transpose(-1, -2)
    got, comp = both(ops, TRIPLES[0])
    err = lambda y: ((y.double() - ref).abs().max().item(), (y.double() - ref).pow(2).mean().sqrt().item())
    (gmax, grms), (cmax, crms) = err(got), err(comp)
    print(f"flash max {gmax:.3e} rms {grms:.3e}; composition max {cmax:.3e} rms {crms:.3e}")
    assert gmax <= cmax and grms <= crms
