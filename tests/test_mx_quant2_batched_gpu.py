"""The batched, strided two-way MX quantizer on the GPU (qs_mx_quant2_batched_v) -- bit for bit against the CPU path of
``mx_quantize_2way_batched`` (the definition: two ``quantize_with_mx`` calls on the whole tensor) and against ``mx_quantize_2way`` of
every slice on the GPU, with the route of every launch asserted by the header's rule.  The shapes are the smallest that reach each
hazard:

    [3, 40, 64], slices scaled by 1, 2^20, 2^-20   a block that leaks across a slice boundary changes a scale byte (R = 40: the last
                                                   block along R is short, the next slice lies right behind it); 2^6 and 2^-6 in
                                                   float16, whose range ends at 65504
    [2, 130, 72] and [2, 144, 72]                  cross the 128 x 64 tile in both directions; with the col pair R = 130 is PLAIN by
                                                   the 2-d rule (R % 16), R = 144 is VEC with both pairs
    [2, 37, 19]                                    PLAIN, short blocks both ways
    [2, 5, 3, 32].transpose(1, 2), [2, 16, 3, 32].transpose(1, 2), a chunk of [2, 33, 3 * 64]
                                                   strides: two levels, a row pitch beyond C, a base 64 elements into the allocation
    [1, 32, 32]                                    a single slice
    G, R or C equal to 0                           nothing is enqueued"""
import ctypes

import pytest
import torch

import mx_ref as R
from mx_guard import guarded, intact
from qsparse_amd import _hip, mx_quantize_2way, mx_quantize_2way_batched
from qsparse_amd.mx_batched_train import _slice_strides

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VEC, PLAIN = _hip.MX_Q2_ROUTE_TILE_VEC, _hip.MX_Q2_ROUTE_TILE_PLAIN
PAIRS = [("mxfp8_e4m3", "mxfp8_e5m2"), ("mxfp6_e2m3", "mxfp6_e3m2"), ("mxfp4_e2m1", "mxfp4_e2m1")]      # one per element width


def randn(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * torch.exp(torch.randn(shape[:-1] + (1,), generator=g) * 2)).to(dtype)


def cases(dtype):
    """(name, base tensor on the CPU, view): the tensor under test is view(base), on either device"""
    ident = lambda t: t
    k = 6 if dtype == torch.float16 else 20            # (2^20 times a normal deviate is past float16's range)
    scaled = torch.randn(3, 40, 64, generator=torch.Generator().manual_seed(1)) * torch.tensor([1.0, 2.0 ** k, 2.0 ** -k]).view(3, 1, 1)
    scaled = scaled.to(dtype)
    return [("slice scales", scaled, ident), ("tile edge, ragged R", randn((2, 130, 72), dtype, 2), ident),
            ("tile edge", randn((2, 144, 72), dtype, 3), ident), ("ragged", randn((2, 37, 19), dtype, 4), ident),
            ("heads, R = 5", randn((2, 5, 3, 32), dtype, 5), lambda t: t.transpose(1, 2)),
            ("heads, R = 16", randn((2, 16, 3, 32), dtype, 6), lambda t: t.transpose(1, 2)),
            ("chunk", randn((2, 33, 192), dtype, 7), lambda t: t.chunk(3, -1)[1]), ("single slice", randn((1, 32, 32), dtype, 8), ident)]


def expected_route(x, col):
    """the header's rule on the strides the binding passes"""
    G0, G1, strides = _slice_strides(x)
    v = 4 if x.dtype == torch.float32 else 8
    ok = x.shape[-1] % v == 0 and x.data_ptr() % 16 == 0 and all(s % v == 0 for s in strides) and (not col or x.shape[-2] % 16 == 0)
    return VEC if ok else PLAIN


def check(base, view, row_fmt, col_fmt, what, sr=None):
    x_cpu, x_dev = view(base), view(base.to(DEV))
    assert x_dev.stride() == x_cpu.stride()
    kw_dev, kw_cpu = {}, {}
    if sr is not None:
        kw_dev = dict(rounding="stochastic", seed=sr, step=torch.tensor([3], device=DEV))
        kw_cpu = dict(rounding="stochastic", seed=sr, step=torch.tensor([3]))
    got = mx_quantize_2way_batched(x_dev, row_fmt, col_fmt, **kw_dev)
    route = _hip.mx_quant2_batched_last_route
    assert route == expected_route(x_dev, col_fmt is not None), (what, route)
    want = mx_quantize_2way_batched(x_cpu, row_fmt, col_fmt, **kw_cpu)
    for name, g, w in zip(("row codes", "row scales", "col codes", "col scales"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.is_cuda and g.dtype == torch.uint8 and g.is_contiguous() and not g.requires_grad
            assert g.shape == w.shape and torch.equal(g.cpu(), w), (what, name, row_fmt, col_fmt, sr)
    if sr is None:                                    # slice by slice the 2-d kernel's bits
        lead = x_dev.shape[:-2]
        flat = [None if g is None else g.reshape((-1,) + g.shape[len(lead):]) for g in got]
        xs = x_dev.reshape((-1,) + x_dev.shape[-2:])
        for s in range(xs.shape[0]):
            for name, g, w in zip(("row codes", "row scales", "col codes", "col scales"), flat, mx_quantize_2way(xs[s], row_fmt, col_fmt)):
                assert g is None or torch.equal(g[s], w), (what, name, s)
    return route


@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_every_shape_against_the_cpu_path_and_the_slices(row_fmt, col_fmt, dtype):
    routes = {}
    for name, base, view in cases(dtype):
        routes[name] = (check(base, view, row_fmt, col_fmt, name), check(base, view, row_fmt, None, name + ", row only"),
                        check(base, view, None, col_fmt, name + ", col only"))
    # both routes are reached, the strided views take the vector route where the rule lets them
    assert routes["tile edge"] == (VEC, VEC, VEC) and routes["tile edge, ragged R"] == (PLAIN, VEC, PLAIN)
    assert routes["ragged"] == (PLAIN, PLAIN, PLAIN) and routes["single slice"] == (VEC, VEC, VEC)
    assert routes["heads, R = 16"] == (VEC, VEC, VEC) and routes["heads, R = 5"] == (PLAIN, VEC, PLAIN)
    assert routes["chunk"] == (PLAIN, VEC, PLAIN) and routes["slice scales"] == (PLAIN, VEC, PLAIN)


@pytest.mark.parametrize("row_fmt,col_fmt", PAIRS)
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_stochastic_rounding_is_the_one_way_quantizer_on_the_whole_tensor(row_fmt, col_fmt, dtype):
    for name, base, view in cases(dtype):
        check(base, view, row_fmt, col_fmt, name, sr=11)
    name, base, view = cases(dtype)[3]
    check(base, view, row_fmt, None, name, sr=12)
    check(base, view, None, col_fmt, name, sr=13)


def test_a_slice_boundary_is_a_block_boundary():
    """slice 1 is 2^20 times slice 0: the short last block of slice 0 along R (rows 32 .. 39) would take its scale from slice 1 if it
    read on; the scale bytes of the col pair must differ by exactly 20 between the slices instead"""
    base = randn((1, 40, 64), torch.float32, 1).abs() + 0.5
    x = torch.cat([base, base * 2.0 ** 20, base * 2.0 ** -20]).to(DEV)
    _, rs, _, cs = mx_quantize_2way_batched(x, "mxfp8_e4m3", "mxfp8_e4m3")
    for s in (rs, cs):
        s = s.cpu().to(torch.int64)
        assert torch.equal(s[1] - s[0], torch.full_like(s[0], 20)) and torch.equal(s[0] - s[2], torch.full_like(s[0], 20))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_a_nonfinite_element_marks_its_block_of_its_slice_only(bad, dtype):
    for shape, (g, i, j) in (((3, 48, 64), (1, 47, 33)), ((2, 37, 19), (0, 36, 18))):
        x = randn(shape, dtype, 9)
        x[g, i, j] = bad
        rc, rs, cc, cs = mx_quantize_2way_batched(x.to(DEV), "mxfp8_e4m3", "mxfp4_e2m1")
        row_ff, col_ff = torch.zeros(rs.shape, dtype=torch.bool), torch.zeros(cs.shape, dtype=torch.bool)
        row_ff[g, i, j // 32] = col_ff[g, j, i // 32] = True
        assert torch.equal(rs.cpu() == 255, row_ff) and torch.equal(cs.cpu() == 255, col_ff)
        assert not rc[g, i, j // 32 * 32:j // 32 * 32 + 32].any() and not cc[g, j, i // 32 * 32:i // 32 * 32 + 32].any()
        check(x, lambda t: t, "mxfp8_e4m3", "mxfp4_e2m1", f"one {bad}")


def test_empty_tensors_enqueue_nothing_and_layouts_beyond_two_levels_are_copied():
    for shape in ((0, 8, 32), (2, 0, 32), (2, 8, 0), (2, 0, 3, 0)):
        rc, rs, cc, cs = mx_quantize_2way_batched(torch.empty(shape, device=DEV), "mxfp8_e4m3", "mxfp8_e4m3")
        assert _hip.mx_quant2_batched_last_route is None
        assert rc.shape == shape and cc.shape == shape[:-2] + (shape[-1], shape[-2])
        assert rs.shape == shape[:-1] + (-(-shape[-1] // 32),) and cs.shape == shape[:-2] + (shape[-1], -(-shape[-2] // 32))
    base = randn((2, 3, 4, 16, 32), torch.bfloat16, 10)
    for view in (lambda t: t.permute(2, 1, 0, 3, 4), lambda t: t.transpose(-1, -2), lambda t: t[..., ::2]):      # three levels; C strided
        assert _slice_strides(view(base)) is None
        check(base, lambda t: view(t).contiguous(), "mxfp6_e2m3", "mxfp4_e2m1", "copied")
        got = mx_quantize_2way_batched(view(base.to(DEV)), "mxfp6_e2m3", "mxfp4_e2m1")
        want = mx_quantize_2way_batched(view(base), "mxfp6_e2m3", "mxfp4_e2m1")
        assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


def descriptor(**kw):
    a = _hip.MxQuant2BatchedArgs()
    a.struct_size = ctypes.sizeof(a)
    fields = dict(row_format=0, col_format=4, x=4096, xdt=_hip._DT[torch.bfloat16], row_codes=8192, row_scales=12288, col_codes=16384,
                  col_scales=20480, R=32, C=64, G0=2, G1=3, x_stride_g0=3 * 32 * 64, x_stride_g1=32 * 64, x_stride_r=64)
    fields.update(kw)
    for k, v in fields.items():
        setattr(a, k, v)
    return ctypes.byref(a)


def test_every_error_of_the_descriptor():
    """the route export runs the checks of the launch and enqueues nothing: the pointers are never followed"""
    route = _hip.load().qs_mx_quant2_batched_route
    ARG, DTYPE, ALIGN = -2, -1, -3                                # QS_ERR_ARG, QS_ERR_DTYPE, QS_ERR_ALIGN
    assert route(None) == ARG and route(descriptor(xdt=99)) == DTYPE and route(descriptor(x=4097)) == ALIGN
    lib2 = _hip.load().qs_mx_quant2_route                         # the same codes as the 2-d entry
    a2 = _hip.MxQuant2Args()
    a2.struct_size, a2.x, a2.row_codes, a2.row_scales, a2.R, a2.C = ctypes.sizeof(a2), 4096, 8192, 12288, 32, 64
    a2.xdt = 99
    assert lib2(ctypes.byref(a2)) == DTYPE
    a2.xdt, a2.x = _hip._DT[torch.bfloat16], 4097
    assert lib2(ctypes.byref(a2)) == ALIGN
    assert route(descriptor()) == VEC
    # qs_mx_quant2_v's: x, the pairs, the formats, the extents, the rounding operands
    for kw in (dict(x=None), dict(row_codes=None, row_scales=None, col_codes=None, col_scales=None), dict(row_scales=None),
               dict(col_codes=None), dict(row_format=9), dict(col_format=-1), dict(R=-1), dict(C=-1), dict(rounding=2),
               dict(rounding=1, index_base=2)):
        assert route(descriptor(**kw)) == ARG, kw
    assert route(descriptor(row_codes=None, row_scales=None, row_format=9)) == VEC      # the format of an absent pair is ignored
    # what the slices add
    for kw in (dict(G0=-1), dict(G1=-1), dict(x_stride_r=63), dict(x_stride_g0=-8), dict(x_stride_g1=-8),
               dict(G0=2 ** 31, G1=2 ** 31, R=2 ** 10, C=2 ** 10),                      # G R C beyond INT64_MAX
               dict(G0=2 ** 32, G1=2 ** 32),                                            # G0 G1 beyond INT64_MAX
               dict(x_stride_g0=2 ** 63 - 1),                                              # the last element of x beyond INT64_MAX
               dict(R=2 ** 40, x_stride_r=2 ** 30),
               dict(G0=2 ** 16, G1=2 ** 15),                                            # 2^31 work-groups: one more than the grid takes
               dict(G0=1, G1=1, R=128 * 2 ** 16, C=64 * 2 ** 15, x_stride_r=64 * 2 ** 15)):
        assert route(descriptor(**kw)) == ARG, kw
    assert route(descriptor(G0=2 ** 16, G1=2 ** 15 - 1, x_stride_g0=(2 ** 15 - 1) * 2048)) == VEC      # 2^31 - 2^16 work-groups
    # dtype and alignment come after the extents' signs and before the empty tensor, as in the 2-d entry
    assert route(descriptor(G0=-1, xdt=99)) == ARG and route(descriptor(G0=0, xdt=99)) == DTYPE and route(descriptor(R=0, x=4097)) == ALIGN
    for kw in (dict(G0=0), dict(G1=0), dict(R=0), dict(C=0), dict(G0=0, x_stride_r=1)):
        assert route(descriptor(**kw)) == 0, kw
    # the vector route's conditions, one at a time
    for kw in (dict(C=60, x_stride_r=64), dict(x=4096 + 2), dict(x_stride_r=68), dict(x_stride_g1=2052), dict(x_stride_g0=6148),
               dict(R=40), dict(col_codes=16385)):
        assert route(descriptor(**kw)) == PLAIN, kw
    assert route(descriptor(R=40, col_codes=None, col_scales=None)) == VEC
    f32 = dict(xdt=_hip._DT[torch.float32])
    assert route(descriptor(x_stride_r=68, **f32)) == VEC and route(descriptor(x_stride_r=66, **f32)) == PLAIN


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_the_bytes_around_all_four_outputs_stay_intact(dtype):
    for base, view, pairs, offset, route in ((randn((2, 144, 72), dtype, 20), lambda t: t, "both", 0, VEC),
                                             (randn((3, 37, 19), dtype, 21), lambda t: t, "both", 0, PLAIN),
                                             (randn((2, 144, 72), dtype, 22), lambda t: t, "both", 3, PLAIN),
                                             (randn((2, 130, 72), dtype, 23), lambda t: t, "row", 0, VEC),
                                             (randn((2, 16, 3, 32), dtype, 24), lambda t: t.transpose(1, 2), "both", 0, VEC),
                                             (randn((2, 33, 192), dtype, 25), lambda t: t.chunk(3, -1)[2], "both", 1, PLAIN)):
        x = view(base.to(DEV))
        before = base.clone()
        (Rr, C), G = x.shape[-2:], x.numel() // (x.shape[-2] * x.shape[-1])
        sizes = (G * Rr * C, G * Rr * -(-C // 32), G * C * Rr, G * C * -(-Rr // 32))
        fmts = ("mxfp8_e4m3" if pairs in ("both", "row") else None, "mxfp4_e2m1" if pairs in ("both", "col") else None)
        carved = [guarded(n, offset) if fmts[i // 2] is not None else None for i, n in enumerate(sizes)]
        G0, G1, strides = _slice_strides(x)
        out = _hip.mx_quant2_batched(x, G0, G1, Rr, C, strides, *fmts, out=tuple(None if c is None else c[1] for c in carved))
        torch.cuda.synchronize()
        what = (tuple(x.shape), pairs, offset)
        assert _hip.mx_quant2_batched_last_route == route, what
        assert torch.equal(base, before)
        want = mx_quantize_2way_batched(view(base), *fmts)
        for c, n, o, w in zip(carved, sizes, out, want):
            if c is not None:
                assert intact(c[0], n, offset), what
                assert torch.equal(o.cpu().reshape(w.shape), w), what
