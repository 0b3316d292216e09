"""``mx_gemm_ref.model_bound`` and ``model_emulate`` on the CPU: the bound that follows the measured accumulation of
v_mfma_scale_f32_16x16x128_f8f6f4 ("Accumulation").  Three things are held here without a GPU: the sizes of the bound's
terms on seed 0, that the float64 emulation of the model stays inside the bound for every pair and ragged K, and that the bound is not
slack enough to hide a wrong kernel -- three mutations of the reference leave it in every affected row or column."""
import pytest
import torch

import mx_gemm_ref as G
import qsparse_amd as qs
from qsparse_amd.quantize import quantize_with_mx

PAIRS = [(a, b) for a in G.FMTS for b in G.FMTS]
FP8 = ("mxfp8_e4m3", "mxfp8_e5m2")
M, N = 45, 33
KS = (1, 8, 33, 40, 64, 90, 129, 200, 320)


@pytest.fixture(autouse=True)
def _quiet():
    before = {k: qs.get_qsparse_option(k) for k in ("log_on_created", "log_during_train")}
    qs.set_qsparse_options(log_on_created=False, log_during_train=False)
    yield
    qs.set_qsparse_options(**before)


def quantized(g, K, fa, fb):
    """codes and scales as the quantizer writes them (CPU path), from randn activations and randn / sqrt(K) weights"""
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
    return tuple(quantize_with_mx(x, fa, -1, return_codes=True)[1:]) + tuple(quantize_with_mx(w, fb, -1, return_codes=True)[1:])


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_sizes_on_seed_0(fa, fb):
    g = torch.Generator().manual_seed(0)
    for K in (40, 64, 200):
        ra, rb = G.scale_windows(K, fa, fb)
        G.assert_exact_class(K, fa, fb, ra, rb)
        ops = G.exact_operand(g, M, K, fa, ra) + G.exact_operand(g, N, K, fb, rb)
        assert not bool(G.inside_groups(*ops[:2], fa, *ops[2:], fb).any()), ("exact class", K)
        ops = quantized(g, K, fa, fb)
        inside = G.inside_groups(*ops[:2], fa, *ops[2:], fb)
        S = G.reference(*ops[:2], fa, *ops[2:], fb)[2]
        print(fa, fb, K, "largest inside-a-group term / S", float((inside / S).max()), "across-groups term / S", G.F_ACROSS * -(-K // 128) * 2.0 ** -23)
        if "fp4" in fa and "fp4" in fb:
            assert not bool(inside.any()), K
        if fa in FP8 or fb in FP8:
            assert bool((inside > 0).any()), K


@pytest.mark.parametrize("fa,fb", PAIRS)
def test_emulation_stays_within_the_bound(fa, fb):
    g = torch.Generator().manual_seed(7 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for K in KS:
        ops = quantized(g, K, fa, fb)
        bias = torch.randn(N, generator=g)
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            for b in (None, bias):
                _, y64, S = G.reference(*ops[:2], fa, *ops[2:], fb, b, dt)
                y = G.model_emulate(*ops[:2], fa, *ops[2:], fb, b, dt)
                ok, ratio = G.within(y, y64, G.model_bound(*ops[:2], fa, *ops[2:], fb, y64, S, b, dt))
                assert ok, (K, dt, b is not None, ratio)


def mutate(ops, which):
    """(the mutated operands, the rows of B it touched)"""
    ac, asc, bc, bsc = (t.clone() for t in ops)
    j = None
    if which == "zero_last_code":             # the code at k = K - 1 of A replaced by the zero code
        ac[:, -1] = 0
    elif which == "raise_last_scale":         # the last scale byte of every row of A raised by one
        asc[:, -1] += 1
    else:                                     # the scale bytes of two neighbouring rows of B swapped: the first two that differ
        j = int((bsc[:-1] != bsc[1:]).any(1).nonzero()[0])
        bsc[[j, j + 1]] = bsc[[j + 1, j]]
    return (ac, asc, bc, bsc), j


@pytest.mark.parametrize("which", ["zero_last_code", "raise_last_scale", "swap_b_scales"])
@pytest.mark.parametrize("fa,fb", PAIRS)
def test_the_bound_does_not_hide_a_wrong_kernel(fa, fb, which):
    """the mutated reference stands in for a wrong kernel: in every affected row of y (every affected column for the swap) at least
    one output must lie outside the bound computed from the true operands"""
    g = torch.Generator().manual_seed(11 + G.FMTS.index(fa) * 5 + G.FMTS.index(fb))
    for K in (40, 64, 200):
        ops = quantized(g, K, fa, fb)
        _, y64, S = G.reference(*ops[:2], fa, *ops[2:], fb)
        bound = G.model_bound(*ops[:2], fa, *ops[2:], fb, y64, S)
        mutated, j = mutate(ops, which)
        wrong = G.reference(*mutated[:2], fa, *mutated[2:], fb)[1]
        changed, outside = wrong != y64, (wrong - y64).abs() > bound
        if which == "swap_b_scales":
            cols = changed.any(0).nonzero().reshape(-1)
            assert cols.tolist() == [j, j + 1]
            assert bool(outside[:, cols].any(0).all()), (K, "a swapped column stays inside the bound")
        else:
            rows = changed.any(1).nonzero().reshape(-1)
            # the scale byte changes every row; the zero code every row whose last code was not the zero code already -- rare among
            # the quantizer's codes but for FP4, which rounds |x| < 2^-2 of the block's scale to zero: still most rows
            assert len(rows) == M if which == "raise_last_scale" else len(rows) >= M // 2, (K, len(rows))
            assert bool(outside[rows].any(1).all()), (K, "an affected row stays inside the bound")
        print(fa, fb, K, which, "flagged", int((outside & changed).sum()), "of", int(changed.sum()), "changed outputs")
