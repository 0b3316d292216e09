"""``mx_flash_decode_paged(shared=...)`` without a GPU: the CPU path is ``_decode_shared_def``; its error against float64 attention next to
the flat definition's at the same number of runs, the degenerate empty prefix, the refusals, and the C ABI's layout and checks."""
import ctypes
import json
import os
import subprocess

import pytest
import torch

import test_mx_flash_decode as TD
from qsparse_amd import MXPagedKVCache, _hip, mx_flash_decode_paged
from qsparse_amd.mx_flash import _decode_paged_def
from qsparse_amd.quantize import mx_dequantize
from test_mx_paged import gather, pool_of

E4 = TD.E4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shared_case(seed, B, Hkv, r, T, page, NP, NPs, d, dv, qk_fmt=E4, v_fmt=E4, device="cpu", guard=False):
    """(q operands, pools, block_table [B, NP], shared_table [NPs], P): random sequences that all begin with sequence 0's first min(NPs,
    NP) pages.  Those pages are in the pool twice -- once per sequence where block_table says, once where shared_table says -- so the
    flat call on block_table sees the same keys; shared_table entries past NP name pages of 0xFF"""
    ops = TD.operands(seed, B, Hkv, r, T, NP * page, d, dv, qk_fmt, v_fmt, device)
    n, cache = min(NPs, NP) * page, [t.clone() for t in ops[2:]]
    for i, t in enumerate(cache):
        w = n if i in (0, 2) else (n if i == 1 else n // 32)
        (t[:, :, :w] if i < 2 else t[..., :w]).copy_((t[:1, :, :w] if i < 2 else t[:1, ..., :w]).clone())
    P = B * NP + NPs + 3
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    table, stable = perm[:B * NP].view(B, NP).to(device), perm[B * NP:B * NP + NPs].to(device)
    pools = pool_of(cache, page, P, table, guard)
    for t in pools:
        t[stable[:min(NPs, NP)].long()] = t[table[0, :min(NPs, NP)].long()]
    return ops[:2], pools, table, stable, P


def slen(n, device="cpu"):
    return torch.tensor([n], dtype=torch.int32, device=device)


def test_error_against_float64_attention_is_the_flat_definitions_at_the_same_run_count():
    """both are the same recurrence cut at different chunks, so their errors against float64 softmax attention on the de-quantized
    operands agree up to the seed-to-seed spread.  Measured on the CPU over six seeds (profiles/mx_decode_shared.json, "cpu_error"): the
    flat definition's rms error is 2.042e-3 with a seed-to-seed spread (std / mean) of 6.1 %, the shared one's 2.052e-3 (ratio 1.005); the
    margin is 1 + that spread, 1.061: one standard deviation of a seed, 2.4 standard errors of the mean of six"""
    B, Hkv, r, page, NP, NPs, sp, so = 3, 2, 4, 128, 5, 3, 2, 3
    prof = json.load(open(os.path.join(ROOT, "profiles", "mx_decode_shared.json")))["cpu_error"]
    kv_len, errs = torch.tensor([640, 500, 385], dtype=torch.int32), []
    for seed in range(6):
        q, pools, table, stable, _ = shared_case(seed, B, Hkv, r, 1, page, NP, NPs, 64, 64)
        kw = dict(scale=0.125, kv_splits=so)
        got = mx_flash_decode_paged(*q, E4, *pools, E4, table, kv_len, shared=(stable, slen(400)), shared_splits=sp, **kw)
        flat = _decode_paged_def(*q, E4, *pools, E4, table, kv_len, 0.125, False, E4, torch.float32, sp + so)
        rep = TD.repeated(q + gather(pools, table), r)
        qf, kf, vt = (mx_dequantize(rep[i], rep[i + 1], E4, -1, torch.float64) for i in (0, 2, 4))
        s = qf @ kf.transpose(-1, -2) * 0.125
        s = s.masked_fill(torch.arange(NP * page) >= kv_len[:, None, None, None], float("-inf"))
        ref = torch.softmax(s, -1) @ vt.transpose(-1, -2)
        errs.append([(y.double() - ref).pow(2).mean().sqrt().item() for y in (got, flat)])
    shared, flat = (sum(e[i] for e in errs) / len(errs) for i in (0, 1))
    print(f"shared rms {shared:.6g}, flat rms {flat:.6g}, ratio {shared / flat:.4f}, margin {prof['margin']}")
    assert shared <= flat * prof["margin"]


@pytest.mark.parametrize("causal", (False, True))
def test_an_empty_prefix_gives_the_flat_definitions_values(causal):
    q, pools, table, stable, _ = shared_case(7, 3, 2, 3, 2, 64, 5, 2, 40, 24, TD.FP4, E4)
    kv_len = torch.tensor([320, 131, 2], dtype=torch.int32)
    for n in (0, 127):                                           # 127 rounds down to no shared chunk
        got = mx_flash_decode_paged(*q, TD.FP4, *pools, E4, table, kv_len, scale=0.3, is_causal=causal, kv_splits=2, shared=(stable, slen(n)),
                                    shared_splits=3)
        want = _decode_paged_def(*q, TD.FP4, *pools, E4, table, kv_len, 0.3, causal, E4, torch.float32, 2)
        assert torch.equal(got.float() + 0.0, want.float() + 0.0)   # (values: a -0 of one may be the other's +0)
    assert bool(want.isfinite().all()) and bool((want != 0).any())


def test_the_cache_forwards_shared_and_auto_splits_are_a_function_of_the_shapes():
    q, pools, table, stable, P = shared_case(8, 2, 2, 4, 1, 32, 8, 4, 32, 16)
    c = MXPagedKVCache(P, 2, 8, 2, 32, 32, 16)
    c.k_pool, c.k_pool_scales, c.vt_pool, c.vt_pool_scales = pools
    c.block_table, c.kv_len = table, torch.tensor([256, 129], dtype=torch.int32)
    got = c.attend(*q, scale=0.3, shared=(stable, slen(128)))
    # auto: so = min(2 chunks, 1024 // (2 * 2 * 1)) = 2, sp = min(Csmax = 1, ...) = 1
    assert torch.equal(got, c.attend(*q, scale=0.3, shared=(stable, slen(128)), kv_splits=2, shared_splits=1)) and bool(got.isfinite().all())


@pytest.mark.parametrize("what", ("not_a_pair", "table_dtype", "table_shape", "table_empty", "len_shape", "len_dtype", "len_device", "splits0",
                                  "splits_bool"))
def test_refusals(what):
    q, pools, table, stable, _ = shared_case(9, 2, 2, 2, 1, 32, 2, 2, 32, 16)
    kv_len, n, kw = torch.tensor([64, 64], dtype=torch.int32), slen(32), {}
    shared = {"not_a_pair": stable, "table_dtype": (stable.long(), n), "table_shape": (stable[None], n), "table_empty": (stable[:0], n),
              "len_shape": (stable, torch.zeros(2, dtype=torch.int32)), "len_dtype": (stable, n.long()),
              "len_device": (stable, n.to("meta"))}.get(what, (stable, n))
    if what.startswith("splits"):
        kw["shared_splits"] = 0 if what == "splits0" else True
    with pytest.raises(ValueError, match="shared"):
        mx_flash_decode_paged(*q, E4, *pools, E4, table, kv_len, scale=1.0, shared=shared, **kw)


# ---- the C ABI without a GPU: layout of the descriptor, and the checks that come before anything is enqueued ----------------------------
def test_the_descriptor_has_the_headers_layout(tmp_path):
    cname, ct = "qs_mx_flash_decode_shared_paged_args", _hip.MxFlashDecodeSharedPagedArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "qsparse_hip.h")}"', 'int main(void) {',
             f'printf("%zu", sizeof({cname}));'] + [f'printf(" %zu", offsetof({cname}, {f}));' for f, _ in ct._fields_] + ['return 0; }']
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    size, *offsets = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()
    assert int(size) == ctypes.sizeof(ct) and [int(o) for o in offsets] == [getattr(ct, f).offset for f, _ in ct._fields_]


def test_the_entry_points_validate_without_a_gpu():
    lib = _hip.load()
    ARG, ALIGN = -2, -3
    route = lib.qs_mx_flash_decode_shared_paged_route
    assert route(None) == ARG and lib.qs_mx_flash_decode_shared_paged_v(None) == ARG

    def desc(size=None, **kw):
        a = _hip.MxFlashDecodeSharedPagedArgs()
        a.struct_size = ctypes.sizeof(a) if size is None else size
        a.q_codes, a.q_scales, a.k_pool, a.k_pool_scales, a.vt_pool, a.vt_pool_scales = (1 << 20) * 1, (1 << 20) * 2, 3 << 20, 4 << 20, 5 << 20, 6 << 20
        a.block_table, a.kv_len, a.shared_table, a.shared_len, a.workspace, a.y = 7 << 20, 8 << 20, 9 << 20, 10 << 20, 11 << 20, 12 << 20
        a.kv_splits, a.shared_splits, a.scale = 2, 3, 1.0
        a.B, a.Hq, a.Hkv, a.T, a.P, a.NP, a.NPs, a.page, a.d, a.dv = 5, 8, 2, 1, 40, 4, 2, 64, 64, 32
        a.workspace_bytes = 5 * 2 * 4 * 5 * 35 * 4                 # B Hkv R (sp + so) (dv + 3) floats
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    assert route(desc()) == _hip.MX_FLASH_ROUTE_VEC
    assert route(desc(d=40)) == _hip.MX_FLASH_ROUTE_PLAIN and route(desc(k_pool=(3 << 20) + 1)) == _hip.MX_FLASH_ROUTE_PLAIN
    assert route(desc(size=_hip.MxFlashDecodeSharedPagedArgs.shared_table.offset)) == ARG           # a descriptor that ends early
    assert route(desc(size=2)) == ARG
    assert route(desc(shared_table=None)) == ARG and route(desc(shared_len=None)) == ARG
    assert route(desc(shared_table=(9 << 20) + 2)) == ALIGN and route(desc(shared_len=(10 << 20) + 1)) == ALIGN
    assert route(desc(workspace=(11 << 20) + 2)) == ALIGN
    assert route(desc(workspace_bytes=5 * 2 * 4 * 5 * 35 * 4 - 1)) == ARG and route(desc(workspace=None)) == ARG
    assert route(desc(shared_splits=0)) == ARG and route(desc(NPs=0)) == ARG and route(desc(page=48)) == ARG
    assert route(desc(B=0)) == 0
