"""An independent reference for the MX rotary embedding (include/qsparse_hip.h, "MX rotary embedding"): a plain Python loop over the
pairs on numpy float32 arrays -- every product, the difference and the sum are numpy float32 operations, each rounded on its own --
not the package's torch expression.  Plus the inputs the rope tests share."""
import numpy as np
import torch

DTS = (torch.float32, torch.bfloat16, torch.float16)


def rope_ref(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, interleaved: bool = False, inverse: bool = False) -> torch.Tensor:
    """the float32 rotation of `x` [..., T, d] (any of the three dtypes; widened exactly) by the float32 tables [T, d / 2]"""
    xn = x.detach().cpu().to(torch.float32).numpy()
    cn, sn = cos.detach().cpu().numpy(), sin.detach().cpu().numpy()
    assert xn.dtype == np.float32 and cn.dtype == np.float32 and sn.dtype == np.float32
    d = xn.shape[-1]
    h = d // 2
    y = np.empty_like(xn)
    with np.errstate(all="ignore"):
        for j in range(h):
            ia, ib = (2 * j, 2 * j + 1) if interleaved else (j, j + h)
            a, b = xn[..., ia], xn[..., ib]                 # [..., T]
            c, s = cn[:, j], sn[:, j]                       # [T]
            if inverse:
                s = -s
            ac, bs, bc, as_ = a * c, b * s, b * c, a * s    # four float32 products
            assert ac.dtype == np.float32
            y[..., ia] = ac - bs
            y[..., ib] = bc + as_
    return torch.from_numpy(y)


def inputs(seed: int, shape, dtype):
    """x of `shape` with magnitudes spread over a few binades, so that neighbouring blocks take different scales"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-3, 4, shape[:-1] + (1,), generator=g).float())
    return x.to(dtype)


def tables(T: int, d: int, seed: int = 0):
    """cos / sin [T, d / 2] of random angles: float32 values that are no table of any position, so nothing cancels by accident"""
    g = torch.Generator().manual_seed(1000 + seed)
    ang = (torch.rand(T, d // 2, generator=g, dtype=torch.float64) - 0.5) * 20.0
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """equal bit for bit, except that a NaN matches any NaN (a NaN's sign and payload are not part of the definition)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    an, bn = a.isnan(), b.isnan()
    if not torch.equal(an, bn):
        return False
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return torch.equal(a.masked_fill(an, 0).contiguous().view(iv), b.masked_fill(bn, 0).contiguous().view(iv))
