"""Test reference of the stochastic rounding of the MX quantizers, written from the definition in include/qsparse_hip.h
("Stochastic rounding of the MX quantizers") in numpy ``uint64`` / ``uint32`` arithmetic.  It shares no code with the package: the
Philox rounds, the word indexing, the block scale and the integer rounding step are all restated here, and the codes are found by
searching the format's enumerated value grid (``grid`` below), not by assembling exponent and mantissa fields."""
import numpy as np
import torch

# name -> (exponent bits, mantissa bits, bias, emax, largest normal)
FORMATS = {
    "mxfp8_e4m3": (4, 3, 7, 8, 448.0),
    "mxfp8_e5m2": (5, 2, 15, 15, 57344.0),
    "mxfp6_e2m3": (2, 3, 1, 2, 7.5),
    "mxfp6_e3m2": (3, 2, 3, 4, 28.0),
    "mxfp4_e2m1": (2, 1, 1, 2, 6.0),
}
BLOCK = 32
M64 = (1 << 64) - 1
U32 = np.uint64(0xFFFFFFFF)

KNOWN_ANSWERS = [   # (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox(ctr, key):
    """Philox4x32-10: `ctr` four and `key` two arrays (or ints) of 32-bit values; returns the four output words as uint64 arrays.
    A 32 x 32-bit product fits a uint64, so the rounds are written as the paper does"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in ctr]
    k = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) for v in key]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s32 = np.uint64(32)
    for r in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & U32, (p0 >> s32) ^ c[3] ^ k[1], p0 & U32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & U32, (k[1] + np.uint64(0xBB67AE85)) & U32]
    return c


def words(numel, seed=0, step=0, stream=0, index_base=0):
    """the random word of the codes 0 .. numel - 1 of one output tensor (uint64 array of 32-bit values), one Philox call each"""
    k = (int(seed) + int(step)) & M64
    j = [(int(index_base) + i) & M64 for i in range(numel)]          # Python integers: no 64-bit wrap to think about
    q = [v >> 2 for v in j]
    o = philox(([v & 0xFFFFFFFF for v in q], [v >> 32 for v in q], [stream] * numel, [0] * numel), (k & 0xFFFFFFFF, k >> 32))
    pick = np.array([v & 3 for v in j])
    return np.stack(o, 0)[pick, np.arange(numel)]


def grid(fmt):
    """{value: code} over the non-negative codes of the format up to its largest normal (the smallest code of a value)"""
    eb, mb, bias, emax, top = FORMATS[fmt]
    seen = {}
    for code in range(1 << (eb + mb)):
        E, M = code >> mb, code & ((1 << mb) - 1)
        val = M / (1 << mb) * 2.0 ** (1 - bias) if E == 0 else (1 + M / (1 << mb)) * 2.0 ** (E - bias)
        if val <= top:
            seen.setdefault(val, code)
    return seen


def reference(x, fmt, dim=-1, out_dtype=torch.float32, seed=0, step=0, stream=0, index_base=0):
    """(y, codes, scales) of the stochastic one-way quantizer, torch tensors shaped as the package's; element by element"""
    eb, mb, bias, emax, top = FORMATS[fmt]
    g = grid(fmt)
    x32 = x.detach().cpu().float().contiguous()
    xs = x32.numpy()
    w = words(xs.size, seed, step, stream, index_base).reshape(xs.shape)
    dim = dim % xs.ndim
    xm, wm = np.moveaxis(xs, dim, -1), np.moveaxis(w, dim, -1)
    n = xm.shape[-1]
    nb = -(-n // BLOCK)
    y = np.zeros(xm.shape, dtype=np.float64)
    codes = np.zeros(xm.shape, dtype=np.uint8)
    scales = np.zeros(xm.shape[:-1] + (nb,), dtype=np.uint8)
    min_exp_biased = 1 - bias + 127
    for line in np.ndindex(*xm.shape[:-1]):
        for b in range(nb):
            blk = xm[line][b * BLOCK:(b + 1) * BLOCK]
            bits = blk.view(np.uint32).astype(np.uint64) & np.uint64(0x7FFFFFFF)
            am = int(bits.max())
            if am >= 0x7F800000:                                  # a NaN or an Inf in the block
                scales[line + (b,)] = 255
                y[line][b * BLOCK:(b + 1) * BLOCK] = np.nan
                continue
            eb127 = max((am >> 23) - emax, 0)                     # e + 127
            scales[line + (b,)] = eb127
            inv = np.float32(2.0) ** np.float32(127 - eb127)      # 2^-e, a normal float32
            for i in range(len(blk)):
                v = np.float32(blk[i]) * inv                      # float32 product
                vb = int(np.float32(v).view(np.uint32))
                neg, ab = vb >> 31, vb & 0x7FFFFFFF
                E = max(ab >> 23, 1)
                m = (ab & 0x7FFFFF) | (0x800000 if ab >> 23 else 0)
                ex = max(E, min_exp_biased)
                sh = (23 - mb) + (ex - E)
                assert sh >= 20
                T = ((m << 32) >> sh) if sh <= 56 else 0
                nsteps = (T + int(wm[line][b * BLOCK + i])) >> 32
                q = min(nsteps * 2.0 ** (ex - 127 - mb), top)
                codes[line][b * BLOCK + i] = g[q] | (neg << (eb + mb))
                y[line][b * BLOCK + i] = (-q if neg else q) * 2.0 ** (eb127 - 127)
    back = lambda a: torch.from_numpy(np.ascontiguousarray(np.moveaxis(a, -1, dim)))
    return back(y).to(out_dtype), back(codes), back(scales)
