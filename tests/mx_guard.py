"""Guard bytes for the out-of-bounds tests of the MX kernels: a tensor under test is carved out of a larger GPU allocation filled
with a byte pattern, and after the launch the margins on both sides must still hold it."""
import torch

DEV = "cuda:0"
PAD = 512          # bytes on either side
PATTERN = 0xA5


def guarded(nbytes, offset=0, pad=PAD, pattern=PATTERN):
    """(raw, body): `body` = nbytes bytes starting pad + offset bytes into an allocation filled with `pattern` (0xFF around an input:
    a NaN in float32, bfloat16 and float16, so an over-read poisons what is computed from it)"""
    raw = torch.full((nbytes + 2 * pad + offset,), pattern, dtype=torch.uint8, device=DEV)
    return raw, raw[pad + offset:pad + offset + nbytes]


def intact(raw, nbytes, offset=0, pad=PAD, pattern=PATTERN):
    return bool((raw[:pad + offset] == pattern).all()) and bool((raw[pad + offset + nbytes:] == pattern).all())
