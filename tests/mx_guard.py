"""Guard bytes for the out-of-bounds tests of the MX kernels: a tensor under test is carved out of a larger GPU allocation filled
with a byte pattern, and after the launch the margins on both sides must still hold it."""
import torch

DEV = "cuda:0"
PAD = 512          # bytes on either side
PATTERN = 0xA5


def guarded(nbytes, offset=0, pad=PAD):
    """(raw, body): `body` = nbytes bytes starting pad + offset bytes into a pattern-filled allocation"""
    raw = torch.full((nbytes + 2 * pad + offset,), PATTERN, dtype=torch.uint8, device=DEV)
    return raw, raw[pad + offset:pad + offset + nbytes]


def intact(raw, nbytes, offset=0, pad=PAD):
    return bool((raw[:pad + offset] == PATTERN).all()) and bool((raw[pad + offset + nbytes:] == PATTERN).all())
