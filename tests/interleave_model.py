"""The symbol-interleaved layout in numpy: block b holds the frames f = b I + j, j < I, and symbol p of
frame f is at symbol index b I n + p I + j of the buffer -- the array [B / I][n][I] read contiguously.  The only
statement of the layout the tests trust."""
import numpy as np


def interleave(x, I):
    """(B, n) frame-major -> (B / I, n, I)"""
    B, n = x.shape
    flat = np.empty(B * n, x.dtype)
    f, p = np.divmod(np.arange(B * n), n)
    flat[(f // I) * I * n + p * I + f % I] = x.reshape(-1)
    return flat.reshape(B // I, n, I)


def deinterleave(y, I):
    """(B / I, n, I) -> (B, n) frame-major"""
    blocks, n, depth = y.shape
    assert depth == I
    f, p = np.divmod(np.arange(blocks * I * n), n)
    return y.reshape(-1)[(f // I) * I * n + p * I + f % I].reshape(blocks * I, n)
