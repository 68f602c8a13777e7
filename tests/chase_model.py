"""The contract of Chase-II decoding (cc_correct_chase_batch) on top of the oracle's hard decoder.

For a frame y of n floats: z = (y < 0); the key of position i is bits(y_i) & 0x7fffffff, ties to the lower position;
L_0 .. L_5 are the six positions with the smallest keys; test pattern j flips L_i for every set bit i of j.  The candidate
of a pattern is what `decoder.correct_hard(BM, z ^ e_j)` returns when it succeeds with at most t corrections; its metric
is the float32 sum, in ascending position, of |y_i| where it differs from z.  The patterns of p are the first 2^p of
p = 6, so `candidates` decodes all 64 once and `pick` answers every p from them.

`decoder` is checkers.Oracle for a full-length code and shortened_model.Shortened(Oracle, N) for a shortened one.
"""
import numpy as np

import soft_model
from checkers import BCH, BM, Oracle
from shortened_model import Shortened
from soft_model import FRAME_LOCATOR, FRAME_OK, metric  # noqa: F401 (the tests read them from here)

MAX_P = 6


def decoder(q, t, N=None):
    mother = Oracle(BCH, q, t)
    return mother if N is None or N == mother.n else Shortened(mother, N)


def hard(y):
    return (np.asarray(y, np.float32) < 0).astype(np.uint8)  # -0.0 < 0 is false


def least_reliable(y, count=MAX_P):
    """(B, min(count, n)) positions in the order of the contract"""
    return soft_model.least_reliable(y, count)


def candidates(dec, y, max_p=MAX_P):
    """words (B, 2^max_p, n) u8, ok (B, 2^max_p) bool, M (B, 2^max_p) f32 of every test pattern; a frame of n < max_p
    positions has the 2^n patterns of p = n and no more"""
    y = np.ascontiguousarray(y, np.float32).reshape(-1, dec.n)
    max_p = min(max_p, dec.n)
    B, n, J = y.shape[0], dec.n, 1 << max_p
    z = hard(y)
    L = least_reliable(y, max_p)
    words = np.zeros((B, J, n), np.uint8)
    ok = np.zeros((B, J), bool)
    bits = (np.arange(J)[:, None] >> np.arange(max_p)[None, :]) & 1  # (J, max_p)
    for f in range(B):
        pat = np.repeat(z[f][None, :], J, axis=0)
        for i in range(max_p):
            pat[:, L[f, i]] ^= bits[:, i].astype(np.uint8)
        out, nerr, st = dec.correct_hard(BM, pat)[:3]
        good = (np.asarray(st) == FRAME_OK) & (np.asarray(nerr) >= 0) & (np.asarray(nerr) <= dec.t)
        words[f], ok[f] = out, good
    M = metric(y[:, None, :], z[:, None, :], words)
    return dict(y=y, z=z, L=L, words=words, ok=ok, M=M)


def pick(cand, p):
    """the contract's outputs for p: out (B, n) u8, nerr (B,) i32, status (B,) i32, metric (B,) f32, winner (B,) (-1: none)"""
    J = 1 << p
    if J > cand["ok"].shape[1]:
        raise ValueError("p = %d asks for %d test patterns, %d were decoded" % (p, J, cand["ok"].shape[1]))
    return soft_model.pick(cand, J, "z")


def chase(dec, y, p):
    return pick(candidates(dec, y, max(p, 0)), min(p, dec.n))
