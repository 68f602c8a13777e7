"""The contract of GMD decoding (cc_correct_gmd_batch) on top of the oracle's errors-and-erasures decoder.

For a frame of n received symbols w and n floats r: the key of position i is bits(r_i) & 0x7fffffff, ties to the lower
position; E_0 .. E_(2t-1) are the 2t positions with the smallest keys.  Trial tau erases E[:2 tau] and runs
`correct_hard(BM, w, erasures=E[:2 tau])`; it is accepted when the oracle succeeds and at most t - tau positions outside
the erased set changed (the oracle's own nerr counts erasures too, so the model counts).  The metric of a candidate is
the float32 sum, in ascending position, of |r_i| where it differs from w; the smallest wins, equal metrics go to the
smallest tau.  `candidates` decodes all t + 1 trials once and `pick` answers every m from them.

A shortened code goes through shortened_model.Shortened.  For mu != 1 (step = 1) the frame goes through the transform T
of rs_roots_model, which scales symbols and keeps positions, so reliabilities and erased sets carry over; the
virtual-position rule of the shortened code is then applied to the padded word by hand.
"""
import numpy as np

import rs_roots_model as R
import soft_model
from checkers import BM, RS, Oracle
from shortened_model import Shortened
from soft_model import FRAME_LOCATOR, FRAME_OK, least_reliable, metric  # noqa: F401 (the tests read them from here)


class Decoder:
    """RS over GF(2^q), t errors, length N (None: 2^q - 1), roots alpha^mu .. alpha^(mu + 2t - 1)"""

    def __init__(self, q, t, N=None, mu=1):
        self.mother = Oracle(RS, q, t)
        self.q, self.t, self.mu, self.nf = q, t, mu, self.mother.n
        self.n = self.nf if N is None else N
        self.k = self.mother.k
        self.l = self.n - self.k
        assert self.n >= 2 * t + 1
        self.short = None if self.n == self.nf or mu != 1 else Shortened(self.mother, self.n)

    def _T(self, w):
        return R.T(w, self.mother.exp, self.mother.log, self.nf, self.mu, 1)

    def _Tinv(self, w2):
        return R.T_inv(w2, self.mother.exp, self.mother.log, self.nf, self.mu, 1, self.n)

    def encode(self, msg):
        """codewords of this code for (B, l) messages (systematic in the (1, 1) image for mu != 1: any bijection onto the
        code serves the tests)"""
        msg = np.asarray(msg, np.uint8).reshape(-1, self.l)
        full = np.zeros((msg.shape[0], self.mother.l), np.uint8)
        full[:, : self.l] = msg
        cw = self.mother.encode(full)
        assert not cw[:, self.n:].any()
        return cw[:, : self.n] if self.mu == 1 else self._Tinv(cw)

    def trial(self, w, erased):
        """(word, ok) of errors-and-erasures decoding of one frame with the positions `erased` erased"""
        erased = [int(p) for p in erased]
        if self.mu == 1 and self.short is None:
            out, _, st, _ = self.mother.correct_hard(BM, w[None, :], erased)
            return out[0], int(st[0]) == FRAME_OK
        if self.mu == 1:
            out, _, st = self.short.correct_hard(BM, w[None, :], [erased])
            return out[0], int(st[0]) == FRAME_OK
        out, _, st, _ = self.mother.correct_hard(BM, self._T(w[None, :]), erased)
        if int(st[0]) != FRAME_OK or out[0, self.n:].any():
            return w.copy(), False
        return self._Tinv(out)[0], True


def candidates(dec, w, r, trials=None):
    """words (B, m, n) u8, ok (B, m) bool, M (B, m) f32 of the first m = trials (None: t + 1) trials"""
    w = np.ascontiguousarray(w, np.uint8).reshape(-1, dec.n)
    r = np.ascontiguousarray(r, np.float32).reshape(-1, dec.n)
    m = dec.t + 1 if trials is None else trials
    B, n = w.shape
    E = least_reliable(r, 2 * dec.t)
    words = np.zeros((B, m, n), np.uint8)
    ok = np.zeros((B, m), bool)
    for f in range(B):
        for tau in range(m):
            erased = E[f, : 2 * tau]
            c, good = dec.trial(w[f], erased)
            if good:
                outside = np.ones(n, bool)
                outside[erased] = False
                good = int(((c != w[f]) & outside).sum()) <= dec.t - tau
            words[f, tau], ok[f, tau] = (c if good else w[f]), good
    M = metric(r[:, None, :], w[:, None, :], words)
    return dict(w=w, r=r, E=E, words=words, ok=ok, M=M)


def pick(cand, m):
    """the contract's outputs for m trials: out (B, n) u8, nerr, status (B,) i32, metric (B,) f32, winner (B,) (-1: none)"""
    if not 1 <= m <= cand["ok"].shape[1]:
        raise ValueError("m = %d trials asked for, %d were decoded" % (m, cand["ok"].shape[1]))
    return soft_model.pick(cand, m, "w")


def gmd(dec, w, r, m=None):
    m = dec.t + 1 if not m else m
    return pick(candidates(dec, w, r, m), m)


def frames_per_wave(t2, n, m):
    """F of the kernel's mapping (gmd.hip: gmd_layout, soft_lanes.hpp: frames_per_wave): the tests place batch
    sizes around it"""
    def lds(F):
        return (128 * t2 + 2 * 128 * (t2 + 1) + 4 * F * n + 2 * F * t2 + F * n + 15) & ~15
    F = 64 // m
    while F > 1 and lds(F) > ((65536 - 1536) // 4 & ~15):
        F -= 1
    return F
