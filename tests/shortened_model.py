"""The contract of a shortened code (cc_desc.n = N < 2^q - 1), stated on top of a full-length model.

A word of the code shortened to N symbols is a word of the mother code whose positions N .. n-1 are zero, cut to N
symbols.  Encode / extract: the mother's on the zero-padded input, cut.  Hard decoding: the mother's decoder on the word
padded with zeros, cut -- except that a frame whose decoded word is non-zero at a position >= N (the mother "corrected"
a symbol the shortened code does not have) fails with CC_FRAME_LOCATOR, returning the hard-decided received word and
nerr = -1.  BCH with the PGZ tag and erasures: the two-trial rule of bch.h:97-149 over two such shortened decodes.
Min-sum: over H[:, :N].

`Shortened(mother, N)` takes any full-length model with encode(msg), extract(cw) and correct_hard(alg, frames,
erasures) on (B, n) arrays: checkers.Oracle (q <= 8), checkers.WideOracle (16-bit symbols, q <= 15: the same
restatement built over uint16, pinned by tests/test_wide_oracle.py), or `Device` below, the device's own full-length
decoder (a second opinion next to the oracle: it decodes the whole batch in one call, so that both handles take the same
route).
"""
import numpy as np

from checkers import BCH, PGZ, Oracle

FRAME_OK, FRAME_LOCATOR, FRAME_RECHECK, FRAME_ERASURES = 0, 2, 3, 4


def native_status(model_st, got_st):
    """the one place where the class of a failure may differ: the shortened decoder counts only roots below N, so a
    frame whose locator has a root at a position >= N fails the root count (CC_FRAME_LOCATOR, cyclic.h:134-143) before
    the re-check that the padded full-length decode fails (CC_FRAME_RECHECK, cyclic.h:243-248).  Returns model_st with
    exactly those frames taken from got_st; every other status must match."""
    model_st, got_st = np.asarray(model_st), np.asarray(got_st)
    return np.where((model_st == FRAME_RECHECK) & (got_st == FRAME_LOCATOR), got_st, model_st)


def pad(a, width):
    a = np.asarray(a)
    out = np.zeros(a.shape[:-1] + (width,), a.dtype)
    out[..., : a.shape[-1]] = a
    return out


class Device:
    """a full-length device code (a cc.cyclic) in the model's interface.  correct_hard takes one erasure list per frame
    and decodes the whole padded batch in one call, so the full-length handle takes the same route as the shortened
    one does for the same call size."""
    batch = True

    def __init__(self, code):
        self.code, self.family, self.q, self.t = code, code.family, code.q, code.t
        self.n, self.k, self.l = code.n, code.k, code.l
        self.dtype = np.uint16 if code.q > 8 else np.uint8

    def encode(self, msg):
        return np.asarray(self.code.encode_batch(np.asarray(msg, self.dtype)))

    def extract(self, cw):
        return np.asarray(self.code.extract_batch(np.asarray(cw, self.dtype)))

    def correct_hard(self, alg, frames, per=None):
        res = self.code.correct_batch(np.asarray(frames, self.dtype), erasures=per)
        return np.asarray(res["out"]), np.asarray(res["nerr"]), np.asarray(res["status"]), None


class Shortened:
    def __init__(self, mother, N):
        assert mother.k < N <= mother.n
        self.m, self.N = mother, N
        self.family, self.q, self.t, self.k = mother.family, mother.q, mother.t, mother.k
        self.n, self.l = N, N - mother.k

    def encode(self, msg):
        return self.m.encode(pad(msg, self.m.l))[:, : self.N]

    def extract(self, cw):
        return self.m.extract(pad(cw, self.m.n))[:, : self.l]

    def _hard(self, w):
        w = np.asarray(w)
        return (w < 0).astype(np.uint8) if w.dtype == np.float32 else w

    def _plain(self, alg, frame, er):
        """one frame, the mother's decoder on the padded word with the virtual-position rule"""
        if len(er) > 2 * self.t:  # the device refuses more erasures than 2t (bch.h:105-107) whatever the tag,
            # on a word with a non-zero syndrome; a codeword comes back as it is
            _, clean_nerr, clean_st, _ = self.m.correct_hard(alg, pad(frame[None, :], self.m.n), [])
            if int(clean_st[0]) == FRAME_OK and int(clean_nerr[0]) == 0:
                return self._hard(frame).copy(), 0, FRAME_OK
            return self._hard(frame).copy(), -1, FRAME_ERASURES
        out, nerr, st, _ = self.m.correct_hard(alg, pad(frame[None, :], self.m.n), er)
        out, nerr, st = out[0], int(nerr[0]), int(st[0])
        if st == FRAME_OK and out[self.N:].any():
            return self._hard(frame).copy(), -1, FRAME_LOCATOR
        if st != FRAME_OK:  # a failing frame returns the (hard-decided) received word
            return self._hard(frame).copy(), -1, st
        return out[: self.N].copy(), nerr, st

    def _rule(self, frames, out, nerr, st):
        """the virtual-position rule on a padded batch decode; failing frames return the received word"""
        virt = (st == FRAME_OK) & out[:, self.N:].any(axis=1)
        st = np.where(virt, FRAME_LOCATOR, st).astype(np.int32)
        bad = st != FRAME_OK
        out = np.where(bad[:, None], self._hard(frames), out[:, : self.N]).astype(out.dtype)
        return out, np.where(bad, -1, nerr).astype(np.int32), st

    def _batch(self, alg, frames, per):
        frames = self._hard(frames)
        B = frames.shape[0]
        if not (per and any(per) and alg == PGZ and self.family == BCH):
            return self._rule(frames, *self.m.correct_hard(alg, pad(frames, self.m.n), per)[:3])
        ne = np.array([len(e) for e in per])
        trials = []
        for v in (0, 1):
            w = frames.copy()
            for f, e in enumerate(per):
                w[f, list(e)] = v
            trials.append(self._rule(w, *self.m.correct_hard(PGZ, pad(w, self.m.n), None)[:3]))
        (o0, e0, s0), (o1, e1, s1) = trials
        pick1 = (s0 != FRAME_OK) | ((s1 == FRAME_OK) & (e1 < e0))
        both_fail = (s0 != FRAME_OK) & (s1 != FRAME_OK)
        out = np.where(pick1[:, None], o1, o0)
        nerr = np.where(pick1, e1, e0)
        st = np.zeros(B, np.int32)
        st[both_fail] = FRAME_LOCATOR
        st[ne > 2 * self.t] = FRAME_ERASURES
        fail = st != FRAME_OK
        out[fail] = frames[fail]
        nerr[fail] = -1
        plain = ne == 0  # no erasures: trial 0 is the plain decode
        out[plain], nerr[plain], st[plain] = o0[plain], e0[plain], s0[plain]
        return out, nerr.astype(np.int32), st

    def correct_hard(self, alg, frames, erasures=None):
        """frames (B, N) symbols or float32; erasures: None or one position list per frame.
        Returns out (B, N), nerr (B,), status (B,)."""
        frames = np.asarray(frames)
        if getattr(self.m, "batch", False):
            return self._batch(alg, frames, erasures)
        B = frames.shape[0]
        out = np.zeros((B, self.N), np.uint16 if self.q > 8 else np.uint8)
        nerr = np.zeros(B, np.int32)
        st = np.zeros(B, np.int32)
        for f in range(B):
            er = list(erasures[f]) if erasures is not None else []
            if er and alg == PGZ and self.family == BCH:
                out[f], nerr[f], st[f] = self._two_trials(frames[f], er)
            else:
                out[f], nerr[f], st[f] = self._plain(alg, frames[f], er)
        return out, nerr, st

    def _two_trials(self, frame, er):
        """bch.h:97-149: erased positions forced to 0 and to 1, two shortened decodes, fewer corrections wins"""
        sym = self._hard(frame)
        if len(er) > 2 * self.t:
            return sym.copy(), -1, FRAME_ERASURES
        trials = []
        for v in (0, 1):
            w = sym.copy()
            w[er] = v
            trials.append(self._plain(PGZ, w, []))
        (o0, e0, s0), (o1, e1, s1) = trials
        if s0 != FRAME_OK and s1 != FRAME_OK:
            return sym.copy(), -1, FRAME_LOCATOR
        if s0 != FRAME_OK or (s1 == FRAME_OK and e1 < e0):
            return o1, e1, FRAME_OK
        return o0, e0, FRAME_OK

    def H(self):
        return self.m.H()[:, : self.N]


def oracle(family, q, t, N, coding=0):
    return Shortened(Oracle(family, q, t, coding=coding), N)


def virtual_frame(model, pos, value=1):
    """c[:N] for the mother's encoding of the message whose only non-zero symbol sits at word position pos >= N: its
    padded decode corrects position pos, which the shortened code does not have"""
    m = model.m
    assert model.N <= pos < m.n
    msg = np.zeros((1, m.l), np.uint16 if model.q > 8 else np.uint8)
    msg[0, pos - m.k] = value
    return m.encode(msg)[0, : model.N]
