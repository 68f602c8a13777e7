"""The contract of ordered-statistics decoding (cc_correct_osd_batch), stated on the generator side --
independently of the kernel, which works on the parity-check matrix.

For a frame y of n floats: z = (y < 0); the key of position i is bits(y_i) & 0x7fffffff; pi orders the positions by
descending key, ties to the lower position.  The rows of G are the oracle's encodings of the unit messages.  Walking pi,
a position joins the basis iff its column of G is independent of the columns already chosen (greedy elimination), until
l positions B_0 .. B_(l-1) are found.  Pattern 0 flips nothing, pattern 1 + a flips B_a, pattern 1 + l + rank(a, b), a < b
in lexicographic order, flips B_a and B_b.  The candidate of a pattern is the codeword that equals z on the basis outside
the flip set and its complement inside; its metric is soft_model.metric; the smallest metric wins, ties to the smallest j.

`decoder` is chase_model.decoder: checkers.Oracle, or shortened_model.Shortened for a shortened code.
"""
import functools

import numpy as np

from chase_model import decoder, hard  # noqa: F401 (the tests read them from here)
from soft_model import FRAME_OK, metric  # noqa: F401

MAX_ORDER = 2  # CC_OSD_MAX_ORDER; the model itself takes any order (order = l is maximum likelihood)


@functools.lru_cache(maxsize=None)
def _generator(q, t, n):
    dec = decoder(q, t, n)
    return np.ascontiguousarray(dec.encode(np.eye(dec.l, dtype=np.uint8)), np.uint8)


def generator(dec):
    """(l, n): the oracle's codewords of the unit messages"""
    return _generator(dec.q, dec.t, dec.n)


def order(y):
    """pi of one frame: descending key, ties to the lower position"""
    keys = np.ascontiguousarray(y, np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.argsort(-keys.astype(np.int64), kind="stable")


def greedy(A, walk, want):
    """Walks the columns of the 0/1 matrix A in the order `walk` and keeps those independent of the ones kept before,
    until `want` are kept.  Returns (kept positions in the order kept, rows: row i of the reduced matrix has a one at
    kept[i] and zeros at every other kept position, skipped: columns passed over as dependent)."""
    A = A.copy()
    free = np.ones(A.shape[0], bool)
    kept, rows, skipped = [], [], 0
    for pos in walk:
        if len(kept) == want:
            break
        cand = np.flatnonzero(free & (A[:, pos] != 0))
        if cand.size == 0:
            skipped += 1
            continue
        r = cand[0]
        others = np.flatnonzero(A[:, pos] != 0)
        others = others[others != r]
        A[others] ^= A[r]
        free[r] = False
        kept.append(int(pos))
        rows.append(r)
    assert len(kept) == want
    return kept, A[rows], skipped


def patterns(l, order_):
    """(J, max(order_, 1)) flip sets in j order -- by size, then lexicographically -- padded with l, "no position" """
    import itertools
    width = max(order_, 1)
    sets = [np.full((1, width), l, np.int64)]
    for size in range(1, order_ + 1):
        if size == 1:
            combos = np.arange(l, dtype=np.int64)[:, None]
        elif size == 2:
            combos = np.stack(np.triu_indices(l, 1), axis=1).astype(np.int64)  # row-major: lexicographic in (a, b)
        else:
            combos = np.array(list(itertools.combinations(range(l), size)), np.int64).reshape(-1, size)
        sets.append(np.concatenate([combos, np.full((combos.shape[0], width - size), l, np.int64)], axis=1))
    return np.concatenate(sets)


def pattern_count(l, order_):
    import math
    return sum(math.comb(l, s) for s in range(order_ + 1))


def frame(dec, y, order_):
    """one frame at the given order and at every lower one: a dict of order -> (out, nerr, metric, winner), and "basis",
    "skipped" """
    y = np.ascontiguousarray(y, np.float32)
    G, l = generator(dec), dec.l
    z = hard(y)
    basis, Gr, skipped = greedy(G, order(y), l)
    c0 = (z[basis].astype(np.int64) @ Gr.astype(np.int64) % 2).astype(np.uint8)  # equals z on the basis
    assert np.array_equal(c0[basis], z[basis])
    rows = np.concatenate([Gr, np.zeros((1, dec.n), np.uint8)])
    P = patterns(l, order_)
    C = np.repeat(c0[None, :], P.shape[0], axis=0)
    for i in range(P.shape[1]):
        C ^= rows[P[:, i]]
    with np.errstate(over="ignore"):
        M = metric(y[None, :], z[None, :], C)
    res = {"basis": basis, "skipped": skipped}
    for o in range(order_ + 1):
        count = pattern_count(l, o)
        j = int(np.argmin(M[:count]))  # the first minimum: equal M goes to the smallest j
        res[o] = (C[j], int((C[j] != z).sum()), M[j], j)
    return res


def osd(dec, y, order_):
    """the contract's outputs: out (B, n) u8, nerr (B,) i32, status (B,) i32, metric (B,) f32, winner (B,), skipped (B,);
    with every lower order under the key ("order", o)"""
    y = np.ascontiguousarray(y, np.float32).reshape(-1, dec.n)
    B = y.shape[0]
    res = {o: dict(out=np.zeros((B, dec.n), np.uint8), nerr=np.zeros(B, np.int32), status=np.full(B, FRAME_OK, np.int32),
                   metric=np.zeros(B, np.float32), winner=np.zeros(B, np.int64), skipped=np.zeros(B, np.int64))
           for o in range(order_ + 1)}
    for f in range(B):
        fr = frame(dec, y[f], order_)
        for o in range(order_ + 1):
            r = res[o]
            r["out"][f], r["nerr"][f], r["metric"][f], r["winner"][f] = fr[o]
            r["skipped"][f] = fr["skipped"]
    top = dict(res[order_])
    for o in range(order_ + 1):
        top[("order", o)] = res[o]
    return top


def maximum_likelihood(dec, y):
    """brute force over all 2^l codewords in message order: (word, metric) of the smallest metric; small codes only"""
    assert dec.l <= 12
    y = np.ascontiguousarray(y, np.float32)
    msgs = ((np.arange(1 << dec.l)[:, None] >> np.arange(dec.l)[None, :]) & 1).astype(np.uint8)
    words = (msgs.astype(np.int64) @ generator(dec).astype(np.int64) % 2).astype(np.uint8)
    z = hard(y)
    M = metric(y[None, :], z[None, :], words)
    return words, M
