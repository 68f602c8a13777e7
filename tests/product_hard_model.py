"""The contract of cc_product_decode_hard in numpy on top of the oracle's hard decoder.

A block is x[w2][w1] bits, e = 1 for the product of the two extended codes; row i is a line of `rows` (n1 + e bits),
column k a line of `cols` (n2 + e bits).  x_0 = z.  Half-iteration h decodes every row (h even) or every column (h odd)
of x_h on its own:

  inner candidate  what `dec.correct_hard(BM, w[0..n))` returns where it succeeds with at most t corrections -- the rule
                   of chase_model.candidates, which is bounded-distance decoding: the codeword within distance t, if any.
                   `dec` is checkers.Oracle, or shortened_model.Shortened for a shortened handle (a correction at a
                   position >= n fails the line).
  plain            with a candidate the line becomes it, without one it stays
  extended         d = d_H(c', w[0..n)) + (parity(c') != w_n); the line becomes (c', parity(c')) iff d <= t, else it stays

out = x_halves; nflip = d_H(out, z); last = the largest h + 1 with x_(h+1) != x_h (0: never); status = FRAME_OK iff every
row and column of out is in the null space of its code's H (and, extended, has even weight), else FRAME_NOT_CONVERGED.
"""
import numpy as np

from checkers import BM
from chase_model import FRAME_OK, decoder  # noqa: F401 (the tests build their decoders with it)
from shortened_model import Shortened, pad

FRAME_NOT_CONVERGED = 1


def decode_lines(dec, lines, extended):
    """one pass over lines (L, n + e): the new lines, and per line whether an inner candidate exists and whether it was
    taken"""
    lines = np.ascontiguousarray(lines, np.uint8)
    n, t = dec.n, dec.t
    inner = np.ascontiguousarray(lines[:, :n])
    out, nerr, st = dec.correct_hard(BM, inner)[:3]
    out, nerr, st = np.asarray(out, np.uint8), np.asarray(nerr), np.asarray(st)
    cand = (st == FRAME_OK) & (nerr >= 0) & (nerr <= t)
    if not extended:
        return np.where(cand[:, None], out, inner), cand, cand
    parity = (out.sum(axis=1) & 1).astype(np.uint8)
    d = (out != inner).sum(axis=1) + (parity != lines[:, n])
    take = cand & (d <= t)
    new = np.where(take[:, None], np.concatenate([out, parity[:, None]], axis=1), lines)
    return new, cand, take


def rejected_for_a_virtual_root(dec, lines):
    """lines of a shortened decoder whose mother code has a word within t that is non-zero at a position >= n"""
    assert isinstance(dec, Shortened)
    inner = np.ascontiguousarray(np.asarray(lines, np.uint8)[:, : dec.n])
    out, nerr, st = dec.m.correct_hard(BM, pad(inner, dec.m.n))[:3]
    return (np.asarray(st) == FRAME_OK) & (np.asarray(nerr) <= dec.t) & np.asarray(out)[:, dec.n:].any(axis=1)


def is_word(dec, lines, extended):
    """per line: in the null space of H (and of even weight where extended)"""
    lines = np.asarray(lines, np.int64)
    H = np.asarray(dec.H(), np.int64)
    ok = ~((lines[:, : dec.n] @ H.T) % 2).any(axis=1)
    return ok & ((lines.sum(axis=1) % 2 == 0) if extended else True)


def turn(x):
    return np.ascontiguousarray(x.transpose(0, 2, 1))


def steps(rows, cols, z, halves, extended, trace=None):
    """[x_1, .., x_halves] for z (B, w2, w1); trace (a list) receives per half-iteration the dict of lines before and
    after the pass (in the orientation of the pass) with the candidate and taken flags"""
    x = np.ascontiguousarray(z, np.uint8)
    B, w2, w1 = x.shape
    e = 1 if extended else 0
    assert (w1, w2) == (rows.n + e, cols.n + e)
    xs = []
    for h in range(halves):
        if h % 2 == 0:
            before = x.reshape(B * w2, w1)
            new, cand, take = decode_lines(rows, before, extended)
            x = new.reshape(B, w2, w1)
        else:
            before = turn(x).reshape(B * w1, w2)
            new, cand, take = decode_lines(cols, before, extended)
            x = turn(new.reshape(B, w1, w2))
        if trace is not None:
            trace.append(dict(before=before, after=new, cand=cand, take=take, column=bool(h % 2)))
        xs.append(x)
    return xs


def outputs(rows, cols, z, xs, halves, extended):
    """the call's outputs after `halves` half-iterations, from the steps of a run of at least as many"""
    z = np.asarray(z, np.uint8)
    B, w2, w1 = z.shape
    chain = [z] + list(xs[:halves])
    out = chain[-1]
    last = np.zeros(B, np.int32)
    for h in range(halves):
        changed = (chain[h + 1] != chain[h]).any(axis=(1, 2))
        last[changed] = h + 1
    ok = is_word(rows, out.reshape(B * w2, w1), extended).reshape(B, w2).all(axis=1)
    ok &= is_word(cols, turn(out).reshape(B * w1, w2), extended).reshape(B, w1).all(axis=1)
    return dict(out=out, nflip=(out != z).sum(axis=(1, 2)).astype(np.int32), last=last,
                status=np.where(ok, FRAME_OK, FRAME_NOT_CONVERGED).astype(np.int32))


def decode(rows, cols, z, halves, extended):
    return outputs(rows, cols, z, steps(rows, cols, z, halves, extended), halves, extended)
