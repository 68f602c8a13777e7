"""The contract of the staircase calls (cc_staircase) in numpy on top of the oracle's hard decoder.

`dec` is what product_hard_model.decoder gives (checkers.Oracle, or shortened_model.Shortened), e = 1 for extended lines,
m = (dec.n + e) / 2, r = (dec.n - dec.l) + e, k_b = m - r.  A stream is x[L][m][m] bits, block 0 (all zero) in front of it
where a function says `full`.  Line j of step i, n + e = 2m bits in the handle's numbering:

  position p < m - e          B_i[j][p]
  position m - e + a, a < m   B_(i-1)[a][j]
  position n (extended)       B_i[j][m - 1]

The line rule is product_hard_model.decode_lines; a line of step 1 whose new word differs from the old one at a position
of block 0 stays (the B_0 rule).  The schedule, finality, nflip and status are those of the public header.
"""
import numpy as np

import product_hard_model as PH
from product_hard_model import FRAME_NOT_CONVERGED, FRAME_OK, decoder  # noqa: F401 (the tests build decoders with it)


def shape(dec, extended):
    """(e, m, r, k_b)"""
    e = 1 if extended else 0
    assert (dec.n + e) % 2 == 0
    m = (dec.n + e) // 2
    r = (dec.n - dec.l) + e
    assert r < m
    return e, m, r, m - r


def with_zero_block(x):
    """(B, L, m, m) -> (B, L + 1, m, m) with block 0 in front"""
    x = np.asarray(x, np.uint8)
    return np.concatenate([np.zeros_like(x[:, :1]), x], axis=1)


def gather(full, i, e):
    """the lines of step i of full (B, L + 1, m, m): (B, m, 2m)"""
    cur, prev = full[:, i], full[:, i - 1]
    m = cur.shape[-1]
    parts = [cur[:, :, : m - e], prev.transpose(0, 2, 1)]
    if e:
        parts.append(cur[:, :, m - 1:])
    return np.ascontiguousarray(np.concatenate(parts, axis=2))


def scatter(full, i, e, lines):
    """the inverse of gather, into full"""
    m = full.shape[-1]
    full[:, i, :, : m - e] = lines[:, :, : m - e]
    full[:, i - 1] = lines[:, :, m - e: 2 * m - e].transpose(0, 2, 1)
    if e:
        full[:, i, :, m - 1] = lines[:, :, 2 * m - 1]


def decode_step(dec, full, i, extended, trace=None):
    """the new lines of step i from the state `full` (not applied): (B, m, 2m)"""
    e, m = (1 if extended else 0), full.shape[-1]
    old = gather(full, i, e)
    B = old.shape[0]
    new, cand, take = PH.decode_lines(dec, old.reshape(B * m, 2 * m), extended)
    new = np.asarray(new, np.uint8).reshape(B, m, 2 * m)
    zero = np.zeros((B, m), bool)
    if i == 1:  # the B_0 rule
        zero = (new[:, :, m - e: 2 * m - e] != old[:, :, m - e: 2 * m - e]).any(axis=2)
        new = np.where(zero[:, :, None], old, new)
    if trace is not None:
        trace.append(dict(step=i, before=old, after=new, cand=cand.reshape(B, m), take=take.reshape(B, m), zero=zero))
    return new


def decode(dec, z, window, iters, extended, trace=None):
    """z (B, L, m, m) -> dict(out=, nflip=, status=); trace (a list) receives one dict per (position, half-pass, step)
    with the lines before and after, the candidate / taken flags and the lines the B_0 rule kept, and one dict
    dict(position=b, changed=[per half-pass (B,) bool]) per position"""
    z = np.ascontiguousarray(z, np.uint8)
    B, L, m, _ = z.shape
    e = 1 if extended else 0
    assert 2 * m - e == dec.n and window >= 2 and iters >= 1
    full = with_zero_block(z)
    b_last = max(0, L - window + 1)
    for b in range(b_last + 1):
        top = min(b + window - 1, L)
        changed = []
        for h in range(2 * iters):
            steps = [i for i in range(b + 1, top + 1) if (top - i) % 2 == h % 2]
            before = full.copy()
            news = [(i, decode_step(dec, before, i, extended, trace)) for i in steps]
            for i, new in news:
                scatter(full, i, e, new)
            changed.append((full != before).any(axis=(1, 2, 3)))
        if trace is not None:
            trace.append(dict(position=b, changed=changed))
    assert not full[:, 0].any()
    out = full[:, 1:]
    return dict(out=np.ascontiguousarray(out), nflip=(out != z).sum(axis=(1, 2, 3)).astype(np.int32),
                status=status(dec, out, extended))


def status(dec, x, extended):
    """FRAME_OK per stream iff every line of every step of x (B, L, m, m) is a word of its code"""
    full = with_zero_block(x)
    B, L1, m, _ = full.shape
    e = 1 if extended else 0
    ok = np.ones(B, bool)
    for i in range(1, L1):
        ok &= PH.is_word(dec, gather(full, i, e).reshape(B * m, 2 * m), extended).reshape(B, m).all(axis=1)
    return np.where(ok, FRAME_OK, FRAME_NOT_CONVERGED).astype(np.int32)


def encode(dec, msg, extended):
    """msg (B, L, m, k_b) -> code streams (B, L, m, m): per step the handle's systematic encoder (message in the
    positions n - l .. n - 1) on the row's message bits followed by the column of the block before"""
    msg = np.asarray(msg, np.uint8)
    B, L, m, kb = msg.shape
    e, mm, r, k_b = shape(dec, extended)
    assert (m, kb) == (mm, k_b)
    full = np.zeros((B, L + 1, m, m), np.uint8)
    for i in range(1, L + 1):
        info = np.concatenate([msg[:, i - 1], full[:, i - 1].transpose(0, 2, 1)], axis=2)  # (B, m, l)
        words = np.asarray(dec.encode(np.ascontiguousarray(info.reshape(B * m, dec.l))), np.uint8).reshape(B, m, dec.n)
        full[:, i, :, : m - e] = words[:, :, : m - e]
        if e:
            full[:, i, :, m - 1] = words.sum(axis=2) & 1
    return np.ascontiguousarray(full[:, 1:])


def extract(dec, cw, extended):
    e, m, r, k_b = shape(dec, extended)
    return np.ascontiguousarray(np.asarray(cw, np.uint8)[:, :, :, dec.n - dec.l: m - e])


def counted_blocks(L, window):
    """L_c: the blocks 1 .. L_c were decoded with a full window ahead of them"""
    return L - window + 1 if L >= window else L
