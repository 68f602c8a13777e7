"""The contract of cc_product_decode_sr in numpy on top of product_hard_model's line rule.

A block is y[w2][w1] float32 channel values.  z = (y < 0); bit v is weak in half-iteration h iff |y_v| < weights[h] in
float32 (a NaN is never weak and decides as 0).  x_0 = z.  Half-iteration h decodes every row (h even) or column (h odd)
of x_h with product_hard_model.decode_lines, whose `take` flag says that a taken word c exists (the line itself where its
syndromes are zero, parity bit mended):

  taken word   x_(h+1)(p) = c(p) where c(p) == z(p) or p is weak in h, else z(p) -- the tie |y| == w reverts
  no taken     x_(h+1)(p) = z(p) at every position of the line

out, nflip (against z), last and status are those of product_hard_model.outputs.
"""
import numpy as np

import product_hard_model as PH
from product_hard_model import FRAME_NOT_CONVERGED, FRAME_OK, decoder, is_word, turn  # noqa: F401


def sigma(rows, cols, extended, ebno_db):
    """cc_product_sigma: 1 / sqrt(2 R 10^(ebno / 10)), R = k1 k2 / N"""
    e = 1 if extended else 0
    rate = rows.l * cols.l / ((rows.n + e) * (cols.n + e))
    return 1.0 / np.sqrt(2.0 * rate * 10.0 ** (ebno_db / 10.0))


def hard(y):
    return (np.asarray(y, np.float32) < 0).astype(np.uint8)


def steps(rows, cols, y, weights, extended, trace=None):
    """[x_1, .., x_H] for y (B, w2, w1) and H = len(weights); trace (a list) receives per half-iteration the number of
    reverted bits (the taken word differs from z at a strong position), of fallback lines (no taken word) and of clean
    lines that changed (a word of the code before the pass, another line after it)"""
    y = np.ascontiguousarray(y, np.float32)
    z = hard(y)
    B, w2, w1 = z.shape
    e = 1 if extended else 0
    assert (w1, w2) == (rows.n + e, cols.n + e)
    x, xs = z, []
    with np.errstate(invalid="ignore"):
        mag = np.abs(y)
        for h, w in enumerate(weights):
            weak = mag < np.float32(w)
            column = bool(h % 2)
            dec = cols if column else rows
            lines = lambda a: (turn(a) if column else a).reshape(-1, w2 if column else w1)
            before, zl, wk = lines(x), lines(z), lines(weak)
            c, _, take = PH.decode_lines(dec, before, extended)
            keep = take[:, None] & ((c == zl) | wk)
            new = np.where(keep, c, zl)
            if trace is not None:
                clean = is_word(dec, before, extended)
                trace.append(dict(reverted=int((take[:, None] & (c != zl) & ~wk).sum()), fallback=int((~take).sum()),
                                  clean_changed=int((clean & (new != before).any(axis=1)).sum()), column=column))
            new = new.reshape(B, w1, w2) if column else new.reshape(B, w2, w1)
            x = turn(new) if column else np.ascontiguousarray(new)
            xs.append(x)
    return xs


def outputs(rows, cols, y, xs, halves, extended):
    return PH.outputs(rows, cols, hard(y), xs, halves, extended)


def decode(rows, cols, y, weights, extended):
    return outputs(rows, cols, y, steps(rows, cols, y, weights, extended), len(weights), extended)
