"""The contract of cc_staircase_decode_sr in numpy: the window, the positions, the half-pass schedule, the
finality of a block and the status of staircase_model (cc_staircase_decode, word for word), with the keep-or-revert rule
of product_sr_model on every line.

A stream is y[L][m][m] float32 channel values, z = (y < 0); block 0 is z = 0 and is never weak.  Bit v is weak in
half-pass h iff |y_v| < weights[h] in float32 (a NaN is never weak and decides as 0); weights[h] belongs to half-pass h of
every window position.  State x = (B_0 = 0, z).  Half-pass h decodes every line of its steps from the state at its start
with product_hard_model.decode_lines, whose `take` flag says that a taken word c exists (the line itself where its
syndromes are zero, parity bit mended):

  B_0 rule     a line of step 1 whose taken word differs from the line at a position of block 0 has no taken word
  taken word   x'(p) = c(p) where c(p) == z(p) or p is weak in h, else z(p) -- the tie |y| == w reverts
  no taken     x'(p) = z(p) at every position of the line, the column half in block i - 1 included

out = the final blocks 1 .. L, nflip = d_H(out, z), status as staircase_model.status.
"""
import numpy as np

import product_hard_model as PH
import staircase_model as SM
from staircase_model import FRAME_NOT_CONVERGED, FRAME_OK, counted_blocks, decoder, shape  # noqa: F401


def hard(y):
    return (np.asarray(y, np.float32) < 0).astype(np.uint8)


def decode(dec, y, weights, window, iters, extended, trace=None):
    """y (B, L, m, m) float32 -> dict(out=, nflip=, status=).  trace (a list) receives one dict per (position,
    half-pass): position, half, steps and per stream, (B,) each: reverted (bits at which a taken word differs from z at a
    strong position), fallback (lines without a taken word; fallback_changed: those that were not the z line), zero_rule (lines of step 1 the B_0 rule left without one),
    clean_changed (lines that were words before the half-pass and another line after it) and changed (bool)"""
    y = np.ascontiguousarray(y, np.float32)
    assert len(weights) == 2 * iters and window >= 2 and iters >= 1
    z = hard(y)
    B, L, m, _ = z.shape
    e = 1 if extended else 0
    assert 2 * m - e == dec.n
    zf = SM.with_zero_block(z)
    full = zf.copy()
    with np.errstate(invalid="ignore"):
        mag = np.concatenate([np.full((B, 1, m, m), np.inf, np.float32), np.abs(y)], axis=1)  # block 0: never weak
        b_last = max(0, L - window + 1)
        for b in range(b_last + 1):
            top = min(b + window - 1, L)
            for h in range(2 * iters):
                weak = mag < np.float32(weights[h])
                steps = [i for i in range(b + 1, top + 1) if (top - i) % 2 == h % 2]
                before = full.copy()
                rec = dict(position=b, half=h, steps=steps)
                for k in ("reverted", "fallback", "zero_rule", "clean_changed"):
                    rec[k] = np.zeros(B, np.int64)
                rec["fallback_changed"] = np.zeros(B, np.int64)
                for i in steps:
                    old = SM.gather(before, i, e)
                    zl, wk = SM.gather(zf, i, e), SM.gather(weak, i, e).astype(bool)
                    c, _, take = PH.decode_lines(dec, old.reshape(B * m, 2 * m), extended)
                    c, take = np.asarray(c, np.uint8).reshape(B, m, 2 * m), take.reshape(B, m)
                    if i == 1:  # the B_0 rule
                        zero = take & (c[:, :, m - e: 2 * m - e] != old[:, :, m - e: 2 * m - e]).any(axis=2)
                        take = take & ~zero
                        rec["zero_rule"] += zero.sum(axis=1)
                    keep = take[:, :, None] & ((c == zl) | wk)
                    new = np.where(keep, c, zl).astype(np.uint8)
                    if trace is not None:
                        clean = PH.is_word(dec, old.reshape(B * m, 2 * m), extended).reshape(B, m)
                        rec["reverted"] += (take[:, :, None] & (c != zl) & ~wk).sum(axis=(1, 2))
                        rec["fallback"] += (~take).sum(axis=1)
                        rec["fallback_changed"] += (~take & (new != old).any(axis=2)).sum(axis=1)
                        rec["clean_changed"] += (clean & (new != old).any(axis=2)).sum(axis=1)
                    SM.scatter(full, i, e, new)
                rec["changed"] = (full != before).any(axis=(1, 2, 3))
                if trace is not None:
                    trace.append(rec)
    assert not full[:, 0].any()
    out = np.ascontiguousarray(full[:, 1:])
    return dict(out=out, nflip=(out != z).sum(axis=(1, 2, 3)).astype(np.int32), status=SM.status(dec, out, extended))
