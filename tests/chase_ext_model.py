"""The contract of Chase decoding of extended BCH codes (cc_correct_chase_extended_batch) on top of
chase_model and chase_soft_model.  A frame is n + 1 floats, position n carrying the overall parity bit of the inner word.
The test patterns and their inner candidates are those of chase_model on y[:, :n] -- so L_0 .. L_(p-1) are inner
positions -- every candidate gets its parity bit appended, and its metric is the float32 sum in ascending position over
all n + 1 columns, the parity position last.  `pick` and `soft` then run unchanged on the widened words, z and y.
"""
import numpy as np

import chase_model as M
import chase_soft_model as S
import soft_model
from soft_model import FRAME_LOCATOR, FRAME_OK  # noqa: F401 (the tests read them from here)


def extend(words):
    """(..., n) -> (..., n + 1): the overall parity bit appended"""
    words = np.asarray(words, np.uint8)
    return np.concatenate([words, words.sum(axis=-1, keepdims=True).astype(np.uint8) & 1], axis=-1)


def candidates(dec, y, max_p=M.MAX_P):
    """chase_model.candidates for frames of dec.n + 1 values: words (B, 2^max_p, n + 1), M over n + 1 columns, z and y
    widened; L stays (B, max_p) inner positions"""
    y = np.ascontiguousarray(y, np.float32).reshape(-1, dec.n + 1)
    inner = M.candidates(dec, np.ascontiguousarray(y[:, : dec.n]), max_p)
    z, words = M.hard(y), extend(inner["words"])
    return dict(y=y, z=z, L=inner["L"], words=words, ok=inner["ok"], M=soft_model.metric(y[:, None, :], z[:, None, :], words))


def chase(dec, y, p):
    return M.pick(candidates(dec, y, max(p, 0)), min(p, dec.n))


def chase_soft(dec, y, p, beta):
    return S.soft(candidates(dec, y, max(p, 0)), min(p, dec.n), beta)


def product_decode(rows, cols, y, p, alpha, beta):
    """chase_soft_model.product_decode over the extended codes: y is (B, cols.n + 1, rows.n + 1)"""
    return S.product_decode(rows, cols, y, p, alpha, beta, decode=chase_soft)
