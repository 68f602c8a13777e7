"""The contract of cc_product_decode_anchor in numpy over product_hard_model.decode_lines, so that the line
rule is literally that of cc_product_decode_hard.  Every pass runs: there is no early stop.

State per line (rows and columns alike): an anchor flag A, a hold flag H, a record R -- the positions the line flipped
when it became an anchor.  Half-iteration h takes the rows (h even) or the columns (h odd) of x_h, the lines; the other
direction is the crossing lines.  Everything of step 1 is decided from the state at the start of the pass.

  1. an anchor is skipped; a held line clears its hold flag and is otherwise skipped; every other line gets its taken
     word from the line rule (a clean line is its own taken word, parity bit mended where extended) and E, the positions
     where the taken word differs from the line; a line without a taken word stays.  No crossing anchor at a position of
     E: the flips are applied, A = 1, R = E.  Otherwise the line stays, every crossing anchor at a position of E counts
     one conflict for this pass and nconf takes one.
  2. behind all lines, every crossing anchor with at least delta conflicts is backtracked: the bits of its record are
     flipped back, its A = 0, R = {}, H = 1 (it sits out its next pass), nback takes one, and every line that holds a
     flipped-back bit loses its anchor flag and its record (its earlier flips stay).  The counts do not survive the pass.

out, nflip, last (which counts bits, not flags) and status are those of product_hard_model.outputs; nback and nconf are
int32 per block.  sit_out=False is the rule without the hold flag, which tests/test_product_anchor_host.py shows cycling.
"""
import numpy as np

import product_hard_model as PH
from product_hard_model import FRAME_NOT_CONVERGED, FRAME_OK, decoder, turn  # noqa: F401 (for the tests)


class State:
    """flags (B, lines) and records (B, lines, crossing lines) of both directions: [0] the rows, [1] the columns"""

    def __init__(self, B, w2, w1):
        self.A = [np.zeros((B, w2), bool), np.zeros((B, w1), bool)]
        self.H = [np.zeros((B, w2), bool), np.zeros((B, w1), bool)]
        self.R = [np.zeros((B, w2, w1), bool), np.zeros((B, w1, w2), bool)]

    def copy(self):
        s = State(0, 0, 0)
        s.A, s.H, s.R = ([a.copy() for a in v] for v in (self.A, self.H, self.R))
        return s

    def same(self, o):
        """per block: the same flags and records"""
        eq = np.ones(self.A[0].shape[0], bool)
        for d in range(2):
            eq &= (self.A[d] == o.A[d]).all(axis=1) & (self.H[d] == o.H[d]).all(axis=1) & (self.R[d] == o.R[d]).all(axis=(1, 2))
        return eq


def one_pass(code, x, st, d, delta, extended, sit_out=True):
    """one half-iteration over x (B, L, W) in the orientation of the pass, d = 0 the rows, 1 the columns; st is updated in
    place.  Returns (x', per block the backtracked anchors, per block the refused lines, what the pass saw)"""
    B, L, W = x.shape
    o = 1 - d
    A, H, Ac = st.A[d].copy(), st.H[d].copy(), st.A[o].copy()  # the state at the start of the pass
    before = x
    new, cand, take = PH.decode_lines(code, x.reshape(B * L, W), extended)
    new, take = new.reshape(B, L, W), take.reshape(B, L)
    active = ~A & ~H
    st.H[d][~A] = False  # a held line clears its hold flag
    taken = active & take
    E = (new != x) & taken[:, :, None]
    conflict = E & Ac[:, None, :]
    refused = conflict.any(axis=2)
    accepted = taken & ~refused
    x = x ^ (E & accepted[:, :, None]).astype(np.uint8)
    st.A[d] |= accepted
    st.R[d] = np.where(accepted[:, :, None], E, st.R[d])
    count = conflict.sum(axis=1)  # (B, W): conflicts per crossing line, all of them at anchors
    back = Ac & (count >= min(int(delta), 1 << 62)) & (count > 0)
    undo = st.R[o] & back[:, :, None]  # (B, W, L): the bits flipped back, crossing line by crossing line
    x = x ^ undo.transpose(0, 2, 1).astype(np.uint8)
    touched = undo.any(axis=1)  # (B, L): the lines that hold a flipped-back bit
    st.A[d][touched] = False
    st.R[d][touched] = False
    st.A[o][back] = False
    st.R[o][back] = False
    if sit_out:
        st.H[o][back] = True
    seen = dict(column=bool(d), before=before, active=active, held=H & ~A, taken=taken, E=E, conflict=conflict,
                refused=refused, accepted=accepted, count=count, back=back, undo=undo, touched=touched,
                lost=touched & (A | accepted), was_anchor=A, cand=cand.reshape(B, L))
    return x, back.sum(axis=1).astype(np.int32), refused.sum(axis=1).astype(np.int32), seen


def steps(rows, cols, z, halves, delta, extended, trace=None, sit_out=True, states=None):
    """(xs, nback, nconf): x_1 .. x_halves for z (B, w2, w1) and per pass and block the backtracked anchors and the
    refused lines, (halves, B) each.  trace (a list) receives what every pass saw, in the orientation of the pass;
    states (a list) the state after every pass."""
    assert int(delta) >= 1
    x = np.ascontiguousarray(z, np.uint8)
    B, w2, w1 = x.shape
    e = 1 if extended else 0
    assert (w1, w2) == (rows.n + e, cols.n + e)
    st = State(B, w2, w1)
    xs, nback, nconf = [], np.zeros((halves, B), np.int32), np.zeros((halves, B), np.int32)
    for h in range(halves):
        if h % 2 == 0:
            x, nback[h], nconf[h], seen = one_pass(rows, x, st, 0, delta, extended, sit_out)
        else:
            xt, nback[h], nconf[h], seen = one_pass(cols, turn(x), st, 1, delta, extended, sit_out)
            x = turn(xt)
        x = np.ascontiguousarray(x)
        if trace is not None:
            trace.append(seen)
        if states is not None:
            states.append(st.copy())
        xs.append(x)
    return xs, nback, nconf


def outputs(rows, cols, z, run, halves, extended):
    """the call's outputs after `halves` half-iterations, from the steps of a run of at least as many"""
    xs, nback, nconf = run
    res = PH.outputs(rows, cols, z, xs, halves, extended)
    res["nback"] = nback[:halves].sum(axis=0).astype(np.int32)
    res["nconf"] = nconf[:halves].sum(axis=0).astype(np.int32)
    return res


def decode(rows, cols, z, halves, delta, extended):
    return outputs(rows, cols, z, steps(rows, cols, z, halves, delta, extended), halves, extended)
