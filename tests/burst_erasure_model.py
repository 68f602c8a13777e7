"""The burst detector of cc_burst_erasure_channel_dev / cc_mc_run_burst_erasure_dev restated in numpy, on top
of the chain and the error draws of tests/burst_model.py:

    thresholds   DB = llround(p_detect 2^32), DG = llround(p_false_alarm 2^32)
    flag         d_t = word t & 3 of Philox counter (gb_lo, gb_hi, t >> 2, 8): symbol t is flagged iff d_t < (s_t bad ? DB : DG)
    received     a flagged symbol is received as 0; an unflagged one as burst_model.channel gives it
    erasures     frame f = b I + j lists its flagged positions p, ascending; one CSR over the frames of a call

The lists are built with a plain loop over frames and positions: this is the checker of the device's list kernels and
shares nothing with them."""
import math

import numpy as np

import burst_model
from test_discrete_host import symbol_words


def detector_thresholds(p_detect, p_false_alarm):
    """(DB, DG): round half away from zero, as llround."""
    fix = lambda x: int(math.floor(x * 2.0 ** 32 + 0.5))  # noqa: E731
    return fix(p_detect), fix(p_false_alarm)


def channel(params, detector, I, seed, first_frame, frames, n, q_sym, sent=None, base=None):
    """(recv, sent, state, flag, wrong) of frames [first_frame, first_frame + frames), each (frames / I, n, I), the
    transmission order.  params = (p_gb, p_bg, p_error_good, p_error_bad), detector = (p_detect, p_false_alarm); wrong:
    the symbols in error that are not flagged.  base: what burst_model.channel returns for the same arguments, where a
    caller has it already (it does not depend on the detector)."""
    recv, s, state, wrong = base if base is not None else burst_model.channel(params, I, seed, first_frame, frames, n,
                                                                                q_sym, sent)
    DB, DG = detector_thresholds(*detector)
    blocks, N = frames // I, n * I
    d = symbol_words(seed, first_frame // I, blocks, N, 8).reshape(blocks, n, I)
    flag = d < np.where(state != 0, np.uint64(DB), np.uint64(DG))
    recv = np.where(flag, 0, recv).astype(np.uint8)
    return recv, s, state, flag.astype(np.uint8), wrong & ~flag


def frame_lists(flag):
    """flag (blocks, n, I) -> the list of every frame f = b I + j: its flagged positions, ascending"""
    blocks, n, I = flag.shape
    lists = []
    for b in range(blocks):
        for j in range(I):
            lists.append([p for p in range(n) if flag[b, p, j]])
    return lists


def csr(lists):
    """(values, offsets) of per-frame lists"""
    off = np.zeros(len(lists) + 1, np.int64)
    vals = []
    for f, positions in enumerate(lists):
        vals.extend(positions)
        off[f + 1] = len(vals)
    return np.asarray(vals, np.int64), off
