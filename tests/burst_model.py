"""The Gilbert-Elliott burst channel of cc_burst_channel_dev / cc_mc_run_burst_dev restated in numpy.

Block gb = gf / I holds the global frames gb I .. gb I + I - 1; its N = n I symbols are sent in the order of the
interleaved layout, index t = p I + j being symbol p of frame j.  Every block runs a two-state chain of its own:

    thresholds   X = llround(x 2^32) for GB (p_gb), BG (p_bg), PG (p_error_good), PB (p_error_bad), S (p_gb / (p_gb + p_bg))
    start        s_0 = bad iff word 0 of Philox counter (gb_lo, gb_hi, 0xFFFFFFFF, 5) < S
    transition   a_t = word t & 3 of counter (gb_lo, gb_hi, t >> 2, 5): good -> bad iff a_t < GB, bad -> good iff a_t < BG
    error        u_t = word t & 3 of counter (.., t >> 2, 6): symbol t is in error iff u_t < (s_t bad ? PB : PG)
    value        v_t = word t & 3 of counter (.., t >> 2, 7): e = 1 + ((v_t (q_sym - 1)) >> 32)

The chain is walked here with a plain loop over t, one step at a time (vectorised over the blocks only): this is the
checker of the device's scan and shares nothing with it."""
import math

import numpy as np

from test_discrete_host import MASK, error_values, philox4x32_10, symbol_words


def thresholds(p_gb, p_bg, p_error_good, p_error_bad):
    """(GB, BG, PG, PB, S): round half away from zero, as llround."""
    fix = lambda x: int(math.floor(x * 2.0 ** 32 + 0.5))  # noqa: E731
    return fix(p_gb), fix(p_bg), fix(p_error_good), fix(p_error_bad), fix(p_gb / (p_gb + p_bg))


def states(p_gb, p_bg, seed, first_block, blocks, N):
    """s_t of every block and transmission index, 0 good / 1 bad: (blocks, N) uint8."""
    GB, BG, _, _, S = thresholds(p_gb, p_bg, 0.0, 0.0)
    gb = np.uint64(first_block) + np.arange(blocks, dtype=np.uint64)
    start = philox4x32_10(gb & MASK, gb >> np.uint64(32), 0xFFFFFFFF, 5, seed & 0xFFFFFFFF, seed >> 32)[0]
    a = symbol_words(seed, first_block, blocks, N, 5)
    to_bad = np.ascontiguousarray((a < np.uint64(GB)).T)     # from good: bad iff a_t < GB
    stay_bad = np.ascontiguousarray(~(a < np.uint64(BG)).T)  # from bad: good iff a_t < BG
    out = np.empty((N, blocks), bool)
    s = start < np.uint64(S)
    for t in range(N):
        out[t] = s
        s = np.where(s, stay_bad[t], to_bad[t])
    return np.ascontiguousarray(out.T).astype(np.uint8)


def to_transmission_order(words, I):
    """frame-major (frames, n) -> (frames / I, n I), symbol p of frame b I + j at [b, p I + j]"""
    frames, n = words.shape
    return np.ascontiguousarray(words.reshape(frames // I, I, n).transpose(0, 2, 1)).reshape(frames // I, n * I)


def channel(params, I, seed, first_frame, frames, n, q_sym, sent=None):
    """(recv, sent, state, wrong) of frames [first_frame, first_frame + frames), each (frames / I, n, I): the interleaved
    layout, which is the transmission order.  params = (p_gb, p_bg, p_error_good, p_error_bad); sent: the frame-major words
    (frames, n), None for the all-zero word."""
    assert frames % I == 0 and first_frame % I == 0
    blocks, first_block, N = frames // I, first_frame // I, n * I
    _, _, PG, PB, _ = thresholds(*params)
    st = states(params[0], params[1], seed, first_block, blocks, N)
    u = symbol_words(seed, first_block, blocks, N, 6)
    wrong = u < np.where(st != 0, np.uint64(PB), np.uint64(PG))
    e = error_values(symbol_words(seed, first_block, blocks, N, 7), q_sym)
    s = np.zeros((blocks, N), np.int64) if sent is None else to_transmission_order(np.asarray(sent, np.int64), I)
    recv = np.where(wrong, s ^ e, s)
    shape = (blocks, n, I)
    return recv.astype(np.uint8).reshape(shape), s.astype(np.uint8).reshape(shape), st.reshape(shape), wrong.reshape(shape)
