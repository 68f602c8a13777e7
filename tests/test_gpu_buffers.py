"""The buffer contract of the core entry points -- cc_correct_soft_batch_dev, cc_correct_hard(_f32)_batch_dev,
cc_encode_batch_dev, cc_extract_batch_dev, cc_decode_hard_batch and the interleaved byte calls -- under the harness of
tests/guarded_buffers.py: buffers of exactly the stated extent at the least alignment of their element type, sentinel
guards round every output, poison round every input, every optional output absent in turn, two poisons.  The expected
arrays are the plain-C oracle's; every comparison is bit for bit.

Batch sizes sit on both sides of the unit a kernel hands to a wavefront or workgroup, and every case asserts the kernel or
route it is named for.  In every batch of two frames or more whose stop rule can fail, the oracle's own status array holds
both outcomes (asserted); a batch of one frame holds one, and O0 ("as shipped") never reports a failure."""
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from checkers import BCH, BM, EUKLID, O0, O1, O2, PGZ, RS, Oracle, WideOracle, awgn_llr
from guarded_buffers import check_call
from interleave_model import interleave

pytestmark = pytest.mark.gpu

HARD_TAGS = {PGZ: cc.peterson_gorenstein_zierler_tag, BM: cc.berlekamp_massey_tag, EUKLID: cc.euklid_tag}


@functools.lru_cache(maxsize=None)
def oracle(family, q, t, coding=0):
    return Oracle(family, q, t, coding=coding)


def lib():
    return capi.lib()


# ------------------------------------------------ soft decoding ------------------------------------------------
# name -> (q, t, tag, stop rule, oracle variant, alpha, iterations, what kernel_info must say, (low, high) Eb/N0 in dB)
SOFT = {
    "four-row": (8, 3, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "four-row", (0.0, 8.0)),
    "butterfly": (8, 3, lambda it: cc.self_correcting_1_min_sum_tag(it), O2, 3, 1.0, 5, "row-pipelined", (0.0, 8.0)),
    "single-O2": (8, 3, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 1, "minsum_diag_kernel", (0.0, 9.0)),
    "single-O0": (8, 3, lambda it: cc.min_sum_tag(it), O0, 0, 1.0, 1, "minsum_diag_kernel", (0.0, 9.0)),
    "g255_16": (8, 2, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_diag_kernel<K=16,", (0.0, 8.0)),
    "g255_32": (8, 4, lambda it: cc.normalized_min_sum_tag(it, (4, 5)), O1, 1, 0.8, 5, "minsum_diag_kernel<K=32,", (0.0, 9.0)),
    "g127": (7, 2, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "LPF=8", (0.0, 8.0)),
    "g63_12": (6, 2, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_diag_kernel<K=12,", (-2.0, 8.0)),
    "g63_24": (6, 4, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_diag_kernel<K=24,", (-2.0, 9.0)),
    "g31_20": (5, 5, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_diag_kernel<K=20,", (-3.0, 10.0)),
    "g15_8": (4, 2, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_diag_kernel<K=8,", (-4.0, 9.0)),
    "generic": (8, 5, lambda it: cc.min_sum_tag(it), O2, 0, 1.0, 5, "minsum_generic_kernel", (0.0, 9.0)),
    "generic-HBM": (8, 18, lambda it: cc.self_correcting_2_min_sum_tag(it), O2, 4, 1.0, 3, "[state in HBM]", (-2.0, 12.0)),
}
SOFT_CASES = [("four-row", 1), ("four-row", 15), ("four-row", 17), ("four-row", 67), ("butterfly", 17), ("single-O2", 17),
              ("single-O0", 17), ("g255_16", 5), ("g255_32", 5), ("g127", 1), ("g127", 31), ("g127", 33), ("g63_12", 9),
              ("g63_24", 9), ("g31_20", 9), ("g15_8", 9), ("generic", 3), ("generic", 65), ("generic-HBM", 3)]


def soft_frames(o, B, seed, levels):
    """B AWGN frames: every third word all-zero, the others random codewords; even frames at levels[0] dB (too noisy to
    decode), odd frames at levels[1] dB"""
    rng = np.random.default_rng(seed)
    cw = o.encode(rng.integers(0, 2, (B, o.l)).astype(np.uint8))
    cw[::3] = 0
    return np.concatenate([awgn_llr(rng, cw[f:f + 1], o.l / o.n, levels[f & 1]) for f in range(B)])


def erasure_lists(rng, B, n, most):
    """per frame 0 .. most distinct positions, ascending; none for the first and the last frame; CSR arrays"""
    per = [sorted(rng.choice(n, int(rng.integers(0, most + 1)), replace=False).tolist()) for _ in range(B)]
    per[0], per[-1] = [], []
    if not any(per):
        per[B // 2] = [n - 1]
    pos = np.array([e for er in per for e in er], np.uint16)
    off = np.concatenate([[0], np.cumsum([len(er) for er in per])]).astype(np.uint32)
    return per, pos, off


def both_outcomes(status, B, stop=O2):
    if B >= 2 and stop != O0:
        assert (status == capi.FRAME_OK).any() and (status == capi.FRAME_NOT_CONVERGED).any(), status


def soft_data(name, B, with_erasures=False):
    """(channel values, CSR erasures or None, the oracle's hard, L, iters, status) -- the oracle alone, no device"""
    q, t, _, stop, variant, alpha, iterations, _, levels = SOFT[name]
    o = oracle(BCH, q, t)
    y = soft_frames(o, B, 1000 * q + 10 * t + B, levels)
    csr, ye = None, y
    if with_erasures:
        per, pos, off = erasure_lists(np.random.default_rng(B), B, o.n, 4)
        csr, ye = (pos, off), y.copy()
        for f, er in enumerate(per):  # an erased position enters the decoder as channel value 0 (cyclic.h:259-262)
            ye[f, er] = 0.0
    return (y, csr) + o.minsum(variant, iterations, ye, alpha, 0.0, stop, fast=True)


def soft_check(code, y, csr, want, what):
    b, L, it, st = want
    B, n = y.shape
    inputs = {"llr": y}
    if csr is not None:
        inputs.update(erasures=csr[0], offsets=csr[1])
        assert csr[1].size == B + 1 and csr[0].size == csr[1][-1] > 0

    def call(p):
        return lib().cc_correct_soft_batch_dev(code._h, p["llr"], p.get("erasures"), p.get("offsets"), p["hard"], p["L"],
                                               p["iters"], p["status"], B, p["stream"])
    outputs = {"hard": (np.uint8, B * n), "L": (np.float32, B * n), "iters": (np.uint16, B), "status": (np.int32, B)}
    expected = {"hard": b, "L": L, "iters": it.astype(np.uint16), "status": st}
    check_call(call, inputs, outputs, expected, optional=("L", "iters", "status"), what=what)


def soft_code(name):
    q, t, tag, stop, _, _, iterations, kernel, _ = SOFT[name]
    code = cc.primitive_bch(q, cc.errors(t), tag(iterations), stop_rule=stop)
    assert kernel in code.kernel_info()["kernel"], (name, code.kernel_info()["kernel"])
    return code


@pytest.mark.parametrize("name,B", SOFT_CASES)
def test_soft_decoding(name, B):
    y, csr, b, L, it, st = soft_data(name, B)
    both_outcomes(st, B, SOFT[name][3])
    soft_check(soft_code(name), y, csr, (b, L, it, st), (name, B))


@pytest.mark.parametrize("name,B", [("four-row", 17), ("g127", 33)])
def test_soft_decoding_with_erasure_lists(name, B):
    y, csr, b, L, it, st = soft_data(name, B, with_erasures=True)
    both_outcomes(st, B)
    soft_check(soft_code(name), y, csr, (b, L, it, st), (name, B, "erasures"))


def any_matrix():
    """the 40 x 257 matrix and the noisy all-zero words of test_min_sum_free_function_any_matrix (same seed)"""
    rows, cols, density = 40, 257, 0.04
    rng = np.random.default_rng(rows * 1000 + cols)
    H = (rng.random((rows, cols)) < density).astype(np.uint8)
    H[2] = 0
    H[:, cols // 2] = 0
    y = (1.0 + 0.9 * rng.standard_normal((67, cols))).astype(np.float32)
    return H, y


def matrix_data():
    H, y = any_matrix()
    y = y[:5].copy()
    y[1::2] = 1.0 + (y[1::2] - 1.0) / 3.0  # the odd frames with a third of the noise: they decode within 5 iterations
    return H, y, Oracle.minsum_H(H, 0, 5, y, 1.0, 0.0, O2)


def test_soft_decoding_over_a_callers_matrix():
    H, y, want = matrix_data()
    both_outcomes(want[3], 5)
    dec = cc.min_sum_decoder(H, cc.min_sum_tag(5))
    assert dec.kernel_info()["kernel"].startswith("minsum_generic_kernel")
    soft_check(dec, y, None, want, "40 x 257")


def wide_data(H):
    """three frames of BCH(511,484): all-zero and random codewords of the 16-bit oracle, over the handle's matrix"""
    o = WideOracle(BCH, 9, 3, poly=0x211)
    rng = np.random.default_rng(511)
    cw = o.encode(rng.integers(0, 2, (3, o.l)).astype(np.uint16)).astype(np.uint8)
    cw[0] = 0
    assert not ((H.astype(np.int64) @ cw.T.astype(np.int64)) % 2).any()
    y = np.concatenate([awgn_llr(rng, cw[f:f + 1], o.l / o.n, (0.0, 8.0)[f & 1]) for f in range(3)])
    return y, Oracle.minsum_H(H, 0, 5, y, 1.0, 0.0, O2)


def test_soft_decoding_beyond_256_columns():
    code = cc.primitive_bch(9, cc.errors(3), cc.min_sum_tag(5), modular_polynomial=0x211)
    assert code.n == 511 and code.kernel_info()["kernel"].startswith("minsum_generic_kernel")
    y, want = wide_data(code.H())
    both_outcomes(want[3], 3)
    soft_check(code, y, None, want, "BCH(511,484)")


@pytest.mark.parametrize("kind", ["high", "trap"])
def test_two_pass_route(kind):
    """2^18 + 777 frames of the headline code, 20 iterations: launch_minsum_diag takes the two-pass route (L is null by
    necessity).  "high": the first pass finishes most frames and twopass_scatter_kernel brings the others back; "trap":
    the list overflows and the general kernel runs over everything.  Values against the oracle on 512 frames at a stride
    and the last 64; guards, the inputs and the two poisons over the whole batch."""
    import torch
    from test_gpu_twopass import FRAMES, batch
    o = oracle(BCH, 8, 3)
    code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
    assert "four-row" in code.kernel_info()["kernel"] and float(FRAMES) * o.n * o.k >= 1.5e9
    y = batch(kind, o.n, o.l / o.n)
    pick = np.unique(np.concatenate([np.arange(0, FRAMES, FRAMES // 512)[:512], np.arange(FRAMES - 64, FRAMES)]))
    b, _, it, st = o.minsum(0, 20, y[pick], 1.0, 0.0, O2, fast=True)
    both_outcomes(st, len(pick))
    if kind == "high":
        assert (it == 0).mean() > 0.9 and (it > 0).any()
    idx = torch.from_numpy(pick).cuda()

    def sampled(want, width):
        def check(view, label):
            got = view.view(FRAMES, width)[idx].cpu().numpy().reshape(want.shape)
            assert np.array_equal(got.view(want.dtype), want), label
        return check
    B, n = FRAMES, o.n

    def call(p):
        return lib().cc_correct_soft_batch_dev(code._h, p["llr"], None, None, p["hard"], p["L"], p["iters"], p["status"], B,
                                               p["stream"])
    outputs = {"hard": (np.uint8, B * n), "L": (np.float32, B * n), "iters": (np.uint16, B), "status": (np.int32, B)}
    expected = {"hard": sampled(b, n), "iters": sampled(it.astype(np.uint16), 1), "status": sampled(st, 1)}
    check_call(call, {"llr": y}, outputs, expected, optional=("iters", "status"), absent=("L",), what=("two-pass", kind))


# ------------------------------------------------ hard decoding ------------------------------------------------
def symbol_type(o):
    """bytes up to GF(2^8), 16-bit symbols beyond (the _u16 entry points)"""
    return np.uint16 if o.q > 8 else np.uint8


def corrupted(o, B, seed):
    """B codewords with 0 .. t + 2 symbol errors each (test_in_place_calls); the first frame is clean"""
    from test_gpu_algebraic import corrupt
    rng = np.random.default_rng(seed)
    hi = 2 if o.family == BCH else 1 << o.q
    cw = o.encode(rng.integers(0, hi, (B, o.l)).astype(symbol_type(o))).astype(symbol_type(o))
    ne = rng.integers(0, o.t + 3, B)
    ne[0] = 0
    if B >= 2:
        ne[1] = o.t + 2
    return np.stack([corrupt(rng, o, cw[f], int(ne[f])) for f in range(B)])


def hard_expected(o, alg, rx, per=None):
    """The oracle's answer in the form of the header: out = the corrected word, the (hard-decided) input where the frame
    fails; nerr = the count, -1 where it fails; status = the oracle's (check_against_oracle, test_gpu_algebraic.py).
    o: checkers.Oracle, or a model that takes one erasure list per frame (checkers.WideOracle, shortened_model.Shortened)."""
    B = rx.shape[0]
    if per is None:
        out, nerr, st = o.correct_hard(alg, rx)[:3]
    elif isinstance(o, Oracle):
        rows = [o.correct_hard(alg, rx[f], per[f]) for f in range(B)]
        out, nerr, st = (np.concatenate([r[i] for r in rows]) for i in range(3))
    else:
        out, nerr, st = o.correct_hard(alg, rx, per)[:3]
    sym = (rx < 0).astype(np.uint8) if rx.dtype == np.float32 else rx
    ok = st == 0
    return (np.where(ok[:, None], out, sym).astype(symbol_type(o)), np.where(ok, nerr, -1).astype(np.int32),
            st.astype(np.int32))


def status_check(st, exact):
    """The failure class (root count against re-check) is defined algorithm for algorithm only for the BM tag and for the
    two-trial rule: "only WHICH failure text a hopeless frame gets may differ" (channelcoding_amd.h, CC_ALG_EUKLID, and
    check_against_oracle).  Elsewhere: the same frames fail, and every call of the case returns the same words."""
    if exact:
        return st
    seen = []

    def check(view, label):
        got = view.cpu().numpy().view(np.int32)
        assert np.array_equal(got != 0, st != 0) and ((got >= 0) & (got <= capi.FRAME_ERASURES)).all(), label
        seen.append(got)
        assert np.array_equal(got, seen[0]), label
    return check


def hard_check(code, alg, rx, want, what, csr=None, exact=None, in_place=False):
    out, nerr, st = want
    B, n = rx.shape
    fn = lib().cc_correct_hard_f32_batch_dev if rx.dtype == np.float32 else lib().cc_correct_hard_batch_dev
    inputs = {"in": rx}
    if csr is not None:
        inputs.update(erasures=csr[0], offsets=csr[1])
        assert csr[1].size == B + 1 and csr[0].size == csr[1][-1] > 0

    def call(p):
        return fn(code._h, p["in"], p.get("erasures"), p.get("offsets"), p["out"], p["nerr"], p["status"], B, p["stream"])
    outputs = {"out": (np.uint8, B * n), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"out": out, "nerr": nerr, "status": status_check(st, alg == BM if exact is None else exact)}
    return check_call(call, inputs, outputs, expected, optional=("nerr", "status"), what=what,
                      in_place={"out": "in"} if in_place else None)


def hard_outcomes(st, B):
    if B >= 2:
        assert (st == 0).any() and (st != 0).any(), st


def hard_code(family, q, t, alg):
    return (cc.primitive_bch if family == BCH else cc.rs)(q, cc.errors(t), HARD_TAGS[alg]())


WAVE, CHUNK, PLANES, LONG, TRIALS = (capi.HARD_ROUTE_WAVE, capi.HARD_ROUTE_CHUNK, capi.HARD_ROUTE_PLANES,
                                     capi.HARD_ROUTE_LONG, capi.HARD_ROUTE_TRIALS)
HARD_CASES = ([(WAVE, BCH, 6, 3, BM, B) for B in (1, 5)] +
              [(CHUNK, RS, 6, 8, alg, B) for alg in (BM, PGZ) for B in (31, 33)] +
              [(PLANES, RS, 8, 16, BM, B) for B in (1, 33, 255, 257)] +
              [(PLANES, BCH, 8, 3, EUKLID, B) for B in (1, 33, 255, 257)] +
              [(LONG, RS, 8, 40, BM, 5)])


@pytest.mark.parametrize("route,family,q,t,alg,B", HARD_CASES)
def test_hard_decoding(route, family, q, t, alg, B):
    o = oracle(family, q, t)
    code = hard_code(family, q, t, alg)
    assert code.hard_route(B) == route
    rx = corrupted(o, B, 100 * q + t + B)
    want = hard_expected(o, alg, rx)
    hard_outcomes(want[2], B)
    hard_check(code, alg, rx, want, (route, family, q, t, alg, B))


def test_hard_decoding_of_signed_values():
    """cc_correct_hard_f32_batch_dev on the plane chain: bit = (x < 0), so +0.0 and -0.0 both decide for 0"""
    o = oracle(BCH, 8, 3)
    code = hard_code(BCH, 8, 3, BM)
    B = 33
    assert code.hard_route(B) == PLANES
    bits = corrupted(o, B, 833)
    rng = np.random.default_rng(834)
    zero = np.array([1.0, 0.0, -0.0], np.float32)[rng.integers(0, 3, bits.shape)]
    y = np.where(bits == 1, np.float32(-1.0), zero).astype(np.float32)
    assert np.signbit(y[bits == 0]).any() and (y == 0).any() and np.array_equal((y < 0).astype(np.uint8), bits)
    want = hard_expected(o, BM, y)
    hard_outcomes(want[2], B)
    hard_check(code, BM, y, want, "f32")


def erased(o, B, seed, most):
    """codewords with 0 .. most erased (zeroed) positions and errors up to one beyond what then can be corrected"""
    rng = np.random.default_rng(seed)
    hi = 2 if o.family == BCH else 1 << o.q
    rx = o.encode(rng.integers(0, hi, (B, o.l)).astype(symbol_type(o))).astype(symbol_type(o))
    per, pos, off = erasure_lists(rng, B, o.n, most)
    for f, er in enumerate(per):
        rx[f, er] = 0
        free = np.setdiff1d(np.arange(o.n), er)
        ne = 0 if f == 0 else (2 * o.t - len(er)) // 2 + 2 if f == 1 else int(rng.integers(0, (2 * o.t - len(er)) // 2 + 2))
        for p in rng.choice(free, ne, replace=False):
            rx[f, p] ^= 1 if o.family == BCH else int(rng.integers(1, hi))
    return rx, per, (pos, off)


@pytest.mark.parametrize("alg", [BM, EUKLID])
def test_hard_decoding_with_erasures_on_the_plane_chain(alg):
    """RS(255,223), 0 .. 6 erased positions per frame: the chain with the BM tag; with Euklid the chain first, then
    Sugiyama over the frames it leaves, reading the chain's status from workspace when the caller passes none"""
    o = oracle(RS, 8, 16)
    code = hard_code(RS, 8, 16, alg)
    B = 65
    assert code.hard_route(B, True) == PLANES
    rx, per, csr = erased(o, B, 6500 + alg, 6)
    want = hard_expected(o, alg, rx, per)
    hard_outcomes(want[2], B)
    hard_check(code, alg, rx, want, ("planes + erasures", alg), csr=csr)


def two_trials_batch(B=9):
    """BCH(63,45) words for the two-trial rule: (oracle, received words, erasure lists, CSR)"""
    o = oracle(BCH, 6, 3)
    rng = np.random.default_rng(909)
    rx = o.encode(rng.integers(0, 2, (B, o.l)).astype(np.uint8))
    per, pos, off = erasure_lists(rng, B, o.n, 7)
    per[1] = sorted(rng.choice(o.n, 7, replace=False).tolist())  # more than 2t: CC_FRAME_ERASURES
    pos = np.array([e for er in per for e in er], np.uint16)
    off = np.concatenate([[0], np.cumsum([len(er) for er in per])]).astype(np.uint32)
    for f in range(B):
        for p in rng.choice(o.n, int(rng.integers(0, 4)), replace=False):
            rx[f, p] ^= 1
    return o, rx, per, (pos, off)


def test_hard_decoding_by_two_trials():
    """BCH(63,45), PGZ tag with erasures (bch.h:97-149): workspace stands in for the count and status the caller leaves out"""
    code = hard_code(BCH, 6, 3, PGZ)
    B = 9
    assert code.hard_route(B, True) == TRIALS
    o, rx, per, csr = two_trials_batch(B)
    want = hard_expected(o, PGZ, rx, per)
    hard_outcomes(want[2], B)
    hard_check(code, PGZ, rx, want, "two trials", csr=csr, exact=True)


def test_hard_decoding_by_two_trials_in_place():
    """out == in: the first trial decodes a copy in workspace, so a frame that fails (here: more than 2t erasures) still
    returns the word received -- with what it held at the erased positions, which the trials overwrite"""
    code = hard_code(BCH, 6, 3, PGZ)
    B = 9
    assert code.hard_route(B, True) == TRIALS
    o, rx, per, csr = two_trials_batch(B)
    want = hard_expected(o, PGZ, rx, per)
    hard_outcomes(want[2], B)
    assert any(want[2][f] != 0 and rx[f, per[f]].any() for f in range(B) if per[f]) and (want[0] != rx).any()
    hard_check(code, PGZ, rx, want, "two trials in place", csr=csr, exact=True, in_place=True)


@pytest.mark.parametrize("route,family,q,t,B", [(PLANES, RS, 8, 16, 257), (WAVE, BCH, 6, 3, 5)])
def test_hard_decoding_in_place(route, family, q, t, B):
    """out == in: one guarded buffer, the answers of the out-of-place call (the oracle's), the bytes round it intact"""
    o = oracle(family, q, t)
    code = hard_code(family, q, t, BM)
    assert code.hard_route(B) == route
    rx = corrupted(o, B, 100 * q + t + B)
    want = hard_expected(o, BM, rx)
    hard_outcomes(want[2], B)
    hard_check(code, BM, rx, want, ("in place", route, B), in_place=True)


# ------------------------------------------------ encode, extract, decode ------------------------------------------------
def messages(o, B, seed):
    """random field elements; the first message all zero, the second all 2^q - 1"""
    top = (1 << o.q) - 1
    msg = np.random.default_rng(seed).integers(0, top + 1, (B, o.l)).astype(symbol_type(o))
    msg[0] = 0
    if B >= 2:
        msg[1] = top
    return msg


def map_check(code, fn, src, want, what, tail=()):
    B = src.shape[0] if not tail else src.shape[0] * tail[0]

    def call(p):
        return fn(code._h, p["src"], p["dst"], B, *tail, p["stream"])
    check_call(call, {"src": src}, {"dst": (want.dtype, want.size)}, {"dst": want}, what=what)


# how launch_encode (csrc/encode.hip) chooses: the GF(2^8) interpolation encoder where bitslice_encode_supported, which
# interleaved_map_route(0, 2) reports; else c = a g for the multiplication tag; else bit planes for a BCH code with at
# most 32 parity symbols; else the division kernel with its table in LDS
def encoder_of(code):
    if code.interleaved_map_route(0, 2) == 1:
        return "bitslice_parity_kernel"
    if code._desc.coding == capi.CODING_MULTIPLICATION:
        return "encode_multiplication_kernel"
    return "encode_bch_planes_kernel" if code.family == capi.FAMILY_BCH and code.k <= 32 else "encode_division_kernel"


ENCODE_CASES = ([("encode_bch_planes_kernel", BCH, q, t, B) for q, t in ((8, 3), (4, 3)) for B in (1, 5)] +
                [("encode_division_kernel", family, q, t, B) for family, q, t in ((BCH, 8, 5), (RS, 4, 3)) for B in (1, 5)] +
                [("bitslice_parity_kernel", RS, 8, t, B) for t in (16, 8) for B in (1, 33, 257)])


@pytest.mark.parametrize("kernel,family,q,t,B", ENCODE_CASES)
def test_encode(kernel, family, q, t, B):
    o = oracle(family, q, t)
    code = hard_code(family, q, t, BM)
    assert encoder_of(code) == kernel and (code.n, code.l) == (o.n, o.l)
    msg = messages(o, B, 10 * q + t)
    map_check(code, lib().cc_encode_batch_dev, msg, o.encode(msg), (kernel, q, t, B))


@pytest.mark.parametrize("family,q,t", [(BCH, 6, 3), (RS, 4, 3)])
def test_multiplication_coding(family, q, t):
    """c = a g and a = b / g (cyclic.h:29-33, :42-46), extraction also of words that are not codewords"""
    o = oracle(family, q, t, 1)
    code = (cc.primitive_bch if family == BCH else cc.rs)(q, cc.errors(t), cc.berlekamp_massey_tag(), coding="multiplication")
    assert encoder_of(code) == "encode_multiplication_kernel"
    B = 5
    msg = messages(o, B, 50 + q)
    cw = o.encode(msg)
    map_check(code, lib().cc_encode_batch_dev, msg, cw, ("multiplication encode", q))
    words = cw.copy()
    words[2:] = np.random.default_rng(60 + q).integers(0, o.n + 1, (B - 2, o.n))
    assert o.syndromes(words[2]).any()
    map_check(code, lib().cc_extract_batch_dev, words, o.extract(words), ("multiplication extract", q))


@pytest.mark.parametrize("B", [5, 257])
def test_extract(B):
    o = oracle(RS, 8, 16)
    code = hard_code(RS, 8, 16, BM)
    assert code._desc.coding == capi.CODING_DIVISION  # extract_division_kernel
    words = np.random.default_rng(B).integers(0, 256, (B, o.n)).astype(np.uint8)
    map_check(code, lib().cc_extract_batch_dev, words, o.extract(words), ("extract", B))


@pytest.mark.parametrize("family,q,t", [(RS, 8, 16), (BCH, 6, 3)])
def test_decode_is_correct_and_extract(family, q, t):
    """cc_decode_hard_batch (host pointers): words absent and present"""
    o = oracle(family, q, t)
    code = hard_code(family, q, t, BM)
    B = 33
    assert code.hard_route(B) == (PLANES if q == 8 else WAVE)
    rx = corrupted(o, B, 33 + q)
    out, nerr, st = hard_expected(o, BM, rx)
    hard_outcomes(st, B)

    def call(p):
        return lib().cc_decode_hard_batch(code._h, p["in"], None, None, p["msg"], p["words"], p["nerr"], p["status"], B)
    outputs = {"msg": (np.uint8, B * o.l), "words": (np.uint8, B * o.n), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"msg": o.extract(out), "words": out, "nerr": nerr, "status": st}
    check_call(call, {"in": rx}, outputs, expected, optional=("words",), device="cpu", what=("decode", q))


# ------------------------------------------------ interleaved byte calls ------------------------------------------------
@pytest.mark.parametrize("I,m", [(I, m) for I in (2, 16, 33) for m in (1, 3)])
def test_interleaved_calls(I, m):
    """RS(255,223), BM: 2-byte and 16-byte runs of the native route, depth 33 on the generic one"""
    o = oracle(RS, 8, 16)
    code = hard_code(RS, 8, 16, BM)
    B = I * m
    native = 1 if I <= 16 else 0
    assert code.interleaved_route(B, I) == native and code.interleaved_map_route(0, I) == native
    msg = messages(o, B, 7 * I + m)
    map_check(code, lib().cc_encode_interleaved_batch_dev, interleave(msg, I), interleave(o.encode(msg), I),
              ("interleaved encode", I, m), tail=(I,))
    rx = corrupted(o, B, 9 * I + m)
    out, nerr, st = hard_expected(o, BM, rx)
    hard_outcomes(st, B)

    def call(p):
        return lib().cc_correct_hard_interleaved_batch_dev(code._h, p["in"], None, None, p["out"], p["nerr"], p["status"],
                                                           B, I, p["stream"])
    outputs = {"out": (np.uint8, B * o.n), "nerr": (np.int32, B), "status": (np.int32, B)}
    expected = {"out": interleave(out, I), "nerr": nerr, "status": st}
    check_call(call, {"in": interleave(rx, I)}, outputs, expected, optional=("nerr", "status"),
               what=("interleaved correct", I, m))
