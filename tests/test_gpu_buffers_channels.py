"""The buffer contract of the channel-only calls -- cc_awgn_llr_dev, cc_awgn_symbols_dev, cc_awgn_product_dev,
cc_discrete_channel_dev, cc_burst_channel_dev, cc_burst_erasure_channel_dev, cc_bsc_packed_channel_dev -- and of the
counters of the Monte-Carlo calls (the first eight and the four routes added since), under the harness of
tests/guarded_buffers.py: every output of exactly the stated extent at the least alignment of its element type, between
sentinel guards, every subset of the optional outputs absent in turn.  These calls read no caller buffer, so there is no
poison to compare.

Expected values: the discrete, burst and packed outputs are bit for bit those of the host models (test_discrete_host,
burst_model, burst_erasure_model, cc.pack_bits of the discrete model), the words sent the plain-C oracle's encoding of the
model's message symbols.  The AWGN floats come from the hardware approximations: they lie within tau(sigma) of
awgn_reference (test_gpu_mc.py), agree in sign outside that band and equal, byte for byte, the same call made into an
ordinary torch tensor -- a frame depends on (seed, global frame index) alone, so the address must not show.

Batches: 1 and 5 frames (blocks, for the burst channels) everywhere; per kernel one batch on the code with the most lanes
per frame that makes the grid take a second grid-stride trip (frames > num_cus 8 256 / G), checked on the first 200 frames,
200 frames round the trip boundary and the last 200 where the model would take more than about a second; 1029 frames
for the two calls that return an erasure CSR (the scan works in tiles of 1024 frames); and every call once with no frames.
An erasure list's capacity is frames n: the entries from off[frames] on are not written (they are still SENTINEL), and
with every symbol erased or flagged the list fills the buffer to its last element."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import burst_erasure_model
import burst_model
import shortened_model as S
from awgn_model import awgn_reference
from checkers import BCH, BM, RS, WideOracle
from guarded_buffers import SENTINEL, check_call
from test_discrete_host import bch_message_bits, channel as discrete_model, erasure_csr, rs_message_symbols
from test_gpu_burst import PARAMS
from test_gpu_burst_erasure import DETECTORS
from test_gpu_mc import sigma_f32, tau

pytestmark = pytest.mark.gpu

SEED, FIRST = 0x1234567890AB, (1 << 33) - 3  # (the low word of the frame index wraps inside a batch of five)
EBNO = 3.0
BURSTY, TYPICAL, ALL = PARAMS[0], DETECTORS[0], DETECTORS[3]
assert BURSTY == (0.02, 0.25, 0.001, 0.5) and TYPICAL == (0.9, 0.002) and ALL == (1.0, 1.0)


def lib():
    return capi.lib()


def is_rs(code):
    return code.family == capi.FAMILY_RS


def q_sym(code):
    return 1 << code.q if is_rs(code) else 2


@functools.lru_cache(maxsize=None)
def model_of(family, q, t, N, poly):
    o = WideOracle(family, q, t, poly or 0)
    return S.Shortened(o, N) if N and N != o.n else o


@functools.lru_cache(maxsize=None)
def _words(family, q, t, N, poly, seed, first, frames):
    o = model_of(family, q, t, N, poly)
    msg = rs_message_symbols(seed, first, frames, o.l, q) if family == RS else bch_message_bits(seed, first, frames, o.l)
    words = o.encode(msg.astype(np.uint16))
    words.setflags(write=False)
    return words


def sent_words(code, seed, first, frames, random_cw, poly=None):
    """the words of frames [first, first + frames): the plain-C oracle's encoding of the model's messages, or zeros"""
    if not random_cw:
        return np.zeros((frames, code.n), np.uint16 if code.q > 8 else np.uint8)
    full = code.n == (1 << code.q) - 1
    words = _words(RS if is_rs(code) else BCH, code.q, code.t, None if full else code.n, poly, seed, first, frames)
    return words if code.q > 8 else words.astype(np.uint8)


def lanes(symbols):
    """the G of the channel kernels: the smallest power of two with 4 G >= symbols"""
    g = 1
    while 4 * g < symbols:
        g *= 2
    return g


def second_trip(G):
    """a batch (of frames, or of blocks) a little beyond what one pass of the largest grid, 8 workgroups of 256 lanes per
    compute unit, covers at G lanes each"""
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return cus * 8 * 256 // G + 9


def spans(frames, boundary=None):
    """the whole batch, or with a trip boundary the first 200 frames, 200 round the boundary and the last 200"""
    if boundary is None or frames <= 600:
        return [(0, frames)]
    assert 300 < boundary < frames
    if frames - 200 <= boundary + 100:  # the trip's second pass is short: one span from before the boundary to the end
        return [(0, 200), (min(boundary - 100, frames - 200), frames)]
    return [(0, 200), (boundary - 100, boundary + 100), (frames - 200, frames)]


def plain(call, outputs):
    """the same call into ordinary torch tensors: name -> the bytes written"""
    import torch
    from guarded_buffers import _torch_dtype
    t = {k: torch.zeros(count, dtype=_torch_dtype(torch, dt), device="cuda") for k, (dt, count) in outputs.items()}
    p = {k: C.c_void_p(v.data_ptr()) for k, v in t.items()}
    p["stream"] = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    capi.check(call(p), "plain")
    torch.cuda.synchronize()
    return {k: v.view(torch.uint8).cpu().numpy() for k, v in t.items()}


def listed(vals, frames, n):
    """an erasure list in its buffer of capacity frames n: the values, and nothing written behind them"""
    vals = np.asarray(vals).astype(np.uint16)

    def check(view, label):
        got = view.cpu().numpy().view(np.uint16)
        assert got.size == frames * n and np.array_equal(got[:vals.size], vals), (label, "the list")
        assert (got[vals.size:].view(np.uint8) == SENTINEL).all(), (label, "entries behind off[frames] were written")
    return check


# ------------------------------------------------ AWGN, binary ------------------------------------------------
def awgn_values(n, sigma, seed, first, frames, bits, same, where):
    """the checker of frames x n channel values; bits(lo, hi): what frames lo .. hi - 1 sent, (hi - lo, n)"""
    t = tau(sigma)

    def check(view, label):
        y = view.cpu().numpy().view(np.float32).reshape(frames, n)
        assert np.array_equal(y.view(np.uint8).reshape(-1), same), (label, "differs from the call into a plain tensor")
        for lo, hi in where:
            ref = awgn_reference(n, sigma, seed, first + lo, hi - lo, bits(lo, hi))
            err = np.abs(y[lo:hi] - ref)
            assert err.max() <= t, (label, lo, float(err.max()), t)
            sure = np.abs(ref) > t
            assert np.array_equal((y[lo:hi] < 0)[sure], (ref < 0)[sure]), (label, lo, "signs")
    return check


AWGN = {"bch7": (3, 1, None, cc.berlekamp_massey_tag), "bch63-ms": (6, 3, None, lambda: cc.min_sum_tag(5)),
        "bch255": (8, 3, None, cc.berlekamp_massey_tag), "bch200": (8, 3, 200, cc.berlekamp_massey_tag)}


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("name", list(AWGN))
def test_awgn_llr(name, random_cw):
    """G = 2 with a 3-value tail, G = 16 and 64 with one, n = 200 without; awgn_kernel's second trip at G = 64"""
    q, t, N, tag = AWGN[name]
    code = cc.primitive_bch(q, cc.errors(t), tag(), n=N)
    n, sigma = code.n, sigma_f32(code, EBNO)
    assert (n % 4 == 0) == (name == "bch200") and code.algorithm.soft == (name == "bch63-ms")
    trip = second_trip(lanes(n))
    for B in (1, 5) + ((trip,) if name == "bch255" else ()):
        sent = sent_words(code, SEED, FIRST, B, random_cw)
        assert bool(sent.any()) == random_cw

        def call(p):
            return lib().cc_awgn_llr_dev(code._h, EBNO, SEED, FIRST, B, int(random_cw), p["llr"], p["sent"], p["stream"])
        same = plain(call, {"llr": (np.float32, B * n), "sent": (np.uint8, B * n)})
        expected = {"llr": awgn_values(n, sigma, SEED, FIRST, B, lambda lo, hi: sent[lo:hi], same["llr"], [(0, B)]),
                    "sent": sent}
        check_call(call, {}, {"llr": (np.float32, B * n), "sent": (np.uint8, B * n)}, expected, optional=("sent",),
                   what=(name, B, random_cw))


# ------------------------------------------------ AWGN, symbols ------------------------------------------------
def bits_of(sym, q):
    return ((sym[:, :, None] >> np.arange(q, dtype=np.uint8)[None, None, :]) & 1).reshape(sym.shape[0], -1).astype(np.uint8)


def symbol_checks(code, sigma, seed, first, frames, sent, same, where):
    """the check of test_gpu_gmd.py on w and rel: rel within the band of the smallest |y| of the symbol's bits and not
    negative, w the model's hard decisions wherever every bit of the symbol is outside the band"""
    n, q, t = code.n, code.q, tau(sigma)
    ref = {}

    def model(lo, hi):
        if (lo, hi) not in ref:
            ref[lo, hi] = awgn_reference(n * q, sigma, seed, first + lo, hi - lo, bits_of(sent[lo:hi], q)).reshape(-1, n, q)
        return ref[lo, hi]

    def words(view, label):
        w = view.cpu().numpy().reshape(frames, n)
        assert np.array_equal(w.reshape(-1), same["words"]), (label, "differs from the call into a plain tensor")
        for lo, hi in where:
            y = model(lo, hi)
            sure = (np.abs(y) > t).all(axis=2)
            w_ref = ((y < 0).astype(np.uint32) << np.arange(q, dtype=np.uint32)).sum(axis=2).astype(np.uint8)
            assert np.array_equal(w[lo:hi][sure], w_ref[sure]), (label, lo)
            assert (~sure).mean() <= 1e-3 or hi - lo < 100, (label, lo)

    def rel(view, label):
        r = view.cpu().numpy().view(np.float32).reshape(frames, n)
        assert np.array_equal(r.view(np.uint8).reshape(-1), same["rel"]), (label, "differs from the call into a plain tensor")
        assert (r >= 0).all(), label
        for lo, hi in where:
            err = np.abs(r[lo:hi].astype(np.float64) - np.abs(model(lo, hi)).min(axis=2))
            assert err.max() <= t, (label, lo, float(err.max()), t)
    return words, rel


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("q,t", [(3, 2), (4, 3), (8, 8)], ids=["rs7-3", "rs15-9", "rs255-239"])
def test_awgn_symbols(q, t, random_cw):
    """awgn_symbols_kernel: a group of 8, 16 and 256 lanes per frame; with 256 a second trip beyond num_cus 8 frames"""
    code = cc.rs(q, cc.errors(t), cc.berlekamp_massey_tag())
    n, sigma = code.n, sigma_f32(code, EBNO)
    trip = second_trip(256)
    for B in (1, 5) + ((trip,) if q == 8 else ()):
        sent = sent_words(code, SEED, FIRST, B, random_cw)
        assert bool(sent.any()) == random_cw

        def call(p):
            return lib().cc_awgn_symbols_dev(code._h, EBNO, SEED, FIRST, B, int(random_cw), p["words"], p["rel"], p["sent"],
                                             p["stream"])
        outputs = {"words": (np.uint8, B * n), "rel": (np.float32, B * n), "sent": (np.uint8, B * n)}
        words, rel = symbol_checks(code, sigma, SEED, FIRST, B, sent, plain(call, outputs), spans(B, trip - 9 if B == trip else None))
        check_call(call, {}, outputs, {"words": words, "rel": rel, "sent": sent}, optional=("sent",), what=(q, t, B, random_cw))


# ------------------------------------------------ AWGN, product blocks ------------------------------------------------
PRODUCTS = {"7x7": ((3, 1), (3, 1), False), "15x7": ((4, 1), (3, 1), False), "e8x8": ((3, 1), (3, 1), True)}


def product_of(name):
    (rq, rt), (cq, ct), extended = PRODUCTS[name]
    mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())  # noqa: E731
    return cc.product_code(mk(rq, rt), mk(cq, ct), extended=extended)


def product_blocks(name, seed, first, blocks, random_cw):
    """the blocks sent: the message bits of frame g of a code with l = k1 k2, rows encoded (and extended), then columns"""
    import chase_model as M
    from test_gpu_product import encode_blocks
    (rq, rt), (cq, ct), extended = PRODUCTS[name]
    rows, cols = M.decoder(rq, rt), M.decoder(cq, ct)
    e = 1 if extended else 0
    if not random_cw:
        return np.zeros((blocks, cols.n + e, rows.n + e), np.uint8)
    msg = bch_message_bits(seed, first, blocks, rows.l * cols.l).reshape(blocks, cols.l, rows.l)
    return encode_blocks(rows, cols, msg, extended)


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("name", list(PRODUCTS))
def test_awgn_product(name, random_cw):
    """N = 49 and 105 (odd: a ragged tail and every second block at 4 mod 8), N = 64; the second trip at N = 105, G = 32"""
    pc = product_of(name)
    N, sigma = pc.n, float(np.float32(pc.sigma(EBNO)))
    assert (pc.n1, pc.n2, N) == {"7x7": (7, 7, 49), "15x7": (15, 7, 105), "e8x8": (8, 8, 64)}[name]
    desc = pc._pc()
    trip = second_trip(lanes(N))
    for B in (1, 5) + ((trip,) if name == "15x7" else ()):
        where = spans(B, trip - 9 if B == trip else None)  # (the model's encoder takes seconds for the whole trip batch)
        parts = [product_blocks(name, SEED, FIRST + lo, hi - lo, random_cw).reshape(hi - lo, N) for lo, hi in where]
        assert all(bool(part.any()) == random_cw for part in parts)

        def call(p):
            return lib().cc_awgn_product_dev(C.byref(desc), EBNO, SEED, FIRST, B, int(random_cw), p["y"], p["sent"], p["stream"])
        outputs = {"y": (np.float32, B * N), "sent": (np.uint8, B * N)}
        same = plain(call, outputs)
        expected = {"y": awgn_values(N, sigma, SEED, FIRST, B, lambda lo, hi: parts[where.index((lo, hi))], same["y"], where),
                    "sent": sampled(parts, where, N)}
        check_call(call, {}, outputs, expected, optional=("sent",), what=(name, B, random_cw))


# ------------------------------------------------ discrete memoryless channels ------------------------------------------------
DISCRETE = {"bch7": lambda: cc.primitive_bch(3, cc.errors(1), cc.berlekamp_massey_tag()),
            "bch63": lambda: cc.primitive_bch(6, cc.errors(3), cc.berlekamp_massey_tag()),
            "rs15": lambda: cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag()),
            "rs223": lambda: cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag()),
            "rs204": lambda: cc.rs(8, cc.errors(8), cc.berlekamp_massey_tag(), n=204)}
POINTS = [(0.03, 0.05), (0.02, 0.0), (0.0, 1.0)]


def discrete_case(code, p, e, B, random_cw, what):
    n = code.n
    sent = sent_words(code, SEED, FIRST, B, random_cw)
    recv, erased, wrong = discrete_model(p, e, SEED, FIRST, B, n, q_sym(code), sent)
    vals, off = erasure_csr(erased)
    if (p, e) == (0.0, 1.0):  # every symbol erased: the list fills its capacity to the last element
        assert vals.size == B * n and np.array_equal(off, np.arange(B + 1) * n) and not recv.any()
    if e == 0:
        assert vals.size == 0 and not off.any()

    def call(q):
        return lib().cc_discrete_channel_dev(code._h, p, e, SEED, FIRST, B, int(random_cw), q["recv"], q["erasures"],
                                             q["offsets"], q["sent"], q["stream"])
    outputs = {"recv": (np.uint8, B * n), "erasures": (np.uint16, B * n), "offsets": (np.uint32, B + 1),
               "sent": (np.uint8, B * n)}
    expected = {"recv": recv, "erasures": listed(vals, B, n), "offsets": off.astype(np.uint32), "sent": sent}
    # the header allows a NULL list only where no erasure can be drawn
    check_call(call, {}, outputs, expected, optional=("sent",) + ((("erasures", "offsets"),) if e == 0 else ()), what=what)


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("name", list(DISCRETE))
def test_discrete_channel(name, random_cw):
    """G = 2 .. 64 lanes per frame, with a tail (n = 7, 63, 15, 255) and without (n = 204); 1029 frames: a second tile of
    the list's scan; discrete_kernel's and discrete_positions_kernel's second trip on RS(255,223), G = 64"""
    code = DISCRETE[name]()
    for p, e in POINTS:
        for B in (1, 5):
            discrete_case(code, p, e, B, random_cw, (name, p, e, B, random_cw))
    if name in ("bch7", "rs15"):
        for p, e in (POINTS[0], POINTS[2]):
            discrete_case(code, p, e, 1029, random_cw, (name, p, e, 1029, random_cw))
    if name == "rs223":
        B = second_trip(lanes(code.n))
        discrete_case(code, *POINTS[0], B, random_cw, (name, "second trip", B, random_cw))


# ------------------------------------------------ burst channels ------------------------------------------------
BURST = {"rs7-I3": (lambda: cc.rs(3, cc.errors(2), cc.berlekamp_massey_tag()), 3),          # N = 21: a 1-symbol tail
         "rs15-I1": (lambda: cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag()), 1),         # depth 1: the dword branch
         "rs239-I2": (lambda: cc.rs(8, cc.errors(8), cc.berlekamp_massey_tag()), 2),        # N = 510: two passes, 2-symbol tail
         "bch63-I16": (lambda: cc.primitive_bch(6, cc.errors(3), cc.berlekamp_massey_tag()), 16)}  # N = 1008: four passes


def burst_spans(blocks, I, trip):
    """spans() in whole blocks, as frame ranges"""
    return [(lo * I, hi * I) for lo, hi in spans(blocks, trip)] if blocks * I > 600 else [(0, blocks * I)]


def sampled(want, where, width):
    """the bytes of the frame (or symbol) ranges `where` of a buffer of `width` bytes per frame"""
    def check(view, label):
        got = view.cpu().numpy()
        for (lo, hi), w in zip(where, want):
            assert np.array_equal(got[lo * width: hi * width], np.asarray(w, np.uint8).reshape(-1)), (label, lo)
    return check


def burst_case(code, I, blocks, random_cw, det, what, trip=None):
    """det None: cc_burst_channel_dev; else cc_burst_erasure_channel_dev with that detector"""
    n, frames = code.n, blocks * I
    first = FIRST // I * I
    where = burst_spans(blocks, I, trip)
    parts = []
    for lo, hi in where:
        sent = sent_words(code, SEED, first + lo, hi - lo, random_cw)
        base = burst_model.channel(BURSTY, I, SEED, first + lo, hi - lo, n, q_sym(code), sent if random_cw else None)
        parts.append(base if det is None else
                     burst_erasure_model.channel(BURSTY, det, I, SEED, first + lo, hi - lo, n, q_sym(code), base=base))
    whole = where == [(0, frames)]
    pick = (lambda i: parts[0][i].reshape(-1)) if whole else (lambda i: sampled([p[i] for p in parts], where, n))
    chan = capi.BurstChannel(I, *BURSTY)
    outputs = {"recv": (np.uint8, frames * n), "sent": (np.uint8, frames * n), "state": (np.uint8, frames * n)}
    expected = {"recv": pick(0), "sent": pick(1), "state": pick(2)}
    if det is None:
        def call(p):
            return lib().cc_burst_channel_dev(code._h, C.byref(chan), SEED, first, frames, int(random_cw), p["recv"], p["sent"],
                                              p["state"], p["stream"])
        return check_call(call, {}, outputs, expected, optional=("sent", "state"), what=what)
    d = capi.BurstDetector(*det)

    def call(p):
        return lib().cc_burst_erasure_channel_dev(code._h, C.byref(chan), C.byref(d), SEED, first, frames, int(random_cw),
                                                  p["recv"], p["sent"], p["state"], p["flag"], p["erasures"], p["offsets"],
                                                  p["stream"])
    outputs.update(flag=(np.uint8, frames * n), erasures=(np.uint16, frames * n), offsets=(np.uint32, frames + 1))
    expected["flag"] = pick(3)
    if whole:
        flag = parts[0][3]
        vals, off = burst_erasure_model.csr(burst_erasure_model.frame_lists(flag))
        if det == ALL:  # every symbol flagged: the list fills its capacity to the last element
            assert vals.size == frames * n and flag.all()
        else:
            assert 0 < vals.size < frames * n or frames * n < 100
        expected.update(erasures=listed(vals, frames, n), offsets=off.astype(np.uint32))
    else:
        # a sample: the offsets of a range relative to its first, the entries they bound, and the rules of the whole list
        seen = {}

        def offsets(view, label):
            off = view.cpu().numpy().view(np.uint32).astype(np.int64)
            assert off[0] == 0 and (np.diff(off) >= 0).all() and (np.diff(off) <= n).all(), label
            for (lo, hi), part in zip(where, parts):
                want = burst_erasure_model.csr(burst_erasure_model.frame_lists(part[3]))[1]
                assert np.array_equal(off[lo:hi + 1] - off[lo], want), (label, lo)
            seen["off"] = off

        def erasures(view, label):
            got, off = view.cpu().numpy().view(np.uint16), seen["off"]
            for (lo, hi), part in zip(where, parts):
                want = burst_erasure_model.csr(burst_erasure_model.frame_lists(part[3]))[0]
                assert np.array_equal(got[off[lo]:off[hi]], want), (label, lo)
            assert (got[off[-1]:].view(np.uint8) == SENTINEL).all(), (label, "entries behind off[frames] were written")
        outputs = {k: outputs[k] for k in ("recv", "sent", "state", "flag", "offsets", "erasures")}  # offsets first
        expected.update(offsets=offsets, erasures=erasures)
    optional = ("sent", "state", "flag", ("erasures", "offsets"))
    return check_call(call, {}, outputs, expected, optional=optional, what=what)


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("name", list(BURST))
def test_burst_channel(name, random_cw):
    """burst_kernel<false>: both branches of store4 (odd N at an odd base), the tail branch, one to four passes; the second
    trip on RS(255,239) at depth 2, a group of 64 lanes per block"""
    make, I = BURST[name]
    code = make()
    for blocks in (1, 5):
        burst_case(code, I, blocks, random_cw, None, (name, blocks, random_cw))
    if name == "rs239-I2":
        trip = second_trip(64)
        burst_case(code, I, trip, random_cw, None, (name, "second trip", trip, random_cw), trip=trip - 9)


@pytest.mark.parametrize("det", [TYPICAL, ALL], ids=["typical", "all"])
@pytest.mark.parametrize("name", list(BURST))
def test_burst_erasure_channel(name, det):
    """burst_kernel<true> and the list kernels behind it; with every symbol flagged the list is full.  1029 frames (343
    blocks of RS(7,3) at depth 3, 1029 of RS(15,9) at depth 1) reach the second tile of the scan."""
    make, I = BURST[name]
    code = make()
    for random_cw in (False, True):
        for blocks in (1, 5):
            burst_case(code, I, blocks, random_cw, det, (name, blocks, random_cw, det))
    if name in ("rs7-I3", "rs15-I1"):
        assert 1029 % I == 0
        burst_case(code, I, 1029 // I, True, det, (name, 1029, det))
    if name == "rs239-I2" and det == TYPICAL:
        trip = second_trip(64)
        burst_case(code, I, trip, True, det, (name, "second trip", trip, det), trip=trip - 9)


# ------------------------------------------------ the BSC on packed words ------------------------------------------------
# (q, t, N, polynomial): P = 1, 2, 8 (1 pad bit), 26 (5 pad bits) and 64 bytes
PACKED = {"bch7": (3, 1, None, None), "bch15": (4, 2, None, None), "bch63": (6, 3, None, None),
          "bch203": (10, 4, 203, 0x409), "bch511": (9, 3, None, 0x211)}


def packed_case(code, poly, prob, B, random_cw, what, trip=None):
    from test_gpu_packed import pad_bits
    from test_gpu_packed_mc import flips_model
    n, P = code.n, code.packed_bytes
    where = spans(B, trip)
    recv, sent = [], []
    for lo, hi in where:
        s = sent_words(code, SEED, FIRST + lo, hi - lo, random_cw, poly)
        flips = flips_model(prob, SEED, FIRST + lo, hi - lo, n)
        assert prob != 1.0 or flips.all()
        recv.append(cc.pack_bits(s ^ flips.astype(s.dtype)))  # (pack_bits writes the pad bits as 0)
        sent.append(cc.pack_bits(s))
        assert not pad_bits(recv[-1], n).any() and not pad_bits(sent[-1], n).any()
    whole = where == [(0, B)]

    def call(p):
        return lib().cc_bsc_packed_channel_dev(code._h, prob, SEED, FIRST, B, int(random_cw), p["recv"], p["sent"], p["stream"])

    def pads(inner):
        def check(view, label):
            got = view.cpu().numpy().reshape(B, P)
            assert not pad_bits(got, n).any(), (label, "pad bits")
            if whole:
                assert np.array_equal(got, inner[0]), (label, "differs from the expected array")
            else:
                sampled(inner, where, P)(view, label)
        return check
    outputs = {"recv": (np.uint8, B * P), "sent": (np.uint8, B * P)}
    check_call(call, {}, outputs, {"recv": pads(recv), "sent": pads(sent)}, optional=("sent",), what=what)


@pytest.mark.parametrize("random_cw", [False, True], ids=["zero", "random"])
@pytest.mark.parametrize("name", list(PACKED))
def test_bsc_packed_channel(name, random_cw):
    """bsc_packed_kernel: no whole dword in a frame (P = 1, 2), odd pitch in dwords (P = 26), sixteen lanes per frame
    (P = 64) with the second trip; p = 1.0 puts the threshold at 2^32"""
    from test_gpu_packed import make
    q, t, N, poly = PACKED[name]
    code = make(q, t, N, "BM", poly)
    assert code.packed_bytes == {"bch7": 1, "bch15": 2, "bch63": 8, "bch203": 26, "bch511": 64}[name]
    assert 8 * code.packed_bytes - code.n == {"bch7": 1, "bch15": 1, "bch63": 1, "bch203": 5, "bch511": 1}[name]
    for prob in (0.05, 1.0):
        for B in (1, 5):
            packed_case(code, poly, prob, B, random_cw, (name, prob, B, random_cw))
    if name == "bch511":
        B = second_trip(16)
        packed_case(code, poly, 0.05, B, random_cw, (name, "second trip", B, random_cw), trip=B - 9)


# ------------------------------------------------ no frames ------------------------------------------------
def test_calls_without_frames_write_nothing():
    """frames = 0: CC_OK, and no byte of any buffer changes -- the one word an offsets array has then included.  (The
    buffers are given a few elements: torch hands out no address for an empty one.)"""
    from test_gpu_packed import make
    bch, rs = DISCRETE["bch63"](), DISCRETE["rs15"]()
    packed = make(6, 3, None, "BM", None)
    pc = product_of("15x7")
    desc = pc._pc()
    chan, det = capi.BurstChannel(3, *BURSTY), capi.BurstDetector(*TYPICAL)

    def untouched(view, label):
        assert (view.cpu().numpy().view(np.uint8) == SENTINEL).all(), (label, "written by a call without frames")
    empty = {"u8": (np.uint8, 16), "f32": (np.float32, 16), "u16": (np.uint16, 16), "off": (np.uint32, 1)}
    calls = {
        "cc_awgn_llr_dev": (lambda p: lib().cc_awgn_llr_dev(bch._h, EBNO, SEED, FIRST, 0, 1, p["llr"], p["sent"], p["stream"]),
                            {"llr": "f32", "sent": "u8"}),
        "cc_awgn_symbols_dev": (lambda p: lib().cc_awgn_symbols_dev(rs._h, EBNO, SEED, FIRST, 0, 1, p["words"], p["rel"],
                                                                    p["sent"], p["stream"]),
                                {"words": "u8", "rel": "f32", "sent": "u8"}),
        "cc_awgn_product_dev": (lambda p: lib().cc_awgn_product_dev(C.byref(desc), EBNO, SEED, FIRST, 0, 1, p["y"], p["sent"],
                                                                    p["stream"]), {"y": "f32", "sent": "u8"}),
        "cc_discrete_channel_dev": (lambda p: lib().cc_discrete_channel_dev(rs._h, 0.03, 0.05, SEED, FIRST, 0, 1, p["recv"],
                                                                            p["erasures"], p["offsets"], p["sent"], p["stream"]),
                                    {"recv": "u8", "erasures": "u16", "offsets": "off", "sent": "u8"}),
        "cc_burst_channel_dev": (lambda p: lib().cc_burst_channel_dev(rs._h, C.byref(chan), SEED, 0, 0, 1, p["recv"], p["sent"],
                                                                      p["state"], p["stream"]),
                                 {"recv": "u8", "sent": "u8", "state": "u8"}),
        "cc_burst_erasure_channel_dev": (lambda p: lib().cc_burst_erasure_channel_dev(
            rs._h, C.byref(chan), C.byref(det), SEED, 0, 0, 1, p["recv"], p["sent"], p["state"], p["flag"], p["erasures"],
            p["offsets"], p["stream"]),
            {"recv": "u8", "sent": "u8", "state": "u8", "flag": "u8", "erasures": "u16", "offsets": "off"}),
        "cc_bsc_packed_channel_dev": (lambda p: lib().cc_bsc_packed_channel_dev(packed._h, 0.05, SEED, FIRST, 0, 1, p["recv"],
                                                                                p["sent"], p["stream"]),
                                      {"recv": "u8", "sent": "u8"}),
    }
    for name, (call, kinds) in calls.items():
        outputs = {k: empty[v] for k, v in kinds.items()}
        check_call(call, {}, outputs, {k: untouched for k in outputs}, what=(name, "no frames"))


# ------------------------------------------------ Monte-Carlo counters ------------------------------------------------
# The one buffer the eight Monte-Carlo calls write: 64 uint64 at 8 mod 16 between guards, slot i preloaded with
# (i + 1) << 40 | 0xFFFFFF00 + i, so that a count of 256 - i carries from the low word into the high one.  After the call
# every slot is its preload plus the count of a host pipeline -- the channel-only call (AWGN routes) or the numpy channel
# model (the others), the plain-C oracle or the model decoder built on it, a comparison in numpy -- and a slot the call
# does not count in, the ones the header calls "not touched" among them, is its preload byte for byte: a store in place of
# an add, a 32-bit add and a write to a slot promised untouched all show.  Every point is chosen so that
# 0 < failures < frames and 0 < word errors: with the model and the oracle on the CPU for the discrete, burst and packed
# routes, and predicted from awgn_reference (asserted below, as for the actual frames) for the AWGN routes.
MC_FRAMES_PER_CALL, MC_SEED, MC_FIRST = 300, 0x5EED00000003, (1 << 32) - 150
PRELOAD = ((np.arange(64, dtype=np.uint64) + np.uint64(1)) << np.uint64(40)) | (np.uint64(0xFFFFFF00) + np.arange(64, dtype=np.uint64))
NOT_TOUCHED = [capi.MC_ITER_SUM] + list(range(capi.MC_ITER_HIST, capi.MC_NCOUNTERS))  # (chase, GMD, product, packed)


def tally(out, failed, sent, channel_errors, erasures=0, per_word=None):
    """the counter slots of a batch by the header's definitions; per_word: the words of a block (product codes)"""
    B = out.shape[0]
    wrong = (out.reshape(B, -1) != sent.reshape(B, -1)).sum(axis=1)
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = B
    c[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int(failed.sum())
    c[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(channel_errors)
    c[capi.MC_CHANNEL_ERASURES] = int(erasures)
    return c


def hard_decode(o, rx, lists=None):
    """the oracle's BM decoder in the form of the header: (out, failed), out = the received word where the frame fails"""
    if lists is None:
        out, _, st, _ = o.correct_hard(BM, rx)
    else:
        rows = [o.correct_hard(BM, rx[f:f + 1], lists[f]) for f in range(rx.shape[0])]
        out, st = np.concatenate([r[0] for r in rows]), np.concatenate([r[2] for r in rows])
    failed = np.asarray(st) != 0
    sym = (rx < 0).astype(np.uint8) if rx.dtype == np.float32 else rx
    return np.where(failed[:, None], sym, out).astype(np.uint8), failed


def oracle_of(family, q, t):
    from checkers import Oracle
    return Oracle(family, q, t)


def count_minsum(y, sent, iterations=5):
    from checkers import O2
    b, _, it, st = oracle_of(BCH, 4, 2).minsum(0, iterations, y, 1.0, 0.0, O2, fast=True)
    failed, it = st != 0, it.astype(np.int64)
    c = tally(b, failed, sent, ((y < 0) != (sent != 0)).sum())
    c[capi.MC_ITER_SUM] = int(np.where(failed, iterations, it + 1).sum())
    c[capi.MC_ITER_HIST:] = np.bincount(it[~failed], minlength=56)[:56]
    return c


def count_bm(y, sent):
    out, failed = hard_decode(oracle_of(BCH, 4, 2), y)
    return tally(out, failed, sent, ((y < 0) != (sent != 0)).sum())


def count_chase(y, sent, p=2):
    import chase_model as M
    want = M.chase(M.decoder(4, 2), y, p)
    return tally(want["out"], want["status"] != M.FRAME_OK, sent, ((y < 0) != (sent != 0)).sum())


def count_gmd(w, rel, sent, trials=2):  # (with all t + 1 trials GMD finds a word for every frame of RS(7,3))
    import gmd_model as M
    want = M.gmd(M.Decoder(3, 2), w, rel, trials)
    pop = np.array([bin(v).count("1") for v in range(256)])
    return tally(want["out"], want["status"] != M.FRAME_OK, sent, pop[w ^ sent].sum())  # (bit errors count symbols)


def count_product(y, sent, p=2, halves=2):  # (four test patterns: with sixteen every word of BCH(15,7) has a candidate)
    import chase_model as M
    from test_gpu_product import ALPHA, BETA, model_steps
    last = model_steps(M.decoder(4, 2), M.decoder(4, 2), y, False, p, ALPHA[:halves], BETA[:halves])[-1]
    return tally(last["out"], (last["status"] != M.FRAME_OK).any(axis=1), sent, ((y < 0) != (sent != 0)).sum())


class Rs7:  # RS(7,3), t = 2: the smallest code the symbol routes serve on which a bounded-distance decoder can fail
    family, q, t, n, l = capi.FAMILY_RS, 3, 2, 7, 3


class Bch15:  # BCH(15,7), t = 2: the same among the binary codes (BCH(7,4) is perfect)
    family, q, t, n, l = capi.FAMILY_BCH, 4, 2, 15, 7


DISCRETE_POINT, BURST_POINT, BURST_DEPTH, PACKED_POINT = (0.1, 0.1), (0.1, 0.3, 0.02, 0.5), 3, 0.12


def frames_of(blocks, I):
    """(blocks, n, I) in transmission order -> frame-major (blocks I, n)"""
    b, n, _ = blocks.shape
    return np.ascontiguousarray(blocks.transpose(0, 2, 1)).reshape(b * I, n)


def count_discrete(frames=MC_FRAMES_PER_CALL):
    sent = sent_words(Rs7, MC_SEED, MC_FIRST, frames, True)
    recv, erased, wrong = discrete_model(*DISCRETE_POINT, MC_SEED, MC_FIRST, frames, 7, 8, sent)
    out, failed = hard_decode(oracle_of(RS, 3, 2), recv, [np.flatnonzero(e).tolist() for e in erased])
    return tally(out, failed, sent, wrong.sum(), erased.sum())


def count_burst(detector, frames=MC_FRAMES_PER_CALL):
    I, first = BURST_DEPTH, MC_FIRST // BURST_DEPTH * BURST_DEPTH
    sent = sent_words(Rs7, MC_SEED, first, frames, True)
    base = burst_model.channel(BURST_POINT, I, MC_SEED, first, frames, 7, 8, sent)
    if detector is None:
        recv, _, _, wrong = base
        out, failed = hard_decode(oracle_of(RS, 3, 2), frames_of(recv, I))
        return tally(out, failed, sent, wrong.sum())
    recv, _, _, flag, wrong = burst_erasure_model.channel(BURST_POINT, detector, I, MC_SEED, first, frames, 7, 8, base=base)
    out, failed = hard_decode(oracle_of(RS, 3, 2), frames_of(recv, I), burst_erasure_model.frame_lists(flag))
    return tally(out, failed, sent, wrong.sum(), flag.sum())


def count_packed(frames=MC_FRAMES_PER_CALL):
    from test_gpu_packed_mc import flips_model
    sent = sent_words(Bch15, MC_SEED, MC_FIRST, frames, True)
    flips = flips_model(PACKED_POINT, MC_SEED, MC_FIRST, frames, 15)
    out, failed = hard_decode(oracle_of(BCH, 4, 2), sent ^ flips)
    return tally(out, failed, sent, flips.sum())


def awgn_frames(code, ebno, frames, symbols=False):
    """the channel-only call of an AWGN route into plain tensors, and the float64 model of the same frames"""
    import torch
    n, sigma = code.n, sigma_f32(code, ebno)
    sent = torch.empty((frames, n), dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    if symbols:
        w = torch.empty((frames, n), dtype=torch.uint8, device="cuda")
        rel = torch.empty((frames, n), dtype=torch.float32, device="cuda")
        capi.check(lib().cc_awgn_symbols_dev(code._h, ebno, MC_SEED, MC_FIRST, frames, 1, ptr(w), ptr(rel), ptr(sent), None), "channel")
        torch.cuda.synchronize()
        s = sent.cpu().numpy()
        y = awgn_reference(n * code.q, sigma, MC_SEED, MC_FIRST, frames, bits_of(s, code.q)).reshape(frames, n, code.q)
        w_ref = ((y < 0).astype(np.uint32) << np.arange(code.q, dtype=np.uint32)).sum(axis=2).astype(np.uint8)
        return (w.cpu().numpy(), rel.cpu().numpy(), s), (w_ref, np.abs(y).min(axis=2).astype(np.float32), s)
    llr = torch.empty((frames, n), dtype=torch.float32, device="cuda")
    capi.check(lib().cc_awgn_llr_dev(code._h, ebno, MC_SEED, MC_FIRST, frames, 1, ptr(llr), ptr(sent), None), "channel")
    torch.cuda.synchronize()
    s = sent.cpu().numpy()
    return (llr.cpu().numpy(), s), (awgn_reference(n, sigma, MC_SEED, MC_FIRST, frames, s).astype(np.float32), s)


def working_point(c, frames, what):
    assert c[capi.MC_FRAMES] == frames and 0 < c[capi.MC_FAILURES] < frames and 0 < c[capi.MC_WORD_ERRORS], (what, c[:8])


MC_EBNO = {"minsum": 3.0, "bm": 3.0, "chase": 2.0, "gmd": 4.0, "product": 3.0}


# The routes added since -- ordered statistics, iBDD and iBDD-SR of a product code, staircase codes: the same preload and
# guards.  Their counts are the models' (osd_model, product_hard_model, product_sr_model, staircase_model) on the values the
# route's own channel call writes; the point of each is chosen with the models alone, on the channel of awgn_model over the
# words the host encoders send (`predicted`, which tests/test_buffer_cases_host.py asserts without a device): every route
# that can fail has 0 < failures < frames, and ordered statistics, which cannot, 0 < word errors < frames.
LATER = {
    "osd": dict(q=4, t=2, order=1, ebno=1.0, frames=300),
    "product-hard": dict(q=4, t=1, halves=6, ebno=4.5, frames=256),
    "product-sr": dict(q=4, t=1, halves=6, ebno=3.5, frames=256),
    "staircase": dict(q=4, t=1, N=14, L=9, W=4, I=2, ebno=5.0, frames=256),  # m = 7: blocks of 49 bits, six of nine counted
}


def sigma_of(rate, ebno):
    """simulation.c++:83-85 in double, as the launchers pass it: rounded to float32"""
    return float(np.float32(1.0 / np.sqrt(2.0 * rate * 10.0 ** (ebno / 10.0))))


def later_weights(route):
    from test_product_sr_host import RISING
    return RISING[:LATER[route]["halves"]]


def later_sent(route):
    """the words, blocks or streams the route's channel sends for random codewords, from the host encoders"""
    import product_hard_model as PH
    import staircase_model as SM
    from test_product_hard_host import encode_blocks
    c = LATER[route]
    frames = c["frames"]
    if route == "osd":
        return sent_words(Bch15, MC_SEED, MC_FIRST, frames, True)
    if route == "staircase":
        dec = SM.decoder(c["q"], c["t"], c["N"])
        _, m, _, kb = SM.shape(dec, False)
        msg = bch_message_bits(MC_SEED, MC_FIRST, frames, c["L"] * m * kb).reshape(frames, c["L"], m, kb)
        return np.asarray(SM.encode(dec, msg, False), np.uint8)
    dec = PH.decoder(c["q"], c["t"])
    msg = bch_message_bits(MC_SEED, MC_FIRST, frames, dec.l * dec.l).reshape(frames, dec.l, dec.l)
    return encode_blocks(dec, dec, msg, False)


def later_rate(route):
    import product_hard_model as PH
    import staircase_model as SM
    c = LATER[route]
    if route == "osd":
        return Bch15.l / Bch15.n
    if route == "staircase":
        _, m, r, _ = SM.shape(SM.decoder(c["q"], c["t"], c["N"]), False)
        return 1.0 - r / m
    dec = PH.decoder(c["q"], c["t"])
    return (dec.l / dec.n) ** 2


def later_count(route, y, sent):
    """the counters of the header for the channel values y (staircase: the hard decisions z) and the words sent"""
    import osd_model
    import product_hard_model as PH
    import product_sr_model as SR
    import staircase_model as SM
    from test_gpu_osd import counted as osd_counted
    from test_gpu_product_hard import counted as product_counted
    from test_gpu_staircase import counted as staircase_counted
    c = LATER[route]
    if route == "osd":
        return osd_counted(osd_model.osd(osd_model.decoder(c["q"], c["t"]), y, c["order"])["out"], sent, y)
    if route == "staircase":
        dec = SM.decoder(c["q"], c["t"], c["N"])
        return staircase_counted(SM.decode(dec, y, c["W"], c["I"], False), sent, y, c["L"], c["W"])
    dec = PH.decoder(c["q"], c["t"])
    if route == "product-hard":
        return product_counted(PH.decode(dec, dec, (y < 0).astype(np.uint8), c["halves"], False), sent, y)
    return product_counted(SR.decode(dec, dec, y, later_weights(route), False), sent, y)


@functools.lru_cache(maxsize=None)
def later_predicted(route):
    """the counts on the float64 channel model over the host encoders' words: no device"""
    c, sent = LATER[route], later_sent(route)
    frames = c["frames"]
    y = awgn_reference(sent[0].size, sigma_of(later_rate(route), c["ebno"]), MC_SEED, MC_FIRST, frames, sent.reshape(frames, -1))
    y = y.astype(np.float32).reshape(sent.shape)
    return later_count(route, (y < 0).astype(np.uint8) if route == "staircase" else y, sent)


def later_point(c, frames, route, what=""):
    if route != "osd":
        return working_point(c, frames, (route, what))
    assert c[capi.MC_FRAMES] == frames and c[capi.MC_FAILURES] == 0 and 0 < c[capi.MC_WORD_ERRORS] < frames, (route, what, c[:8])


MC_ROUTES = ["minsum", "bm", "chase", "gmd", "product", "discrete", "burst", "burst-erasure", "packed"] + list(LATER)


@pytest.mark.parametrize("route", MC_ROUTES)
def test_monte_carlo_counters(route):
    frames = MC_FRAMES_PER_CALL
    bch = lambda tag: cc.primitive_bch(4, cc.errors(2), tag)  # noqa: E731
    rs7 = lambda: cc.rs(3, cc.errors(2), cc.berlekamp_massey_tag())  # noqa: E731
    untouched = []
    if route in ("minsum", "bm", "chase"):
        code = bch(cc.min_sum_tag(5) if route == "minsum" else cc.berlekamp_massey_tag())
        count = {"minsum": count_minsum, "bm": count_bm, "chase": count_chase}[route]
        actual, model = awgn_frames(code, MC_EBNO[route], frames)
        working_point(count(*model), frames, (route, "predicted"))
        counts = count(*actual)
        if route == "chase":
            untouched = NOT_TOUCHED

            def call(p):
                return lib().cc_mc_run_chase_dev(code._h, 2, MC_EBNO[route], MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
        else:
            assert code.algorithm.soft == (route == "minsum")

            def call(p):
                return lib().cc_mc_run_dev(code._h, MC_EBNO[route], MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
    elif route == "gmd":
        code, untouched = rs7(), NOT_TOUCHED
        actual, model = awgn_frames(code, MC_EBNO[route], frames, symbols=True)
        working_point(count_gmd(*model), frames, (route, "predicted"))
        counts = count_gmd(*actual)

        def call(p):
            return lib().cc_mc_run_gmd_dev(code._h, 2, MC_EBNO[route], MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
    elif route == "product":
        from test_gpu_product import ALPHA, BETA
        frames = 256  # blocks of 15 x 15: the fewest whose count carries out of the low word of slot 0
        pc, untouched = cc.product_code(bch(cc.berlekamp_massey_tag()), bch(cc.berlekamp_massey_tag())), NOT_TOUCHED
        ch = pc.channel(MC_EBNO[route], MC_SEED, MC_FIRST, frames, True)
        y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
        sigma = float(np.float32(pc.sigma(MC_EBNO[route])))
        ref = awgn_reference(pc.n, sigma, MC_SEED, MC_FIRST, frames, sent.reshape(frames, -1)).astype(np.float32).reshape(y.shape)
        working_point(count_product(ref, sent), frames, (route, "predicted"))
        counts = count_product(y, sent)
        desc = pc._pc(2, ALPHA[:2], BETA[:2])

        def call(p):
            return lib().cc_mc_run_product_dev(C.byref(desc), MC_EBNO[route], MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
    elif route == "discrete":
        code, counts = rs7(), count_discrete()

        def call(p):
            return lib().cc_mc_run_discrete_dev(code._h, *DISCRETE_POINT, MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
    elif route in ("burst", "burst-erasure"):
        code, chan = rs7(), capi.BurstChannel(BURST_DEPTH, *BURST_POINT)
        first = MC_FIRST // BURST_DEPTH * BURST_DEPTH
        det = capi.BurstDetector(*TYPICAL)
        counts = count_burst(TYPICAL if route == "burst-erasure" else None)

        def call(p):
            if route == "burst":
                return lib().cc_mc_run_burst_dev(code._h, C.byref(chan), MC_SEED, first, frames, 1, p["counters"], p["stream"])
            return lib().cc_mc_run_burst_erasure_dev(code._h, C.byref(chan), C.byref(det), MC_SEED, first, frames, 1,
                                                     p["counters"], p["stream"])
    elif route in LATER:
        c = LATER[route]
        frames, ebno = c["frames"], c["ebno"]
        later_point(later_predicted(route), frames, route, "predicted")
        if route == "osd":
            code, untouched = bch(cc.berlekamp_massey_tag()), [capi.MC_FAILURES] + NOT_TOUCHED
            (y, sent), _ = awgn_frames(code, ebno, frames)

            def call(p):
                return lib().cc_mc_run_osd_dev(code._h, c["order"], ebno, MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
        elif route == "staircase":
            from channelcoding_amd.codes import staircase_code
            sc, untouched = staircase_code(cc.primitive_bch(c["q"], cc.errors(c["t"]), cc.berlekamp_massey_tag(), n=c["N"]),
                                           c["L"], c["W"], c["I"]), NOT_TOUCHED
            ch = sc.channel(ebno, MC_SEED, MC_FIRST, frames, True)
            y, sent, desc = ch["z"].cpu().numpy(), ch["sent"].cpu().numpy(), sc._sc()

            def call(p):
                return lib().cc_mc_run_staircase_dev(C.byref(desc), ebno, MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
        else:  # (iBDD and iBDD-SR count iterations: CC_MC_ITER_SUM and the histogram are theirs)
            from channelcoding_amd.codes import _sr_weights
            mk = lambda: cc.primitive_bch(c["q"], cc.errors(c["t"]), cc.berlekamp_massey_tag())  # noqa: E731
            pc = cc.product_code(mk(), mk())
            ch = pc.channel(ebno, MC_SEED, MC_FIRST, frames, True)
            y, sent, desc = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy(), pc._pc_hard(c["halves"])
            weights = _sr_weights(later_weights(route))

            def call(p):
                if route == "product-hard":
                    return lib().cc_mc_run_product_hard_dev(C.byref(desc), ebno, MC_SEED, MC_FIRST, frames, 1, p["counters"],
                                                            p["stream"])
                return lib().cc_mc_run_product_sr_dev(C.byref(desc), weights, ebno, MC_SEED, MC_FIRST, frames, 1, p["counters"],
                                                      p["stream"])
        assert np.array_equal(sent, later_sent(route).reshape(sent.shape))  # the host encoders send the same words
        counts = later_count(route, y, sent)
        if route != "osd" and route != "staircase":
            assert counts[capi.MC_ITER_SUM] > 0 and counts[capi.MC_ITER_HIST:].sum() == frames
    else:
        code, counts = bch(cc.berlekamp_massey_tag()), count_packed()
        untouched = NOT_TOUCHED + [capi.MC_CHANNEL_ERASURES]

        def call(p):
            return lib().cc_mc_run_bsc_packed_dev(code._h, PACKED_POINT, MC_SEED, MC_FIRST, frames, 1, p["counters"], p["stream"])
    (later_point if route in LATER else working_point)(counts, frames, route)
    assert not counts[untouched].any() and (counts >= 0).all()
    assert (PRELOAD[0] & np.uint64(0xFFFFFFFF)) + np.uint64(frames) > np.uint64(0xFFFFFFFF)  # the frame count carries
    want = PRELOAD + counts.astype(np.uint64)

    def slots(view, label):
        got = view.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (label, [(int(i), hex(int(got[i])), hex(int(want[i])), int(counts[i])) for i in bad])
        for i in untouched:
            assert got[i] == PRELOAD[i], (label, "a slot the header calls not touched", i)
    check_call(call, {}, {"counters": (np.uint64, capi.MC_NCOUNTERS, PRELOAD)}, {"counters": slots}, what=route)
