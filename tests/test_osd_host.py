"""CPU tests of ordered-statistics decoding (cc_correct_osd_batch, cc_correct_osd_batch_dev, cc_mc_run_osd_dev): the
model of tests/osd_model.py against maximum likelihood (a brute force over every word of three small codes, which the
model must equal at order = l), against itself across the orders and against the parity-check side (the complement of
its basis is the greedy basis of the oracle's H taken from the least reliable end); the refusals and their order on
CC_DEVICE_NONE handles; and the bindings.  tests/test_gpu_osd.py holds the device against the model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi
from channelcoding_amd.montecarlo import OsdBackend, awgn_simulation
import osd_model as M
from checkers import awgn_llr
from test_discrete_host import StubBackend, StubCode

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_correct_osd_batch", "cc_correct_osd_batch_dev", "cc_mc_run_osd_dev", "cc_osd_frames_per_wavefront")
SMALL = [(3, 1), (4, 2), (4, 1)]  # BCH(7,4), BCH(15,7), BCH(15,11)


def frames_of(dec, seed, count=120):
    """random codewords over AWGN at 1 dB, every third frame quantised to multiples of 0.5 so that keys and metrics tie"""
    rng = np.random.default_rng(seed)
    words = dec.encode(rng.integers(0, 2, (count, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words, dec.l / dec.n, 1.0)
    y[::3] = (np.round(y[::3] * 2) / 2).astype(np.float32)
    y[::9, 2] = np.float32(-0.0)
    return np.ascontiguousarray(y, np.float32)


# ---- the model ----
@pytest.mark.parametrize("q,t", SMALL, ids=["bch7", "bch15-7", "bch15-11"])
def test_model_at_order_l_is_maximum_likelihood(q, t):
    dec = M.decoder(q, t)
    y = frames_of(dec, 70 + q + t)
    assert (y[::3] * 2 == np.round(y[::3] * 2)).all()
    tied = improved = 0
    for f in range(y.shape[0]):
        words, Mw = M.maximum_likelihood(dec, y[f])
        assert words.shape[0] == 1 << dec.l and len({w.tobytes() for w in words}) == 1 << dec.l
        res = M.frame(dec, y[f], dec.l)
        out, nerr, met, j = res[dec.l]
        best = Mw.min()
        assert met.view(np.uint32) == best.view(np.uint32), f
        nearest = words[Mw == best]
        # (several words at the smallest metric: maximum likelihood does not say which, the order of the patterns does)
        assert (nearest == out[None, :]).all(axis=1).any(), f
        if nearest.shape[0] == 1:
            assert np.array_equal(out, nearest[0])
        tied += nearest.shape[0] > 1
        assert nerr == int((out != M.hard(y[f])).sum())
        # the orders nest
        assert res[2][2] <= res[1][2] <= res[0][2] and res[dec.l][2] <= res[2][2]
        improved += res[2][2] < res[0][2]
        assert res[0][3] == 0 and res[1][3] <= dec.l
    assert tied > 0 and improved > 5


@pytest.mark.parametrize("q,t", SMALL + [(5, 3), (6, 3)], ids=["bch7", "bch15-7", "bch15-11", "bch31", "bch63"])
def test_basis_is_the_complement_of_the_least_reliable_basis_of_H(q, t):
    dec = M.decoder(q, t)
    H = (np.asarray(dec.H(), np.int64) % 2).astype(np.uint8)
    k = dec.n - dec.l
    assert H.shape == (k, dec.n)
    y = frames_of(dec, 900 + q + t, 60)
    skipped = 0
    for f in range(y.shape[0]):
        pi = M.order(y[f])
        basis, Gr, sk = M.greedy(M.generator(dec), pi, dec.l)
        parity, _, _ = M.greedy(H, pi[::-1], k)
        assert sorted(basis + parity) == list(range(dec.n)), f
        assert [p for p in pi if p in set(basis)] == basis  # B_0 .. B_(l-1) come in pi order
        assert np.array_equal(Gr[:, basis], np.eye(dec.l, dtype=np.uint8))
        skipped += sk > 0
    assert skipped >= y.shape[0] // 8  # dependent columns are met on the way


def test_order_of_positions_and_pattern_numbering():
    y = np.array([0.5, -0.5, 0.0, 1.0, -0.0, 0.5, -1.5, 1e-40, -1e-40], np.float32)
    assert M.order(y).tolist() == [6, 3, 0, 1, 5, 7, 8, 2, 4]
    assert M.patterns(4, 2).tolist() == [[4, 4], [0, 4], [1, 4], [2, 4], [3, 4], [0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    assert M.patterns(1, 2).tolist() == [[1, 1], [0, 1]] and M.patterns(3, 0).tolist() == [[3]]
    assert [M.pattern_count(247, o) for o in (0, 1, 2)] == [1, 248, 30629]


def test_shortened_code_uses_the_words_of_the_shortened_code():
    dec = M.decoder(4, 2, 12)  # BCH(15,7) shortened to (12,4)
    msgs = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    words = dec.encode(msgs)
    y = frames_of(dec, 12, 60)
    for f in range(y.shape[0]):
        out, nerr, met, j = M.frame(dec, y[f], dec.l)[dec.l]
        Mw = M.metric(y[f][None, :], M.hard(y[f])[None, :], words)
        assert met.view(np.uint32) == Mw.min().view(np.uint32) and (words == out[None, :]).all(axis=1).any()


# ---- the C interface on handles without a device ----
def _correct(code, order, llr=True, out=True, dev=False, B=4):
    n = code.n if code is not None else 15
    y = np.ones((B, n), np.float32)
    o = np.zeros((B, n), np.uint8)
    args = [code._h if code is not None else None, y.ctypes.data_as(C.c_void_p) if llr else None, order,
            o.ctypes.data_as(C.c_void_p) if out else None, None, None, None, B]
    if dev:
        return capi.lib().cc_correct_osd_batch_dev(*args, None)
    return capi.lib().cc_correct_osd_batch(*args)


def _run(code, order, counters=True):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_osd_dev(code._h if code is not None else None, order, 4.0, 0, 0, 16, 1,
                                        buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def calls():
    return [lambda c, o: _correct(c, o), lambda c, o: _correct(c, o, dev=True), _run]


def served():
    return [cc.primitive_bch(3, cc.errors(1), BM(), **NONE),
            cc.primitive_bch(6, cc.errors(3), cc.peterson_gorenstein_zierler_tag(), **NONE),
            cc.primitive_bch(8, cc.errors(18), cc.euklid_tag(), **NONE),  # 2t = 36: no algebraic decoder is needed
            cc.primitive_bch(8, cc.errors(63), BM(), **NONE),
            cc.primitive_bch(8, cc.errors(3), BM(), n=200, **NONE),
            cc.primitive_bch(8, cc.errors(3), BM(), n=25, **NONE)]


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert re.search(r"#define CC_OSD_MAX_ORDER 2\b", header) and capi.OSD_MAX_ORDER == 2
    assert "cyclic.h:254-267" in header[header.index("Ordered-statistics decoding"):header.index("#define CC_OSD_MAX_ORDER")]


def test_valid_calls_reach_the_device_check():
    for code in served():
        for order in range(capi.OSD_MAX_ORDER + 1):
            for call in calls():
                assert call(code, order) == capi.ERR_NO_DEVICE, (code.to_string(), order)
            assert capi.lib().cc_osd_frames_per_wavefront(code._h, order) >= 1
        assert capi.lib().cc_osd_frames_per_wavefront(code._h, capi.OSD_MAX_ORDER + 1) == 0
    assert capi.lib().cc_osd_frames_per_wavefront(None, 0) == 0


def test_refusals_and_their_order():
    lib = capi.lib()
    ok = served()[1]
    bch_ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(bch_ms.H(), cc.min_sum_tag(10), **NONE)
    # 1. null pointers, whatever else is wrong with the call
    for order in (0, 99):
        assert _correct(None, order) == capi.ERR_INVALID_ARGUMENT
        assert _correct(None, order, dev=True) == capi.ERR_INVALID_ARGUMENT
        assert _run(None, order) == capi.ERR_INVALID_ARGUMENT
        for code in (ok, matrix, bch_ms):
            for dev in (False, True):
                assert _correct(code, order, llr=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
                assert _correct(code, order, out=False, dev=dev) == capi.ERR_INVALID_ARGUMENT
            assert _run(code, order, counters=False) == capi.ERR_INVALID_ARGUMENT
    # 2. a parity-check matrix without a code: invalid, before anything the code or the order would be refused for
    for call in calls():
        for order in (0, 99):
            assert call(matrix, order) == capi.ERR_INVALID_ARGUMENT
            assert "cc_minsum_create" in lib.cc_last_error().decode()
    # 3. unsupported, with a text that names the reason
    refused = [(cc.rs(8, cc.errors(16), BM(), **NONE), 2, "Reed-Solomon"),
               (bch_ms, 2, "min-sum"),
               (cc.primitive_bch(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE), 2, "q <= 8"),
               (ok, capi.OSD_MAX_ORDER + 1, "CC_OSD_MAX_ORDER"),
               (ok, 0xFFFFFFFF, "CC_OSD_MAX_ORDER")]
    for code, order, text in refused:
        for call in calls():
            assert call(code, order) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
        assert lib.cc_osd_frames_per_wavefront(code._h, order) == 0
    # the handle is looked at before the order
    rs = refused[0][0]
    for call in calls():
        assert call(rs, 99) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in lib.cc_last_error().decode()
    # and only a call that passes all of this asks for a device
    for call in calls():
        assert call(ok, 2) == capi.ERR_NO_DEVICE
    # an empty batch needs no pointers, as in the Chase call
    assert _correct(ok, 1, llr=False, out=False, B=0) == capi.ERR_NO_DEVICE
    assert _correct(ok, 1, llr=False, out=False, B=0, dev=True) == capi.ERR_NO_DEVICE


# ---- Python ----
def test_correct_batch_refuses_combinations():
    code = served()[1]
    y = np.ones((2, code.n), np.float32)
    for kw in (dict(erasures=[[1], []]), dict(want_L=True), dict(packed=True), dict(interleave=2),
               dict(out=np.zeros((2, code.n), np.uint8)), dict(chase=2), dict(gmd=1, reliability=y), dict(soft=0.5),
               dict(extended=True), dict(chase=2, soft=0.5), dict(chase=2, extended=True)):
        with pytest.raises(TypeError, match="osd="):
            code.correct_batch(y, osd=1, **kw)
    for kw in (dict(packed=True), dict(chase=1), dict(interleave=2)):
        with pytest.raises(TypeError, match="osd="):
            code.decode_batch(y, osd=1, **kw)
    with pytest.raises(TypeError, match="float32"):
        code.correct_batch(np.ones((2, code.n), np.uint8), osd=1)
    with pytest.raises(ValueError, match="osd="):
        code.correct_batch(y, osd=-1)
    with pytest.raises(cc.CcError):
        code.correct_batch(np.ones((2, code.n + 1), np.float32), osd=1)
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(y, osd=2)
    assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        code.decode_batch(y, osd=0)
    assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(y, osd=3)
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_simulation_log_name_sharding_and_cli(tmp_path):
    backend = StubBackend()
    sim = awgn_simulation(StubCode(), backend=backend, max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path), osd=1)
    res = sim()
    assert (tmp_path / "(255, 223, 33)-STUB-osd1.log").exists() and sim.osd == 1 and sim.chase is None
    # every point draws its frames from its own stretch of the global sequence; one rank takes all of them
    assert backend.calls == [(4.0, 0, 1000), (4.5, 1 << 40, 1000)] and [r["frames"] for r in res] == [1000, 1000]
    plain = awgn_simulation(StubCode(), backend=StubBackend(), max_samples=1000, start=4.0, stop=5.0, log_dir=str(tmp_path))
    plain()
    assert (tmp_path / "(255, 223, 33)-STUB.log").exists() and plain.osd is None
    for kw in (dict(chase=2), dict(gmd=1)):
        with pytest.raises(TypeError, match="osd="):
            awgn_simulation(StubCode(), backend=StubBackend(), osd=1, **kw)
    assert OsdBackend.symbol == "cc_mc_run_osd_dev" and issubclass(OsdBackend, object)
    assert "--osd" in benchmark.usage_text()
    assert benchmark.main(["--simulation", "bsc", "--osd", "1"]) == 1
    assert benchmark.main(["--osd", "3"]) == 1
    assert benchmark.main(["--osd", "1", "--chase", "2"]) == 1
    assert benchmark.main(["--osd", "1", "--algorithm", "ms"]) == 1  # no hard-tag decoder left in the selection
