"""CPU tests of the burst channel with a burst detector (cc_burst_erasure_channel_dev / cc_mc_run_burst_erasure_dev,
montecarlo.burst_simulation(p_detect=, p_false_alarm=), `benchmark --simulation burst --p-detect`): the C ABI's argument
checks on handles without a device and their order, the harness with a stub backend, and the identities of the numpy model
of tests/burst_erasure_model.py, against which tests/test_gpu_burst_erasure.py compares the device byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import BurstBackend, burst_simulation
import burst_erasure_model
import burst_model
from test_discrete_host import StubBackend, StubCode
from test_host_logic import header_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOOD = dict(interleave=4, p_gb=0.02, p_bg=0.25, p_error_good=0.001, p_error_bad=0.5)
NAMES = ("cc_burst_erasure_channel_dev", "cc_mc_run_burst_erasure_dev")


# ---- the C ABI ----
def test_symbols_are_declared_bound_and_exported():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert name in header_symbols() and name in capi.exported_symbols() and hasattr(lib, name)
    assert C.sizeof(capi.BurstDetector) == 24
    det = capi.BurstDetector(0.9, 0.002)
    assert (det.struct_size, det.reserved, det.p_detect, det.p_false_alarm) == (24, 0, 0.9, 0.002)
    text = open(os.path.join(ROOT, "include", "channelcoding_amd.h")).read()
    assert "typedef struct cc_burst_detector {" in text and "} cc_burst_detector;" in text
    assert C.sizeof(capi.BurstChannel) == 40  # the channel's struct is untouched
    assert "burst_erasure_channel" in cc.__all__


def _ref(x):
    return C.byref(x) if x is not None else None


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _mc(code, ch, det, first=0, frames=16, counters=True, random_cw=0):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_burst_erasure_dev(code._h, _ref(ch), _ref(det), 0, first, frames, random_cw,
                                                  _p(buf) if counters else None, None)


def _channel(code, ch, det, first=0, frames=16, recv=True, er=True, off=True):
    buf = np.zeros((max(frames, 1), code.n), np.uint8)
    e, o = np.zeros(frames * code.n + 1, np.uint16), np.zeros(frames + 1, np.uint32)
    return capi.lib().cc_burst_erasure_channel_dev(code._h, _ref(ch), _ref(det), 0, first, frames, 0,
                                                   _p(buf) if recv else None, None, None, None, _p(e) if er else None,
                                                   _p(o) if off else None, None)


def _last():
    return capi.lib().cc_last_error().decode()


def _codes():
    return (cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE),
            cc.primitive_bch(6, cc.errors(3), cc.peterson_gorenstein_zierler_tag(), device=capi.DEVICE_NONE),
            cc.rs(8, cc.errors(8), cc.euklid_tag(), n=204, device=capi.DEVICE_NONE),
            cc.primitive_bch(6, cc.errors(3), cc.min_sum_tag(10), device=capi.DEVICE_NONE))


def test_good_arguments_reach_the_device_check():
    for code in _codes():
        for kw in (GOOD, dict(GOOD, interleave=1), dict(GOOD, interleave=256, p_gb=1.0, p_bg=1.0)):
            ch = capi.BurstChannel(**kw)
            frames = 2 * kw["interleave"]
            for d in ((0.9, 0.002), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)):
                det = capi.BurstDetector(*d)
                assert _mc(code, ch, det, 4 * kw["interleave"], frames) == capi.ERR_NO_DEVICE, (kw, d)
                assert _channel(code, ch, det, 0, frames) == capi.ERR_NO_DEVICE, (kw, d)
                assert _channel(code, ch, det, 0, frames, er=False, off=False) == capi.ERR_NO_DEVICE  # the CSR is optional
        assert _mc(code, capi.BurstChannel(**GOOD), capi.BurstDetector(0.9, 0.002), frames=0) == capi.ERR_NO_DEVICE


def test_everything_the_burst_route_refuses_is_refused():
    det = capi.BurstDetector(0.9, 0.002)
    bad = [dict(GOOD, interleave=0), dict(GOOD, interleave=257), dict(GOOD, p_gb=0.0, p_bg=0.0)]
    for name in ("p_gb", "p_bg", "p_error_good", "p_error_bad"):
        bad += [dict(GOOD, **{name: v}) for v in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf"))]
    for code in _codes():
        for kw in bad:
            ch = capi.BurstChannel(**kw)
            assert _mc(code, ch, det) == capi.ERR_INVALID_ARGUMENT, kw
            assert _channel(code, ch, det) == capi.ERR_INVALID_ARGUMENT, kw
        ch = capi.BurstChannel(**GOOD)
        for size in (0, 39, 48):  # struct_size of the channel
            ch.struct_size = size
            assert _mc(code, ch, det) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch, det) == capi.ERR_INVALID_ARGUMENT
        ch = capi.BurstChannel(**GOOD)
        assert _mc(code, None, det) == capi.ERR_INVALID_ARGUMENT and _channel(code, None, det) == capi.ERR_INVALID_ARGUMENT
        assert _mc(code, ch, det, counters=False) == capi.ERR_INVALID_ARGUMENT
        assert _channel(code, ch, det, recv=False) == capi.ERR_INVALID_ARGUMENT
        assert _mc(code, ch, det, 0, 18) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch, det, 0, 18) == capi.ERR_INVALID_ARGUMENT
        assert _mc(code, ch, det, 6, 16) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch, det, 6, 16) == capi.ERR_INVALID_ARGUMENT
        assert "multiples of the interleaving depth" in _last()
    ch = capi.BurstChannel(**GOOD)
    wide = cc.rs(9, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x211, device=capi.DEVICE_NONE)
    assert _mc(wide, ch, det) == capi.ERR_UNSUPPORTED and _channel(wide, ch, det) == capi.ERR_UNSUPPORTED
    mu0 = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), mu=0, device=capi.DEVICE_NONE)
    assert _mc(mu0, ch, det) == capi.ERR_UNSUPPORTED and "mu = step = 1" in _last()
    bch = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    matrix_only = cc.min_sum_decoder(bch.H(), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    assert _mc(matrix_only, ch, det) == capi.ERR_INVALID_ARGUMENT and _channel(matrix_only, ch, det) == capi.ERR_INVALID_ARGUMENT


def _detector(size=24, reserved=0, p_detect=0.9, p_false_alarm=0.002):
    det = capi.BurstDetector(p_detect, p_false_alarm)
    det.struct_size, det.reserved = size, reserved
    return det


def test_the_detector_refusals_and_their_order():
    """After the burst channel's own checks: NULL det, struct_size, reserved, the probabilities, one CSR pointer, RS + PGZ
    -- each the first complaint of a call that also has every later fault, and none of them before a fault of the channel."""
    ch = capi.BurstChannel(**GOOD)
    rs_pgz = cc.rs(8, cc.errors(8), cc.peterson_gorenstein_zierler_tag(), device=capi.DEVICE_NONE)
    bad_p = float("nan")
    # the ladder on the channel-only call, which has every fault to offer: (det, er, off, status, text of cc_last_error)
    ladder = [
        (None, True, False, capi.ERR_INVALID_ARGUMENT, "cc_burst_detector: NULL"),
        (_detector(size=16, reserved=1, p_detect=bad_p), True, False, capi.ERR_INVALID_ARGUMENT, "struct_size"),
        (_detector(reserved=1, p_detect=bad_p), True, False, capi.ERR_INVALID_ARGUMENT, "reserved must be 0"),
        (_detector(p_detect=bad_p), True, False, capi.ERR_INVALID_ARGUMENT, "p_detect and p_false_alarm"),
        (_detector(), True, False, capi.ERR_INVALID_ARGUMENT, "both or neither"),
        (_detector(), False, True, capi.ERR_INVALID_ARGUMENT, "both or neither"),
        (_detector(), True, True, capi.ERR_UNSUPPORTED, "PGZ-Algorithm does not support erasure decoding"),
    ]
    for det, er, off, status, text in ladder:
        assert _channel(rs_pgz, ch, det, er=er, off=off) == status, text
        assert text in _last()
        # a fault of the channel comes first
        assert _channel(rs_pgz, capi.BurstChannel(**dict(GOOD, interleave=0)), det, er=er, off=off) == capi.ERR_INVALID_ARGUMENT
        assert "interleaving depth is 1 .. 256" in _last()
    for det, _, _, status, text in ladder[:4] + ladder[6:]:
        assert _mc(rs_pgz, ch, det) == status and text in _last()
        assert _mc(rs_pgz, ch, det, 0, 18) == capi.ERR_INVALID_ARGUMENT and "multiples of the interleaving depth" in _last()
    # every probability fault, on handles that have no other
    for code in _codes():
        for size in (0, 23, 32):
            assert _mc(code, ch, _detector(size=size)) == capi.ERR_INVALID_ARGUMENT
            assert _channel(code, ch, _detector(size=size)) == capi.ERR_INVALID_ARGUMENT
        for name in ("p_detect", "p_false_alarm"):
            for v in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
                det = _detector(**{name: v})
                assert _mc(code, ch, det) == capi.ERR_INVALID_ARGUMENT, (name, v)
                assert _channel(code, ch, det) == capi.ERR_INVALID_ARGUMENT, (name, v)
    # RS + PGZ is refused for the erasures only: a detector that never flags reaches the device check, as does BCH + PGZ
    assert _mc(rs_pgz, ch, _detector(p_detect=0.0, p_false_alarm=0.0)) == capi.ERR_NO_DEVICE
    assert _channel(rs_pgz, ch, _detector(p_detect=0.0, p_false_alarm=0.0)) == capi.ERR_NO_DEVICE
    assert _mc(rs_pgz, ch, _detector(p_detect=0.0, p_false_alarm=1e-11)) == capi.ERR_NO_DEVICE  # llround gives DG = 0
    assert _mc(rs_pgz, ch, _detector(p_detect=0.0, p_false_alarm=1e-9)) == capi.ERR_UNSUPPORTED
    # the erasure offsets are 32-bit
    rs = cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)
    one = [np.zeros(1, t) for t in (np.uint8, np.uint16, np.uint32)]
    frames = ((1 << 32) // 255 + 4) // 4 * 4
    call = lambda f, er: capi.lib().cc_burst_erasure_channel_dev(  # noqa: E731  (the buffers are never touched)
        rs._h, C.byref(ch), C.byref(_detector()), 0, 0, f, 0, _p(one[0]), None, None, None, _p(one[1]) if er else None,
        _p(one[2]) if er else None, None)
    assert call(frames, True) == capi.ERR_INVALID_ARGUMENT and "32-bit" in _last()
    assert call(frames - 4, True) == capi.ERR_NO_DEVICE and call(frames, False) == capi.ERR_NO_DEVICE


# ---- the model ----
def test_model_identities():
    params, I, seed, first, frames, n = (0.02, 0.25, 0.001, 0.5), 3, 11, 3 << 33, 24, 7
    sent = np.arange(frames * n).reshape(frames, n) % 7 + 1  # no symbol 0: a flagged symbol shows in recv
    recv0, s0, state0, wrong0 = burst_model.channel(params, I, seed, first, frames, n, 8, sent)
    assert state0.any() and not state0.all()
    recv, s, state, flag, wrong = burst_erasure_model.channel(params, (1.0, 0.0), I, seed, first, frames, n, 8, sent)
    assert np.array_equal(flag, state) and np.array_equal(state, state0) and np.array_equal(s, s0)
    assert not recv[flag != 0].any() and np.array_equal(recv[flag == 0], recv0[flag == 0])
    assert np.array_equal(wrong, wrong0 & (state == 0))
    recv, _, state, flag, _ = burst_erasure_model.channel(params, (0.0, 1.0), I, seed, first, frames, n, 8, sent)
    assert np.array_equal(flag, 1 - state)
    recv, _, _, flag, wrong = burst_erasure_model.channel(params, (0.0, 0.0), I, seed, first, frames, n, 8, sent)
    assert not flag.any() and np.array_equal(recv, recv0) and np.array_equal(wrong, wrong0)
    recv, _, _, flag, wrong = burst_erasure_model.channel(params, (1.0, 1.0), I, seed, first, frames, n, 8, sent)
    assert flag.all() and not recv.any() and not wrong.any()
    assert burst_erasure_model.detector_thresholds(1.0, 0.0) == (1 << 32, 0)
    assert burst_erasure_model.detector_thresholds(0.25, 1e-11) == (1 << 30, 0)


def test_model_lists_are_per_frame_in_frame_major_numbering():
    flag = np.zeros((2, 5, 3), np.uint8)  # 2 blocks of depth 3, n = 5
    flag[0, 4, 1] = flag[0, 0, 1] = flag[1, 2, 0] = flag[1, 3, 2] = flag[1, 1, 2] = 1
    lists = burst_erasure_model.frame_lists(flag)
    assert lists == [[], [0, 4], [], [2], [], [1, 3]]
    vals, off = burst_erasure_model.csr(lists)
    assert vals.tolist() == [0, 4, 2, 1, 3] and off.tolist() == [0, 0, 2, 2, 3, 3, 5]
    # the rows of the de-interleaved flags
    rows = cc.deinterleave(flag, 3)
    assert [np.flatnonzero(r).tolist() for r in rows] == lists


# ---- the harness with a stub backend ----
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return capi.OK
        return fn


def test_backend_picks_the_entry_point(monkeypatch):
    torch = pytest.importorskip("torch")
    rec = _Recorder()
    monkeypatch.setattr(capi, "lib", lambda: rec)
    code = StubCode()
    code._h = None

    def backend(**kw):
        b = BurstBackend.__new__(BurstBackend)
        b.torch, b.code, b.device, b.random_codewords = torch, code, "cpu", True
        b.interleave, b.p_gb, b.p_bg, b.p_error_good = 4, 0.02, 0.25, 0.001
        b.p_detect, b.p_false_alarm = kw.get("p_detect", 0.0), kw.get("p_false_alarm", 0.0)
        return b

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device: type("S", (), {"cuda_stream": 0})())
    backend().run(0.5, 1, 8, 16)
    backend(p_detect=0.9, p_false_alarm=0.002).run(0.5, 1, 8, 16)
    backend(p_false_alarm=0.01).run(0.5, 1, 8, 16)
    assert [c[0] for c in rec.calls] == ["cc_mc_run_burst_dev", "cc_mc_run_burst_erasure_dev",
                                         "cc_mc_run_burst_erasure_dev"]
    assert len(rec.calls[0][1]) == 8 and len(rec.calls[1][1]) == 9  # exactly the call as it was, then with the detector
    det = rec.calls[1][1][2]._obj
    assert (det.struct_size, det.reserved, det.p_detect, det.p_false_alarm) == (24, 0, 0.9, 0.002)


def test_burst_simulation_with_a_detector(tmp_path):
    kw = dict(interleave=16, p_gb=0.005, p_bg=0.1, p_error_good=1e-4, points=[0.3, 0.1], max_samples=20000)
    plain = burst_simulation(StubCode(), backend=StubBackend(), log_dir=str(tmp_path / "a"), **kw)
    zero = burst_simulation(StubCode(), backend=StubBackend(), log_dir=str(tmp_path / "b"), p_detect=0.0,
                            p_false_alarm=0.0, **kw)
    det = burst_simulation(StubCode(), backend=StubBackend(), log_dir=str(tmp_path / "c"), p_detect=0.9,
                           p_false_alarm=0.002, **kw)
    for d in "abc":
        (tmp_path / d).mkdir()
    r_plain, r_zero, r_det = plain(), zero(), det()
    name = "(255, 223, 33)-STUB.burst.log"
    a, b, c = ((tmp_path / d / name).read_bytes() for d in "abc")
    assert a == b and a.splitlines()[0] == b"      p                   wer"  # no detector: byte-identical
    assert r_plain == r_zero and "p_detect" not in r_plain[0]
    lines = c.decode().splitlines()
    assert lines[0] == "      p                   wer  detector p_detect=0.9 p_false_alarm=0.002"
    assert lines[1:] == a.decode().splitlines()[1:]  # the stub does not know the detector: the same rows
    assert r_det[0]["p_detect"] == 0.9 and r_det[0]["p_false_alarm"] == 0.002 and "channel_erasures" in r_det[0]
    with pytest.raises(TypeError):  # keyword-only
        burst_simulation(StubCode(), 16, 0.005, 0.1, 1e-4, None, [0.3], 0, True, StubBackend(), None, None, None, 0.9)
    for bad in (dict(p_detect=1.5), dict(p_false_alarm=-0.1), dict(p_detect=float("nan"))):
        with pytest.raises(ValueError):
            burst_simulation(StubCode(), backend=StubBackend(), **bad)


def test_cli_takes_the_detector(monkeypatch, tmp_path):
    from channelcoding_amd import benchmark
    seen = []

    def fake(code, **kw):
        seen.append(kw)
        return lambda: [{"frames": 5}]

    monkeypatch.setattr(benchmark, "burst_simulation", fake)
    monkeypatch.setattr(benchmark, "build", lambda name, k, d, stop_rule: benchmark.cc.primitive_bch(
        k, benchmark.cc.dmin(d), benchmark.ALGORITHMS[name](), stop_rule=stop_rule, device=capi.DEVICE_NONE))
    argv = ["--simulation", "burst", "--algorithm", "bm", "--k", "5", "--dmin", "5", "--log-dir", str(tmp_path)]
    assert benchmark.main(argv + ["--p-detect", "0.9", "--p-false-alarm", "0.002", "--interleave", "8"]) == 0
    assert seen[-1]["p_detect"] == 0.9 and seen[-1]["p_false_alarm"] == 0.002 and seen[-1]["interleave"] == 8
    assert benchmark.main(argv + ["--p-false-alarm", "0.01"]) == 0
    assert seen[-1]["p_detect"] == 0.0 and seen[-1]["p_false_alarm"] == 0.01
    assert benchmark.main(argv) == 0
    assert "p_detect" not in seen[-1] and "p_false_alarm" not in seen[-1]  # the defaults: the call as it always was
    usage = benchmark.usage_text()
    assert "--p-detect <value>" in usage and "--p-false-alarm <value>" in usage
