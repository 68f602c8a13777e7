"""CPU tests of the Monte-Carlo route on packed words (cc_mc_run_bsc_packed_dev / cc_bsc_packed_channel_dev,
montecarlo.discrete_simulation(packed=True), montecarlo.hard_decision_p, `benchmark --simulation bsc --packed`): the
refusals and their order on CC_DEVICE_NONE handles -- every one of them comes before a device is asked for -- and the host
logic around the calls.  tests/test_gpu_packed_mc.py compares the device against the numpy channel model."""
import ctypes as C
import math

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import PackedBscBackend, discrete_simulation, hard_decision_p
from test_discrete_host import StubBackend, StubCode

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag


def _run(code, p, counters=True, random=0):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_bsc_packed_dev(code._h, float(p), 0, 0, 16, random,
                                               buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def _channel(code, p, recv=True, random=0):
    buf = np.zeros((16, (code.n + 7) // 8), np.uint8)
    return capi.lib().cc_bsc_packed_channel_dev(code._h, float(p), 0, 0, 16, random,
                                                buf.ctypes.data_as(C.c_void_p) if recv else None, None, None)


def served():
    """the handles of the packed calls: BCH, a hard tag, q = 3 .. 15, full length or shortened"""
    return [cc.primitive_bch(3, cc.errors(1), BM(), **NONE),
            cc.primitive_bch(8, cc.errors(3), cc.peterson_gorenstein_zierler_tag(), **NONE),
            cc.primitive_bch(8, cc.errors(3), cc.euklid_tag(), n=100, **NONE),
            cc.primitive_bch(8, cc.errors(3), BM(), coding="multiplication", **NONE),
            cc.primitive_bch(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE),
            cc.primitive_bch(14, cc.errors(12), BM(), modular_polynomial=0x402B, n=3240, **NONE),
            cc.primitive_bch(15, cc.errors(2), cc.euklid_tag(), modular_polynomial=0x8003, **NONE)]


def test_symbols_are_bound():
    for name in ("cc_mc_run_bsc_packed_dev", "cc_bsc_packed_channel_dev"):
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name)
    assert cc.bsc_packed_channel is not None and "bsc_packed_channel" in cc.__all__


def test_valid_calls_reach_the_device_check():
    for code in served():
        for p in (0.0, 0.004, 0.5, 1.0):
            for random in (0, 1):
                assert _run(code, p, random=random) == capi.ERR_NO_DEVICE, (code.to_string(), p)
                assert _channel(code, p, random=random) == capi.ERR_NO_DEVICE, (code.to_string(), p)


def test_bad_arguments_are_refused_before_the_device():
    for code in served():
        for p in (-1e-9, 1.0 + 1e-9, 1.5, float("nan"), float("inf"), -float("inf")):
            assert _run(code, p) == capi.ERR_INVALID_ARGUMENT, p
            assert _channel(code, p) == capi.ERR_INVALID_ARGUMENT, p
            assert "p_error" in capi.lib().cc_last_error().decode()
        assert _run(code, 0.01, counters=False) == capi.ERR_INVALID_ARGUMENT
        assert _channel(code, 0.01, recv=False) == capi.ERR_INVALID_ARGUMENT
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    assert capi.lib().cc_mc_run_bsc_packed_dev(None, 0.01, 0, 0, 16, 0, buf.ctypes.data_as(C.c_void_p),
                                               None) == capi.ERR_INVALID_ARGUMENT


def test_handles_without_a_packed_form_are_unsupported_with_the_packed_calls_text():
    bch = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    refused = [(cc.rs(8, cc.errors(16), BM(), **NONE), "binary (BCH)"),
               (cc.rs(10, cc.errors(4), BM(), modular_polynomial=0x409, **NONE), "binary (BCH)"),
               (bch, "hard-decision"),
               (cc.min_sum_decoder(bch.H(), cc.min_sum_tag(10), **NONE), "cc_minsum_create")]
    lib = capi.lib()
    for code, text in refused:
        assert lib.cc_packed_bytes(code._h, 0) == -capi.ERR_UNSUPPORTED
        want = lib.cc_last_error().decode()
        assert text in want
        for call in (_run, _channel):
            # the handle decides before the probability does: a bad p on such a handle is still "unsupported"
            for p in (0.01, 1.5):
                assert call(code, p) == capi.ERR_UNSUPPORTED, (text, p)
                assert lib.cc_last_error().decode() == want


def test_the_decoders_refusals_are_the_monte_carlo_calls():
    """The 16-bit route refuses the Euklid tag beyond t = 31: the Monte-Carlo call, which decodes, says so before the
    device; the channel-only call decodes nothing and reaches the device check."""
    code = cc.primitive_bch(10, cc.errors(32), cc.euklid_tag(), modular_polynomial=0x409, **NONE)
    assert _run(code, 0.01) == capi.ERR_UNSUPPORTED and "Euklid" in capi.lib().cc_last_error().decode()
    assert _run(code, 1.5) == capi.ERR_INVALID_ARGUMENT  # (arguments first)
    assert _channel(code, 0.01) == capi.ERR_NO_DEVICE
    bm = cc.primitive_bch(10, cc.errors(32), BM(), modular_polynomial=0x409, **NONE)
    assert _run(bm, 0.01) == capi.ERR_NO_DEVICE


def test_the_byte_monte_carlo_calls_keep_refusing_long_codes():
    code = cc.primitive_bch(10, cc.errors(2), BM(), modular_polynomial=0x409, **NONE)
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    rc = capi.lib().cc_mc_run_discrete_dev(code._h, 0.01, 0.0, 0, 0, 16, 0, buf.ctypes.data_as(C.c_void_p), None)
    assert rc == capi.ERR_UNSUPPORTED


def test_packed_simulation_is_the_bsc_only():
    for channel in ("bec", "bsec", "BEC"):
        with pytest.raises(ValueError, match="packed"):
            discrete_simulation(StubCode(), channel=channel, packed=True, backend=StubBackend())
    with pytest.raises(ValueError):
        discrete_simulation(StubCode(), channel="fading", packed=True, backend=StubBackend())
    sim = discrete_simulation(StubCode(), channel="bsc", packed=True, backend=StubBackend(), points=[0.01])
    assert sim.packed and sim.points() == [0.01]
    assert not discrete_simulation(StubCode(), backend=StubBackend()).packed
    assert PackedBscBackend.run is not None


def test_packed_simulation_log_name(tmp_path):
    sim = discrete_simulation(StubCode(), "bsc", points=[0.1, 0.03], backend=StubBackend(), max_samples=1000,
                              log_dir=str(tmp_path), packed=True)
    res = sim()
    assert [r["p_error"] for r in res] == [0.1, 0.03]
    lines = (tmp_path / "(255, 223, 33)-STUB.bsc.log").read_text().splitlines()  # the byte route's name
    assert lines[0] == "%7s %21s" % ("p", "wer") and len(lines) == 3


def test_hard_decision_p():
    code = cc.primitive_bch(8, cc.errors(3), BM(), **NONE)
    long_code = cc.primitive_bch(14, cc.errors(12), BM(), modular_polynomial=0x402B, n=3240, **NONE)
    for c in (code, long_code):
        for ebno in (0.0, 6.5):
            sigma = 1.0 / math.sqrt(2.0 * c.rate * 10.0 ** (ebno / 10.0))  # simulation.c++:83-85
            assert c.sigma(ebno) == pytest.approx(sigma, rel=1e-12)
            want = 0.5 * math.erfc(1.0 / (sigma * math.sqrt(2.0)))
            assert hard_decision_p(c, ebno) == pytest.approx(want, rel=1e-12)
    # Q(sqrt(2 R Eb/N0)): BCH(255,231) at 6.5 dB, R = 231/255, is Q(2.84479); a table of the normal distribution has
    # Q(2.84) = 2.2557e-3 and Q(2.85) = 2.1860e-3, linear interpolation between them 2.2223e-3 (good to ~1e-6)
    assert hard_decision_p(code, 6.5) == pytest.approx(2.2223e-3, rel=1e-3)
    assert 0.0 < hard_decision_p(code, 8.0) < hard_decision_p(code, 6.5) < hard_decision_p(code, 0.0) < 0.5


def test_cli_packed_flag(monkeypatch, tmp_path):
    from channelcoding_amd import benchmark
    seen = []

    def fake(code, channel, points=None, seed=0, log_dir=None, max_samples=None, **kw):
        seen.append((code.to_string(), channel, points, kw))
        return lambda: [{"frames": 5}]

    monkeypatch.setattr(benchmark, "discrete_simulation", fake)
    monkeypatch.setattr(benchmark, "build", lambda name, k, d, stop_rule: benchmark.cc.primitive_bch(
        k, benchmark.cc.dmin(d), benchmark.ALGORITHMS[name](), stop_rule=stop_rule, device=capi.DEVICE_NONE))
    argv = ["--algorithm", "bm", "--k", "5", "--dmin", "5", "--log-dir", str(tmp_path)]
    assert benchmark.main(["--simulation", "bsc", "--packed", "--p", "0.01"] + argv) == 0
    assert seen == [("(31, 21, 5)-BM", "bsc", [0.01], {"packed": True})]
    assert benchmark.main(["--simulation", "bsc", "--p", "0.01"] + argv) == 0 and seen[-1][3] == {}
    assert benchmark.main(["--simulation", "bec", "--packed"] + argv) == 1 and len(seen) == 2
    assert benchmark.main(["--simulation", "awgn", "--packed"] + argv) == 1 and len(seen) == 2
    assert "--packed" in benchmark.usage_text()
