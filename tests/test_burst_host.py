"""CPU tests of the Gilbert-Elliott burst channel (cc_burst_channel_dev / cc_mc_run_burst_dev,
montecarlo.burst_simulation, `benchmark --simulation burst`): the C ABI's argument checks on handles without a device,
the harness with a stub backend, and the sanity of the numpy model of tests/burst_model.py, against which
tests/test_gpu_burst.py compares the device symbol for symbol."""
import ctypes as C
import math

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import (CHANNELS, DISCRETE_COUNTER_NAMES, burst_simulation, discrete_ladder, samples,
                                          shard, shard_blocks)
import burst_model
from test_discrete_host import StubBackend, StubCode
from test_host_logic import header_symbols

GOOD = dict(interleave=4, p_gb=0.02, p_bg=0.25, p_error_good=0.001, p_error_bad=0.5)


# ---- the C ABI ----
def test_symbols_are_declared_bound_and_exported():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("cc_burst_channel_dev", "cc_mc_run_burst_dev"):
        assert name in header_symbols() and name in capi.exported_symbols() and hasattr(lib, name)
    assert C.sizeof(capi.BurstChannel) == 40 and capi.BurstChannel().struct_size == 40
    assert CHANNELS == ("bsc", "bec", "bsec")  # the burst channel is a simulation of its own


def _mc(code, ch, first=0, frames=16, counters=True, random_cw=0):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_burst_dev(code._h, C.byref(ch) if ch is not None else None, 0, first, frames, random_cw,
                                          buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def _channel(code, ch, first=0, frames=16, recv=True):
    buf = np.zeros((frames, code.n), np.uint8)
    return capi.lib().cc_burst_channel_dev(code._h, C.byref(ch) if ch is not None else None, 0, first, frames, 0,
                                           buf.ctypes.data_as(C.c_void_p) if recv else None, None, None, None)


def _codes():
    return (cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE),
            cc.rs(8, cc.errors(8), cc.euklid_tag(), n=204, device=capi.DEVICE_NONE),
            cc.primitive_bch(6, cc.errors(3), cc.min_sum_tag(10), device=capi.DEVICE_NONE))


def test_good_arguments_reach_the_device_check():
    for code in _codes():
        for kw in (GOOD, dict(GOOD, interleave=1), dict(GOOD, interleave=256, p_gb=1.0, p_bg=1.0),
                   dict(GOOD, p_gb=0.0, p_error_good=0.0, p_error_bad=1.0), dict(GOOD, p_bg=0.0)):
            ch = capi.BurstChannel(**kw)
            frames = 2 * kw["interleave"]
            assert _mc(code, ch, 4 * kw["interleave"], frames) == capi.ERR_NO_DEVICE, kw
            assert _channel(code, ch, 0, frames) == capi.ERR_NO_DEVICE, kw
        assert _mc(code, capi.BurstChannel(**GOOD), frames=0) == capi.ERR_NO_DEVICE


def test_bad_arguments_are_refused():
    bad = [dict(GOOD, interleave=0), dict(GOOD, interleave=257), dict(GOOD, p_gb=0.0, p_bg=0.0)]
    for name in ("p_gb", "p_bg", "p_error_good", "p_error_bad"):
        bad += [dict(GOOD, **{name: v}) for v in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf"))]
    for code in _codes():
        for kw in bad:
            ch = capi.BurstChannel(**kw)
            assert _mc(code, ch) == capi.ERR_INVALID_ARGUMENT, kw
            assert _channel(code, ch) == capi.ERR_INVALID_ARGUMENT, kw
        ch = capi.BurstChannel(**GOOD)
        for size in (0, 39, 48):  # struct_size
            ch.struct_size = size
            assert _mc(code, ch) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch) == capi.ERR_INVALID_ARGUMENT
        ch = capi.BurstChannel(**GOOD)
        assert _mc(code, None) == capi.ERR_INVALID_ARGUMENT and _channel(code, None) == capi.ERR_INVALID_ARGUMENT
        assert _mc(code, ch, counters=False) == capi.ERR_INVALID_ARGUMENT
        assert _channel(code, ch, recv=False) == capi.ERR_INVALID_ARGUMENT
        # frames and first_frame are multiples of the depth
        assert _mc(code, ch, 0, 18) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch, 0, 18) == capi.ERR_INVALID_ARGUMENT
        assert _mc(code, ch, 6, 16) == capi.ERR_INVALID_ARGUMENT and _channel(code, ch, 6, 16) == capi.ERR_INVALID_ARGUMENT
        assert "multiples of the interleaving depth" in capi.lib().cc_last_error().decode()


def test_handles_the_burst_route_does_not_serve():
    ch = capi.BurstChannel(**GOOD)
    wide = cc.rs(9, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x211, device=capi.DEVICE_NONE)
    assert _mc(wide, ch) == capi.ERR_UNSUPPORTED and _channel(wide, ch) == capi.ERR_UNSUPPORTED
    mu0 = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), mu=0, device=capi.DEVICE_NONE)
    assert _mc(mu0, ch) == capi.ERR_UNSUPPORTED and "mu = step = 1" in capi.lib().cc_last_error().decode()
    bch = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    matrix_only = cc.min_sum_decoder(bch.H(), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    assert _mc(matrix_only, ch) == capi.ERR_INVALID_ARGUMENT and _channel(matrix_only, ch) == capi.ERR_INVALID_ARGUMENT


# ---- the harness with a stub backend ----
def test_shards_are_whole_blocks_and_cover_the_total():
    for I in (1, 3, 16, 256):
        for total_blocks in (0, 1, 7, 1000):
            for world in (1, 2, 3, 8):
                parts = [shard_blocks(total_blocks * I, r, world, I) for r in range(world)]
                assert all(lo % I == 0 and count % I == 0 for lo, count in parts)
                assert parts[0][0] == 0 and sum(count for _, count in parts) == total_blocks * I
                assert all(a[0] + a[1] == b[0] for a, b in zip(parts, parts[1:]))
    assert shard_blocks(1000, 1, 3, 1) == shard(1000, 1, 3)


def test_burst_simulation_with_a_stub_backend(tmp_path):
    backend = StubBackend()
    sim = burst_simulation(StubCode(), interleave=16, p_gb=0.005, p_bg=0.1, p_error_good=1e-4, points=[0.3, 0.1, 0.03],
                           backend=backend, max_samples=60000, log_dir=str(tmp_path))
    assert sim.counter_names is DISCRETE_COUNTER_NAMES
    res = sim()
    assert res[0]["frames"] == 10000  # wer = 0.5 seeds 10000 samples, a multiple of 16
    for r0, r1 in zip(res, res[1:]):
        want = min(60000, samples(r0["word_errors"] / r0["frames"]))
        assert r1["frames"] == -(-want // 16) * 16  # whole blocks
    assert all(first % 16 == 0 and frames % 16 == 0 for _, first, frames in backend.calls)
    assert [c[1] for c in backend.calls] == [(i << 40) // 16 * 16 for i in range(3)]
    assert res[1]["p_error_bad"] == 0.1 and res[1]["interleave"] == 16 and "channel_erasures" in res[1]
    text = (tmp_path / "(255, 223, 33)-STUB.burst.log").read_text().splitlines()
    assert text[0] == "      p                   wer" and len(text) == 4 and text[1].startswith("    0.3 ")
    with pytest.raises(RuntimeError, match="already exists"):
        sim()
    # a depth that does not divide 2^40: every point still starts on a block
    backend = StubBackend()
    burst_simulation(StubCode(), interleave=12, points=[0.3, 0.1], backend=backend, samples_per_point=100)()
    assert [(first % 12, frames) for _, first, frames in backend.calls] == [(0, 108), (0, 108)]
    assert burst_simulation(StubCode(), backend=StubBackend()).points() == discrete_ladder()
    assert burst_simulation(StubCode(), p_error_bad=0.25, backend=StubBackend()).points() == [0.25]
    for kw in (dict(interleave=0), dict(interleave=257), dict(p_gb=0.0, p_bg=0.0), dict(p_gb=1.5), dict(points=[-0.1]),
               dict(p_error_good=float("nan"))):
        with pytest.raises(ValueError):
            burst_simulation(StubCode(), backend=StubBackend(), **kw)


def test_cli_runs_the_burst_simulation(monkeypatch, tmp_path):
    from channelcoding_amd import benchmark
    seen = []

    def fake(code, **kw):
        seen.append((code.to_string(), kw))
        return lambda: [{"frames": 5}]

    monkeypatch.setattr(benchmark, "burst_simulation", fake)
    monkeypatch.setattr(benchmark, "build", lambda name, k, d, stop_rule: benchmark.cc.primitive_bch(
        k, benchmark.cc.dmin(d), benchmark.ALGORITHMS[name](), stop_rule=stop_rule, device=capi.DEVICE_NONE))
    argv = ["--algorithm", "bm", "--k", "5", "--dmin", "5", "--seed", "9", "--log-dir", str(tmp_path)]
    assert benchmark.main(["--simulation", "burst", "--interleave", "8", "--p-gb", "0.02", "--p-bg", "0.2", "--p-good",
                           "0.001", "--p", "0.5", "--p", "0.25", "--max-samples", "1000"] + argv) == 0
    assert seen == [("(31, 21, 5)-BM", dict(interleave=8, p_gb=0.02, p_bg=0.2, p_error_good=0.001, points=[0.5, 0.25],
                                             seed=9, log_dir=str(tmp_path), max_samples=1000))]
    assert benchmark.main(["--simulation", "burst"] + argv) == 0
    assert seen[-1][1]["points"] is None and seen[-1][1]["interleave"] == 1  # the default ladder at depth 1
    assert benchmark.main(["--simulation", "fading"]) == 1
    usage = benchmark.usage_text()
    for word in ("burst", "--interleave", "--p-gb", "--p-bg", "--p-good"):
        assert word in usage


# ---- the model ----
def test_model_thresholds_and_edges():
    assert burst_model.thresholds(0.0, 1.0, 0.25, 1.0) == (0, 1 << 32, 1 << 30, 1 << 32, 0)
    assert burst_model.thresholds(0.5, 0.5, 0.0, 0.0)[4] == 1 << 31
    # p_gb = 0: never bad; p_gb = p_bg = 1: every step swaps the state, whatever the start
    assert not burst_model.states(0.0, 0.3, 7, 5, 4, 300).any()
    st = burst_model.states(1.0, 1.0, 7, (1 << 32) - 2, 6, 301)
    assert np.array_equal(st, st[:, :1] ^ (np.arange(301) & 1)[None, :]) and len(set(st[:, 0])) == 2
    recv, sent, state, wrong = burst_model.channel((0.5, 0.5, 1.0, 1.0), 3, 5, 9, 6, 7, 8)
    assert recv.shape == (2, 7, 3) and wrong.all() and recv.min() >= 1 and recv.max() <= 7 and not sent.any()
    recv, _, state, wrong = burst_model.channel((0.3, 0.3, 0.0, 1.0), 2, 5, 0, 8, 15, 2)
    assert np.array_equal(wrong, state != 0) and np.array_equal(recv, state)  # BCH: e = 1 exactly where bad
    words = np.arange(6 * 7).reshape(6, 7)
    assert np.array_equal(burst_model.to_transmission_order(words, 3).reshape(2, 7, 3), cc.interleave(words, 3))


def test_model_stationary_fraction_and_run_lengths():
    """One fixed seed, M = 2^20 symbols in 16 blocks of 65536.  The bad-state fraction is the sample mean of a stationary
    two-state chain with second eigenvalue lam = 1 - p_gb - p_bg: its variance over N steps is at most
    pi_G pi_B (1 + lam) / ((1 - lam) N) for lam >= 0 (the finite-N correction is negative), and the blocks are
    independent.  A bad run is geometric with parameter p_bg from wherever it is entered (mean 1 / p_bg, variance
    (1 - p_bg) / p_bg^2), runs are independent of each other; the runs cut by a block's end, one per block at the most,
    are left out (16 of several thousand: their weight in the mean is far below the bound).  Both within 6 standard
    deviations."""
    p_gb, p_bg, blocks, N = 0.02, 0.25, 16, 1 << 16
    st = burst_model.states(p_gb, p_bg, 0xC0FFEE, 1 << 33, blocks, N)
    M = blocks * N
    pi_b = p_gb / (p_gb + p_bg)
    lam = 1.0 - p_gb - p_bg
    sd = math.sqrt((1 - pi_b) * pi_b * (1 + lam) / ((1 - lam) * M))
    assert abs(st.mean() - pi_b) < 6 * sd, (st.mean(), pi_b, sd)
    runs = []
    for row in st:
        edges = np.flatnonzero(np.diff(np.concatenate(([0], row, [0]))))
        starts, ends = edges[0::2], edges[1::2]
        runs.append((ends - starts)[ends < N])
    runs = np.concatenate(runs)
    assert runs.size > 5000
    sd = math.sqrt((1 - p_bg) / p_bg ** 2 / runs.size)
    assert abs(runs.mean() - 1 / p_bg) < 6 * sd, (runs.mean(), 1 / p_bg, sd)
