"""CPU tests of the discrete-channel Monte-Carlo (cc_mc_run_discrete_dev / cc_discrete_channel_dev,
montecarlo.discrete_simulation, `benchmark --simulation bsc|bec`).

The channel model is restated here in numpy -- Philox4x32-10, the class draw, the error value, the messages -- and
tests/test_gpu_discrete_mc.py compares the device against this restatement symbol for symbol."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import (CHANNELS, DISCRETE_COUNTER_NAMES, awgn_simulation, channel_probabilities,
                                          discrete_ladder, discrete_simulation, samples)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = np.uint64(0xFFFFFFFF)


# ---- the numpy restatement of the channel ----
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123) on arrays of counters; returns the four output words as uint64 arrays < 2^32."""
    c = [np.asarray(x, np.uint64) & MASK for x in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(k0) & MASK, np.uint64(k1) & MASK
    M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def thresholds(p_error, p_erasure):
    """(E, E + P): erased below E, in error in [E, E + P); round half away from zero, as llround."""
    E = int(math.floor(p_erasure * 2.0 ** 32 + 0.5))
    P = int(math.floor(p_error * 2.0 ** 32 + 0.5))
    return E, E + P


def symbol_words(seed, first, frames, length, domain):
    """word (j & 3) of counter (gf_lo, gf_hi, j >> 2, domain) for every frame gf and symbol j: (frames, length)."""
    gf = np.uint64(first) + np.arange(frames, dtype=np.uint64)[:, None]
    j = np.arange(length, dtype=np.uint64)[None, :]
    w = philox4x32_10(gf & MASK, gf >> np.uint64(32), j >> np.uint64(2), domain, seed & 0xFFFFFFFF, seed >> 32)
    sel = (j & np.uint64(3)).astype(np.int64)
    return np.choose(np.broadcast_to(sel, (frames, length)), w)


def error_values(v, q_sym):
    """e = 1 + ((v (q_sym - 1)) >> 32): uniform over the non-zero symbols."""
    return (np.uint64(1) + ((np.asarray(v, np.uint64) * np.uint64(q_sym - 1)) >> np.uint64(32))).astype(np.int64)


def channel(p_error, p_erasure, seed, first, frames, n, q_sym, sent=None):
    """received symbols, erased mask, in-error mask of frames [first, first + frames) for the words `sent`."""
    E, EP = thresholds(p_error, p_erasure)
    u = symbol_words(seed, first, frames, n, 2)
    erased = u < np.uint64(E)
    wrong = ~erased & (u < np.uint64(EP))
    e = error_values(symbol_words(seed, first, frames, n, 3), q_sym)
    s = np.zeros((frames, n), np.int64) if sent is None else np.asarray(sent, np.int64)
    recv = np.where(erased, 0, np.where(wrong, s ^ e, s))
    return recv.astype(np.uint8), erased, wrong


def erasure_csr(erased):
    """frame f's erased positions, ascending, are values[off[f] .. off[f + 1])"""
    off = np.zeros(erased.shape[0] + 1, np.int64)
    off[1:] = np.cumsum(erased.sum(axis=1))
    return np.nonzero(erased)[1].astype(np.int64), off


def bch_message_bits(seed, first, frames, l):
    """message bit j = bit (j & 31) of word ((j >> 5) & 3) of counter (gf_lo, gf_hi, j >> 7, 1) (random_bits_kernel)."""
    gf = np.uint64(first) + np.arange(frames, dtype=np.uint64)[:, None]
    j = np.arange(l, dtype=np.uint64)[None, :]
    w = philox4x32_10(gf & MASK, gf >> np.uint64(32), j >> np.uint64(7), 1, seed & 0xFFFFFFFF, seed >> 32)
    sel = np.broadcast_to(((j >> np.uint64(5)) & np.uint64(3)).astype(np.int64), (frames, l))
    return ((np.choose(sel, w) >> (j & np.uint64(31))) & np.uint64(1)).astype(np.uint8)


def rs_message_symbols(seed, first, frames, l, q):
    """message symbol i = the low q bits of word (i & 3) of counter (gf_lo, gf_hi, i >> 2, 4)."""
    return (symbol_words(seed, first, frames, l, 4) & np.uint64((1 << q) - 1)).astype(np.uint8)


# ---- the restatement itself ----
def test_philox_known_answers():
    """Random123's known answers for philox4x32_10."""
    got = [int(w[()]) for w in philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    got = [int(w[()]) for w in philox4x32_10(f, f, f, f, f, f)]
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_class_thresholds_at_the_edges():
    assert thresholds(0.0, 0.0) == (0, 0)
    assert thresholds(0.0, 1.0) == (1 << 32, 1 << 32)
    assert thresholds(0.25, 0.75) == (3 << 30, 1 << 32)
    assert thresholds(1.0, 0.0) == (0, 1 << 32)
    frames, n = 40, 255
    recv, erased, wrong = channel(0.0, 0.2, 5, 1 << 33, frames, n, 256)
    assert not wrong.any() and erased.any() and (recv[erased] == 0).all()
    recv, erased, wrong = channel(0.0, 1.0, 5, 0, frames, n, 256)  # epsilon = 1: every symbol erased
    assert erased.all() and not wrong.any() and not recv.any()
    recv, erased, wrong = channel(0.3, 0.7, 5, 0, frames, n, 256)  # p + epsilon = 1: nothing intact
    assert (erased | wrong).all() and not (erased & wrong).any()
    assert (recv[wrong] != 0).all()  # error values are never 0
    recv, erased, wrong = channel(1.0, 0.0, 5, 0, frames, n, 2)  # BSC with p = 1 flips every bit
    assert (recv == 1).all()
    _, erased, wrong = channel(0.05, 0.0, 5, 0, frames, n, 2)
    assert not erased.any() and 0 < wrong.sum() < frames * n


def test_error_value_map():
    top = (1 << 32) - 1
    for q_sym in (2, 16, 256):
        e = error_values([0, 1, 1 << 31, top], q_sym)
        assert e.min() == 1 and e.max() == q_sym - 1 and e[0] == 1 and e[-1] == q_sym - 1
    assert (error_values(np.arange(0, 1 << 32, 65537, dtype=np.uint64), 2) == 1).all()  # BCH: always 1
    # every non-zero symbol of GF(2^8) takes the same share of the 2^32 words (to within one): value k + 1 from
    # v = ceil(k 2^32 / 255) on
    edges = [-(-(k << 32) // 255) for k in range(256)]
    counts = np.diff(edges)
    assert counts.max() - counts.min() <= 1
    for k in (1, 5, 254):
        assert error_values([edges[k] - 1, edges[k]], 256).tolist() == [k, k + 1]


def test_erasure_csr_order():
    erased = np.array([[0, 1, 0, 1], [0, 0, 0, 0], [1, 0, 0, 1]], bool)
    vals, off = erasure_csr(erased)
    assert off.tolist() == [0, 2, 2, 4] and vals.tolist() == [1, 3, 0, 3]


def test_message_restatements_shape():
    bits = bch_message_bits(3, 1 << 40, 50, 231)
    assert bits.shape == (50, 231) and set(np.unique(bits)) <= {0, 1} and 0.45 < bits.mean() < 0.55
    sym = rs_message_symbols(3, 1 << 40, 50, 223, 8)
    assert sym.shape == (50, 223) and 100 < sym.mean() < 155


# ---- the C ABI's argument checks (no GPU needed) ----
def _discrete(code, p, e, counters=True):
    buf = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    return capi.lib().cc_mc_run_discrete_dev(code._h, float(p), float(e), 0, 0, 16, 0,
                                             buf.ctypes.data_as(C.c_void_p) if counters else None, None)


def _channel(code, p, e):
    recv = np.zeros((16, code.n), np.uint8)
    return capi.lib().cc_discrete_channel_dev(code._h, float(p), float(e), 0, 0, 16, 0, recv.ctypes.data_as(C.c_void_p),
                                              None, None, None, None)


def test_bad_probabilities_are_refused():
    for code in (cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE),
                 cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)):
        for p, e in ((-0.1, 0.0), (0.0, -1e-9), (float("nan"), 0.0), (0.0, float("inf")), (0.6, 0.5), (1.5, 0.0)):
            assert _discrete(code, p, e) == capi.ERR_INVALID_ARGUMENT, (p, e)
            assert _channel(code, p, e) == capi.ERR_INVALID_ARGUMENT, (p, e)
        assert _discrete(code, 0.01, 0.0, counters=False) == capi.ERR_INVALID_ARGUMENT
        # valid points reach the device check
        for p, e in ((0.0, 0.0), (0.01, 0.0), (0.0, 1.0), (0.25, 0.75)):
            assert _discrete(code, p, e) == capi.ERR_NO_DEVICE, (p, e)
            assert _channel(code, p, 0.0) == capi.ERR_NO_DEVICE, (p, e)


def test_handles_the_discrete_route_does_not_serve():
    wide = cc.rs(10, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x409, device=capi.DEVICE_NONE)
    assert _discrete(wide, 0.01, 0.0) == capi.ERR_UNSUPPORTED
    bch = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    matrix_only = cc.min_sum_decoder(bch.H(), cc.min_sum_tag(10), device=capi.DEVICE_NONE)
    assert _discrete(matrix_only, 0.01, 0.0) == capi.ERR_INVALID_ARGUMENT
    assert _channel(matrix_only, 0.01, 0.0) == capi.ERR_INVALID_ARGUMENT
    for p, e in ((0.01, 0.0), (0.0, 0.01)):
        assert _discrete(bch, p, e) == capi.ERR_NO_DEVICE


def test_erasure_lists_of_one_call_fit_their_offsets():
    """cc_discrete_channel_dev's offsets are 32-bit (the Python tensor int32): one call's frames * n is bounded."""
    code = cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)
    recv, er, off = (np.zeros(1, t) for t in (np.uint8, np.uint16, np.uint32))
    frames = (1 << 32) // 255 + 1  # frames * 255 >= 2^32; the buffers are never touched
    rc = capi.lib().cc_discrete_channel_dev(code._h, 0.0, 0.1, 0, 0, frames, 0, recv.ctypes.data_as(C.c_void_p),
                                            er.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), None, None)
    assert rc == capi.ERR_INVALID_ARGUMENT and "32-bit" in capi.lib().cc_last_error().decode()
    rc = capi.lib().cc_discrete_channel_dev(code._h, 0.0, 0.1, 0, 0, frames - 1, 0, recv.ctypes.data_as(C.c_void_p),
                                            er.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), None, None)
    assert rc == capi.ERR_NO_DEVICE  # below the bound the call reaches the device check
    with pytest.raises(ValueError, match="2\\^31"):
        code.discrete_channel(0.0, 0.1, 0, 0, (1 << 31) // 255 + 1)


def test_counter_slot_and_names():
    assert capi.MC_CHANNEL_ERASURES == 7 and capi.MC_CHANNEL_ERASURES < capi.MC_ITER_HIST
    assert DISCRETE_COUNTER_NAMES["channel_erasures"] == capi.MC_CHANNEL_ERASURES
    from channelcoding_amd.montecarlo import COUNTER_NAMES
    assert "channel_erasures" not in COUNTER_NAMES  # awgn_simulation's result dicts stay as they are
    assert "cc_mc_run_discrete_dev" in capi.exported_symbols() and "cc_discrete_channel_dev" in capi.exported_symbols()


# ---- the harness with a stub backend ----
class StubCode:
    n, rate = 255, 223 / 255

    def to_string(self):
        return "(255, 223, 33)-STUB"


class StubBackend:
    """word error iff hash(global frame) falls under a threshold growing with the channel's probabilities"""

    def __init__(self):
        self.calls = []

    def run(self, point, seed, first_frame, frames):
        import torch
        self.calls.append((point, first_frame, frames))
        pe = point if not isinstance(point, tuple) else point[0] + 2 * point[1]
        idx = np.arange(first_frame, first_frame + frames, dtype=np.uint64)
        h = (idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(seed)) >> np.uint64(40)
        err = h < np.uint64(int((1 << 24) * min(1.0, 4 * pe)))
        c = np.zeros(capi.MC_NCOUNTERS, np.int64)
        c[capi.MC_FRAMES] = frames
        c[capi.MC_WORD_ERRORS] = int(err.sum())
        c[capi.MC_BIT_ERRORS] = int((h[err] % np.uint64(5)).sum())
        c[capi.MC_CHANNEL_ERASURES] = int((h % np.uint64(3)).sum())
        return torch.from_numpy(c)


def test_default_ladder():
    pts = discrete_ladder()
    assert len(pts) == 13 and pts[0] == pytest.approx(0.1) and pts[-1] == pytest.approx(1e-4)
    assert all(a > b for a, b in zip(pts, pts[1:]))  # noisiest first
    assert all(abs(x - 10 ** (-k / 4)) < 1e-15 for k, x in zip(range(4, 17), pts))
    assert discrete_simulation(StubCode(), "bsc", backend=StubBackend()).points() == pts
    assert discrete_simulation(StubCode(), "BEC", backend=StubBackend()).points() == pts
    assert discrete_simulation(StubCode(), "bsec", backend=StubBackend()).points() == [(x, x) for x in pts]
    assert CHANNELS == ("bsc", "bec", "bsec")


def test_points_are_checked():
    assert channel_probabilities("bsc", 0.01) == (0.01, 0.0)
    assert channel_probabilities("bec", 0.2) == (0.0, 0.2)
    assert channel_probabilities("bsec", (0.1, 0.3)) == (0.1, 0.3)
    for chan, pt in (("bsc", -0.1), ("bec", 1.5), ("bsec", (0.7, 0.7)), ("bsc", float("nan"))):
        with pytest.raises(ValueError):
            discrete_simulation(StubCode(), chan, points=[pt], backend=StubBackend())
    with pytest.raises(ValueError):
        discrete_simulation(StubCode(), "fading", backend=StubBackend())


def run_single(channel="bsc", points=(0.1, 0.03, 0.01, 0.003), log_dir=None):
    sim = discrete_simulation(StubCode(), channel, points=list(points), backend=StubBackend(), max_samples=60000,
                              log_dir=log_dir)
    return [(r["frames"], r["word_errors"], r["bit_errors"], r["channel_erasures"]) for r in sim()]


def test_adaptive_counts_and_frame_bases():
    backend = StubBackend()
    sim = discrete_simulation(StubCode(), "bsc", points=[0.1, 0.03, 0.01, 0.003], backend=backend, max_samples=60000)
    res = sim()
    assert res[0]["frames"] == 10000  # wer = 0.5 seeds 10000 samples
    for r0, r1 in zip(res, res[1:]):
        assert r1["frames"] == min(60000, samples(r0["word_errors"] / r0["frames"]))
    assert [c[1] for c in backend.calls] == [i << 40 for i in range(4)]
    assert res[1]["p_error"] == 0.03 and res[1]["p_erasure"] == 0.0 and "channel_erasures" in res[1]
    assert res[2]["wer"] == res[2]["word_errors"] / res[2]["frames"]
    assert res[2]["ber"] == res[2]["bit_errors"] / (res[2]["frames"] * 255)
    fixed = discrete_simulation(StubCode(), "bec", points=[0.2, 0.1], backend=StubBackend(), samples_per_point=777)()
    assert [r["frames"] for r in fixed] == [777, 777] and fixed[0]["p_erasure"] == 0.2


def test_log_format(tmp_path):
    run_single("bsc", log_dir=str(tmp_path))
    text = (tmp_path / "(255, 223, 33)-STUB.bsc.log").read_text().splitlines()
    assert text[0] == "%7s %21s" % ("p", "wer") == "      p                   wer"
    assert len(text) == 5 and text[1].startswith("    0.1 ") and text[2].startswith("   0.03 ")
    assert text[4].split()[0] == "0.003" and len(text[1]) == len("%7s %s" % ("0.1", "%16.15e" % 0.5))
    sim = discrete_simulation(StubCode(), "bsec", points=[(0.02, 0.1)], backend=StubBackend(), max_samples=100,
                              log_dir=str(tmp_path))
    sim()
    assert (tmp_path / "(255, 223, 33)-STUB.bsec.log").read_text().splitlines()[1].split()[0] == "0.02"  # shows p
    with pytest.raises(RuntimeError, match="already exists"):
        run_single("bsc", log_dir=str(tmp_path))
    # the AWGN log keeps its name and layout
    awgn_simulation(StubCode(), backend=StubBackend(), max_samples=100, start=7.0, log_dir=str(tmp_path))()
    lines = (tmp_path / "(255, 223, 33)-STUB.log").read_text().splitlines()
    assert lines[0] == "   ebno                   wer" and lines[1].startswith("      7 ") and lines[2].startswith("    7.5 ")


WORKER = r"""
import json, os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import torch.distributed as dist
from test_discrete_host import run_single
dist.init_process_group("gloo")
res = run_single("bsec", points=[(0.05, 0.1), (0.01, 0.02), (0.002, 0.001)])
with open(os.path.join(%(out)r, "rank%%d.json" %% dist.get_rank()), "w") as f:
    json.dump(res, f)
dist.barrier(); dist.destroy_process_group()
"""


def test_two_ranks_equal_one_rank(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % {"root": ROOT, "out": str(tmp_path)})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29637", str(script)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for rank in (0, 1):
        with open(tmp_path / ("rank%d.json" % rank)) as f:
            got[rank] = json.load(f)
    single = [list(x) for x in run_single("bsec", points=[(0.05, 0.1), (0.01, 0.02), (0.002, 0.001)])]
    assert got[0] == single and got[1] == single


# ---- the command line ----
def test_cli_runs_discrete_simulations(monkeypatch, tmp_path):
    from channelcoding_amd import benchmark
    seen = []

    def fake(code, channel, points=None, seed=0, log_dir=None, max_samples=None):
        seen.append((code.to_string(), channel, points, seed, log_dir, max_samples))
        return lambda: [{"frames": 5}]

    monkeypatch.setattr(benchmark, "discrete_simulation", fake)
    monkeypatch.setattr(benchmark, "build", lambda name, k, d, stop_rule: benchmark.cc.primitive_bch(
        k, benchmark.cc.dmin(d), benchmark.ALGORITHMS[name](), stop_rule=stop_rule, device=capi.DEVICE_NONE))
    argv = ["--algorithm", "bm", "--k", "5", "--dmin", "5", "--seed", "9", "--log-dir", str(tmp_path)]
    assert benchmark.main(["--simulation", "bsc", "--p", "0.01"] + argv) == 0
    assert seen == [("(31, 21, 5)-BM", "bsc", [0.01], 9, str(tmp_path), None)]
    assert benchmark.main(["--simulation", "bec", "--p", "0.1", "--p", "0.02", "--max-samples", "1000"] + argv) == 0
    assert seen[-1][1:3] == ("bec", [0.1, 0.02]) and seen[-1][5] == 1000
    assert benchmark.main(["--simulation", "bsc"] + argv) == 0 and seen[-1][2] is None  # the default ladder
    assert benchmark.main(["--simulation", "fading"]) == 1
    usage = benchmark.usage_text()
    assert "bsc" in usage and "bec" in usage and "--p <value>" in usage
