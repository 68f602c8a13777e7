"""GPU tests of the burst channel with a burst detector: cc_burst_erasure_channel_dev against the numpy model of
tests/burst_erasure_model.py (flags from a plain compare, per-frame lists from a plain loop) byte for byte, and
cc_mc_run_burst_erasure_dev (channel -> erase the flagged symbols -> decode -> count) against a host count over the very
same blocks: channel-only call -> cc.deinterleave -> plain correct_batch with the per-frame lists -> numpy.  Neither
depends on how a call is split or chunked, and a detector that never flags is the errors-only route word for word."""
import ctypes as C

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import BurstBackend
import burst_erasure_model
import burst_model
from test_gpu_burst import CODES, GEOMETRIES, sent_words

pytestmark = pytest.mark.gpu

CHANNELS = [(0.02, 0.25, 0.001, 0.5), (1.0, 1.0, 0.0, 1.0)]
DETECTORS = [(0.9, 0.002), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0), (0.0, 0.0)]
DET = DETECTORS[0]


def device_channel(code, params, det, I, seed, first, frames, random_cw=True):
    return cc.burst_erasure_channel(code, I, *params, *det, seed=seed, first_frame=first, frames=frames,
                                    random_codewords=random_cw)


def mc(code, params, det, I, seed, first, frames, random_cw=True):
    backend = BurstBackend(code, I, params[0], params[1], params[2], random_cw, p_detect=det[0], p_false_alarm=det[1])
    return backend.run(params[3], seed, first, frames).cpu().numpy()


# ---- 1. the channel, byte for byte ----
_base = {}


def model(which, I, blocks, params, det, seed, first):
    """the model's output; the errors-only channel under it is computed once per (geometry, channel)"""
    code = CODES[which]()
    frames = blocks * I
    q_sym = 1 << code.q if code.family == capi.FAMILY_RS else 2
    key = (which, I, blocks, params, seed, first)
    if key not in _base:
        _base[key] = burst_model.channel(params, I, seed, first, frames, code.n, q_sym, sent_words(code, seed, first, frames))
    return code, burst_erasure_model.channel(params, det, I, seed, first, frames, code.n, q_sym, base=_base[key])


def assert_equals_model(ch, recv, sent, state, flag):
    assert np.array_equal(ch["sent"].cpu().numpy(), sent)
    assert np.array_equal(ch["state"].cpu().numpy(), state)
    assert np.array_equal(ch["flag"].cpu().numpy(), flag)
    assert np.array_equal(ch["recv"].cpu().numpy(), recv)
    vals, off = burst_erasure_model.csr(burst_erasure_model.frame_lists(flag))
    assert np.array_equal(ch["erasure_offsets"].cpu().numpy().astype(np.int64), off)
    assert np.array_equal(ch["erasures"].cpu().numpy().astype(np.int64), vals)


@pytest.mark.parametrize("det", DETECTORS, ids=["typical", "state", "not-state", "all", "off"])
@pytest.mark.parametrize("params", CHANNELS, ids=["bursty", "swap"])
@pytest.mark.parametrize("which,I,blocks", GEOMETRIES, ids=["%s-I%d" % g[:2] for g in GEOMETRIES])
def test_channel_equals_model(which, I, blocks, params, det):
    import torch
    seed, first = 0x1234567890AB, ((1 << 41) + 987654) * I
    code, (recv, sent, state, flag, _) = model(which, I, blocks, params, det, seed, first)
    frames, n = blocks * I, code.n
    ch = device_channel(code, params, det, I, seed, first, frames)
    assert_equals_model(ch, recv, sent, state, flag)
    if det == (1.0, 0.0):
        assert torch.equal(ch["flag"], ch["state"])
    if det == (0.0, 1.0):
        assert torch.equal(ch["flag"], 1 - ch["state"])
    if det == (1.0, 1.0):  # everything flagged: off[f] = f n, positions 0 .. n - 1
        assert np.array_equal(ch["erasure_offsets"].cpu().numpy(), np.arange(frames + 1) * n)
        assert np.array_equal(ch["erasures"].cpu().numpy(), np.tile(np.arange(n), frames)) and not ch["recv"].any()
    if det == (0.0, 0.0):  # nothing flagged: the errors-only channel
        assert not ch["erasure_offsets"].any() and ch["erasures"].numel() == 0 and not ch["flag"].any()
        plain = cc.burst_channel(code, I, *params, seed=seed, first_frame=first, frames=frames, random_codewords=True)
        for a, b in zip(plain, (ch["recv"], ch["sent"], ch["state"])):
            assert torch.equal(a, b)


def test_channel_where_the_block_index_crosses_2_32():
    I, blocks, params = 3, 6, CHANNELS[0]
    seed, first = 77, ((1 << 32) - 2) * I
    code, (recv, sent, state, flag, _) = model("rs7", I, blocks, params, DET, seed, first)
    assert_equals_model(device_channel(code, params, DET, I, seed, first, blocks * I), recv, sent, state, flag)
    assert flag.any() and not flag.all()


def test_all_zero_word_and_optional_outputs():
    import torch
    code, I, frames, params = CODES["bch15"](), 4, 32, CHANNELS[0]
    recv, sent, state, flag, _ = burst_erasure_model.channel(params, DET, I, 3, 8, frames, code.n, 2)
    ch = device_channel(code, params, DET, I, 3, 8, frames, random_cw=False)
    assert not ch["sent"].any() and flag.any()
    assert_equals_model(ch, recv, sent, state, flag)
    alone = torch.zeros_like(ch["recv"])  # d_sent, d_state, d_flag and the list are optional
    chan, det = capi.BurstChannel(I, *params), capi.BurstDetector(*DET)
    capi.check(capi.lib().cc_burst_erasure_channel_dev(code._h, C.byref(chan), C.byref(det), 3, 8, frames, 0,
                                                       C.c_void_p(alone.data_ptr()), None, None, None, None, None, None),
               "cc_burst_erasure_channel_dev")
    torch.cuda.synchronize()
    assert torch.equal(alone, ch["recv"])


# ---- 2. splitting a call ----
def joined(a, b):
    import torch
    out = {k: torch.cat([a[k], b[k]]) for k in ("recv", "sent", "state", "flag", "erasures")}
    out["erasure_offsets"] = torch.cat([a["erasure_offsets"], b["erasure_offsets"][1:] + a["erasure_offsets"][-1]])
    return out


@pytest.mark.parametrize("which,I", [("rs7", 3), ("rs239", 16)])
def test_split_invariance(which, I):
    import torch
    code, params, seed, first = CODES[which](), CHANNELS[0], 21, 5 * I << 20
    whole = device_channel(code, params, DET, I, seed, first, 8 * I)
    parts = joined(device_channel(code, params, DET, I, seed, first, 4 * I),
                   device_channel(code, params, DET, I, seed, first + 4 * I, 4 * I))
    for k in whole:
        assert torch.equal(whole[k], parts[k]), k
    assert int(whole["erasure_offsets"][-1]) == int(whole["flag"].sum()) > 0
    c = mc(code, params, DET, I, seed, first, 8 * I)
    two = mc(code, params, DET, I, seed, first, 4 * I) + mc(code, params, DET, I, seed, first + 4 * I, 4 * I)
    assert np.array_equal(c, two) and c[capi.MC_FRAMES] == 8 * I
    assert c[capi.MC_CHANNEL_ERASURES] == int(whole["flag"].sum())


def test_chunk_boundary():
    """3 * 349600 frames are more than the 2^20 of one chunk: the second chunk starts on a block, its part of the list
    behind the first chunk's."""
    import torch
    code, I, params, seed, first = CODES["rs7"](), 3, CHANNELS[0], 9, 3 << 36
    frames, x = 3 * 349600, 3 * 200001
    whole = mc(code, params, DET, I, seed, first, frames)
    two = mc(code, params, DET, I, seed, first, x) + mc(code, params, DET, I, seed, first + x, frames - x)
    assert np.array_equal(whole, two)
    assert whole[capi.MC_FRAMES] == frames and 0 < whole[capi.MC_WORD_ERRORS] < frames
    ch = device_channel(code, params, DET, I, seed, first, frames)
    parts = joined(device_channel(code, params, DET, I, seed, first, x),
                   device_channel(code, params, DET, I, seed, first + x, frames - x))
    for k in ch:
        assert torch.equal(ch[k], parts[k]), k
    assert whole[capi.MC_CHANNEL_ERASURES] == int(ch["flag"].sum()) == int(ch["erasure_offsets"][-1])
    # the list is the frame-major flag map read row by row
    rows, cols = torch.nonzero(cc.deinterleave(ch["flag"], I), as_tuple=True)
    assert torch.equal(cols.to(torch.int16), ch["erasures"])
    assert torch.equal(torch.bincount(rows, minlength=frames).cumsum(0).to(torch.int32), ch["erasure_offsets"][1:])


# ---- 3. counters against the host pipeline ----
PGZ = cc.peterson_gorenstein_zierler_tag
FIRST = (0.02, 0.25, 0.001, 0.5)
# name, code, tag, I, frames, channel, then the model's own figures for these inputs (seed 5, first ((3 << 40) + 12345) I,
# detector (0.9, 0.002)): frames with rho > 2t and frames within 2e + rho <= 2t.  They do not come from the device: the
# model alone gives them on the CPU.
CASES = [
    ("bch63-bm-I8", "bch63", cc.berlekamp_massey_tag, 8, 4096, FIRST, 686, 3038),
    ("bch63-pgz-I1", "bch63", PGZ, 1, 4096, FIRST, 1042, 2893),
    ("rs239-bm-I16", "rs239", cc.berlekamp_massey_tag, 16, 4096, (0.005, 0.1, 1e-4, 0.9), 420, 3048),
    ("rs15-euklid-I5", "rs15", cc.euklid_tag, 5, 4000, (0.02, 0.25, 0.001, 0.9), 3, 3980),
    ("rs204-bm-I12", "rs204", cc.berlekamp_massey_tag, 12, 3072, (0.005, 0.1, 1e-4, 0.9), 149, 2650),
    ("bch63-ms10-I4", "bch63", lambda: cc.min_sum_tag(10), 4, 4096, FIRST, None, None),
]
SEED = 5


def lists_of(ch, frames):
    vals, off = ch["erasures"].cpu().numpy(), ch["erasure_offsets"].cpu().numpy()
    return [vals[off[f]:off[f + 1]].tolist() for f in range(frames)]


@pytest.mark.parametrize("name,which,tag,I,frames,params,beyond,within", CASES, ids=[c[0] for c in CASES])
def test_counters_match_host_pipeline(name, which, tag, I, frames, params, beyond, within):
    import torch
    code = CODES[which](tag)
    first = ((3 << 40) + 12345) * I
    c = mc(code, params, DET, I, SEED, first, frames)
    ch = device_channel(code, params, DET, I, SEED, first, frames)
    rx, tx, fl = (cc.deinterleave(ch[k], I) for k in ("recv", "sent", "flag"))
    if code.algorithm.soft:
        y = 1.0 - 2.0 * rx.float()
        y[fl != 0] = 0.0
        res = code.correct_batch(y)
    else:
        lists = lists_of(ch, frames)
        res = code.correct_batch(rx, lists)
        block = code.correct_batch(ch["recv"], lists, interleave=I)  # the same blocks as the receiver holds them
        assert torch.equal(cc.deinterleave(block["out"], I), res["out"]) and torch.equal(block["status"], res["status"])
    errs = (res["out"] != tx).sum(dim=1)
    failed = res["status"] != 0
    rho = fl.sum(dim=1)
    e = ((rx != tx) & (fl == 0)).sum(dim=1)
    want = {capi.MC_FRAMES: frames, capi.MC_CHANNEL_ERASURES: int(ch["flag"].sum()),
            capi.MC_CHANNEL_BIT_ERRORS: int(e.sum()), capi.MC_BIT_ERRORS: int(errs.sum()),
            capi.MC_FAILURES: int(failed.sum()), capi.MC_WORD_ERRORS: int((failed | (errs > 0)).sum()),
            capi.MC_UNDETECTED: int((~failed & (errs > 0)).sum()), capi.MC_ITER_SUM: 0}
    hist = np.zeros(56, np.int64)
    if code.algorithm.soft:
        it = res["iters"].to(torch.int64)
        run = it + 1
        run[failed] = code.algorithm.iterations
        want[capi.MC_ITER_SUM] = int(run.sum())
        hist = np.bincount(it[~failed].cpu().numpy(), minlength=56)[:56]
    print(name, {k: (int(c[k]), v) for k, v in want.items()}, "rho > 2t:", int((rho > 2 * code.t).sum()),
          "within:", int((2 * e + rho <= 2 * code.t).sum()))
    for k, v in want.items():
        assert c[k] == v, (k, int(c[k]), v)
    assert np.array_equal(c[capi.MC_ITER_HIST:capi.MC_ITER_HIST + 56], hist)
    assert c[capi.MC_CHANNEL_ERASURES] == int(ch["erasure_offsets"][-1]) == int(rho.sum())
    assert 0 < c[capi.MC_WORD_ERRORS] < frames  # a point where the decoder has work to do
    good = ~failed & (errs == 0)
    assert bool((good & (rho > 0)).any())  # erasures were filled
    if beyond is not None:  # the model's figures
        assert int((rho > 2 * code.t).sum()) == beyond and int((2 * e + rho <= 2 * code.t).sum()) == within
    if name in ("bch63-bm-I8", "rs239-bm-I16"):
        assert bool((rho > 2 * code.t).any())  # frames beyond the erasure budget are among those counted


# ---- 4. the detector off ----
@pytest.mark.parametrize("name,which,tag,I,frames,params", [c[:6] for c in (CASES[0], CASES[2], CASES[5])],
                         ids=[CASES[0][0], CASES[2][0], CASES[5][0]])
def test_detector_off_is_the_errors_only_route(name, which, tag, I, frames, params):
    import torch
    code = CODES[which](tag)
    first = ((3 << 40) + 12345) * I
    plain = BurstBackend(code, I, params[0], params[1], params[2], True).run(params[3], SEED, first, frames).cpu().numpy()
    dcnt = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    chan, det = capi.BurstChannel(I, *params), capi.BurstDetector(0.0, 0.0)
    capi.check(capi.lib().cc_mc_run_burst_erasure_dev(code._h, C.byref(chan), C.byref(det), SEED, first, frames, 1,
                                                      C.c_void_p(dcnt.data_ptr()), None), "cc_mc_run_burst_erasure_dev")
    torch.cuda.synchronize()
    off = dcnt.cpu().numpy()
    assert np.array_equal(off, plain) and off[capi.MC_FRAMES] == frames and off[capi.MC_CHANNEL_ERASURES] == 0
    assert 0 < off[capi.MC_WORD_ERRORS]
    on = mc(code, params, DET, I, SEED, first, frames)
    assert on[capi.MC_CHANNEL_ERASURES] > 0 and not np.array_equal(on, plain)  # and the detector changes the count


# ---- 5. refusals with a device present ----
def test_refusals_on_the_device():
    import torch
    lib = capi.lib()
    dcnt = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    cnt = C.c_void_p(dcnt.data_ptr())
    ch, det = capi.BurstChannel(4, 0.02, 0.25, 0.001, 0.5), capi.BurstDetector(*DET)
    run = lambda code, first=0, frames=64, d=det: lib.cc_mc_run_burst_erasure_dev(  # noqa: E731
        code._h, C.byref(ch), C.byref(d), 0, first, frames, 0, cnt, None)
    rs_pgz = CODES["rs239"](PGZ)
    assert run(rs_pgz) == capi.ERR_UNSUPPORTED and "PGZ-Algorithm does not support erasure" in lib.cc_last_error().decode()
    wide = cc.rs(9, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x211)
    assert run(wide) == capi.ERR_UNSUPPORTED
    mu0 = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), mu=0)
    assert run(mu0) == capi.ERR_UNSUPPORTED and "mu = step = 1" in lib.cc_last_error().decode()
    rs = CODES["rs239"]()
    assert run(rs, 0, 66) == capi.ERR_INVALID_ARGUMENT and run(rs, 2, 64) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError):
        cc.burst_erasure_channel(rs, 4, 0.02, 0.25, 0.001, 0.5, 0.9, 0.002, frames=66)
    with pytest.raises(cc.CcError):
        cc.burst_erasure_channel(rs_pgz, 4, 0.02, 0.25, 0.001, 0.5, 0.9, 0.002, frames=64)
    torch.cuda.synchronize()
    assert int(dcnt.abs().sum()) == 0  # a refused call counts nothing
    assert run(rs) == capi.OK
    torch.cuda.synchronize()
    assert int(dcnt[capi.MC_FRAMES]) == 64
    dcnt.zero_()
    assert run(rs_pgz, d=capi.BurstDetector(0.0, 0.0)) == capi.OK  # RS + PGZ is refused for the erasures only
    torch.cuda.synchronize()
    assert int(dcnt[capi.MC_FRAMES]) == 64 and int(dcnt[capi.MC_CHANNEL_ERASURES]) == 0
