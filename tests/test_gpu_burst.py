"""GPU tests of the Gilbert-Elliott burst channel: cc_burst_channel_dev against the numpy model of tests/burst_model.py
(whose chain is a plain loop over t) byte for byte, and cc_mc_run_burst_dev (channel -> decode -> count) against a host
count over the very same blocks: channel-only call -> cc.deinterleave -> plain correct_batch -> numpy.  Neither depends
on how a call is split or chunked."""
import ctypes as C

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import BurstBackend
import burst_model
from test_discrete_host import bch_message_bits, rs_message_symbols

pytestmark = pytest.mark.gpu

BM = cc.berlekamp_massey_tag
CODES = {
    "rs7": lambda tag=BM: cc.rs(3, cc.errors(2), tag()),                 # RS(7,3)
    "bch15": lambda tag=BM: cc.primitive_bch(4, cc.errors(2), tag()),    # BCH(15,7)
    "bch31": lambda tag=BM: cc.primitive_bch(5, cc.errors(3), tag()),    # BCH(31,16)
    "bch63": lambda tag=BM: cc.primitive_bch(6, cc.errors(3), tag()),    # BCH(63,45)
    "rs15": lambda tag=BM: cc.rs(4, cc.errors(3), tag()),                # RS(15,9)
    "rs239": lambda tag=BM: cc.rs(8, cc.errors(8), tag()),               # RS(255,239)
    "rs223": lambda tag=BM: cc.rs(8, cc.errors(16), tag()),              # RS(255,223)
    "rs204": lambda tag=BM: cc.rs(8, cc.errors(8), tag(), n=204),        # shortened RS(204,188)
}
PARAMS = [(0.02, 0.25, 0.001, 0.5), (0.0, 0.3, 0.01, 1.0), (1.0, 1.0, 0.0, 1.0), (0.5, 0.5, 1.0, 1.0)]


def sent_words(code, seed, first, frames):
    msg = (rs_message_symbols(seed, first, frames, code.l, code.q) if code.family == capi.FAMILY_RS
           else bch_message_bits(seed, first, frames, code.l))
    return code.encode_batch(msg)


def device_channel(code, params, I, seed, first, frames, random_cw=True):
    recv, sent, state = cc.burst_channel(code, I, *params, seed=seed, first_frame=first, frames=frames,
                                         random_codewords=random_cw)
    return recv, sent, state


def mc(code, params, I, seed, first, frames, random_cw=True):
    return BurstBackend(code, I, params[0], params[1], params[2], random_cw).run(params[3], seed, first,
                                                                                 frames).cpu().numpy()


# ---- 1. the channel, byte for byte ----
# N = n I: not a multiple of 4 and several blocks in a wavefront (RS(7,3)), the tail lane (BCH(31,16)), sixteen passes of
# 256 symbols (RS(255,239) at depth 16), the longest block there is (RS(255,223) at depth 256), a shortened code
GEOMETRIES = [("rs7", 1, 40), ("rs7", 2, 40), ("rs7", 3, 40), ("rs7", 5, 40), ("bch15", 4, 24), ("bch31", 1, 70),
              ("rs239", 16, 5), ("rs223", 256, 3), ("rs204", 12, 4)]
_sent = {}


def model(which, I, blocks, params, seed, first):
    code = CODES[which]()
    frames = blocks * I
    key = (which, I, blocks, seed, first)
    if key not in _sent:  # the transmitted words do not depend on the channel's parameters
        _sent[key] = sent_words(code, seed, first, frames)
    q_sym = 1 << code.q if code.family == capi.FAMILY_RS else 2
    return code, burst_model.channel(params, I, seed, first, frames, code.n, q_sym, _sent[key])


@pytest.mark.parametrize("params", PARAMS, ids=["bursty", "never-bad", "swap", "all-wrong"])
@pytest.mark.parametrize("which,I,blocks", GEOMETRIES, ids=["%s-I%d" % g[:2] for g in GEOMETRIES])
def test_channel_equals_model(which, I, blocks, params):
    seed, first = 0x1234567890AB, ((1 << 41) + 987654) * I
    code, (recv, sent, state, wrong) = model(which, I, blocks, params, seed, first)
    d_recv, d_sent, d_state = device_channel(code, params, I, seed, first, blocks * I)
    assert np.array_equal(d_sent.cpu().numpy(), sent)
    assert np.array_equal(d_state.cpu().numpy(), state)
    assert np.array_equal(d_recv.cpu().numpy(), recv)
    if params == PARAMS[2]:  # the swap map: states alternate along every block
        st = d_state.cpu().numpy().reshape(blocks, -1)
        assert np.array_equal(st, st[:, :1] ^ (np.arange(st.shape[1]) & 1)[None, :])
    if params == PARAMS[3] and code.family == capi.FAMILY_RS:  # every symbol in error: the values are never 0
        e = (d_recv ^ d_sent).cpu().numpy()
        assert e.min() >= 1 and e.max() < 1 << code.q and len(np.unique(e)) == min(e.size, (1 << code.q) - 1)


def test_channel_where_the_block_index_crosses_2_32():
    I, blocks, params = 3, 6, PARAMS[0]
    seed, first = 77, ((1 << 32) - 2) * I
    code, (recv, sent, state, _) = model("rs7", I, blocks, params, seed, first)
    d_recv, d_sent, d_state = device_channel(code, params, I, seed, first, blocks * I)
    assert np.array_equal(d_sent.cpu().numpy(), sent) and np.array_equal(d_state.cpu().numpy(), state)
    assert np.array_equal(d_recv.cpu().numpy(), recv)


def test_all_zero_word_and_optional_outputs():
    import torch
    code, I, frames, params = CODES["bch15"](), 4, 32, PARAMS[0]
    recv, sent, state, _ = burst_model.channel(params, I, 3, 8, frames, code.n, 2)
    d_recv, d_sent, d_state = device_channel(code, params, I, 3, 8, frames, random_cw=False)
    assert not d_sent.any() and np.array_equal(d_recv.cpu().numpy(), recv) and np.array_equal(d_state.cpu().numpy(), state)
    alone = torch.zeros_like(d_recv)  # d_sent and d_state are optional
    ch = capi.BurstChannel(I, *params)
    capi.check(capi.lib().cc_burst_channel_dev(code._h, C.byref(ch), 3, 8, frames, 0, C.c_void_p(alone.data_ptr()), None,
                                               None, None), "cc_burst_channel_dev")
    torch.cuda.synchronize()
    assert torch.equal(alone, d_recv)


# ---- 2. / 3. splitting a call ----
@pytest.mark.parametrize("which,I", [("rs7", 3), ("rs239", 16)])
def test_split_invariance(which, I):
    import torch
    code, params, seed, first = CODES[which](), PARAMS[0], 21, 5 * I << 20
    whole = device_channel(code, params, I, seed, first, 8 * I)
    a = device_channel(code, params, I, seed, first, 4 * I)
    b = device_channel(code, params, I, seed, first + 4 * I, 4 * I)
    for w, x, y in zip(whole, a, b):
        assert torch.equal(w, torch.cat([x, y]))
    c = mc(code, params, I, seed, first, 8 * I)
    parts = mc(code, params, I, seed, first, 4 * I) + mc(code, params, I, seed, first + 4 * I, 4 * I)
    assert np.array_equal(c, parts) and c[capi.MC_FRAMES] == 8 * I and c[capi.MC_CHANNEL_BIT_ERRORS] > 0


def test_chunk_boundary():
    """3 * 349600 frames are more than the 2^20 of one chunk: the second chunk starts on a block."""
    code, I, params, seed, first = CODES["rs7"](), 3, PARAMS[0], 9, 3 << 36
    frames, x = 3 * 349600, 3 * 200001
    whole = mc(code, params, I, seed, first, frames)
    parts = mc(code, params, I, seed, first, x) + mc(code, params, I, seed, first + x, frames - x)
    assert np.array_equal(whole, parts)
    assert whole[capi.MC_FRAMES] == frames and 0 < whole[capi.MC_WORD_ERRORS] < frames


# ---- 4. counters against the host pipeline ----
CASES = [
    ("bch63-bm-I8", "bch63", cc.berlekamp_massey_tag, 8, 1 << 12, (0.02, 0.25, 0.001, 0.5)),
    ("bch63-pgz-I1", "bch63", cc.peterson_gorenstein_zierler_tag, 1, 1 << 12, (0.02, 0.25, 0.001, 0.5)),
    ("rs239-bm-I16", "rs239", cc.berlekamp_massey_tag, 16, 1 << 12, (0.005, 0.1, 1e-4, 0.3)),
    ("rs15-euklid-I5", "rs15", cc.euklid_tag, 5, 5 * 800, (0.02, 0.25, 0.001, 0.5)),
    ("bch63-ms10-I4", "bch63", lambda: cc.min_sum_tag(10), 4, 1 << 12, (0.02, 0.25, 0.001, 0.5)),
]


@pytest.mark.parametrize("name,which,tag,I,frames,params", CASES, ids=[c[0] for c in CASES])
def test_counters_match_host_pipeline(name, which, tag, I, frames, params):
    import torch
    code = CODES[which](tag)
    seed, first = 5, ((3 << 40) + 12345) * I
    c = mc(code, params, I, seed, first, frames)
    recv, sent, state = device_channel(code, params, I, seed, first, frames)
    rx, tx = cc.deinterleave(recv, I), cc.deinterleave(sent, I)
    res = code.correct_batch(1.0 - 2.0 * rx.float()) if code.algorithm.soft else code.correct_batch(rx)
    errs = (res["out"] != tx).sum(dim=1)
    failed = res["status"] != 0
    assert c[capi.MC_FRAMES] == frames
    assert c[capi.MC_CHANNEL_ERASURES] == 0
    assert c[capi.MC_CHANNEL_BIT_ERRORS] == int((recv != sent).sum())
    assert c[capi.MC_BIT_ERRORS] == int(errs.sum())
    assert c[capi.MC_FAILURES] == int(failed.sum())
    assert c[capi.MC_WORD_ERRORS] == int((failed | (errs > 0)).sum())
    assert c[capi.MC_UNDETECTED] == int((~failed & (errs > 0)).sum())
    assert 0 < c[capi.MC_WORD_ERRORS] < frames  # a point where the decoder has work to do
    if code.algorithm.soft:
        run = res["iters"].to(torch.int64) + 1
        run[failed] = code.algorithm.iterations
        assert c[capi.MC_ITER_SUM] == int(run.sum())
    else:
        assert c[capi.MC_ITER_SUM] == 0


# ---- 5. refusals with a device present ----
def test_refusals_on_the_device():
    import torch
    lib = capi.lib()
    dcnt = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    cnt = C.c_void_p(dcnt.data_ptr())
    ch = capi.BurstChannel(4, 0.02, 0.25, 0.001, 0.5)
    wide = cc.rs(9, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x211)
    assert lib.cc_mc_run_burst_dev(wide._h, C.byref(ch), 0, 0, 64, 0, cnt, None) == capi.ERR_UNSUPPORTED
    mu0 = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), mu=0)
    assert lib.cc_mc_run_burst_dev(mu0._h, C.byref(ch), 0, 0, 64, 0, cnt, None) == capi.ERR_UNSUPPORTED
    assert "mu = step = 1" in lib.cc_last_error().decode()
    rs = CODES["rs239"]()
    assert lib.cc_mc_run_burst_dev(rs._h, C.byref(ch), 0, 0, 66, 0, cnt, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_mc_run_burst_dev(rs._h, C.byref(ch), 0, 2, 64, 0, cnt, None) == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError):
        cc.burst_channel(rs, 4, 0.02, 0.25, 0.001, 0.5, frames=66)
    torch.cuda.synchronize()
    assert int(dcnt.abs().sum()) == 0  # a refused call counts nothing
    assert lib.cc_mc_run_burst_dev(rs._h, C.byref(ch), 0, 0, 64, 0, cnt, None) == capi.OK
    torch.cuda.synchronize()
    assert int(dcnt[capi.MC_FRAMES]) == 64
