"""GPU tests of the discrete-channel Monte-Carlo: cc_discrete_channel_dev against the numpy restatement of
tests/test_discrete_host.py, and cc_mc_run_discrete_dev (channel -> decode -> count) against a host count over the
very same frames decoded through the plain batch API.  The counters must not depend on chunking or sharding."""
import ctypes as C
import math

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import DiscreteBackend, discrete_simulation
from test_discrete_host import bch_message_bits, channel, erasure_csr, rs_message_symbols

pytestmark = pytest.mark.gpu

BIG = 1 << 20


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def mc(code, p, e, seed, first, frames, random_cw):
    return DiscreteBackend(code, "bsec", random_cw).run((p, e), seed, first, frames).cpu().numpy()


def awgn_sent(code, seed, first, frames):
    import torch
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, 4.0, seed, first, frames, 1, ptr(llr), ptr(sent), None),
               "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return sent


def erased_mask(ch, frames, n):
    import torch
    off = ch["erasure_offsets"].long()
    m = torch.zeros((frames, n), dtype=torch.bool, device="cuda")
    if ch["erasures"].numel():
        rows = torch.repeat_interleave(torch.arange(frames, device="cuda"), off[1:] - off[:-1])
        m[rows, ch["erasures"].long()] = True
    return m


def decode(code, ch, frames):
    """The channel's frames through the existing batch API: the erasure CSR to cc_correct_hard_batch_dev, or the
    +-1 / 0 floats to correct_batch for min-sum."""
    import torch
    recv = ch["recv"]
    if code.algorithm.soft:
        y = 1.0 - 2.0 * recv.float()
        y[erased_mask(ch, frames, code.n)] = 0.0
        return code.correct_batch(y)
    er, off = ch["erasures"], ch["erasure_offsets"]
    use_er = int(off[-1]) > 0
    if use_er and er.numel() == 0:
        er = torch.zeros(1, dtype=torch.int16, device="cuda")
    out = torch.empty_like(recv)
    nerr = torch.empty(frames, dtype=torch.int32, device="cuda")
    status = torch.empty(frames, dtype=torch.int32, device="cuda")
    capi.check(capi.lib().cc_correct_hard_batch_dev(code._h, ptr(recv), ptr(er) if use_er else None,
                                                     ptr(off) if use_er else None, ptr(out), ptr(nerr), ptr(status),
                                                     frames, None), "cc_correct_hard_batch_dev")
    torch.cuda.synchronize()
    return dict(out=out, status=status, nerr=nerr)


def channel_np(code, p, e, seed, first, frames, random_cw):
    q_sym = 1 << code.q if code.family == capi.FAMILY_RS else 2
    sent = None
    if random_cw:
        msg = (rs_message_symbols(seed, first, frames, code.l, code.q) if code.family == capi.FAMILY_RS
               else bch_message_bits(seed, first, frames, code.l))
        sent = code.encode_batch(msg)
    recv, erased, wrong = channel(p, e, seed, first, frames, code.n, q_sym, sent)
    return recv, erased, wrong, (np.zeros((frames, code.n), np.uint8) if sent is None else sent)


# ---- the channel, symbol for symbol ----
# every frame length: G = 2, 4, .. 64 lanes per frame (group_count's ballot masks, group_log2 = 1 .. 6); RS over GF(2^q)
# for every q (error values uniform over the 2^q - 1 non-zero symbols)
GEOMETRIES = {
    "bch": lambda: cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag()),
    "rs": lambda: cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag()),
    "bch7": lambda: cc.primitive_bch(3, cc.errors(1), cc.berlekamp_massey_tag()),
    "bch15": lambda: cc.primitive_bch(4, cc.errors(2), cc.berlekamp_massey_tag()),
    "bch63": lambda: cc.primitive_bch(6, cc.errors(3), cc.berlekamp_massey_tag()),
    "bch127": lambda: cc.primitive_bch(7, cc.errors(4), cc.berlekamp_massey_tag()),
    "rs15": lambda: cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag()),
    "rs31": lambda: cc.rs(5, cc.errors(4), cc.berlekamp_massey_tag()),
    "rs63": lambda: cc.rs(6, cc.errors(8), cc.berlekamp_massey_tag()),
    "rs127": lambda: cc.rs(7, cc.errors(8), cc.berlekamp_massey_tag()),
}


@pytest.mark.parametrize("which", list(GEOMETRIES))
@pytest.mark.parametrize("random_cw", [False, True])
@pytest.mark.parametrize("p,e", [(0.03, 0.05), (0.02, 0.0), (0.0, 0.1)])
def test_channel_equals_numpy(which, random_cw, p, e):
    code = GEOMETRIES[which]()
    seed, first, frames = 0x1234567890AB, (1 << 41) + 987654321, 300
    ch = code.discrete_channel(p, e, seed, first, frames, random_cw)
    recv, erased, wrong, sent = channel_np(code, p, e, seed, first, frames, random_cw)
    assert np.array_equal(ch["sent"].cpu().numpy(), sent)
    assert np.array_equal(ch["recv"].cpu().numpy(), recv)
    vals, off = erasure_csr(erased)
    assert np.array_equal(ch["erasure_offsets"].cpu().numpy().astype(np.int64), off)
    assert np.array_equal(ch["erasures"].cpu().numpy().astype(np.int64), vals)
    if e == 0:
        assert ch["erasures"].numel() == 0 and int(ch["erasure_offsets"].abs().sum()) == 0
    if p > 0 and code.family == capi.FAMILY_RS:  # the error values reach every non-zero symbol of GF(2^q) and no other
        vals = (ch["recv"] ^ ch["sent"]).cpu().numpy()[wrong]
        assert vals.min() >= 1 and vals.max() < 1 << code.q
    if random_cw:
        chk = code.correct_batch(sent)
        assert (chk["status"] == 0).all() and (chk["nerr"] == 0).all()  # the transmitted words are codewords
        if code.family == capi.FAMILY_BCH:  # the words of cc_awgn_llr_dev for the same seed and frames
            assert np.array_equal(awgn_sent(code, seed, first, frames).cpu().numpy(), sent)


def test_channel_csr_across_chunks_and_calls():
    """One call over more than 2^20 frames is one CSR; its pieces equal calls over the parts."""
    import torch
    code = cc.rs(8, cc.errors(16), cc.euklid_tag())
    seed, first, frames, x = 11, 1 << 35, BIG + 777, BIG - 5
    whole = code.discrete_channel(0.01, 0.02, seed, first, frames, True)
    a = code.discrete_channel(0.01, 0.02, seed, first, x, True)
    b = code.discrete_channel(0.01, 0.02, seed, first + x, frames - x, True)
    off = whole["erasure_offsets"]
    assert torch.equal(whole["recv"], torch.cat([a["recv"], b["recv"]]))
    assert torch.equal(whole["sent"], torch.cat([a["sent"], b["sent"]]))
    assert torch.equal(off[: x + 1], a["erasure_offsets"])
    assert torch.equal(off[x:] - off[x], b["erasure_offsets"])
    assert torch.equal(whole["erasures"], torch.cat([a["erasures"], b["erasures"]]))
    assert int(off[-1]) == whole["erasures"].numel() and bool((off[1:] >= off[:-1]).all())
    # positions ascend inside every frame
    er = whole["erasures"].long()
    step = er[1:] - er[:-1]
    inner = torch.ones_like(step, dtype=torch.bool)
    bounds = off[1:-1].long()
    bounds = bounds[(bounds > 0) & (bounds < er.numel())]
    inner[bounds - 1] = False
    assert bool((step[inner] > 0).all())
    # the tail against numpy
    recv, erased, _, _ = channel_np(code, 0.01, 0.02, seed, first + frames - 200, 200, True)
    assert np.array_equal(whole["recv"][-200:].cpu().numpy(), recv)


def test_channel_csr_across_chunks_small_code():
    """More than DISCRETE_CHUNK frames of RS(15,9) (four lanes per frame) in one call: the CSR built across chunks, the
    RS messages and the error values over GF(16), all against numpy."""
    code = cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag())
    seed, first, frames = (3 << 32) + 1, (1 << 32) - 7777, BIG + 4321
    ch = code.discrete_channel(0.02, 0.04, seed, first, frames, True)
    recv, erased, _, sent = channel_np(code, 0.02, 0.04, seed, first, frames, True)
    assert np.array_equal(ch["sent"].cpu().numpy(), sent)
    assert np.array_equal(ch["recv"].cpu().numpy(), recv)
    vals, off = erasure_csr(erased)
    assert np.array_equal(ch["erasure_offsets"].cpu().numpy().astype(np.int64), off)
    assert np.array_equal(ch["erasures"].cpu().numpy().astype(np.int64), vals)


# ---- counters against a host count ----
BCH = lambda tag: cc.primitive_bch(8, cc.errors(3), tag)  # noqa: E731  BCH(255,231)
RS = lambda tag: cc.rs(8, cc.errors(16), tag)  # noqa: E731      RS(255,223)
# On the erasure-only points of decoders that read an erased position as 0 the words are random: with the all-zero word
# the 0 an erased position receives is the symbol sent, and such a decoder sees a codeword whenever no error was drawn.
# BCH PGZ refuses rho > 2t itself (the two-trial rule), so it runs there on the all-zero word.
CASES = [
    ("bch-pgz-bsc", lambda: BCH(cc.peterson_gorenstein_zierler_tag()), 0.012, 0.0, True),
    ("bch-bm-bsc", lambda: BCH(cc.berlekamp_massey_tag()), 0.012, 0.0, False),
    ("bch-ms-bsc", lambda: BCH(cc.min_sum_tag(20)), 0.01, 0.0, True),
    ("bch-pgz-bec", lambda: BCH(cc.peterson_gorenstein_zierler_tag()), 0.0, 0.025, False),
    ("bch-ms-bec", lambda: BCH(cc.min_sum_tag(20)), 0.0, 0.03, True),
    ("bch-pgz-bsec", lambda: BCH(cc.peterson_gorenstein_zierler_tag()), 0.006, 0.012, False),
    ("bch-ms-bsec", lambda: BCH(cc.min_sum_tag(20)), 0.006, 0.012, True),
    ("rs-bm-qsc", lambda: RS(cc.berlekamp_massey_tag()), 0.05, 0.0, True),
    ("rs-euklid-qsc", lambda: RS(cc.euklid_tag()), 0.05, 0.0, False),
    ("rs-bm-bec", lambda: RS(cc.berlekamp_massey_tag()), 0.0, 0.11, True),
    ("rs-euklid-bec", lambda: RS(cc.euklid_tag()), 0.0, 0.11, True),
    ("rs-bm-bsec", lambda: RS(cc.berlekamp_massey_tag()), 0.03, 0.05, True),
    ("rs-euklid-bsec", lambda: RS(cc.euklid_tag()), 0.03, 0.05, False),
    # below GF(2^8): 16, 8 and 4 lanes per frame, error values over GF(64) and GF(16)
    ("bch63-bm-bsec", lambda: cc.primitive_bch(6, cc.errors(3), cc.berlekamp_massey_tag()), 0.01, 0.01, True),
    ("bch63-ms-bsec", lambda: cc.primitive_bch(6, cc.errors(3), cc.min_sum_tag(20)), 0.01, 0.01, True),
    ("rs15-bm-bsec", lambda: cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag()), 0.03, 0.05, True),
    ("rs15-euklid-bsec", lambda: cc.rs(4, cc.errors(3), cc.euklid_tag()), 0.03, 0.05, False),
    ("rs63-bm-bsec", lambda: cc.rs(6, cc.errors(8), cc.berlekamp_massey_tag()), 0.03, 0.05, True),
    ("rs63-euklid-bsec", lambda: cc.rs(6, cc.errors(8), cc.euklid_tag()), 0.03, 0.05, False),
]


@pytest.mark.parametrize("name,make,p,e,random_cw", CASES, ids=[c[0] for c in CASES])
def test_counters_match_host_count(name, make, p, e, random_cw):
    import torch
    code = make()
    seed, first, frames = 5, (3 << 40) + 12345, BIG + 4097  # a chunk boundary inside the call
    c = mc(code, p, e, seed, first, frames, random_cw)
    ch = code.discrete_channel(p, e, seed, first, frames, random_cw)
    res = decode(code, ch, frames)
    sent, recv = ch["sent"], ch["recv"]
    erased = erased_mask(ch, frames, code.n)
    wrong = (recv != sent) & ~erased
    errs = (res["out"] != sent).sum(dim=1)
    failed = res["status"] != 0
    assert c[capi.MC_FRAMES] == frames
    assert c[capi.MC_CHANNEL_ERASURES] == int(erased.sum()) == int(ch["erasure_offsets"][-1])
    assert c[capi.MC_CHANNEL_BIT_ERRORS] == int(wrong.sum())
    assert c[capi.MC_BIT_ERRORS] == int(errs.sum())
    assert c[capi.MC_FAILURES] == int(failed.sum())
    assert c[capi.MC_WORD_ERRORS] == int((failed | (errs > 0)).sum())
    assert c[capi.MC_UNDETECTED] == int((~failed & (errs > 0)).sum())
    assert 0 < c[capi.MC_WORD_ERRORS] < frames  # a point where the decoder has work to do
    if code.algorithm.soft:
        it = res["iters"].to(torch.int64)
        run = it + 1
        run[failed] = code.algorithm.iterations
        assert c[capi.MC_ITER_SUM] == int(run.sum())
        hist = np.bincount(it[~failed].cpu().numpy(), minlength=56)[:56]
        assert np.array_equal(c[capi.MC_ITER_HIST:capi.MC_ITER_HIST + 56], hist)
    else:
        assert c[capi.MC_ITER_SUM] == 0


def test_sharding_is_additive():
    code = RS(cc.berlekamp_massey_tag())
    a, F, x = (7 << 40) + 3, 300000, 123457
    whole = mc(code, 0.03, 0.05, 9, a, F, True)
    parts = mc(code, 0.03, 0.05, 9, a, x, True) + mc(code, 0.03, 0.05, 9, a + x, F - x, True)
    assert np.array_equal(whole, parts)
    code = BCH(cc.min_sum_tag(20))
    whole = mc(code, 0.01, 0.01, 9, a, F, False)
    parts = mc(code, 0.01, 0.01, 9, a, x, False) + mc(code, 0.01, 0.01, 9, a + x, F - x, False)
    assert np.array_equal(whole, parts)


# ---- bounded-distance identities, frame by frame ----
def test_bch_pgz_bsc_fails_exactly_beyond_t():
    code = cc.primitive_bch(8, cc.errors(2), cc.peterson_gorenstein_zierler_tag())  # BCH(255,239)
    frames = 200000
    ch = code.discrete_channel(0.008, 0.0, 3, 1 << 36, frames, True)
    res = decode(code, ch, frames)
    nchan = (ch["recv"] != ch["sent"]).sum(dim=1)
    werr = (res["status"] != 0) | (res["out"] != ch["sent"]).any(dim=1)
    assert bool((werr == (nchan > code.t)).all())
    assert 0 < int(werr.sum()) < frames


def test_rs_bm_within_capability_decodes():
    code = RS(cc.berlekamp_massey_tag())
    frames = 200000
    ch = code.discrete_channel(0.03, 0.05, 4, 5 << 38, frames, True)
    res = decode(code, ch, frames)
    erased = erased_mask(ch, frames, code.n)
    e = ((ch["recv"] != ch["sent"]) & ~erased).sum(dim=1)
    rho = erased.sum(dim=1)
    inside = 2 * e + rho <= 2 * code.t
    ok = (res["status"] == 0) & (res["out"] == ch["sent"]).all(dim=1)
    assert bool(ok[inside].all())
    assert bool((2 * e + rho)[~ok].gt(2 * code.t).all())
    assert 0 < int((~inside).sum()) < frames


def test_bch_pgz_bec_two_trial_rule():
    code = BCH(cc.peterson_gorenstein_zierler_tag())
    frames = 200000
    ch = code.discrete_channel(0.0, 0.025, 6, 9 << 36, frames, True)
    res = decode(code, ch, frames)
    off = ch["erasure_offsets"].long()
    rho = off[1:] - off[:-1]
    inside = rho <= 2 * code.t
    ok = (res["status"] == 0) & (res["out"] == ch["sent"]).all(dim=1)
    assert bool(ok[inside].all())
    assert bool((res["status"][~inside] == capi.FRAME_ERASURES).all())
    assert 0 < int((~inside).sum()) < frames


# ---- statistics (loose: 6 sigma) ----
def test_class_fractions_and_uniform_error_values():
    import torch
    code = RS(cc.berlekamp_massey_tag())
    p, e, frames = 0.03, 0.05, 40000  # 1.02e7 symbols
    ch = code.discrete_channel(p, e, 21, 1 << 30, frames, True)
    N = frames * code.n
    erased = erased_mask(ch, frames, code.n)
    wrong = (ch["recv"] != ch["sent"]) & ~erased
    for frac, prob in ((float(erased.sum()) / N, e), (float(wrong.sum()) / N, p)):
        assert abs(frac - prob) < 6 * math.sqrt(prob * (1 - prob) / N), (frac, prob)
    vals = (ch["recv"] ^ ch["sent"])[wrong].long()
    counts = torch.bincount(vals, minlength=256).cpu().numpy()
    assert counts[0] == 0
    expected = vals.numel() / 255.0
    chi2 = float(((counts[1:] - expected) ** 2 / expected).sum())
    assert chi2 < 254 + 6 * math.sqrt(2 * 254), chi2  # 254 degrees of freedom


def test_bch_pgz_wer_matches_binomial_tail():
    code = cc.primitive_bch(8, cc.errors(2), cc.peterson_gorenstein_zierler_tag())  # BCH(255,239), t = 2
    p, frames = 0.005, 1 << 22
    c = mc(code, p, 0.0, 17, 1 << 39, frames, True)
    tail = 1.0 - sum(math.comb(255, k) * p ** k * (1 - p) ** (255 - k) for k in range(3))
    wer = c[capi.MC_WORD_ERRORS] / frames
    assert abs(wer - tail) < 6 * math.sqrt(tail * (1 - tail) / frames), (wer, tail)
    assert abs(c[capi.MC_CHANNEL_BIT_ERRORS] / (frames * 255) - p) < 6 * math.sqrt(p / (frames * 255))


# ---- the entry points' refusals and the harness ----
def test_refusals_on_the_device():
    import torch
    rs_pgz = RS(cc.peterson_gorenstein_zierler_tag())
    dcnt = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    lib = capi.lib()
    assert lib.cc_mc_run_discrete_dev(rs_pgz._h, 0.0, 0.01, 0, 0, 64, 0, ptr(dcnt), None) == capi.ERR_UNSUPPORTED
    assert "PGZ-Algorithm does not support erasure" in lib.cc_last_error().decode()
    assert lib.cc_mc_run_discrete_dev(rs_pgz._h, 0.05, 0.0, 0, 0, 64, 0, ptr(dcnt), None) == capi.OK  # no erasures
    torch.cuda.synchronize()
    assert int(dcnt[capi.MC_FRAMES]) == 64 and int(dcnt[capi.MC_CHANNEL_ERASURES]) == 0
    mu2 = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), mu=2)
    assert lib.cc_mc_run_discrete_dev(mu2._h, 0.01, 0.0, 0, 0, 64, 0, ptr(dcnt), None) == capi.ERR_UNSUPPORTED
    bch = BCH(cc.berlekamp_massey_tag())
    recv = torch.empty((64, 255), dtype=torch.uint8, device="cuda")
    # p_erasure > 0 needs the list buffers
    assert lib.cc_discrete_channel_dev(bch._h, 0.0, 0.1, 0, 0, 64, 0, ptr(recv), None, None, None,
                                       None) == capi.ERR_INVALID_ARGUMENT


def test_awgn_route_leaves_the_erasure_slot_zero():
    from channelcoding_amd.montecarlo import DeviceBackend
    c = DeviceBackend(BCH(cc.berlekamp_massey_tag()), True).run(4.0, 1, 0, 20000).cpu().numpy()
    assert c[capi.MC_FRAMES] == 20000 and c[capi.MC_CHANNEL_ERASURES] == 0


def test_discrete_simulation_end_to_end(tmp_path):
    code = cc.rs(8, cc.errors(16), cc.berlekamp_massey_tag())
    res = discrete_simulation(code, "bec", points=[0.14, 0.1], max_samples=30000, log_dir=str(tmp_path))()  # random words
    assert [r["frames"] for r in res] == [10000, res[1]["frames"]] and res[1]["frames"] <= 30000
    assert res[0]["wer"] > res[1]["wer"] and res[0]["channel_erasures"] > 0 and res[0]["p_erasure"] == 0.14
    text = (tmp_path / (code.to_string() + ".bec.log")).read_text().splitlines()
    assert text[0] == "      p                   wer" and len(text) == 3 and text[1].split()[0] == "0.14"
    bsc = discrete_simulation(cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20)), "bsc", points=[0.02],
                              samples_per_point=5000, random_codewords=True)()
    assert bsc[0]["frames"] == 5000 and bsc[0]["channel_bit_errors"] > 0 and bsc[0]["iter_sum"] >= 5000
