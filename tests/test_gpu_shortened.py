"""GPU tests of shortened codes (cc_desc.n = N < 2^q - 1) against tests/shortened_model.py: encode and extract, hard
decoding on every route and entry point, the 16-bit path, min-sum over H[:, :N] and both Monte-Carlo routes."""
import ctypes as C

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from awgn_model import awgn_reference
from checkers import BCH, BM, EUKLID, PGZ, RS, Oracle, WideOracle
import shortened_model as S
from test_discrete_host import bch_message_bits
from test_gpu_discrete_mc import decode as discrete_decode, erased_mask, mc as discrete_mc
from test_gpu_mc import awgn, mc as awgn_mc, sigma_f32, tau

pytestmark = pytest.mark.gpu

TAGS = {PGZ: cc.peterson_gorenstein_zierler_tag, BM: cc.berlekamp_massey_tag, EUKLID: cc.euklid_tag}


def make(family, q, t, N, alg=BM, **kw):
    cls = cc.primitive_bch if family == BCH else cc.rs
    tag = TAGS[alg]() if alg in TAGS else alg
    return cls(q, cc.errors(t), tag, n=N, **kw)


# ---- encode / extract ----
def lengths(family, q, t):
    k = Oracle(family, q, t).k
    n = (1 << q) - 1
    cand = {k + 1, n - 1, n - 2, k + 3}
    for base in (64, 128, 192):
        cand |= {base - 1, base, base + 1, base + 63}
    return sorted(N for N in cand if k < N < n)


ENC_CODES = [(BCH, 3, 1), (BCH, 4, 2), (BCH, 5, 3), (BCH, 6, 3), (BCH, 7, 4), (BCH, 8, 3), (BCH, 8, 12),
             (RS, 3, 1), (RS, 4, 2), (RS, 5, 4), (RS, 6, 8), (RS, 7, 8), (RS, 8, 8), (RS, 8, 16)]


@pytest.mark.parametrize("coding", [0, 1])
@pytest.mark.parametrize("family,q,t", ENC_CODES, ids=["%s%d-%d" % ("rs" if f else "bch", q, t) for f, q, t in ENC_CODES])
def test_encode_extract_against_model(family, q, t, coding):
    import torch
    rng = np.random.default_rng(q * 100 + t)
    for N in lengths(family, q, t):
        m = S.oracle(family, q, t, N, coding=coding)
        code = make(family, q, t, N, coding="multiplication" if coding else "division")
        hi = 2 if family == BCH else 1 << q
        msg = rng.integers(0, hi, (37, m.l)).astype(np.uint8)
        cw = code.encode_batch(msg)
        assert np.array_equal(cw, m.encode(msg)), N
        dev = code.encode_batch(torch.from_numpy(msg).cuda()).cpu().numpy()
        assert np.array_equal(dev, cw), N
        noisy = cw.copy()
        noisy[:, ::3] ^= rng.integers(0, hi, noisy[:, ::3].shape).astype(np.uint8)
        assert np.array_equal(code.extract_batch(noisy), m.extract(noisy)), N
        assert np.array_equal(code.extract_batch(torch.from_numpy(noisy).cuda()).cpu().numpy(), m.extract(noisy))


# ---- hard decoding ----
def mixed_batch(rng, m, B, symbols_high=True):
    """frames with 0..t errors, t+1..t+3 errors and virtual-position frames; RS words carry symbol values >= N"""
    hi = 2 if m.family == BCH else 1 << m.q
    msg = rng.integers(0, hi, (B, m.l)).astype(np.uint8)
    if m.family == RS and symbols_high:
        msg[:, ::5] = rng.integers(max(m.N, 0xCC) if m.q == 8 else hi // 2, hi, msg[:, ::5].shape)
    cw = m.encode(msg)
    rx = cw.copy()
    for f in range(B):
        kind = f % 6
        if kind == 5:
            pos = m.N + int(rng.integers(0, m.m.n - m.N))
            rx[f] = S.virtual_frame(m, pos, int(rng.integers(1, hi)))
            continue
        ne = int(rng.integers(0, m.t + 1)) if kind < 3 else m.t + 1 + int(rng.integers(0, 3))
        for p in rng.choice(m.N, min(ne, m.N), replace=False):
            rx[f, p] ^= 1 if m.family == BCH else int(rng.integers(1, hi))
    return rx


def erasure_lists(rng, m, B):
    per = []
    for f in range(B):
        ne = int(rng.integers(0, min(m.N, 2 * m.t + 2)))
        per.append(sorted(rng.choice(m.N, ne, replace=False).tolist()))
    return per


def check(res, model, alg, rx, per):
    out, nerr, st = model.correct_hard(alg, rx, per)
    got_st = np.asarray(res["status"])
    assert np.array_equal(got_st == 0, st == 0)
    assert np.array_equal(np.asarray(res["out"]), out)
    ok = st == 0
    assert np.array_equal(np.asarray(res["nerr"])[ok], nerr[ok])
    assert (np.asarray(res["nerr"])[~ok] == -1).all()
    virt = st == S.FRAME_LOCATOR
    if alg == BM:
        assert np.array_equal(got_st, S.native_status(st, got_st))
    return virt


HARD_CODES = [(RS, 8, 8, 204), (BCH, 8, 3, 200), (RS, 5, 4, 23), (BCH, 4, 2, 11), (RS, 8, 16, 129),
              (BCH, 7, 4, 65)]


@pytest.mark.parametrize("alg", [BM, PGZ, EUKLID])
@pytest.mark.parametrize("family,q,t,N", HARD_CODES)
def test_hard_decoding_against_model(family, q, t, N, alg):
    import torch
    rng = np.random.default_rng(N * 7 + alg)
    m = S.oracle(family, q, t, N)
    code = make(family, q, t, N, alg)
    for B in (1, 31, 33, 4161):
        rx = mixed_batch(rng, m, B)
        res = code.correct_batch(rx)
        virt = check(res, m, alg, rx, None)
        if B > 6:
            assert virt.sum() >= B // 6 - 1  # every constructed virtual frame fails
        dev = code.correct_batch(torch.from_numpy(rx).cuda())
        assert all(np.array_equal(np.asarray(res[k]), dev[k].cpu().numpy()) for k in ("out", "nerr", "status"))
        if B == 33:  # signed values, and in place on the device
            y = np.where(rx & 1, -1.0, 1.0).astype(np.float32) * rng.uniform(0.1, 2, rx.shape).astype(np.float32)
            if family == BCH:
                check(code.correct_batch(y), m, alg, y, None)
            d = torch.from_numpy(rx).cuda()
            nerr = torch.empty(B, dtype=torch.int32, device="cuda")
            st = torch.empty(B, dtype=torch.int32, device="cuda")
            capi.check(capi.lib().cc_correct_hard_batch_dev(code._h, C.c_void_p(d.data_ptr()), None, None,
                                                            C.c_void_p(d.data_ptr()), C.c_void_p(nerr.data_ptr()),
                                                            C.c_void_p(st.data_ptr()), B, None), "in place")
            torch.cuda.synchronize()
            assert np.array_equal(d.cpu().numpy(), np.asarray(res["out"]))
            assert np.array_equal(st.cpu().numpy(), np.asarray(res["status"]))
        if alg == PGZ and family == RS:
            continue  # "The PGZ-Algorithm does not support erasure decoding"
        per = erasure_lists(rng, m, B)
        res = code.correct_batch(rx, erasures=per)
        check(res, S.Shortened(S.Device(make(family, q, t, None, alg)), N), alg, rx, per)
        dev = code.correct_batch(torch.from_numpy(rx).cuda(), erasures=per)
        assert all(np.array_equal(np.asarray(res[k]), dev[k].cpu().numpy()) for k in ("out", "nerr", "status"))


def test_symbol_checks_use_the_field():
    code = make(RS, 8, 8, 204)
    rx = np.full((2, 204), 0xFF, np.uint8)  # 0xFF is a symbol of GF(256), above N
    res = code.correct_batch(rx)
    assert res["status"].shape == (2,)
    with pytest.raises(IndexError):  # a position >= N is refused as one >= n is on a full-length handle
        code.correct_batch(rx, erasures=[[204], []])
    er = np.array([204], np.uint16)
    off = np.array([0, 1, 1], np.uint32)
    out = np.zeros_like(rx)
    assert capi.lib().cc_correct_hard_batch(code._h, rx.ctypes.data_as(C.c_void_p), er.ctypes.data_as(C.c_void_p),
                                            off.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), None, None,
                                            2) == capi.ERR_INVALID_ARGUMENT
    r = make(RS, 5, 4, 20)
    r.correct_batch(np.full((1, 20), 31, np.uint8))  # 31 > N is a symbol of GF(32)
    with pytest.raises(cc.CcError) as e:
        r.correct_batch(np.full((1, 20), 32, np.uint8))
    assert e.value.status == capi.ERR_NOT_IN_FIELD


def test_long_locators_rs_t40():
    rng = np.random.default_rng(40)
    m = S.oracle(RS, 8, 40, 200)
    for alg in (BM, EUKLID):
        code = make(RS, 8, 40, 200, alg)
        rx = mixed_batch(rng, m, 120)
        check(code.correct_batch(rx), m, alg, rx, None)
        per = erasure_lists(rng, m, 120)
        check(code.correct_batch(rx, erasures=per), S.Shortened(S.Device(make(RS, 8, 40, None, alg)), 200), alg, rx, per)


def test_routes():
    assert "bit planes" in make(RS, 8, 8, 204).kernel_info()["kernel"]
    assert "bit planes" in make(BCH, 8, 3, 200).kernel_info()["kernel"]
    assert make(RS, 8, 8, 204).kernel_info() == cc.rs(8, cc.errors(8), cc.berlekamp_massey_tag()).kernel_info()
    soft = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20), n=200)
    assert soft.kernel_info()["kernel"].startswith("minsum_generic_kernel")


@pytest.mark.parametrize("alg", [BM, PGZ, EUKLID])
def test_at_scale_against_the_full_length_decoder(alg):
    """2^20 frames: RS(204,188) on the q-ary symmetric channel, BCH(200,176) on AWGN near the waterfall.  The shortened
    decode equals the rule applied to the full-length device decode of the padded words, frame for frame."""
    import torch
    frames = 1 << 20
    for family, q, t, N in ((RS, 8, 8, 204), (BCH, 8, 3, 200)):
        sh = make(family, q, t, N, alg)
        full = make(family, q, t, None, alg)
        if family == RS:
            rx = sh.discrete_channel(0.03, 0.0, 11, 1 << 33, frames, True)["recv"]
        else:
            llr, _ = awgn(sh, 6.0, 12, 1 << 34, frames, True)
            rx = (llr < 0).to(torch.uint8)
        res = sh.correct_batch(rx)
        padded = torch.zeros((frames, full.n), dtype=torch.uint8, device="cuda")
        padded[:, :N] = rx
        ref = full.correct_batch(padded)
        virt = (ref["out"][:, N:] != 0).any(dim=1)
        want_out = torch.where(virt[:, None], rx, ref["out"][:, :N])
        want_st = torch.where(virt, torch.full_like(ref["status"], S.FRAME_LOCATOR), ref["status"])
        loc_first = (want_st == S.FRAME_RECHECK) & (res["status"] == S.FRAME_LOCATOR)
        want_st = torch.where(loc_first, res["status"], want_st)
        want_ne = torch.where(virt, torch.full_like(ref["nerr"], -1), ref["nerr"])
        assert torch.equal(res["out"], want_out) and torch.equal(res["status"], want_st)
        assert torch.equal(res["nerr"], want_ne)
        assert 0 < int((want_st != 0).sum()) < frames // 2


# ---- 16-bit symbols ----
WIDE = [(BCH, 14, 12, 3000, 0x402B), (RS, 10, 6, 600, 0x409)]


@pytest.mark.parametrize("family,q,t,N,poly", WIDE)
def test_wide_against_full_length_device(family, q, t, N, poly):
    """against the device's own full-length decode, and on the same frames against the 16-bit oracle"""
    rng = np.random.default_rng(q)
    mm = S.Shortened(WideOracle(family, q, t, poly), N)
    for alg in (BM, EUKLID, PGZ):
        full = make(family, q, t, None, alg, modular_polynomial=poly)
        m = S.Shortened(S.Device(full), N)
        code = make(family, q, t, N, alg, modular_polynomial=poly)
        hi = 2 if family == BCH else 1 << q
        msg = rng.integers(0, hi, (40, m.l)).astype(np.uint16)
        cw = np.asarray(code.encode_batch(msg))
        assert np.array_equal(cw, m.encode(msg)) and np.array_equal(cw, mm.encode(msg))
        assert np.array_equal(np.asarray(code.extract_batch(cw)), msg) and np.array_equal(mm.extract(cw), msg)
        rx = cw.copy()
        for f in range(40):
            if f % 5 == 4:
                rx[f] = S.virtual_frame(m, N + int(rng.integers(0, full.n - N)), int(rng.integers(1, hi)))
                continue
            for p in rng.choice(N, int(rng.integers(0, t + 3)), replace=False):
                rx[f, p] ^= 1 if family == BCH else int(rng.integers(1, hi))
        res = code.correct_batch(rx)
        check(res, m, alg, rx, None)
        check(res, mm, alg, rx, None)
        if alg == PGZ and family == RS:
            continue
        per = erasure_lists(rng, m, 40)
        res = code.correct_batch(rx, erasures=per)
        check(res, m, alg, rx, per)
        check(res, mm, alg, rx, per)


# ---- min-sum over H[:, :N] ----
SOFT = [(4, 2, 11), (5, 2, 15), (6, 3, 50), (7, 4, 100), (8, 3, 200), (8, 2, 129)]
VARIANTS = [cc.min_sum_tag(8), cc.normalized_min_sum_tag(8, (3, 4)), cc.offset_min_sum_tag(8, (1, 4)),
            cc.self_correcting_1_min_sum_tag(8), cc.self_correcting_2_min_sum_tag(8),
            cc.normalized_2d_min_sum_tag(8, (3, 4), (1, 8))]


@pytest.mark.parametrize("q,t,N", SOFT + [(10, 3, 700)])
def test_minsum_against_oracle(q, t, N):
    rng = np.random.default_rng(N)
    kw = {"modular_polynomial": 0x409} if q == 10 else {}
    base = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), n=N, **kw)
    H = base.H()
    msg = rng.integers(0, 2, (24, base.l)).astype(np.uint8)
    cw = np.asarray(base.encode_batch(msg.astype(np.uint16) if q > 8 else msg)).astype(np.uint8)
    y = ((1.0 - 2.0 * cw) + rng.normal(0, 0.6, cw.shape)).astype(np.float32)
    per = [sorted(rng.choice(N, f % 4, replace=False).tolist()) for f in range(24)]
    ye = y.copy()
    for f, e in enumerate(per):
        ye[f, e] = 0.0
    for tag in VARIANTS:
        for stop in (capi.STOP_AS_SHIPPED, capi.STOP_PUBLISHED, capi.STOP_PARITY):
            code = cc.primitive_bch(q, cc.errors(t), tag, n=N, stop_rule=stop, **kw)
            assert code.kernel_info()["kernel"].startswith("minsum_generic_kernel")
            res = code.correct_batch(y, erasures=per, want_L=True)
            ob, oL, oit, ost = Oracle.minsum_H(H, tag.alg - capi.ALG_MS, tag.iterations, ye, alpha=tag.alpha,
                                               beta=tag.beta, stop=stop)
            assert np.array_equal(res["out"], ob), (tag, stop)
            assert np.array_equal(res["status"], ost)
            assert np.array_equal(res["iters"].astype(np.uint32), oit)
            assert np.allclose(res["L"], oL, rtol=0, atol=1e-5)


# ---- Monte-Carlo ----
@pytest.mark.parametrize("q,t,N", [(4, 2, 11), (6, 3, 50), (8, 3, 200), (8, 3, 251)])
@pytest.mark.parametrize("random_cw", [False, True])
def test_awgn_channel_equals_model(q, t, N, random_cw):
    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), n=N)
    assert abs(code.sigma(3.0) - 1.0 / np.sqrt(2.0 * ((N - code.k) / N) * 10 ** 0.3)) < 1e-12
    seed, first, frames = (3 << 32) + 5, (1 << 32) - 700, 2000
    llr, sent = awgn(code, 3.0, seed, first, frames, random_cw)
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    if random_cw:
        assert np.array_equal(s, S.oracle(BCH, q, t, N).encode(bch_message_bits(seed, first, frames, code.l)))
    else:
        assert not s.any()
    sig = sigma_f32(code, 3.0)
    assert np.abs(y - awgn_reference(N, sig, seed, first, frames, s)).max() <= tau(sig)


@pytest.mark.parametrize("alg,ebno", [(BM, 5.0), (PGZ, 5.0), ("ms", 3.5)])
@pytest.mark.parametrize("random_cw", [False, True])
def test_mc_counters_equal_batch_api(alg, ebno, random_cw):
    import torch
    for q, t, N in ((8, 3, 200), (4, 2, 11)):
        code = (cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(10), n=N) if alg == "ms" else
                make(BCH, q, t, N, alg))
        frames = 40000 if N > 16 else 20000
        seed, first = 9, 1 << 35
        c = awgn_mc(code, ebno, seed, first, frames, random_cw)
        llr, sent = awgn(code, ebno, seed, first, frames, random_cw)
        res = code.correct_batch(llr)
        errs = (res["out"] != sent).sum(dim=1)
        failed = res["status"] != 0
        assert c[capi.MC_FRAMES] == frames
        assert c[capi.MC_BIT_ERRORS] == int(errs.sum())
        assert c[capi.MC_FAILURES] == int(failed.sum())
        assert c[capi.MC_WORD_ERRORS] == int((failed | (errs > 0)).sum())
        assert c[capi.MC_CHANNEL_BIT_ERRORS] == int(((llr < 0).to(torch.uint8) != sent).sum())
        assert 0 < c[capi.MC_WORD_ERRORS] < frames
        if not code.algorithm.soft:  # the decoder against the model
            m = S.oracle(BCH, q, t, N)
            out, _, st = m.correct_hard(alg, llr[:3000].cpu().numpy())
            assert np.array_equal(res["out"][:3000].cpu().numpy(), out)
            assert np.array_equal(res["status"][:3000].cpu().numpy() == 0, st == 0)


def test_mc_across_the_chunk():
    code = make(BCH, 5, 3, 25)
    frames, seed, first = (1 << 20) + 3000, 4, 77
    c = awgn_mc(code, 4.0, seed, first, frames, True)
    llr, sent = awgn(code, 4.0, seed, first, frames, True)
    res = code.correct_batch(llr)
    errs = (res["out"] != sent).sum(dim=1)
    assert c[capi.MC_BIT_ERRORS] == int(errs.sum()) and c[capi.MC_FAILURES] == int((res["status"] != 0).sum())


@pytest.mark.parametrize("which,p,e", [("bch", 0.004, 0.0), ("bch", 0.0, 0.02), ("bch-pgz", 0.002, 0.01),
                                       ("rs", 0.03, 0.0), ("rs", 0.01, 0.04), ("bch11", 0.02, 0.03)])
def test_discrete_counters_equal_batch_api(which, p, e):
    code = {"bch": lambda: make(BCH, 8, 3, 200), "bch-pgz": lambda: make(BCH, 8, 3, 200, PGZ),
            "rs": lambda: make(RS, 8, 8, 204), "bch11": lambda: make(BCH, 4, 2, 11)}[which]()
    seed, first, frames = 6, 3 << 36, (1 << 20) + 513
    c = discrete_mc(code, p, e, seed, first, frames, True)
    ch = code.discrete_channel(p, e, seed, first, frames, True)
    res = discrete_decode(code, ch, frames)
    sent, recv = ch["sent"], ch["recv"]
    erased = erased_mask(ch, frames, code.n)
    errs = (res["out"] != sent).sum(dim=1)
    failed = res["status"] != 0
    assert c[capi.MC_FRAMES] == frames
    assert c[capi.MC_CHANNEL_ERASURES] == int(erased.sum())
    assert c[capi.MC_CHANNEL_BIT_ERRORS] == int(((recv != sent) & ~erased).sum())
    assert c[capi.MC_BIT_ERRORS] == int(errs.sum())
    assert c[capi.MC_FAILURES] == int(failed.sum())
    assert c[capi.MC_WORD_ERRORS] == int((failed | (errs > 0)).sum())
    # the channel's words are the shortened code's
    m = S.oracle(code.family, code.q, code.t, code.n)
    s = sent[:500].cpu().numpy()
    assert np.array_equal(m.encode(m.extract(s)), s)
