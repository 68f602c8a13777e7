"""GPU parity tests of RS hard decoding with roots alpha^(mu + i step) other than alpha^1 .. alpha^2t.

The checker is the equivalence of tests/rs_roots_model.py, not the reference (whose rs::error_values builds its system
from x^1, x^2, .. whatever mu is and fails every frame with an error): for every frame, out / nerr / status of the
(mu, step) handle equal T^-1 of what the plain-C oracle's (1, 1) decoder gives for T(w) -- miscorrections beyond the
capability and the Euklid tag's odd-erasure frames included.  Frames the oracle fences (ref_ub) are checked by the sent
word only; tests/test_rs_roots_host.py pins that the seeds used here keep them under 5 %.  GF(2^10): frames within the
capability must return the sent word, every frame must equal the device's own (1, 1) decode of T(w), and every frame must
equal what the 16-bit oracle (checkers.WideOracle) gives for the (mu, step) code.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import rs_roots_model as M
import shortened_model as S
from checkers import BM, EUKLID, PGZ, RS, Oracle, WideOracle
from test_rs_roots_host import through_oracle

import channelcoding_amd as cc
from channelcoding_amd import capi

pytestmark = pytest.mark.gpu

TAGS = {PGZ: cc.peterson_gorenstein_zierler_tag, BM: cc.berlekamp_massey_tag, EUKLID: cc.euklid_tag}
SIZES = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4161)


def check(res, alg, rx, cw, within, expect):
    """res of the (mu, step) handle against expect = (out, nerr, status, ref_ub) through the (1, 1) oracle"""
    out, nerr, st, ub = expect
    print("frames %d  fenced %d  decoded %d  device decoded %d" % (len(st), (ub != 0).sum(), (st == 0).sum(),
                                                                   (res["status"] == 0).sum()))
    assert (ub != 0).mean() <= 0.05
    keep = ub == 0
    ok = keep & (st == 0)
    assert np.array_equal((res["status"] == 0)[keep], (st == 0)[keep])
    assert np.array_equal(res["out"][ok], out[ok])
    assert np.array_equal(res["nerr"][ok], nerr[ok])
    bad = keep & (st != 0)
    assert (res["nerr"][bad] == -1).all()
    assert np.array_equal(res["out"][bad], rx[bad])  # a failed frame returns the received word
    if alg == BM:  # the failure class is defined algorithm for algorithm for BM only (tests/test_gpu_algebraic.py)
        assert np.array_equal(res["status"][keep], st[keep])
    fenced_within = ~keep & within  # fenced frames: by the sent word
    assert (res["status"][fenced_within] == 0).all() and np.array_equal(res["out"][fenced_within], cw[fenced_within])
    assert (res["status"][within] == 0).all() and np.array_equal(res["out"][within], cw[within])


@pytest.mark.parametrize("q,t,mu,step", M.SETS)
def test_parity_with_the_1_1_decode(q, t, mu, step):
    o, o11 = Oracle(RS, q, t, mu, step), Oracle(RS, q, t)
    rng = np.random.default_rng(7000 + 10 * q + t)
    cw = o.encode(rng.integers(0, 1 << q, (200, o.l)).astype(np.uint8))
    for with_erasures in (False, True):
        rx, per, within = M.make_frames(rng, cw, t, q, with_erasures)
        for alg in (BM, EUKLID) if with_erasures else (BM, EUKLID, PGZ):
            code = cc.rs(q, cc.errors(t), TAGS[alg](), mu=mu, step=step)
            assert np.array_equal(code.encode_batch(cw[:, o.k:]), cw)
            expect = through_oracle(o11, alg, rx, per, o.n, mu, step)
            check(code.correct_batch(rx, per), alg, rx, cw, within, expect)
            dec = code.decode_batch(rx, per)
            good = expect[2] == 0
            assert np.array_equal(dec["msg"][good & (expect[3] == 0)], expect[0][good & (expect[3] == 0)][:, o.k:])
    with pytest.raises(cc.CcError) as e:  # RS + PGZ + erasures stays refused
        cc.rs(q, cc.errors(t), TAGS[PGZ](), mu=mu, step=step).correct_batch(rx, per)
    assert e.value.status == capi.ERR_UNSUPPORTED


def test_dvb_rs_204_188():
    """RS(204,188) with first root alpha^0, shortened from 255: step = 1 keeps positions, the words go to the oracle padded"""
    o, o11 = Oracle(RS, 8, 8, 0, 1), Oracle(RS, 8, 8)
    rng = np.random.default_rng(7204)
    msg = np.zeros((300, o.l), np.uint8)
    msg[:, :188] = rng.integers(0, 256, (300, 188))
    cw = o.encode(msg)[:, :204]
    for with_erasures in (False, True):
        rx, per, within = M.make_frames(rng, cw, 8, 8, with_erasures)
        for alg in (BM, EUKLID) if with_erasures else (BM, EUKLID, PGZ):
            code = cc.rs(8, cc.errors(8), TAGS[alg](), mu=0, step=1, n=204)
            assert code.hard_route(300, with_erasures) == (capi.HARD_ROUTE_PLANES if not with_erasures or alg != PGZ else -1)
            assert np.array_equal(code.encode_batch(msg[:, :188]), cw)
            out, nerr, st, ub = through_oracle(o11, alg, rx, per, 255, 0, 1, n=204)
            # a locator root at a position >= 204 fails the shortened code: the padded decode "corrects" a
            # symbol the word does not have
            pad = M.T_inv(o11.correct_hard(alg, M.T(rx, o11.exp, o11.log, 255, 0, 1))[0], o11.exp, o11.log, 255, 0, 1) \
                if not with_erasures else None
            if pad is not None:
                virtual = (st == 0) & (pad[:, 204:] != 0).any(1)
                st, nerr = np.where(virtual, capi.FRAME_LOCATOR, st), np.where(virtual, -1, nerr)
            else:
                virtual = np.zeros(300, bool)
                for f in np.nonzero(st == 0)[0]:
                    er = list(per[f])
                    full = M.T_inv(o11.correct_hard(alg, M.T(rx[f:f + 1], o11.exp, o11.log, 255, 0, 1), er)[0], o11.exp,
                                   o11.log, 255, 0, 1)
                    virtual[f] = (full[0, 204:] != 0).any()
                st, nerr = np.where(virtual, capi.FRAME_LOCATOR, st), np.where(virtual, -1, nerr)
            check(code.correct_batch(rx, per), alg, rx, cw, within, (out, nerr, st, ub))


def _wide_frames(rng, code, frames, t, with_erasures):
    msg = rng.integers(0, 1 << 10, (frames, code.l)).astype(np.uint16)
    cw = code.encode_batch(msg)
    rx, per, within = M.make_frames(rng, cw, t, 10, with_erasures)
    nerrors = (rx != cw).sum(1)
    return cw, rx, per, within, nerrors


@pytest.mark.parametrize("n", [None, 544])
def test_gf1024_against_its_own_1_1_decode(n):
    """(q, t, mu, step) = (10, 15, 0, 1), polynomial 0x409, full length and shortened to 544 (802.3 RS(544,514))"""
    exp, log = M.field_tables(10, 0x409)
    rng = np.random.default_rng(7100 + (n or 0))
    model = WideOracle(RS, 10, 15, 0x409, 0, 1)
    if n:
        model = S.Shortened(model, n)
    for with_erasures in (False, True):
        for alg in (BM, EUKLID) if with_erasures else (BM, EUKLID, PGZ):
            kw = dict(modular_polynomial=0x409, n=n)
            code = cc.rs(10, cc.errors(15), TAGS[alg](), mu=0, step=1, **kw)
            twin = cc.rs(10, cc.errors(15), TAGS[alg](), **kw)
            assert code.hard_route(64, with_erasures) == capi.HARD_ROUTE_WIDE
            cw, rx, per, within, nerrors = _wide_frames(rng, code, 96, 15, with_erasures)
            N = code.n
            tw = M.T(cw, exp, log, 1023, 0, 1)[:, :N]
            assert np.array_equal(twin.encode_batch(tw[:, twin.k:]), tw)  # T(codeword) is a word of the (1, 1) code
            res = code.correct_batch(rx, per)
            assert (res["status"][within] == 0).all() and np.array_equal(res["out"][within], cw[within])
            # nerr counts the roots of the locator: the erased positions (whatever they carry) and the errors elsewhere
            rho = np.array([len(p) for p in per] if with_erasures else [0] * 96)
            for f in range(96):
                if with_erasures:
                    nerrors[f] = np.delete(rx[f] != cw[f], per[f]).sum()
            print("nerr expected", (nerrors + rho)[within][:12], "device", res["nerr"][within][:12])
            assert np.array_equal(res["nerr"][within], (nerrors + rho)[within])
            ref = twin.correct_batch(M.T(rx, exp, log, 1023, 0, 1)[:, :N], per)
            back = np.zeros((96, 1023), np.uint16)
            back[:, :N] = ref["out"]
            assert np.array_equal(res["out"], M.T_inv(back, exp, log, 1023, 0, 1, N))
            assert np.array_equal(res["nerr"], ref["nerr"]) and np.array_equal(res["status"], ref["status"])
            # and the same frames against the 16-bit oracle (tests/test_gpu_wide_model.py has the rule)
            want_out, want_nerr, want_st = model.correct_hard(alg, rx, per)[:3]
            assert np.array_equal(res["status"] == 0, want_st == 0)
            assert np.array_equal(res["out"], np.where((want_st == 0)[:, None], want_out, rx))
            assert np.array_equal(res["nerr"], np.where(want_st == 0, want_nerr, -1))
            if alg == BM:
                assert np.array_equal(res["status"], S.native_status(want_st, res["status"]) if n else want_st)
            print("GF(1024) n %d alg %d erasures %d: decoded %d / 96" % (N, alg, with_erasures, (res["status"] == 0).sum()))


@pytest.mark.parametrize("t,alg", [(8, BM), (16, BM), (16, PGZ), (8, EUKLID)])
def test_chain_boundaries(t, alg):
    """mu = 0 on the bit-plane chain (the suite runs with the planes threshold at 0) at every layout boundary: 32 frames per
    group, 64 per chunk, 2048 per block; all-clean, all-dirty and hopeless chunks; in place; float input is below."""
    import torch
    o, o11 = Oracle(RS, 8, t, 0, 1), Oracle(RS, 8, t)
    code = cc.rs(8, cc.errors(t), TAGS[alg](), mu=0, step=1)
    rng = np.random.default_rng(7300 + t + alg)
    pool = o.encode(rng.integers(0, 256, (320, o.l)).astype(np.uint8))
    rxp, _, withinp = M.make_frames(rng, pool, t, 8, False)
    rxp[:64] = pool[:64]  # an all-clean chunk
    withinp[:64] = True
    rxp[64:128] = np.stack([M.make_frames(rng, pool[f:f + 1], t, 8, False)[0][0] for f in range(64, 128)])
    for f in range(128, 192):  # an all-dirty chunk at the capability, then a hopeless one
        rxp[f] = pool[f]
        for p in rng.choice(255, t, replace=False):
            rxp[f, p] ^= int(rng.integers(1, 256))
        withinp[f] = True
    for f in range(192, 256):
        rxp[f] = pool[f]
        for p in rng.choice(255, 2 * t + 8, replace=False):
            rxp[f, p] ^= int(rng.integers(1, 256))
        withinp[f] = False
    withinp[64:128] = (rxp[64:128] != pool[64:128]).sum(1) <= t
    ex = through_oracle(o11, alg, rxp, None, 255, 0, 1)
    for frames in SIZES:
        assert code.hard_route(frames) == capi.HARD_ROUTE_PLANES
        idx = np.arange(frames) % 320
        rx, cw, within = rxp[idx], pool[idx], withinp[idx]
        expect = tuple(a[idx] for a in ex)
        check(code.correct_batch(rx), alg, rx, cw, within, expect)
        if frames in (33, 2049):  # device pointers, in place
            buf = torch.from_numpy(rx).cuda()
            n_, s_ = torch.empty(frames, dtype=torch.int32, device="cuda"), torch.empty(frames, dtype=torch.int32, device="cuda")
            P = lambda x: x.data_ptr()
            capi.check(capi.lib().cc_correct_hard_batch_dev(code._h, P(buf), None, None, P(buf), P(n_), P(s_), frames, None),
                       "cc_correct_hard_batch_dev")
            torch.cuda.synchronize()
            check(dict(out=buf.cpu().numpy(), nerr=n_.cpu().numpy(), status=s_.cpu().numpy()), alg, rx, cw, within, expect)


def test_chain_with_erasures_and_table_routes():
    """erasures on the chain (BM: the chain; Euklid: the chain first, Sugiyama over what it leaves), and the routes"""
    for t in (8, 16):
        o, o11 = Oracle(RS, 8, t, 0, 1), Oracle(RS, 8, t)
        rng = np.random.default_rng(7400 + t)
        cw = o.encode(rng.integers(0, 256, (257, o.l)).astype(np.uint8))
        rx, per, within = M.make_frames(rng, cw, t, 8, True)
        for alg in (BM, EUKLID):
            code = cc.rs(8, cc.errors(t), TAGS[alg](), mu=0, step=1)
            assert code.hard_route(257, True) == capi.HARD_ROUTE_PLANES
            check(code.correct_batch(rx, per), alg, rx, cw, within, through_oracle(o11, alg, rx, per, 255, 0, 1))
    bm = cc.berlekamp_massey_tag
    assert cc.rs(8, cc.errors(8), bm(), mu=0, step=1).hard_route(4096) == capi.HARD_ROUTE_PLANES
    assert cc.rs(8, cc.errors(8), bm()).hard_route(4096) == capi.HARD_ROUTE_PLANES
    assert cc.rs(8, cc.errors(4), bm(), mu=2, step=1).hard_route(4096) == capi.HARD_ROUTE_CHUNK
    assert cc.rs(8, cc.errors(3), bm(), mu=7, step=7).hard_route(4096) == capi.HARD_ROUTE_WAVE  # fewer than 8 syndromes
    assert cc.rs(8, cc.errors(8), bm(), mu=7, step=7).hard_route(4096) == capi.HARD_ROUTE_CHUNK
    assert cc.rs(4, cc.errors(3), bm(), mu=0, step=1).hard_route(4096) == capi.HARD_ROUTE_WAVE
    lib = capi.lib()
    assert lib.cc_hard_route(cc.rs(4, cc.errors(2), bm(), mu=1, step=3)._h, 64, 0) == -capi.ERR_UNSUPPORTED
    assert lib.cc_hard_route(cc.rs(4, cc.errors(3), bm(), mu=10, step=1)._h, 64, 0) == -capi.ERR_UNSUPPORTED
    assert lib.cc_hard_route(cc.rs(8, cc.errors(16), bm(), mu=112, step=11)._h, 64, 0) == -capi.ERR_UNSUPPORTED
    pgz = cc.rs(8, cc.errors(8), cc.peterson_gorenstein_zierler_tag(), mu=0, step=1)
    assert lib.cc_hard_route(pgz._h, 64, 1) == -capi.ERR_UNSUPPORTED and pgz.hard_route(4096) == capi.HARD_ROUTE_PLANES
    for code in (cc.rs(4, cc.errors(2), bm(), mu=1, step=3), cc.rs(4, cc.errors(3), bm(), mu=10, step=1)):
        with pytest.raises(cc.CcError) as e:
            code.correct_batch(np.zeros((1, 15), np.uint8))
        assert e.value.status == capi.ERR_UNSUPPORTED


def test_float_input():
    """hard decision of a signed sequence (bit = x < 0) through the mu = 0 kernels: the words are 0 / 1 symbols"""
    o, o11 = Oracle(RS, 8, 8, 0, 1), Oracle(RS, 8, 8)
    rng = np.random.default_rng(7500)
    cw = np.zeros((2100, 255), np.uint8)
    rx = cw.copy()
    for f in range(2100):
        for p in rng.choice(255, int(rng.integers(0, 12)), replace=False):
            rx[f, p] = 1
    within = rx.sum(1) <= 8
    soft = np.where(rx != 0, -1.0, 1.0).astype(np.float32) * rng.uniform(0.1, 3.0, rx.shape).astype(np.float32)
    expect = through_oracle(o11, BM, rx, None, 255, 0, 1)
    for mu, step, n in ((0, 1, 2100), (2, 1, 300)):
        if (mu, step) != (0, 1):
            expect = through_oracle(Oracle(RS, 8, 8), BM, rx[:n], None, 255, mu, step)
        code = cc.rs(8, cc.errors(8), TAGS[BM](), mu=mu, step=step)
        a, b = code.correct_batch(rx[:n]), code.correct_batch(soft[:n])
        for key in ("out", "status", "nerr"):
            assert np.array_equal(a[key], b[key]), key
        check(b, BM, rx[:n], cw[:n], within[:n], tuple(x[:n] for x in expect))


_ALT = (
    "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np\n"
    "import rs_roots_model as M\n"
    "from checkers import BM, EUKLID, PGZ, RS, Oracle\n"
    "from test_rs_roots_host import through_oracle\n"
    "from test_gpu_rs_roots import TAGS, check\n"
    "import channelcoding_amd as cc\n"
    "from channelcoding_amd import capi\n"
    "rng = np.random.default_rng(7600)\n"
    "for t, alg in ((8, BM), (16, PGZ), (16, EUKLID)):\n"
    "    o, o11 = Oracle(RS, 8, t, 0, 1), Oracle(RS, 8, t)\n"
    "    code = cc.rs(8, cc.errors(t), TAGS[alg](), mu=0, step=1)\n"
    "    assert code.hard_route(2200) != capi.HARD_ROUTE_PLANES\n"
    "    for frames in (1, 65, 2200):\n"
    "        cw = o.encode(rng.integers(0, 256, (min(frames, 300), o.l)).astype(np.uint8))\n"
    "        rx, _, within = M.make_frames(rng, cw, t, 8, False)\n"
    "        ex = through_oracle(o11, alg, rx, None, 255, 0, 1)\n"
    "        idx = np.arange(frames) %% cw.shape[0]\n"
    "        check(code.correct_batch(rx[idx]), alg, rx[idx], cw[idx], within[idx], tuple(a[idx] for a in ex))\n"
    "    cw = o.encode(rng.integers(0, 256, (200, o.l)).astype(np.uint8))\n"
    "    if alg != PGZ:\n"
    "        rx, per, within = M.make_frames(rng, cw, t, 8, True)\n"
    "        check(code.correct_batch(rx, per), alg, rx, cw, within, through_oracle(o11, alg, rx, per, 255, 0, 1))\n"
    "print('ALT OK')\n")


@pytest.mark.parametrize("switch", ["CC_AMD_NO_BITSLICE", "CC_AMD_NO_CHUNK"])
def test_table_kernels_agree(switch):
    """the same mu = 0 codes through the table kernels; the switches are read once per process, so in one of its own"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)  # (either switch alone keeps the calls off the plane chain: it needs the chunk kernels)
    env.pop("CC_AMD_NO_BITSLICE", None)
    env.pop("CC_AMD_NO_CHUNK", None)
    env[switch] = "1"
    out = subprocess.run([sys.executable, "-c", _ALT % (here, os.path.dirname(here))], env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and "ALT OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("t", [8, 16])
def test_encode_mu0_on_planes(t):
    """RS(255,239) / RS(255,223) with first root alpha^0: evaluation at alpha^0 .. alpha^(2t-1) and interpolation"""
    o = Oracle(RS, 8, t, 0, 1)
    code = cc.rs(8, cc.errors(t), TAGS[BM](), mu=0, step=1)
    rng = np.random.default_rng(7700 + t)
    for frames in SIZES:
        msg = rng.integers(0, 256, (frames, o.l)).astype(np.uint8)
        msg[0] = 0
        if frames > 2:
            msg[1] = 255
            msg[2, :-1] = 0
        cw = code.encode_batch(msg)
        assert np.array_equal(cw, o.encode(msg)), frames
        assert np.array_equal(code.extract_batch(cw), msg)


def test_unchanged_behaviour():
    """mu = step = 1 RS(255,223) against the oracle as before; the Monte-Carlo entry points still refuse mu = 2"""
    import torch
    from test_gpu_algebraic import check_against_oracle, corrupt
    o = Oracle(RS, 8, 16)
    rng = np.random.default_rng(7800)
    cw = o.encode(rng.integers(0, 256, (700, o.l)).astype(np.uint8))
    rx = np.stack([corrupt(rng, o, cw[f], int(rng.integers(0, 20))) for f in range(700)])
    for alg in (BM, PGZ, EUKLID):
        check_against_oracle(cc.rs(8, cc.errors(16), TAGS[alg]()).correct_batch(rx), o, alg, rx)
    mu2 = cc.rs(8, cc.errors(4), TAGS[BM](), mu=2)
    cnt = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    lib = capi.lib()
    assert lib.cc_mc_run_discrete_dev(mu2._h, 0.01, 0.0, 0, 0, 64, 0, cnt.data_ptr(), None) == capi.ERR_UNSUPPORTED
    assert lib.cc_mc_run_dev(mu2._h, 5.0, 0, 0, 64, 0, cnt.data_ptr(), None) == capi.ERR_UNSUPPORTED
    assert int(cnt.sum()) == 0
