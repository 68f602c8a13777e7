"""The checker of RS decoding with roots alpha^(mu + i step) (tests/rs_roots_model.py) against the plain-C oracle, on the
CPU: T carries (mu, step) codewords onto (1, 1) codewords, T^-1 T is the identity, decoding a received word through
T^-1 . oracle(1, 1) . T returns the sent word up to the capability -- with erasures too -- and the seeds of the GPU parity
tests keep the oracle's fenced frames (ref_ub) under 5 %.  And what stays refused, on CC_DEVICE_NONE handles."""
import ctypes as C

import numpy as np
import pytest

import rs_roots_model as M
from checkers import BM, EUKLID, PGZ, RS, Oracle

import channelcoding_amd as cc
from channelcoding_amd import capi

NONE = capi.DEVICE_NONE


@pytest.mark.parametrize("q,t,mu,step", M.SETS)
def test_twist_maps_codewords_onto_the_1_1_code(q, t, mu, step):
    o, o11 = Oracle(RS, q, t, mu, step), Oracle(RS, q, t)
    nf = o.n
    rng = np.random.default_rng(40 + q + t)
    cw = o.encode(rng.integers(0, 1 << q, (64, o.l)).astype(np.uint8))
    tw = M.T(cw, o11.exp, o11.log, nf, mu, step)
    for f in range(64):
        assert (o.syndromes(cw[f]) == 0).all()
        assert (o11.syndromes(tw[f]) == 0).all(), f
    if (mu, step) != (1, 1):
        assert any((o11.syndromes(cw[f]) != 0).any() for f in range(64))  # (the untwisted words are no (1, 1) codewords)
    x = rng.integers(0, 1 << q, (64, nf)).astype(np.uint8)
    assert np.array_equal(M.T_inv(M.T(x, o11.exp, o11.log, nf, mu, step), o11.exp, o11.log, nf, mu, step), x)
    assert np.array_equal(M.T(M.T_inv(x, o11.exp, o11.log, nf, mu, step), o11.exp, o11.log, nf, mu, step), x)
    # Hamming weights and positions: T is a monomial map
    assert np.array_equal((M.T(x, o11.exp, o11.log, nf, mu, step) != 0).sum(1), (x != 0).sum(1))


def through_oracle(o11, alg, rx, per, nf, mu, step, n=None):
    """T^-1 . oracle(1, 1) . T, frame by frame: out, nerr, status, ref_ub"""
    B = rx.shape[0]
    out = np.zeros_like(rx)
    nerr, st, ub = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tw = M.T(rx, o11.exp, o11.log, nf, mu, step)
    for f in range(B):
        er = [M.position(p, nf, step) for p in per[f]] if per is not None else ()
        o_, n_, s_, u_ = o11.correct_hard(alg, tw[f:f + 1], er)
        out[f] = M.T_inv(o_, o11.exp, o11.log, nf, mu, step, n)[0]
        nerr[f], st[f], ub[f] = n_[0], s_[0], u_[0]
    return out, nerr, st, ub


@pytest.mark.parametrize("q,t,mu,step", M.SETS)
def test_decoding_through_the_oracle_returns_the_sent_word(q, t, mu, step):
    o, o11 = Oracle(RS, q, t, mu, step), Oracle(RS, q, t)
    rng = np.random.default_rng(7000 + 10 * q + t)  # (the seeds of tests/test_gpu_rs_roots.py)
    cw = o.encode(rng.integers(0, 1 << q, (200, o.l)).astype(np.uint8))
    for with_erasures in (False, True):
        rx, per, within = M.make_frames(rng, cw, t, q, with_erasures)
        for alg in (BM, EUKLID) if with_erasures else (BM, EUKLID, PGZ):
            out, nerr, st, ub = through_oracle(o11, alg, rx, per, o.n, mu, step)
            assert (st[within] == 0).all() and np.array_equal(out[within], cw[within]), (alg, with_erasures)
            assert (ub != 0).mean() <= 0.05, (alg, with_erasures, (ub != 0).mean())


def test_shortened_code_keeps_its_positions():
    """step = 1: T keeps positions, so RS(204,188) with mu = 0 is checked on words padded to 255 symbols."""
    o, o11 = Oracle(RS, 8, 8, 0, 1), Oracle(RS, 8, 8)
    rng = np.random.default_rng(7204)
    msg = np.zeros((100, o.l), np.uint8)
    msg[:, :188] = rng.integers(0, 256, (100, 188))
    cw = o.encode(msg)[:, :204]  # message symbols 188 .. 238 are zero: positions 204 .. 254 of the word
    assert (o.encode(msg)[:, 204:] == 0).all()
    rx, per, within = M.make_frames(rng, cw, 8, 8, True)
    out, nerr, st, ub = through_oracle(o11, BM, rx, per, 255, 0, 1, n=204)
    assert (st[within] == 0).all() and np.array_equal(out[within], cw[within])


def _refused(code, erasures=None):
    """status of a hard-decode call on a handle without a device: what the decoders refuse is answered before the device
    is asked for (CC_ERR_UNSUPPORTED), a call that would run answers CC_ERR_NO_DEVICE"""
    buf = np.zeros(code.n, np.uint8)
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    er = off = None
    if erasures is not None:
        er, off = np.asarray(erasures, np.uint16), np.asarray([0, len(erasures)], np.uint32)
    return capi.lib().cc_correct_hard_batch(code._h, P(buf), P(er), P(off), P(buf), None, None, 1)


def test_what_stays_refused():
    bm, pgz = cc.berlekamp_massey_tag, cc.peterson_gorenstein_zierler_tag
    lib = capi.lib()
    # a step that shares a factor with 2^q - 1 = 15: alpha^(3 p) does not name the position p
    assert _refused(cc.rs(4, cc.errors(2), bm(), mu=1, step=3, device=NONE)) == capi.ERR_UNSUPPORTED
    assert b"gcd(step" in lib.cc_last_error()
    # an exponent reaching nf = 2^q - 1: mu + (2t - 1) step = 10 + 5 = 15, and the CCSDS setting (112, 11) at t = 16
    assert _refused(cc.rs(4, cc.errors(3), bm(), mu=10, step=1, device=NONE)) == capi.ERR_UNSUPPORTED
    assert _refused(cc.rs(8, cc.errors(16), bm(), mu=112, step=11, device=NONE)) == capi.ERR_UNSUPPORTED
    # RS with the PGZ tag and erasures
    assert _refused(cc.rs(8, cc.errors(8), pgz(), mu=0, step=1, device=NONE), erasures=[3]) == capi.ERR_UNSUPPORTED
    assert b"PGZ" in lib.cc_last_error()
    # what is in scope gets as far as the device check: the last exponent at nf - 1 exactly, the six parity sets,
    # the PGZ tag without erasures, BM with them
    assert _refused(cc.rs(4, cc.errors(3), bm(), mu=9, step=1, device=NONE)) == capi.ERR_NO_DEVICE
    for q, t, mu, step in M.SETS:
        assert _refused(cc.rs(q, cc.errors(t), bm(), mu=mu, step=step, device=NONE)) == capi.ERR_NO_DEVICE
    assert _refused(cc.rs(8, cc.errors(8), pgz(), mu=0, step=1, device=NONE)) == capi.ERR_NO_DEVICE
    assert _refused(cc.rs(8, cc.errors(8), bm(), mu=0, step=1, device=NONE), erasures=[3]) == capi.ERR_NO_DEVICE
    for code, er in ((cc.rs(4, cc.errors(2), bm(), mu=1, step=3, device=NONE), 0),
                     (cc.rs(8, cc.errors(8), pgz(), mu=0, step=1, device=NONE), 1)):
        assert lib.cc_hard_route(code._h, 64, er) == -capi.ERR_UNSUPPORTED
    assert lib.cc_hard_route(cc.rs(8, cc.errors(8), bm(), mu=0, step=1, device=NONE)._h, 64, 0) == -capi.ERR_NO_DEVICE
    # 16-bit symbols: refused when the handle is made
    for mu, step in ((1, 3), (1020, 1)):  # gcd(3, 1023) = 3; 1020 + 3 = 1023
        with pytest.raises(cc.CcError) as e:
            cc.rs(10, cc.errors(2), bm(), mu=mu, step=step, modular_polynomial=0x409, device=NONE)
        assert e.value.status == capi.ERR_UNSUPPORTED
