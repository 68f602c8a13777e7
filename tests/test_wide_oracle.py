"""The 16-bit build of the plain-C oracle (oracle/cc_oracle_wide.c, checkers.WideOracle) pinned on the CPU:

* symbol for symbol against the byte build (checkers.Oracle, itself pinned to the real reference) on every code of
  checkers.REF_CODES and on the q = 3 .. 8 extremes of test_gpu_algebraic.test_extreme_code_parameters;
* against tests/golden/wide.npz, the real reference's vectors for BCH(511,484) and RS(1023,1015), under the fences of
  tests/test_oracle_golden.py (F3 through ref_ub, Q9 for PGZ);
* against the real reference itself where oracle/_ref carries the wide driver;
* the library's host construction for q = 9 .. 15 against the model's, on handles without a device.
"""
import os

import numpy as np
import pytest

import rs_roots_model as M
from checkers import BCH, BM, EUKLID, PGZ, REF_CODES, RS, Oracle, RefWide, WideOracle
from test_rs_roots_host import through_oracle

import channelcoding_amd as cc
from channelcoding_amd import capi

ALGS = ((PGZ, "pgz", "PGZ"), (BM, "bm", "BM"), (EUKLID, "euklid", "EUKLID"))
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide.npz"))
# the (fam, q, t) of tests/test_gpu_algebraic.py::test_extreme_code_parameters
EXTREMES = [(BCH, 3, 1), (BCH, 4, 1), (BCH, 5, 7), (BCH, 8, 1), (RS, 8, 1), (RS, 8, 32), (RS, 8, 31), (RS, 5, 12),
            (BCH, 8, 30)]
BYTE_CODES = sorted(set(REF_CODES.values()) | set(EXTREMES))


def frames_for(rng, o, B):
    """B received words: random codewords (the first two: the all-zero message and the message made of the largest
    symbol) with 0 .. t + 3 symbol errors, every count at least once when B allows"""
    hi = 2 if o.family == BCH else 1 << o.q
    msg = rng.integers(0, hi, (B, o.l))
    msg[0], msg[1] = 0, hi - 1
    cw = o.encode(msg.astype(np.uint16))
    rx = cw.copy()
    for f in range(B):
        ne = min(o.n, f % (o.t + 4) if f < 2 * (o.t + 4) else int(rng.integers(0, o.t + 4)))
        for p in rng.choice(o.n, ne, replace=False):
            rx[f, p] ^= 1 if o.family == BCH else int(rng.integers(1, hi))
    return msg, cw, rx


def erasure_frames(rng, o, cw):
    """rho erasures and e errors up to and one past 2 e + rho = 2 t; every fifth frame more than 2 t erasures; erased
    symbols carry anything, the sent symbol included"""
    hi = 2 if o.family == BCH else 1 << o.q
    rx, per = cw.copy(), []
    for f in range(cw.shape[0]):
        if f % 5 == 4:
            rho, e = min(o.n, 2 * o.t + 1 + f % 3), f % 2
        else:
            rho = int(rng.integers(0, min(2 * o.t, o.n) + 1))
            room = (2 * o.t - rho) // 2
            e = int(rng.integers(0, room + 1)) if f % 4 else room + 1
        e = min(e, o.n - rho)
        pos = rng.choice(o.n, rho + e, replace=False)
        for p in pos[:rho]:
            rx[f, p] = int(rng.integers(0, hi)) if f % 3 else cw[f, p]
        for p in pos[rho:]:
            rx[f, p] ^= 1 if o.family == BCH else int(rng.integers(1, hi))
        per.append(sorted(int(p) for p in pos[:rho]))
    return rx, per


def same_constants(w, o):
    assert (w.n, w.k, w.l, w.dmin, w.t) == (o.n, o.k, o.l, o.dmin, o.t)
    for name in ("g", "h", "roots"):
        assert np.array_equal(getattr(w, name), getattr(o, name)), name
    assert np.array_equal(w.exp[: 2 * o.n], o.exp[: 2 * o.n]) and np.array_equal(w.log[: o.n + 1], o.log[: o.n + 1])
    for _, _, name in ALGS:
        assert w.to_string(name) == o.to_string(name)


def same_decoding(w, o, rng, B):
    """encode, extract, syndromes, the three locators and correct_hard of the two builds on the same frames"""
    msg, cw, rx = frames_for(rng, w, B)
    assert np.array_equal(o.encode(msg.astype(np.uint8)), cw)
    assert np.array_equal(w.extract(rx), o.extract(rx.astype(np.uint8)))
    for f in range(B):
        S = w.syndromes(rx[f])
        assert np.array_equal(S, o.syndromes(rx[f].astype(np.uint8)))
        if S.any():
            for alg, _, _ in ALGS:
                a, b = w.locator(alg, S), o.locator(alg, S.astype(np.uint8))
                assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], (alg, f)
    classes = set()
    for alg, _, _ in ALGS:
        a, b = w.correct_hard(alg, rx, raw=True), o.correct_hard(alg, rx.astype(np.uint8))
        for x, y in zip(a, b):
            assert np.array_equal(x, y), alg
        classes |= set(a[2].tolist())
    rxe, per = erasure_frames(rng, w, cw)
    for alg in (BM, EUKLID) + ((PGZ,) if w.family == BCH else ()):
        a = w.correct_hard(alg, rxe, per, raw=True)
        for f in range(B):
            b = o.correct_hard(alg, rxe[f].astype(np.uint8), per[f])
            for x, y in zip(a, b):
                assert np.array_equal(x[f], y[0]), (alg, f, per[f])
        classes |= set(a[2].tolist())
    return classes


@pytest.mark.parametrize("fam,q,t", BYTE_CODES, ids=["%s%d-%d" % ("rs" if f else "bch", q, t) for f, q, t in BYTE_CODES])
def test_agrees_with_the_byte_build(fam, q, t):
    w, o = WideOracle(fam, q, t), Oracle(fam, q, t)
    same_constants(w, o)
    classes = same_decoding(w, o, np.random.default_rng(900 + 100 * q + t), 40 if t > 16 else 60)
    assert 0 in classes and (2 in classes or (q, t) in ((3, 1), (4, 1), (8, 1)))  # (perfect / tiny codes decode anything)


@pytest.mark.parametrize("fam,q,t", [(BCH, 6, 3), (RS, 4, 3), (RS, 8, 16)])
def test_multiplication_coding_agrees_with_the_byte_build(fam, q, t):
    w, o = WideOracle(fam, q, t, coding=1), Oracle(fam, q, t, coding=1)
    rng = np.random.default_rng(q + t)
    msg, cw, rx = frames_for(rng, w, 30)
    assert np.array_equal(o.encode(msg.astype(np.uint8)), cw)
    assert np.array_equal(w.extract(rx), o.extract(rx.astype(np.uint8)))


@pytest.mark.parametrize("q,t,mu,step", M.SETS)
def test_rs_root_conventions_agree_with_the_byte_build(q, t, mu, step):
    """the C code of both builds symbol for symbol (raw: the reference's own behaviour for such codes), and
    WideOracle.correct_hard -- the decode through T, the checker of DESIGN 4.9 -- against the same through the byte
    oracle's (1, 1) code"""
    w, o, o11 = WideOracle(RS, q, t, 0, mu, step), Oracle(RS, q, t, mu, step), Oracle(RS, q, t)
    same_constants(w, o)
    rng = np.random.default_rng(950 + 10 * q + t)
    same_decoding(w, o, rng, 40)
    msg, cw, rx = frames_for(rng, w, 40)
    rxe, per = erasure_frames(rng, w, cw)
    for alg, _, _ in ALGS:
        got = w.correct_hard(alg, rx)
        want = through_oracle(o11, alg, rx.astype(np.uint8), None, o.n, mu, step)
        for x, y in zip(got, want):
            assert np.array_equal(x, y), alg
        ok = (rx != cw).sum(1) <= t
        assert (got[2][ok] == 0).all() and np.array_equal(got[0][ok], cw[ok])
    few = np.array([len(e) <= 2 * t for e in per])
    for alg in (BM, EUKLID):
        got = w.correct_hard(alg, rxe, per)
        want = through_oracle(o11, alg, rxe.astype(np.uint8), per, o.n, mu, step)
        for x, y in zip(got, want):
            assert np.array_equal(x[few], y[few]), alg
        # more than 2t erasures: the device's class for them, the word untouched
        many = ~few & np.array([w.syndromes(r).any() for r in rxe])
        assert many.any() and (got[2][many] == 4).all() and (got[1][many] == -1).all()
        assert np.array_equal(got[0][many], rxe[many])


def test_non_default_polynomial_of_gf256():
    """GF(2^8) over 0x12B: against the library's host construction, and a decode that returns the sent words"""
    w, std = WideOracle(RS, 8, 4, 0x12B), WideOracle(RS, 8, 4)
    assert w.poly == 0x12B and std.poly == 0x11D and not np.array_equal(w.g, std.g)
    code = cc.rs(8, cc.errors(4), cc.berlekamp_massey_tag(), modular_polynomial=0x12B, device=capi.DEVICE_NONE)
    assert (code.n, code.k, code.l, code.dmin) == (w.n, w.k, w.l, w.dmin)
    assert np.array_equal(code.g, w.g) and np.array_equal(code.h, w.h) and np.array_equal(code.roots, w.roots)
    assert code.to_string() == w.to_string("BM")
    rng = np.random.default_rng(12)
    msg, cw, rx = frames_for(rng, w, 40)
    for alg, _, _ in ALGS:
        out, nerr, st, ub = w.correct_hard(alg, rx)
        ok = (rx != cw).sum(1) <= 4
        assert (st[ok] == 0).all() and np.array_equal(out[ok], cw[ok]) and np.array_equal(nerr[ok], (rx != cw).sum(1)[ok])
        assert (st[~ok] != 0).any()


def test_polynomials_are_checked_by_counting():
    lib = WideOracle.lib()
    for q, poly in ((9, 0x211), (10, 0x409), (11, 0x805), (12, 0x1053), (13, 0x201B), (14, 0x4443), (15, 0x8003)):
        assert lib.orcw_is_primitive(q, poly) == 1
    # x^10 + 1 (reducible), x^4 + x^3 + x^2 + x + 1 (irreducible, order 5), wrong degree, no constant term
    for q, poly in ((10, 0x401), (4, 0x1F), (10, 0x211), (9, 0x409), (9, 0x212)):
        assert lib.orcw_is_primitive(q, poly) == 0
        with pytest.raises(ValueError):
            WideOracle(RS, q, 2, poly)
    with pytest.raises(ValueError):
        WideOracle(RS, 9, 2)  # no default beyond q = 8 (galois.h:57-67)


# ---- tests/golden/wide.npz: the real reference's vectors ----
def wide_oracle_for(wid):
    fam, q, t, poly = [int(v) for v in GOLD["w%d_params" % wid][:4]]
    return WideOracle(fam, q, t, poly)


@pytest.mark.parametrize("wid", [0, 1])
def test_wide_golden_constants_and_encode(wid):
    p = "w%d_" % wid
    o = wide_oracle_for(wid)
    assert [o.n, o.k, o.l, o.dmin] == [int(v) for v in GOLD[p + "params"][4:]]
    assert np.array_equal(o.g, GOLD[p + "g"]) and np.array_equal(o.h, GOLD[p + "h"])
    assert np.array_equal(o.roots, GOLD[p + "roots"])
    assert [o.to_string(name) for _, _, name in ALGS] == list(GOLD[p + "names"])
    assert np.array_equal(o.encode(GOLD[p + "msg"]), GOLD[p + "cw"])
    assert np.array_equal(o.extract(GOLD[p + "cw"]), GOLD[p + "msg"])


def fenced(alg, r_st, ub, r_st_euklid):
    """frames on which the reference's own answer is not the algorithm's: "not solvable" out of rs::error_values (Q9b,
    status 2), F3 under BM (ref_ub), PGZ's elimination (Q9a: PGZ and Euklid disagree on success)"""
    skip = r_st == 2
    if alg == BM:
        skip = skip | ub.astype(bool)
    if alg == PGZ:
        skip = skip | ((r_st == 0) != (r_st_euklid == 0))
    return skip


@pytest.mark.parametrize("wid", [0, 1])
def test_wide_golden_hard_decode(wid):
    p = "w%d_" % wid
    o = wide_oracle_for(wid)
    rx, cw = GOLD[p + "rx"], GOLD[p + "cw"]
    true_nerr = (rx != cw).sum(1)
    for alg, key, name in ALGS:
        out, nerr, st, ub = o.correct_hard(alg, rx)
        r_st, r_out = GOLD[p + key + "_status"], GOLD[p + key + "_out"]
        keep = ~fenced(alg, r_st, ub, GOLD[p + "euklid_status"])
        assert keep.sum() >= 0.8 * len(keep)
        if alg == BM:  # an exception other than decoding_failure (array::at, status 3) is F3: the oracle flags it
            assert ub[r_st == 3].all()
        assert np.array_equal((st == 0)[keep], (r_st == 0)[keep]), name
        ok = keep & (st == 0)
        assert np.array_equal(out[ok], r_out[ok]) and np.array_equal(nerr[ok], (r_out != rx).sum(1)[ok]), name
        assert np.array_equal(o.extract(out[ok]), GOLD[p + key + "_msg"][ok])
        easy = keep & (true_nerr <= o.t)
        assert (st[easy] == 0).all() and np.array_equal(out[easy], cw[easy])
        assert (r_st[keep & (st != 0)] == 1).all()  # decoding_failure


@pytest.mark.parametrize("wid,key", [(0, "bm"), (0, "euklid"), (0, "pgz"), (1, "bm"), (1, "euklid")])
def test_wide_golden_erasures(wid, key):
    p = "w%d_" % wid
    o = wide_oracle_for(wid)
    alg = {"pgz": PGZ, "bm": BM, "euklid": EUKLID}[key]
    rxe, off, er = GOLD[p + "rxe"], GOLD[p + "er_off"], GOLD[p + "er"]
    per = [er[off[f]:off[f + 1]].tolist() for f in range(rxe.shape[0])]
    out, nerr, st, ub = o.correct_hard(alg, rxe, per, raw=True)
    r_st, r_out = GOLD[p + key + "_e_status"], GOLD[p + key + "_e_out"]
    keep = ~fenced(alg, r_st, ub, r_st) & (r_st != 3)
    assert keep.sum() >= 0.6 * len(keep)
    assert np.array_equal((st == 0)[keep], (r_st == 0)[keep])
    ok = keep & (st == 0)
    assert ok.sum() >= 8 and np.array_equal(out[ok], r_out[ok])
    if alg == PGZ:
        many = np.array([len(e) > 2 * o.t for e in per])
        assert (st[many] == 4).all() and (r_st[many] == 1).all()  # bch.h:105-107


# ---- the real reference, where oracle/_ref carries the wide driver ----
@pytest.mark.parametrize("wid", sorted(RefWide.CODES))
def test_against_the_real_reference(wid):
    if not RefWide.available():
        pytest.skip("oracle/_ref is not built here, or predates the wide section")
    r = RefWide(wid)
    fam, q, t, poly = RefWide.CODES[wid]
    o = WideOracle(fam, q, t, poly)
    assert (o.n, o.k, o.l, o.t, o.dmin) == (r.n, r.k, r.l, r.t, r.dmin)
    assert np.array_equal(o.g, r.poly(0)) and np.array_equal(o.h, r.poly(1)) and np.array_equal(o.roots, r.poly(2))
    rng = np.random.default_rng(5000 + wid)
    msg, cw, rx = frames_for(rng, o, 80)
    assert np.array_equal(r.encode(msg), cw)
    ref = {alg: r.correct(alg, rx) for alg, _, _ in ALGS}
    for alg, _, name in ALGS:
        out, nerr, st, ub = o.correct_hard(alg, rx)
        r_out, r_st, r_msg = ref[alg]
        keep = ~fenced(alg, r_st, ub, ref[EUKLID][1])
        assert keep.sum() >= 0.8 * len(keep), name
        assert np.array_equal((st == 0)[keep], (r_st == 0)[keep]), name
        ok = keep & (st == 0)
        assert np.array_equal(out[ok], r_out[ok]), name
        for f in np.nonzero(keep & (st != 0))[0]:
            assert r_st[f] == 1, r_msg[f]
            if alg != PGZ:  # failure class: root count (2) against re-check (3)
                assert st[f] == (3 if "not a codeword" in r_msg[f] else 2), (name, f, r_msg[f])
    rxe, per = erasure_frames(rng, o, cw)
    for alg in (BM, EUKLID) + ((PGZ,) if fam == BCH else ()):
        out, nerr, st, ub = o.correct_hard(alg, rxe, per, raw=True)
        r_out, r_st, r_msg = r.correct(alg, rxe, per)
        keep = ~fenced(alg, r_st, ub, r_st) & (r_st != 3)
        # beyond 2t erasures the reference's BM / Euklid have no defined answer: not compared
        if alg != PGZ:
            keep &= np.array([len(e) <= 2 * t for e in per])
        assert keep.sum() >= 0.5 * len(keep)
        assert np.array_equal((st == 0)[keep], (r_st == 0)[keep]), alg
        ok = keep & (st == 0)
        assert np.array_equal(out[ok], r_out[ok]), alg


# ---- host construction of the library for every 16-bit field ----
WIDE_FIELDS = [(9, 0x211), (10, 0x409), (11, 0x805), (12, 0x1053), (13, 0x201B), (14, 0x4443), (15, 0x8003)]


@pytest.mark.parametrize("q,poly", WIDE_FIELDS)
def test_host_construction_equals_the_model(q, poly):
    tags = ((cc.peterson_gorenstein_zierler_tag, "PGZ"), (cc.berlekamp_massey_tag, "BM"), (cc.euklid_tag, "EUKLID"))
    for fam, t in ((BCH, 2 + q % 5), (RS, 3 + q % 6)):
        o = WideOracle(fam, q, t, poly)
        mk = cc.primitive_bch if fam == BCH else cc.rs
        for tag, name in tags:
            code = mk(q, cc.errors(t), tag(), modular_polynomial=poly, device=capi.DEVICE_NONE)
            assert (code.n, code.k, code.l, code.dmin) == (o.n, o.k, o.l, o.dmin)
            assert code.to_string() == o.to_string(name)
        assert np.array_equal(code.g, o.g) and np.array_equal(code.h, o.h) and np.array_equal(code.roots, o.roots)
    if q != 10:
        return
    kp4 = WideOracle(RS, 10, 15, 0x409, 0, 1)  # KP4 RS(544,514)'s mother code: first root alpha^0
    code = cc.rs(10, cc.errors(15), cc.berlekamp_massey_tag(), mu=0, step=1, modular_polynomial=0x409,
                 device=capi.DEVICE_NONE)
    assert np.array_equal(code.g, kp4.g) and np.array_equal(code.roots, kp4.roots) and code.dmin == kp4.dmin
