"""The 16-bit symbol route (csrc/wide.hip through the _u16 entry points, q = 9 .. 15) against an independent model:
checkers.WideOracle, the 16-bit build of the plain-C oracle, pinned on the CPU by tests/test_wide_oracle.py.

The comparison is the rule of test_gpu_algebraic.check_against_oracle: the set of decoded frames equals the model's, out
and nerr are equal on those, nerr = -1 and out = the received word on the others, and under the BM tag the failure class
is equal frame for frame.  Shortened codes: shortened_model.Shortened over the WideOracle, with native_status as the only
licence for a differing class.

Every parametrised case first checks its own frames on the model's output alone (`shares`): at least a quarter decode
with nerr > 0 and at least a tenth fail.  The classes the BM tag shows are collected per suite and checked at the end of
the module (`test_status_classes_of_every_suite`).
"""
import collections
import ctypes as C

import numpy as np
import pytest

import shortened_model as S
from checkers import BCH, BM, EUKLID, PGZ, RS, WideOracle

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.codes import _erasure_csr

pytestmark = pytest.mark.gpu

TAGS = {PGZ: cc.peterson_gorenstein_zierler_tag, BM: cc.berlekamp_massey_tag, EUKLID: cc.euklid_tag}
POLY = {9: 0x211, 10: 0x409, 11: 0x805, 12: 0x1053, 13: 0x201B, 14: 0x4443, 15: 0x8003}
LOCATOR, RECHECK, ERASURES = capi.FRAME_LOCATOR, 3, 4
SEEN = collections.defaultdict(lambda: {"cases": set(), "classes": collections.Counter()})


def make(fam, q, t, alg, N=None, mu=1, step=1):
    cls = cc.primitive_bch if fam == BCH else cc.rs
    kw = dict(mu=mu, step=step) if fam == RS else {}
    return cls(q, cc.errors(t), TAGS[alg](), modular_polynomial=POLY[q], n=N, **kw)


def hi_of(o):
    return 2 if o.family == BCH else 1 << o.q


def codewords(rng, o, B):
    """random codewords; the first two carry the all-zero message and the message made of the symbol 2^q - 1"""
    msg = rng.integers(0, hi_of(o), (B, o.l)).astype(np.uint16)
    msg[0] = 0
    if B > 1:
        msg[1] = (1 << o.q) - 1
    return o.encode(msg)


def corrupt(rng, o, cw, counts):
    rx = cw.copy()
    for f, ne in enumerate(counts):
        for p in rng.choice(o.n, min(int(ne), o.n), replace=False):
            rx[f, p] ^= 1 if o.family == BCH else int(rng.integers(1, hi_of(o)))
    return rx


def error_counts(rng, t, B):
    """0 .. t + 3 errors, weighted towards t and t + 1"""
    base = [t, t + 1, t, t + 1, max(t - 1, 0), t + 2, 0, t + 3, 1, t, t + 1, t // 2]
    return [base[f % len(base)] for f in range(B)]


def shares(suite, case, alg, nerr, st):
    """the condition on the model's own output, before the device is asked; records the BM classes of the suite"""
    nerr, st = np.asarray(nerr), np.asarray(st)
    assert ((st == 0) & (nerr > 0)).mean() >= 0.25, (suite, case, "decoded with nerr > 0", ((st == 0) & (nerr > 0)).mean())
    assert (st != 0).mean() >= 0.10, (suite, case, "failed", (st != 0).mean())
    SEEN[suite]["cases"].add(case)
    if alg == BM:
        SEEN[suite]["classes"].update(st.tolist())


def compare(res, model, rx, alg, shortened=False):
    out, nerr, st = model[:3]
    got_out, got_nerr, got_st = (np.asarray(res[k]) for k in ("out", "nerr", "status"))
    assert np.array_equal(got_st == 0, st == 0), np.nonzero((got_st == 0) != (st == 0))[0][:8]
    ok = st == 0
    assert np.array_equal(got_out[ok], out[ok])
    assert np.array_equal(got_nerr[ok], nerr[ok])
    assert (got_nerr[~ok] == -1).all()
    assert np.array_equal(got_out[~ok], rx[~ok])
    if alg == BM:
        assert np.array_equal(got_st, S.native_status(st, got_st) if shortened else st), (got_st[~ok][:8], st[~ok][:8])


def on_device(code, rx, per=None):
    import torch
    res = code.correct_batch(torch.from_numpy(np.ascontiguousarray(rx).view(np.int16)).cuda(), erasures=per)
    return {"out": res["out"].cpu().numpy().view(np.uint16), "nerr": res["nerr"].cpu().numpy(),
            "status": res["status"].cpu().numpy()}


def same(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("out", "nerr", "status"))


# ---- every field, full length ----
FIELD_CODES = [(BCH, 9, 5), (RS, 9, 8), (BCH, 10, 3), (RS, 10, 6), (BCH, 11, 4), (RS, 11, 2), (BCH, 12, 8), (RS, 12, 5),
               (BCH, 13, 2), (RS, 13, 7), (BCH, 14, 6), (RS, 14, 3), (BCH, 15, 7), (RS, 15, 4)]


@pytest.mark.parametrize("alg", [PGZ, BM, EUKLID])
@pytest.mark.parametrize("fam,q,t", FIELD_CODES, ids=["%s%d-%d" % ("rs" if f else "bch", q, t) for f, q, t in FIELD_CODES])
def test_every_field(fam, q, t, alg):
    """RECHECK is not reached here: without erasures a locator whose root count equals its degree gives, with Forney's
    values (or ones, BCH), a word that passes the re-check in every seeded frame."""
    o = WideOracle(fam, q, t, POLY[q])
    rng = np.random.default_rng(1000 * q + 10 * t + fam)
    B = 48 if q <= 12 else 16
    cw = codewords(rng, o, B)
    rx = corrupt(rng, o, cw, error_counts(rng, t, B))
    model = o.correct_hard(alg, rx)
    shares("every_field", (fam, q, t, alg), alg, model[1], model[2])
    code = make(fam, q, t, alg)
    assert (code.n, code.k, code.dmin) == (o.n, o.k, o.dmin)
    assert np.array_equal(code.encode_batch(o.extract(cw)), cw)
    compare(code.correct_batch(rx), model, rx, alg)
    within = (rx != cw).sum(1) <= t
    assert (model[2][within] == 0).all() and np.array_equal(model[0][within], cw[within])


@pytest.mark.parametrize("alg", [PGZ, BM, EUKLID])
def test_single_error_code(alg):
    """RS(511,509), t = 1: deg = 1, mtop = 1 in Forney's denominator.  At full length nearly every two-error word lands
    on another codeword (any S_2 / S_1 names a position), so the failing share is steered: every fourth frame carries
    two errors with e_2 = e_1 X_1 / X_2, i.e. S_1 = 0, which no single error explains (CC_FRAME_LOCATOR).  RECHECK is
    unreachable: one root, one value, two syndromes matched exactly."""
    o = WideOracle(RS, 9, 1, POLY[9])
    rng = np.random.default_rng(91)
    B = 48
    cw = codewords(rng, o, B)
    rx = corrupt(rng, o, cw, [(0, 1, 1, 2, 1, 3)[f % 6] for f in range(B)])
    for f in range(3, B, 4):
        p1, p2 = (int(p) for p in rng.choice(o.n, 2, replace=False))
        e1 = int(rng.integers(1, 512))
        e2 = int(o.exp[(int(o.log[e1]) + p1 - p2) % o.n])
        rx[f] = cw[f]
        rx[f, p1] ^= e1
        rx[f, p2] ^= e2
    model = o.correct_hard(alg, rx)
    shares("single_error", alg, alg, model[1], model[2])
    assert (model[2][3::4] == LOCATOR).all()
    compare(make(RS, 9, 1, alg).correct_batch(rx), model, rx, alg)


# ---- lane limits: RS over GF(2^10) ----
@pytest.mark.parametrize("alg,t", [(EUKLID, 31), (BM, 32), (PGZ, 32)])
def test_lane_limits(alg, t):
    """exactly t - 1, t and t + 1 random errors, four frames each.  RECHECK: not reached (t + 1 errors leave a locator
    whose root count differs from its degree)."""
    o = WideOracle(RS, 10, t, POLY[10])
    rng = np.random.default_rng(3200 + t + alg)
    cw = codewords(rng, o, 12)
    rx = corrupt(rng, o, cw, [t - 1, t, t + 1] * 4)
    model = o.correct_hard(alg, rx)
    shares("lane_limits", (alg, t), alg, model[1], model[2])
    assert model[1].tolist()[:2] == [t - 1, t] and model[2][2] != 0
    compare(make(RS, 10, t, alg).correct_batch(rx), model, rx, alg)


def erasure_mix(rng, o, cw, rhos, t):
    """for every rho: rho erasures plus floor((2t - rho) / 2) errors, and one error more than that, two frames each"""
    plan = [(rho, (2 * t - rho) // 2 + extra) for rho in rhos for extra in (0, 1)] * 2
    rx, per = cw[: len(plan)].copy(), []
    for f, (rho, e) in enumerate(plan):
        pos = rng.choice(o.n, rho + e, replace=False)
        for p in pos[:rho]:  # (BCH: the erased bit is wrong, every sixth frame anything -- see the erasure suite)
            rx[f, p] = int(rng.integers(0, hi_of(o))) if o.family == RS or f % 6 == 5 else rx[f, p] ^ 1
        for p in pos[rho:]:
            rx[f, p] ^= 1 if o.family == BCH else int(rng.integers(1, hi_of(o)))
        per.append(sorted(int(p) for p in pos[:rho]))
    return rx, per


@pytest.mark.parametrize("alg,t,rhos", [(BM, 31, (0, 1, 61, 62)), (EUKLID, 16, (0, 1, 16, 31, 32))])
def test_lane_limits_with_erasures(alg, t, rhos):
    """the erasure pre-load at the largest t the kernel takes with erasures.  (Euklid with an odd number of erasures:
    the reference's integer stop rule (2t + rho) / 2 decodes some frames one beyond the capability, to an answer of its
    own -- model and device follow it alike.)"""
    o = WideOracle(RS, 10, t, POLY[10])
    rng = np.random.default_rng(3300 + t)
    cw = codewords(rng, o, 4 * len(rhos))
    rx, per = erasure_mix(rng, o, cw, rhos, t)
    model = o.correct_hard(alg, rx, per)
    shares("lane_limits_erasures", (alg, t), alg, model[1], model[2])
    code = make(RS, 10, t, alg)
    res = code.correct_batch(rx, erasures=per)
    compare(res, model, rx, alg)
    assert same(res, on_device(code, rx, per))


def test_above_the_lane_limits_is_refused():
    for alg, t in ((BM, 32), (EUKLID, 17)):
        code = make(RS, 10, t, alg)
        rx = np.zeros((2, code.n), np.uint16)
        with pytest.raises(cc.CcError) as e:
            code.correct_batch(rx, erasures=[[1], [2, 3]])
        assert e.value.status == capi.ERR_UNSUPPORTED


@pytest.mark.parametrize("alg", [PGZ, BM, EUKLID])
def test_bch_with_many_roots(alg):
    """BCH(1023, t = 10): 20 syndromes, deg >> q, error values all ones.  RECHECK: not reached without erasures."""
    o = WideOracle(BCH, 10, 10, POLY[10])
    rng = np.random.default_rng(1010 + alg)
    cw = codewords(rng, o, 36)
    rx = corrupt(rng, o, cw, error_counts(rng, 10, 36))
    model = o.correct_hard(alg, rx)
    shares("bch_many_roots", alg, alg, model[1], model[2])
    compare(make(BCH, 10, 10, alg).correct_batch(rx), model, rx, alg)


# ---- erasures on several fields ----
ERASURE_CODES = [(BCH, 9, 4), (RS, 9, 3), (BCH, 11, 3), (RS, 11, 5), (BCH, 13, 3), (RS, 13, 4)]


def erasure_cases(rng, o, cw):
    """the mixes of erasure_mix for rho = 0 .. 2t, then the edges: erased positions 0 and n - 1; erasures on a clean word;
    more than 2t erasures on a clean and on a corrupted word; an erased position whose received symbol is the sent one"""
    t, n, hi = o.t, o.n, hi_of(o)
    rx, per = erasure_mix(rng, o, cw, (1, 2, t, 2 * t - 1, 2 * t), t)
    edge = len(per)
    extra = cw[edge: edge + 8].copy()
    flip = lambda f, p: extra.__setitem__((f, p), extra[f, p] ^ (1 if o.family == BCH else int(rng.integers(1, hi))))
    lists = []
    flip(0, 0), flip(0, n - 1), flip(0, 7)          # erasures at both ends, both wrong, and one error
    lists.append([0, n - 1])
    lists.append(sorted(rng.choice(n, t, replace=False).tolist()))  # clean word, t erasures
    lists.append([5])                                # clean word, one erasure
    lists.append(sorted(rng.choice(n, 2 * t + 1, replace=False).tolist()))  # clean word, more than 2t erasures
    many = sorted(rng.choice(n, 2 * t + 2, replace=False).tolist())  # corrupted word, more than 2t erasures
    flip(4, many[0]), flip(4, many[1])
    lists.append(many)
    flip(5, 100), flip(5, 200)                       # position 300 is erased but carries the sent symbol
    lists.append([100, 300])
    flip(6, n - 1)                                   # erasure and error at the last position only
    lists.append([n - 1])
    flip(7, 0), flip(7, 1), flip(7, 2)               # position 0 erased and wrong, two errors next to it
    lists.append([0])
    return np.concatenate([rx, extra]), per + lists


@pytest.mark.parametrize("alg", [BM, EUKLID, PGZ])
@pytest.mark.parametrize("fam,q,t", ERASURE_CODES, ids=["%s%d-%d" % ("rs" if f else "bch", q, t) for f, q, t in ERASURE_CODES])
def test_erasures_on_several_fields(fam, q, t, alg):
    """BCH: the reference takes error values of one at every locator root (bch.h:80-83), erased positions included, so an
    erased position that carries the sent symbol is flipped and the frame fails the re-check: CC_FRAME_RECHECK is
    reached on the BCH codes.  More than 2t erasures on a word with a non-zero syndrome: CC_FRAME_ERASURES."""
    if fam == RS and alg == PGZ:
        code = make(fam, q, t, alg)
        with pytest.raises(cc.CcError) as e:  # hard_decision.h:66-68
            code.correct_batch(np.zeros((1, code.n), np.uint16), erasures=[[1]])
        assert e.value.status == capi.ERR_UNSUPPORTED
        return
    o = WideOracle(fam, q, t, POLY[q])
    rng = np.random.default_rng(4000 + 100 * q + 10 * t + alg)
    cw = codewords(rng, o, 40)
    rx, per = erasure_cases(rng, o, cw)
    model = o.correct_hard(alg, rx, per)
    shares("erasures", (fam, q, t, alg), alg, model[1], model[2])
    B = len(per)
    # more than 2t erasures: on a clean word nothing to do -- but the two-trial rule refuses first (bch.h:105-107)
    assert model[2][B - 8 + 3] == (ERASURES if alg == PGZ else 0) and model[2][B - 8 + 4] == ERASURES
    code = make(fam, q, t, alg)
    res = code.correct_batch(rx, erasures=per)
    compare(res, model, rx, alg)
    assert same(res, on_device(code, rx, per))
    # nerr and status may be NULL: the word alone comes back
    er, off = _erasure_csr(per, B, code.n)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros_like(rx)
    assert capi.lib().cc_correct_hard_batch_u16(code._h, P(rx), P(er), P(off), P(out), None, None, B) == 0
    assert np.array_equal(out, res["out"])


@pytest.mark.parametrize("q", [9, 8])
def test_pgz_trials_ignore_positions_outside_the_frame(q):
    """A device erasure list is not read on the host, so positions >= n reach the two-trial rule (bch.h:97-149) as they
    are: force_erasures_kernel skips them.  BCH, t = 2, shortened to n = 100, PGZ tag, 8 frames with 0 .. 3 valid
    positions each plus the entries n, n + 5 and 65535: words, nerr and status equal those of the call without the three.
    q = 9: cc_correct_hard_batch_u16_dev; q = 8: the byte route, cc_correct_hard_batch_dev -- one kernel serves both."""
    import torch
    n, B = 100, 8
    kw = dict(modular_polynomial=POLY[9]) if q == 9 else {}
    code = cc.primitive_bch(q, cc.errors(2), cc.peterson_gorenstein_zierler_tag(), n=n, **kw)
    assert code.n == n
    rng = np.random.default_rng(9100 + q)
    dt = np.uint16 if q == 9 else np.uint8
    rx = np.asarray(code.encode_batch(rng.integers(0, 2, (B, code.l)).astype(dt))).astype(dt)
    valid = []
    for f in range(B):
        pos = rng.choice(n, f % 4 + 1, replace=False)  # the erased positions, then one plain error
        valid.append(sorted(int(p) for p in pos[: f % 4]))
        for p in pos:
            rx[f, p] ^= 1
    valid[1] = [n - 1]
    d_rx = torch.from_numpy(rx.view(np.int16) if q == 9 else rx).cuda()
    entry = getattr(capi.lib(), "cc_correct_hard_batch_u16_dev" if q == 9 else "cc_correct_hard_batch_dev")
    P = lambda t: C.c_void_p(t.data_ptr())

    def run(per):
        er = torch.from_numpy(np.array([p for l in per for p in l], np.uint16).view(np.int16)).cuda()
        off = torch.from_numpy(np.cumsum([0] + [len(l) for l in per]).astype(np.uint32).view(np.int32)).cuda()
        # guard words around the output: nothing outside the B * n symbols may change
        out = torch.full((B + 2, n), 0x55, dtype=d_rx.dtype, device="cuda")
        nerr, st = (torch.full((B,), 99, dtype=torch.int32, device="cuda") for _ in range(2))
        capi.check(entry(code._h, P(d_rx), P(er), P(off), P(out[1]), P(nerr), P(st), B, None), "correct")
        torch.cuda.synchronize()
        assert (out[0] == 0x55).all() and (out[B + 1] == 0x55).all()
        return out[1: B + 1].cpu().numpy(), nerr.cpu().numpy(), st.cpu().numpy()

    want = run(valid)
    assert (want[2] == 0).sum() >= B // 2 and (want[1] > 0).any()  # the lists matter: frames decode through the trials
    for order in (lambda l: l + [n, n + 5, 65535], lambda l: [65535, n] + l + [n + 5]):
        got = run([order(l) for l in valid])
        for g, w in zip(got, want):
            assert np.array_equal(g, w)


# ---- launch geometry ----
def test_launch_geometry():
    """RS(511,503), BM: B = 1, 3, 4, 5, 63 (four waves per workgroup, one scratch each) and more frames than the grid
    has waves (num_cus * 8 workgroups of 4: the grid-stride loop); host and device pointers.  Every frame against the
    model, through a pool of 251 distinct frames."""
    import torch
    o = WideOracle(RS, 9, 4, POLY[9])
    rng = np.random.default_rng(9400)
    cw = codewords(rng, o, 251)
    pool = corrupt(rng, o, cw, error_counts(rng, 4, 251))
    per_pool = [sorted(rng.choice(o.n, f % 4, replace=False).tolist()) for f in range(251)]
    model = o.correct_hard(BM, pool)
    model_e = o.correct_hard(BM, pool, per_pool)
    shares("geometry", 0, BM, model[1], model[2])
    shares("geometry", 1, BM, model_e[1], model_e[2])
    code = make(RS, 9, 4, BM)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (1, 3, 4, 5, 63, cus * 32 + 5):
        idx = (np.arange(B) * 7 + B) % 251
        rx = pool[idx]
        res = code.correct_batch(rx)
        compare(res, tuple(a[idx] for a in model), rx, BM)
        assert same(res, on_device(code, rx))
        per = [per_pool[i] for i in idx]
        res = code.correct_batch(rx, erasures=per)
        compare(res, tuple(a[idx] for a in model_e), rx, BM)
        assert same(res, on_device(code, rx, per))


# ---- root conventions: wide_correct_kernel<true> ----
# (RS with the PGZ tag takes no erasures, hard_decision.h:66-68: refused, see test_erasures_on_several_fields)
@pytest.mark.parametrize("alg,with_erasures", [(BM, False), (BM, True), (EUKLID, False), (EUKLID, True), (PGZ, False)])
@pytest.mark.parametrize("t,mu,step,N", [(15, 0, 1, 544), (15, 0, 1, None), (6, 5, 2, None)])
def test_root_conventions(t, mu, step, N, alg, with_erasures):
    """GF(2^10): KP4 RS(544,514) (first root alpha^0) shortened and at full length, and roots alpha^(5 + 2i)"""
    full = WideOracle(RS, 10, t, POLY[10], mu, step)
    o = S.Shortened(full, N) if N else full
    rng = np.random.default_rng(5000 + 10 * t + mu + (N or 0) + alg)
    B = 36
    msg = rng.integers(0, 1024, (B, o.l)).astype(np.uint16)
    msg[0], msg[1] = 0, 1023
    cw = o.encode(msg)
    if with_erasures:
        rx, per = erasure_mix(rng, o, cw, (1, 2, t, 2 * t - 1, 2 * t), t)
    else:
        rx, per = corrupt(rng, o, cw, error_counts(rng, t, B)), None
    model = o.correct_hard(alg, rx, per)
    shares("root_conventions", (t, mu, step, N, alg, with_erasures), alg, model[1], model[2])
    code = make(RS, 10, t, alg, N, mu, step)
    assert np.array_equal(code.encode_batch(msg[: len(rx)]), cw[: len(rx)])
    res = code.correct_batch(rx, erasures=per)
    compare(res, model, rx, alg, shortened=N is not None)
    assert same(res, on_device(code, rx, per))


# ---- shortened 16-bit codes ----
SHORT = [(BCH, 10, 3, N) for N in (31, 127, 128, 129)] + [(RS, 9, 4, N) for N in (9, 191, 192, 193)]


@pytest.mark.parametrize("alg", [BM, EUKLID, PGZ])
@pytest.mark.parametrize("fam,q,t,N", SHORT, ids=["%s%d-%d-%d" % ("rs" if f else "bch", q, t, N) for f, q, t, N in SHORT])
def test_shortened(fam, q, t, N, alg):
    """N = k + 1 and around a multiple of the wavefront; every sixth frame is a virtual_frame (the padded decode corrects
    a position the shortened code does not have)"""
    m = S.Shortened(WideOracle(fam, q, t, POLY[q]), N)
    rng = np.random.default_rng(6000 + N + alg)
    B = 36
    hi = hi_of(m)
    msg = rng.integers(0, hi, (B, m.l)).astype(np.uint16)
    msg[0], msg[1] = 0, hi - 1
    cw = m.encode(msg)
    rx = cw.copy()
    counts = error_counts(rng, t, B)
    for f in range(B):
        if f % 6 == 5:
            rx[f] = S.virtual_frame(m, N + int(rng.integers(0, m.m.n - N)), int(rng.integers(1, hi)))
            continue
        for p in rng.choice(N, min(counts[f], N), replace=False):
            rx[f, p] ^= 1 if fam == BCH else int(rng.integers(1, hi))
    model = m.correct_hard(alg, rx, None)
    shares("shortened", (fam, q, t, N, alg), alg, model[1], model[2])
    code = make(fam, q, t, alg, N)
    assert np.array_equal(code.encode_batch(msg), cw) and np.array_equal(code.extract_batch(rx), m.extract(rx))
    compare(code.correct_batch(rx), model, rx, alg, shortened=True)
    if fam == RS and alg == PGZ:
        return
    per = [sorted(rng.choice(N, int(rng.integers(0, min(N, 2 * t + 2))), replace=False).tolist()) for f in range(B)]
    model = m.correct_hard(alg, rx, per)
    compare(code.correct_batch(rx, erasures=per), model, rx, alg, shortened=True)


# ---- encoder ----
# k = 63 | 64 | 65 | 126, 130 (no 16-bit code has k = 128 or 129 within t <= 32: k = 2t for RS, a multiple of q for these
# BCH codes) | 319
ENCODE = [(BCH, 9, 7, 63), (RS, 10, 32, 64), (BCH, 13, 5, 65), (BCH, 9, 14, 126), (BCH, 10, 13, 130), (BCH, 11, 29, 319)]


@pytest.mark.parametrize("fam,q,t,k", ENCODE, ids=["k%d" % c[3] for c in ENCODE])
def test_encoder_chunks(fam, q, t, k):
    """wide_encode_kernel updates its feedback register in 64-stage chunks, top down: k on both sides of 64 and of 128 and
    five chunks.  B = 5 and B = 260 through a pool of 20 distinct messages."""
    import torch
    o = WideOracle(fam, q, t, POLY[q])
    assert o.k == k
    code = make(fam, q, t, BM)
    rng = np.random.default_rng(7000 + k)
    top = (1 << q) - 1
    pool = rng.integers(0, hi_of(o), (20, o.l)).astype(np.uint16)
    pool[0], pool[1] = 0, top
    pool[2, ::2], pool[3, 1::3] = top, 0
    want = o.encode(pool)
    noisy = want ^ rng.integers(0, hi_of(o), want.shape).astype(np.uint16)
    for B in (5, 260):
        idx = (np.arange(B) * 3) % 20
        cw = code.encode_batch(pool[idx])
        assert np.array_equal(cw, want[idx])
        dev = code.encode_batch(torch.from_numpy(pool[idx].view(np.int16)).cuda()).cpu().numpy().view(np.uint16)
        assert np.array_equal(dev, want[idx])
        assert np.array_equal(code.extract_batch(noisy[idx]), o.extract(noisy[idx]))


# ---- what the suites showed ----
EXPECT = {  # suite: (parametrised cases, CC_FRAME_RECHECK reached by the model under BM)
    "every_field": (len(FIELD_CODES) * 3, False), "single_error": (3, False), "lane_limits": (3, False),
    "lane_limits_erasures": (2, False), "bch_many_roots": (3, False), "erasures": (len(ERASURE_CODES) * 3 - 3, True),
    "geometry": (2, False), "root_conventions": (15, False), "shortened": (len(SHORT) * 3, False),
}


def test_status_classes_of_every_suite():
    """under the BM tag every suite that ran in full shows CC_FRAME_LOCATOR, and CC_FRAME_RECHECK where the model reaches
    it within the seeded frames (EXPECT; each suite's docstring says why not where it does not)"""
    for suite, (cases, recheck) in EXPECT.items():
        seen = SEEN[suite]
        if len(seen["cases"]) < cases:
            continue  # (a partial run, -k)
        print(suite, dict(seen["classes"]))
        assert seen["classes"][LOCATOR] > 0, suite
        assert (seen["classes"][RECHECK] > 0) == recheck, (suite, dict(seen["classes"]))
