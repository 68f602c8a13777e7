"""CPU-side checks of iterated hard-decision decoding of product codes (cc_product_decode_hard) on
CC_DEVICE_NONE handles: the symbols are declared, bound and exported; every refusal in the order the header states; the
model of tests/product_hard_model.py against brute force on BCH(7,4)^2 and eBCH(8,4)^2; the fixed point; product_code's
TypeErrors and ValueErrors; product_hard_simulation's log name, ladder and sharding over a stub; the benchmark's options;
and what the batches of tests/test_gpu_product_hard.py are chosen for, decoded by the model alone: CASES, TRIPS (later
blocks of a workgroup) and LONG (many half-iterations).

What the batches are chosen for, and where a condition cannot hold (test_model_batches_are_not_degenerate):
- a block that converges to a wrong block needs miscorrections that agree along rows and columns: the 15 x 15 batch has
  one at its error rate, the longer codes do not in a handful of blocks;
- a t = 1 full-length component is perfect: every line has an inner candidate, so "no candidate" never happens in the
  plain 15 x 15 rows, and blocks that fail to converge there end in a cycle rather than in stuck lines;
- a candidate that the parity rule rejects is asserted for every extended case; a line rejected for a root at a position
  >= n for the shortened case alone."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi, montecarlo
import product_hard_model as PH
from shortened_model import Shortened

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_product_decode_hard", "cc_product_decode_hard_dev", "cc_mc_run_product_hard_dev")
HALVES = 8

# name: rows (q, t, N or None), cols, extended, BSC flip probability chosen with the model, blocks, seed.  The GPU tests
# decode the same batches on the device (tests/test_gpu_product_hard.py says what each shape is there for).
CASES = {
    "15_11x15_7": ((4, 1, None), (4, 2, None), False, 0.06, 67, 7),
    "e16_11xe32_26": ((4, 1, None), (5, 1, None), True, 0.04, 64, 7),
    "s40_22x15_7": ((6, 3, 40), (4, 2, None), False, 0.05, 32, 7),
    "63_45x63_45": ((6, 3, None), (6, 3, None), False, 0.04, 32, 7),
    "e64_51xe64_51": ((6, 2, None), (6, 2, None), True, 0.035, 32, 7),
    "127_113x15_11": ((7, 2, None), (4, 1, None), False, 0.02, 16, 7),
    "e256_239xe8_4": ((8, 2, None), (3, 1, None), True, 0.006, 16, 7),
    "e8_4xe256_239": ((3, 1, None), (8, 2, None), True, 0.006, 16, 7),
    "255_239x255_239": ((8, 2, None), (8, 2, None), False, 0.008, 2, 7),
    "e256_239xe256_239": ((8, 2, None), (8, 2, None), True, 0.008, 2, 7),
    "e256_239xe256_239_noisy": ((8, 2, None), (8, 2, None), True, 0.012, 2, 8),
    "255_131x15_11": ((8, 16, None), (4, 1, None), False, 0.045, 8, 7),
    "255_131x255_239": ((8, 16, None), (8, 2, None), False, 0.055, 1, 7),
}


def encode_blocks(rows, cols, info, extended):
    """rows encoded (and extended), then all columns encoded (and extended): (B, w2, w1)"""
    B = info.shape[0]
    e = 1 if extended else 0
    ext = (lambda w: np.concatenate([w, (w.sum(axis=1, keepdims=True) & 1).astype(np.uint8)], axis=1)) if extended else (lambda w: w)
    wide = ext(np.asarray(rows.encode(info.reshape(-1, rows.l)), np.uint8)).reshape(B, cols.l, rows.n + e)
    tall = ext(np.asarray(cols.encode(PH.turn(wide).reshape(-1, cols.l)), np.uint8))
    return PH.turn(tall.reshape(B, rows.n + e, cols.n + e))


@functools.lru_cache(maxsize=None)
def case(name):
    """model decoders, the blocks sent, the received blocks, the model's steps x_1 .. x_8 and their trace, made once"""
    (rq, rt, rn), (cq, ct, cn), extended, p, blocks, seed = CASES[name]
    rows, cols = PH.decoder(rq, rt, rn), PH.decoder(cq, ct, cn)
    rng = np.random.default_rng(seed)
    sent = encode_blocks(rows, cols, rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8), extended)
    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)
    trace = []
    xs = PH.steps(rows, cols, z, HALVES, extended, trace)
    for a in [sent, z] + xs:
        a.setflags(write=False)
    return rows, cols, extended, sent, z, xs, trace


def model_outputs(name, halves, blocks=slice(None)):
    rows, cols, extended, sent, z, xs, _ = case(name)
    return PH.outputs(rows, cols, z[blocks], [x[blocks] for x in xs], halves, extended)


# ---- batches past the first trip of a workgroup (tests/test_gpu_product_hard.py decodes them on the device) ----
# name: rows (q, t), cols (q, t), flips in 256 of the BSC chosen with the model, blocks the largest grid holds per compute
# unit (8 workgroups of one block, or of four wavefronts with a block each)
TRIPS = {
    "127_113x7_4": ((7, 2), (3, 1), 7, 8),     # 7 x 127: two wavefronts of the workgroup have no line in either pass
    "7_4x127_113": ((3, 1), (7, 2), 7, 8),     # 127 x 7: its turn, the second wavefront one lane short in the row pass
    "63_45x63_45": ((6, 3), (6, 3), 14, 32),   # a wavefront per block at full width, t = 3
}
TRIP_HALVES = 5


def trips_batch(name, cus):
    """2 * capacity + 77 blocks for a device of `cus` compute units, so that every workgroup (wavefront) of the largest
    grid decodes a second and a third block in the LDS the first left behind, and the model's outputs and trace on a picked
    subset: a prefix, a stretch around an odd cut past the capacity, the suffix"""
    (rq, rt), (cq, ct), flips, per_cu = TRIPS[name]
    rows, cols = PH.decoder(rq, rt), PH.decoder(cq, ct)
    cap = per_cu * cus
    B = 2 * cap + 77
    rng = np.random.default_rng(77)
    few = encode_blocks(rows, cols, rng.integers(0, 2, (256, cols.l, rows.l)).astype(np.uint8), False)
    z = few[rng.integers(0, 256, B)]
    z ^= rng.integers(0, 256, z.shape, dtype=np.uint8) < flips
    cut = (cap + cap // 3) | 1
    pick = np.unique(np.concatenate([np.arange(50), np.arange(cut - 25, cut + 25), np.arange(B - 50, B)]))
    trace = []
    xs = PH.steps(rows, cols, z[pick], TRIP_HALVES, False, trace)
    want = PH.outputs(rows, cols, z[pick], xs, TRIP_HALVES, False)
    return dict(rows=rows, cols=cols, z=z, cap=cap, cut=cut, pick=pick, want=want, trace=trace)


def trips_batch_is_not_degenerate(name, batch):
    """among the picked blocks that are no workgroup's first: `last` takes three values, both statuses occur, and where a
    component can be without a candidate (t = 3: 16 % of the syndromes are decodable) a line is"""
    late = batch["pick"] >= batch["cap"]
    want = batch["want"]
    lasts, statuses = set(want["last"][late].tolist()), set(want["status"][late].tolist())
    stuck = sum(int((~tr["cand"].reshape(late.size, -1)[late]).sum()) for tr in batch["trace"])
    print(name, "blocks", batch["z"].shape[0], "picked", late.size, "past the first trip", int(late.sum()), "last",
          sorted(lasts), "not converged", int((want["status"][late] != PH.FRAME_OK).sum()), "lines without a candidate", stuck)
    assert late.sum() >= 100 and late.size <= 150
    assert len(lasts) >= 3, lasts
    assert statuses == {PH.FRAME_OK, PH.FRAME_NOT_CONVERGED}, statuses
    if name == "63_45x63_45":
        assert stuck > 0


# ---- many half-iterations: `last` beyond the 8 of CASES, at and around the last slot of the Monte-Carlo histogram ----
LONG = ((4, 1), 0.06, 64, 7)  # BCH(15,11)^2, plain: (q, t) of both sides, BSC flip probability, blocks, seed
LONG_HALVES = (56, 57, 60)


@functools.lru_cache(maxsize=None)
def long_case():
    """the decoder, the received blocks and the model's steps x_1 .. x_60, made once"""
    (q, t), p, blocks, seed = LONG
    dec = PH.decoder(q, t)
    rng = np.random.default_rng(seed)
    sent = encode_blocks(dec, dec, rng.integers(0, 2, (blocks, dec.l, dec.l)).astype(np.uint8), False)
    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)
    xs = PH.steps(dec, dec, z, max(LONG_HALVES), False)
    for a in [z] + xs:
        a.setflags(write=False)
    return dec, z, xs


def long_outputs(halves):
    dec, z, xs = long_case()
    return PH.outputs(dec, dec, z, xs, halves, False)


def bch(q, t, **kw):
    return cc.primitive_bch(q, cc.errors(t), BM(), **dict(NONE, **kw))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert C.sizeof(capi.Product) == 2 * C.sizeof(C.c_void_p) + 4 + 4 + 4 + 4 + 2 * C.sizeof(C.c_void_p)
    assert callable(montecarlo.ProductHardBackend) and callable(montecarlo.product_hard_simulation)
    for name in ("correct_hard_batch", "decode_hard_batch"):
        assert callable(getattr(cc.product_code, name))


class Call:
    """one cc_product_decode_hard(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, rows, cols, extended=False, halves=4, B=2):
        self.pc = cc.product_code(rows, cols, extended)
        # p = 99 and no schedule: the hard-decision calls do not look at either
        self.desc = capi.Product(rows._h, cols._h, int(bool(extended)), 99, halves, None, None)
        self.B, N = B, self.pc.n
        self.inp, self.out = np.zeros(B * N, np.uint8), np.zeros(B * N, np.uint8)
        self.nflip, self.last, self.status = (np.zeros(B, np.int32) for _ in range(3))

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), inp=vp(self.inp), out=vp(self.out), nflip=vp(self.nflip), last=vp(self.last),
                 status=vp(self.status), B=self.B)
        a.update(replace)
        lib = capi.lib()
        if dev:
            return lib.cc_product_decode_hard_dev(a["desc"], a["inp"], a["out"], a["nflip"], a["last"], a["status"], a["B"], None)
        return lib.cc_product_decode_hard(a["desc"], a["inp"], a["out"], a["nflip"], a["last"], a["status"], a["B"])


def test_refusals_and_their_order():
    lib = capi.lib()
    rows, cols = bch(4, 1), bch(4, 2)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
    good = Call(rows, cols)
    counters = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    run = lambda desc, c: lib.cc_mc_run_product_hard_dev(desc, 3.0, 1, 0, 16, 1, vp(c), None)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check: p = 99 and NULL alpha / beta do not matter, the three
        # per-block outputs may be NULL, out == in is allowed
        assert good(dev) == capi.ERR_NO_DEVICE
        assert good(dev, nflip=None, last=None, status=None) == capi.ERR_NO_DEVICE
        assert good(dev, out=vp(good.inp)) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        bad = Call(rs, ms, halves=0)
        for call in (good, bad):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("inp", "out"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        for field in ("rows", "cols"):
            c = Call(rs, ms, halves=0)
            setattr(c.desc, field, None)
            assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. no half-iteration: before the handles are looked at
        assert Call(rs, ms, halves=0)(dev) == capi.ERR_INVALID_ARGUMENT
        # 3. what the Chase call refuses at p = 0 for rows, then for cols, before the buffers are looked at
        for r, c_, text in ((rs, ms, "Reed-Solomon"), (ms, rs, "min-sum"), (rows, rs, "Reed-Solomon"), (rows, ms, "min-sum"),
                            (bch(8, 17), ms, "2t <= 32"), (rows, bch(8, 17), "2t <= 32")):
            c = Call(r, c_)
            assert c(dev, out=vp(c.inp[1:])) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
        c = Call(rows, cols)
        c.desc.cols = matrix._h
        assert c(dev, out=vp(c.inp[1:])) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in lib.cc_last_error().decode()
        c = Call(rows, cols)
        c.desc.rows = matrix._h
        c.desc.cols = rs._h
        assert c(dev) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in lib.cc_last_error().decode()
        # 5. out overlapping in other than out == in, by any byte
        c = Call(rows, cols)
        N = c.pc.n
        whole = np.zeros(3 * c.B * N, np.uint8)
        for out in (whole[1:], whole[c.B * N - 1:]):
            assert c(dev, inp=vp(whole), out=vp(out)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, inp=vp(whole[1:]), out=vp(whole)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, inp=vp(whole), out=vp(whole[c.B * N:])) == capi.ERR_NO_DEVICE  # adjacent is not overlapping
        # B = 0 answers after these checks: the device check is one of them
        assert good(dev, B=0, inp=None, out=None) == capi.ERR_NO_DEVICE
        assert Call(rs, cols)(dev, B=0, inp=None, out=None) == capi.ERR_UNSUPPORTED
        assert Call(rows, cols, halves=0)(dev, B=0, inp=None, out=None) == capi.ERR_INVALID_ARGUMENT
    # a value that is no bit is looked at only once a device is there: the device check comes first
    c = Call(rows, cols)
    c.inp[5] = 2
    assert c(False) == capi.ERR_NO_DEVICE
    # the Monte-Carlo call: NULL pc / counters first, then the same order
    assert run(C.byref(good.desc), counters) == capi.ERR_NO_DEVICE
    worst = Call(rs, ms, halves=0)
    assert run(None, counters) == capi.ERR_INVALID_ARGUMENT and run(C.byref(worst.desc), None) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), counters) == capi.ERR_INVALID_ARGUMENT
    worst.desc.halves = 3
    assert run(C.byref(worst.desc), counters) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in lib.cc_last_error().decode()
    assert not counters.any()


# ---- the model against brute force ----
def nearest_word_rule(words, t, lines):
    """per line the nearest of `words` if it is within t, else the line: bounded-distance decoding by enumeration"""
    d = (lines[:, None, :] != words[None, :, :]).sum(axis=2)
    best = d.argmin(axis=1)
    hit = d[np.arange(lines.shape[0]), best] <= t
    return np.where(hit[:, None], words[best], lines)


@pytest.mark.parametrize("extended", [False, True], ids=["7_4", "e8_4"])
def test_model_against_brute_force(extended):
    dec = PH.decoder(3, 1)
    msgs = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    words = np.asarray(dec.encode(msgs), np.uint8)
    if extended:
        words = np.concatenate([words, (words.sum(axis=1, keepdims=True) & 1).astype(np.uint8)], axis=1)
    assert min(int((a != b).sum()) for i, a in enumerate(words) for b in words[:i]) == (4 if extended else 3)
    w = 8 if extended else 7
    rng = np.random.default_rng(21)
    sent = encode_blocks(dec, dec, rng.integers(0, 2, (300, 4, 4)).astype(np.uint8), extended)
    z = sent ^ (rng.random(sent.shape) < 0.08).astype(np.uint8)
    z[0] = 0
    z[1] = sent[1]
    xs = PH.steps(dec, dec, z, 6, extended)
    x = z
    lasts = np.zeros(300, np.int32)
    for h in range(6):
        if h % 2 == 0:
            new = nearest_word_rule(words, 1, x.reshape(-1, w)).reshape(300, w, w)
        else:
            new = PH.turn(nearest_word_rule(words, 1, PH.turn(x).reshape(-1, w)).reshape(300, w, w))
        lasts[(new != x).any(axis=(1, 2))] = h + 1
        x = new
        assert np.array_equal(xs[h], x), h
    got = PH.outputs(dec, dec, z, xs, 6, extended)
    assert np.array_equal(got["last"], lasts) and np.array_equal(got["nflip"], (x != z).sum(axis=(1, 2)))
    in_code = lambda lines: (lines[:, None, :] == words[None, :, :]).all(axis=2).any(axis=1)
    ok = in_code(x.reshape(-1, w)).reshape(300, w).all(axis=1) & in_code(PH.turn(x).reshape(-1, w)).reshape(300, w).all(axis=1)
    assert np.array_equal(got["status"] == PH.FRAME_OK, ok)
    assert ok.any() and not ok.all() and len(set(lasts.tolist())) >= 3
    assert got["last"][0] == 0 == got["nflip"][0] and got["status"][0] == PH.FRAME_OK  # the zero block
    assert got["last"][1] == 0 == got["nflip"][1] and got["status"][1] == PH.FRAME_OK  # a code block


@pytest.mark.parametrize("name", ["15_11x15_7", "e16_11xe32_26", "s40_22x15_7"])
def test_after_the_last_change_and_one_more_pass_nothing_changes(name):
    """the fixed point the device may stop at: two successive passes without a change.  `last` + 1 quiet passes make no
    fixed point yet (the pass after a quiet one can change the block again); two do, whatever follows."""
    rows, cols, extended, sent, z, xs, _ = case(name)
    long = PH.steps(rows, cols, z, 14, extended)
    chain = [z] + long
    quiet = [~(chain[h + 1] != chain[h]).any(axis=(1, 2)) for h in range(14)]
    seen = 0
    for h in range(1, 13):
        fixed = quiet[h - 1] & quiet[h]
        seen += int(fixed.sum())
        for later in range(h + 1, 14):
            assert quiet[later][fixed].all(), (name, h, later)
    assert seen > 0
    # in the call's terms: a block whose `last` after 8 half-iterations leaves two quiet passes is what 14 give
    last = PH.outputs(rows, cols, z, long, HALVES, extended)["last"]
    settled = last + 2 <= HALVES
    assert settled.any() and np.array_equal(chain[HALVES][settled], chain[14][settled])
    assert np.array_equal(PH.outputs(rows, cols, z, long, 14, extended)["last"][settled], last[settled])


# ---- the Python layer ----
def test_product_code_type_and_value_errors():
    pc = cc.product_code(bch(4, 1), bch(3, 1))
    z = np.zeros((2, 7, 15), np.uint8)
    for call in (pc.correct_hard_batch, pc.decode_hard_batch):
        with pytest.raises(cc.CcError) as e:
            call(z, 4)
        assert e.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(cc.CcError) as e:
            call(np.zeros((2, 15, 7), np.uint8), 4)
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(cc.CcError) as e:
            call(np.zeros((7, 15), np.uint8), 4)
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="uint8"):
            call(np.zeros((2, 7, 15), np.float32), 4)
        for halves in (0, -1):
            with pytest.raises(ValueError):
                call(z, halves)
    with pytest.raises(ValueError):
        montecarlo.product_hard_simulation(pc, 0, backend=object())
    # the existing methods are as they were
    with pytest.raises(TypeError, match="float32"):
        pc.correct_batch(z, 2, (0.0,), (0.5,))


class StubBackend:
    """counts what it is asked for: one block error in a hundred, three half-iterations and a half per block"""

    def __init__(self):
        self.calls = []

    def run(self, point, seed, first, blocks):
        self.calls.append((point, seed, first, blocks))
        c = np.zeros(capi.MC_NCOUNTERS, np.int64)
        c[capi.MC_FRAMES], c[capi.MC_WORD_ERRORS], c[capi.MC_BIT_ERRORS] = blocks, blocks // 100, blocks // 50
        c[capi.MC_ITER_SUM] = 7 * blocks // 2
        return c


def test_simulation_log_name_ladder_and_sharding(tmp_path, monkeypatch):
    pc = cc.product_code(bch(6, 3), bch(6, 3), extended=True)
    stub = StubBackend()
    sim = montecarlo.product_hard_simulation(pc, 6, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    start, _ = montecarlo.ladder(pc.rate, 0.5)
    soft = montecarlo.product_simulation(pc, 4, (0.0,), (0.5,), backend=StubBackend())
    assert sim.start == start == soft.start and sim.points() == soft.points()
    res = sim()
    path = tmp_path / "(63, 45, 7)-BMx(63, 45, 7)-BM-ext-hard-h6.log"
    assert path.exists()
    assert len(res) == len(sim.points()) == len(stub.calls)
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["ber"] == 20 / (1000 * 4096)
    assert res[0]["mean_last"] == 3.5
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["ebno", "wer", "mean_last"] and len(lines) == 1 + len(res)
    first = lines[1].split()
    assert float(first[0]) == start and float(first[1]) == 0.01 and float(first[2]) == 3.5
    assert [c[2] for c in stub.calls[:3]] == [0, 1 << 40, 2 << 40] and all(c[1] == 0 for c in stub.calls)
    with pytest.raises(RuntimeError, match="already exists"):
        sim()

    class Dist:
        def get_rank(self):
            return 1

        def get_world_size(self):
            return 3

        def all_reduce(self, counters, op=None):
            pass

        class ReduceOp:
            SUM = None

    stub2 = StubBackend()
    sim2 = montecarlo.product_hard_simulation(pc, 6, backend=stub2)
    monkeypatch.setattr(sim2, "_dist", lambda: Dist())
    sim2.run_point(3.0, 1000, 2)
    lo, count = montecarlo.shard(1000, 1, 3)
    assert stub2.calls == [(3.0, 0, (2 << 40) + lo, count)]


def test_benchmark_options():
    assert "--halves" in benchmark.usage_text()
    base = ["--simulation", "product", "--k", "6", "--dmin", "7"]
    assert benchmark.main(base) == 1  # neither a schedule nor --halves
    assert benchmark.main(base + ["--halves", "0"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--alpha", "0,0.3"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--beta", "0.2"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--alpha", "0", "--beta", "0.2"]) == 1
    assert benchmark.main(["--simulation", "product", "--halves", "4"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--cols-dmin", "4"]) == 1

    def parsed(extra):
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("--simulation")
        for name in ("--k", "--dmin"):
            ap.add_argument(name, action="append")
        for name in ("--cols-k", "--cols-dmin", "--chase", "--halves"):
            ap.add_argument(name, type=int, default=None)
        ap.add_argument("--alpha")
        ap.add_argument("--beta")
        return benchmark.product_hard_arguments(ap.parse_args(base + extra))

    assert parsed(["--halves", "6"]) == ((6, 7), (6, 7), 6)
    assert parsed(["--halves", "1", "--cols-k", "4", "--cols-dmin", "3"]) == ((6, 7), (4, 3), 1)
    assert isinstance(parsed(["--halves", "6", "--alpha", "0"]), str)


# ---- what the GPU batches hold ----
def test_model_batches_are_not_degenerate():
    right = stuck = wrong = 0
    lasts = set()
    miscorrected = False
    for name in sorted(CASES):
        rows, cols, extended, sent, z, xs, trace = case(name)
        got = PH.outputs(rows, cols, z, xs, HALVES, extended)
        B = z.shape[0]
        ok = got["status"] == PH.FRAME_OK
        correct = (got["out"] == sent).all(axis=(1, 2))
        print(name, "blocks", B, "converged", int(ok.sum()), "right", int(correct.sum()), "converged wrong",
              int((ok & ~correct).sum()), "last", sorted(set(got["last"].tolist())), "nflip", int(got["nflip"].min()), "..",
              int(got["nflip"].max()))
        assert (z != sent).any(axis=(1, 2)).all() or name.startswith("e256_239xe8") or name.startswith("e8_4"), name
        assert got["last"].max() >= 2 and got["nflip"].max() > 0, name
        right, stuck, wrong = right + int(correct.sum()), stuck + int((~ok).sum()), wrong + int((ok & ~correct).sum())
        lasts |= set(got["last"].tolist())
        # a line changed to a word other than the one sent
        w2, w1 = z.shape[1:]
        for h, tr in enumerate(trace):
            s = (PH.turn(sent) if tr["column"] else sent).reshape(tr["after"].shape)
            changed = (tr["after"] != tr["before"]).any(axis=1)
            miscorrected = miscorrected or bool((changed & (tr["after"] != s).any(axis=1)).any())
        if extended:
            assert any((tr["cand"] & ~tr["take"]).any() for tr in trace), name
        if isinstance(rows, Shortened):
            assert any(PH.rejected_for_a_virtual_root(rows, tr["before"]).any() for tr in trace if not tr["column"]), name
    assert right > 0 and stuck > 0 and wrong > 0, (right, stuck, wrong)
    assert len(lasts) >= 3 and min(lasts) < HALVES and HALVES in lasts, lasts
    assert miscorrected
    # the two ends of the full block: everything converges at p = 0.008, nothing at 0.012
    assert (model_outputs("e256_239xe256_239", HALVES)["status"] == PH.FRAME_OK).all()
    assert (model_outputs("e256_239xe256_239_noisy", HALVES)["status"] != PH.FRAME_OK).all()


@pytest.mark.parametrize("name", sorted(TRIPS))
def test_trip_batches_are_not_degenerate(name):
    """at the 256 compute units of an MI355X; the GPU test asserts the same at the count of the device it runs on"""
    trips_batch_is_not_degenerate(name, trips_batch(name, 256))


def test_long_batch_cycles_to_the_last_half_iteration_and_settles_early():
    """BCH(15,11)^2 at p = 0.06: blocks that never settle change in every pass up to the last, whichever it is, and are
    not converged; others reach a fixed point within a few passes.  56, 57 and 60 half-iterations lie on both sides of
    the clamp of the Monte-Carlo histogram (slot 55) and end on a row and on a column pass."""
    for halves in LONG_HALVES:
        got = long_outputs(halves)
        cycling = got["last"] == halves
        early = (got["last"] >= 2) & (got["last"] <= 8) & (got["status"] == PH.FRAME_OK)
        print(halves, "half-iterations: last == halves in", int(cycling.sum()), "blocks, settled with 2 <= last <= 8 in",
              int(early.sum()), "of", got["last"].size)
        assert cycling.sum() >= 5 and early.sum() >= 5
        assert (got["status"][cycling] == PH.FRAME_NOT_CONVERGED).all()
