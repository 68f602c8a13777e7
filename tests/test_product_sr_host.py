"""CPU-side checks of iBDD with scaled reliability of product codes (cc_product_decode_sr) on CC_DEVICE_NONE
handles: the symbols are declared, bound and exported; every refusal in the order the header states, with its text;
product_code's argument checks; the benchmark's --weights option; product_sr_simulation's log name, ladder and sharding
over a stub; what the batches of tests/test_gpu_product_sr.py hold, decoded by tests/product_sr_model.py alone; and the
gain over plain iBDD on eBCH(64,51)^2 at 4.0 dB."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi, montecarlo
import product_hard_model as PH
import product_sr_model as SR
from test_product_hard_host import StubBackend, encode_blocks

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_product_decode_sr", "cc_product_decode_sr_dev", "cc_mc_run_product_sr_dev")
INF = math.inf
RISING = (0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 2.0, INF)

# the schedules every GPU case runs (tests/test_gpu_product_sr.py)
SCHEDULES = {
    "rising": RISING,
    "constant": (1.0,) * 6,
    "nonmonotone": (1.2, 0.4, 1.2, 0.4, INF, INF),
    "late": (0.0, 0.0, INF, INF),
    "single": (0.8,),
    "odd": (0.6, 1.0, 1.4, 2.0, INF),
    "fifteen": tuple(0.25 + 0.125 * i for i in range(14)) + (INF,),
}

# name: rows (q, t, N or None), cols, extended, Eb/N0 chosen with the model so that the batch is mixed, blocks, seed
CASES = {
    "15_7x15_11": ((4, 2, None), (4, 1, None), False, 3.0, 256, 11),         # different t per direction
    "e16_11xe32_26": ((4, 1, None), (5, 1, None), True, 4.0, 256, 11),       # extended, rectangular
    "s40_22x15_7": ((6, 3, 40), (4, 2, None), False, 3.5, 64, 11),           # a locator root at a position >= n
    "63_45x63_45": ((6, 3, None), (6, 3, None), False, 3.5, 128, 11),        # a full wavefront per block, t = 3
    "e64_51xe64_51": ((6, 2, None), (6, 2, None), True, 4.0, 128, 11),       # position n in its own dword
    "127_113x7_4": ((7, 2, None), (3, 1, None), False, 4.5, 32, 11),         # workgroup shape with idle wavefronts
    "7_4x127_113": ((3, 1, None), (7, 2, None), False, 4.5, 32, 11),         # its turn
    "e256_239xe8_4": ((8, 2, None), (3, 1, None), True, 5.0, 16, 11),        # four chunks per line
    "e256_239xe256_239": ((8, 2, None), (8, 2, None), True, 4.7, 2, 11),     # the large layout
    "255_131x15_11": ((8, 16, None), (4, 1, None), False, 5.0, 4, 11),       # 2t = 32 columns of Berlekamp-Massey
}


def noisy(rows, cols, extended, sent, ebno, rng):
    s = SR.sigma(rows, cols, extended, ebno)
    return ((1.0 - 2.0 * sent) + s * rng.standard_normal(sent.shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """model decoders, the blocks sent and the channel values, made once"""
    (rq, rt, rn), (cq, ct, cn), extended, ebno, blocks, seed = CASES[name]
    rows, cols = SR.decoder(rq, rt, rn), SR.decoder(cq, ct, cn)
    rng = np.random.default_rng(seed)
    sent = encode_blocks(rows, cols, rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8), extended)
    y = noisy(rows, cols, extended, sent, ebno, rng)
    sent.setflags(write=False)
    y.setflags(write=False)
    return rows, cols, extended, sent, y


@functools.lru_cache(maxsize=None)
def model_steps(name, schedule):
    rows, cols, extended, sent, y = case(name)
    trace = []
    xs = SR.steps(rows, cols, y, SCHEDULES[schedule], extended, trace)
    for x in xs:
        x.setflags(write=False)
    return xs, trace


def model_outputs(name, schedule, halves=None, blocks=slice(None)):
    rows, cols, extended, sent, y = case(name)
    xs, _ = model_steps(name, schedule)
    halves = len(xs) if halves is None else halves
    return SR.outputs(rows, cols, y[blocks], [x[blocks] for x in xs], halves, extended)


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
    assert "#define CC_PRODUCT_SR_MAX_LEVELS 15" in header and capi.PRODUCT_SR_MAX_LEVELS == 15
    assert callable(montecarlo.ProductSrBackend) and callable(montecarlo.product_sr_simulation)
    for name in ("correct_sr_batch", "decode_sr_batch"):
        assert callable(getattr(cc.product_code, name))
    assert "product_code" in cc.__all__


class Call:
    """one cc_product_decode_sr(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, rows, cols, extended=False, weights=(0.5, 1.0, INF, INF), B=2, halves=None):
        self.pc = cc.product_code(rows, cols, extended)
        self.w = np.array(weights, np.float32)
        # p = 99 and no schedule: the call does not look at either
        self.desc = capi.Product(rows._h, cols._h, int(bool(extended)), 99, len(weights) if halves is None else halves, None, None)
        self.B, N = B, self.pc.n
        self.y, self.out = np.zeros(B * N, np.float32), np.zeros(B * N, np.uint8)
        self.nflip, self.last, self.status = (np.zeros(B, np.int32) for _ in range(3))

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), w=vp(self.w), y=vp(self.y), out=vp(self.out), nflip=vp(self.nflip),
                 last=vp(self.last), status=vp(self.status), B=self.B)
        a.update(replace)
        lib = capi.lib()
        if dev:
            return lib.cc_product_decode_sr_dev(a["desc"], a["w"], a["y"], a["out"], a["nflip"], a["last"], a["status"], a["B"], None)
        return lib.cc_product_decode_sr(a["desc"], a["w"], a["y"], a["out"], a["nflip"], a["last"], a["status"], a["B"])


def test_refusals_and_their_order():
    lib = capi.lib()
    text = lambda: lib.cc_last_error().decode()
    rows, cols = bch(4, 1), bch(4, 2)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
    good = Call(rows, cols)
    nan, neg = np.array([0.5, np.nan, -1.0, 1.0], np.float32), np.array([0.5, 1.0, -1.0, np.nan], np.float32)
    sixteen, fifteen = np.arange(16, dtype=np.float32), np.arange(15, dtype=np.float32)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check; the three per-block outputs may be NULL
        assert good(dev) == capi.ERR_NO_DEVICE
        assert good(dev, nflip=None, last=None, status=None) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        bad = Call(rs, ms, halves=0)
        for call in (good, bad):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("w", "y", "out"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        for field in ("rows", "cols"):
            c = Call(rs, ms, halves=0)
            setattr(c.desc, field, None)
            assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. no half-iteration: before the handles and the weights are looked at
        assert Call(rs, ms, halves=0)(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT
        # 3. what the hard call refuses for rows, then for cols, with its texts, before weights and buffers
        for r, c_, what in ((rs, ms, "Reed-Solomon"), (ms, rs, "min-sum"), (rows, rs, "Reed-Solomon"), (rows, ms, "min-sum"),
                            (bch(8, 17), ms, "2t <= 32"), (rows, bch(8, 17), "2t <= 32")):
            c = Call(r, c_)
            assert c(dev, w=vp(nan), out=vp(c.y.view(np.uint8)[1:])) == capi.ERR_UNSUPPORTED, what
            assert what in text(), what
        c = Call(rows, cols)
        c.desc.cols = matrix._h
        assert c(dev, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in text()
        # 5. the weights, before the overlap: the first bad one is named; -0.0 is not negative; 15 distinct values pass
        c = Call(rows, cols)
        over = vp(c.y.view(np.uint8)[1:])
        assert c(dev, w=vp(nan), out=over) == capi.ERR_INVALID_ARGUMENT and "weights[1] is NaN" in text()
        assert c(dev, w=vp(neg), out=over) == capi.ERR_INVALID_ARGUMENT and "weights[2] is negative" in text()
        assert c(dev, w=vp(np.array([-np.inf] * 4, np.float32))) == capi.ERR_INVALID_ARGUMENT and "weights[0] is negative" in text()
        assert c(dev, w=vp(np.array([-0.0, 0.0, INF, INF], np.float32))) == capi.ERR_NO_DEVICE
        many = Call(rows, cols, weights=sixteen)
        assert many(dev) == capi.ERR_INVALID_ARGUMENT and "more than 15 distinct weights" in text()
        assert Call(rows, cols, weights=fifteen)(dev) == capi.ERR_NO_DEVICE
        assert Call(rows, cols, weights=tuple(fifteen) * 3)(dev) == capi.ERR_NO_DEVICE  # 45 half-iterations, 15 values
        # 6. out overlapping y, by any byte
        N = c.pc.n
        whole = np.zeros(5 * c.B * N + 4, np.uint8)
        fl = lambda a: a[: 4 * c.B * N].view(np.float32)
        for out in (whole[1:], whole[4 * c.B * N - 1:]):
            assert c(dev, y=vp(fl(whole)), out=vp(out)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(fl(whole[4:])), out=vp(whole)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(fl(whole)), out=vp(whole[4 * c.B * N:])) == capi.ERR_NO_DEVICE  # adjacent is not overlapping
        # B = 0 answers after these checks: the device check is one of them
        assert good(dev, B=0, y=None, out=None) == capi.ERR_NO_DEVICE
        assert good(dev, B=0, y=None, out=None, w=vp(nan)) == capi.ERR_INVALID_ARGUMENT
        assert good(dev, B=0, y=None, out=None, w=None) == capi.ERR_INVALID_ARGUMENT
        assert Call(rs, cols)(dev, B=0, y=None, out=None) == capi.ERR_UNSUPPORTED
        assert Call(rows, cols, halves=0)(dev, B=0, y=None, out=None) == capi.ERR_INVALID_ARGUMENT
    # the Monte-Carlo call: NULL pc / weights / counters first, then the same order
    counters = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    run = lambda desc, w, c: lib.cc_mc_run_product_sr_dev(desc, vp(w), 3.0, 1, 0, 16, 1, vp(c), None)
    assert run(C.byref(good.desc), good.w, counters) == capi.ERR_NO_DEVICE
    worst = Call(rs, ms, halves=0)
    assert run(None, good.w, counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), None, counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), nan, None) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), nan, counters) == capi.ERR_INVALID_ARGUMENT
    worst.desc.halves = 4
    assert run(C.byref(worst.desc), nan, counters) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in text()
    assert run(C.byref(good.desc), nan, counters) == capi.ERR_INVALID_ARGUMENT and "weights[1] is NaN" in text()
    assert run(C.byref(Call(rows, cols, weights=sixteen).desc), sixteen, counters) == capi.ERR_INVALID_ARGUMENT
    assert not counters.any()


# ---- the Python layer ----
def test_product_code_type_and_value_errors():
    pc = cc.product_code(bch(4, 1), bch(3, 1))
    y = np.zeros((2, 7, 15), np.float32)
    for call in (pc.correct_sr_batch, pc.decode_sr_batch):
        with pytest.raises(cc.CcError) as e:
            call(y, RISING)
        assert e.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(cc.CcError) as e:
            call(np.zeros((2, 15, 7), np.float32), RISING)
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(cc.CcError) as e:
            call(np.zeros((7, 15), np.float32), RISING)
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="float32"):
            call(np.zeros((2, 7, 15), np.uint8), RISING)
        with pytest.raises(ValueError):
            call(y, ())
        for weights, what in (((0.5, math.nan), "NaN"), ((0.5, -0.25), "negative"), (range(16), "distinct")):
            with pytest.raises(cc.CcError) as e:
                call(y, weights)
            assert e.value.status == capi.ERR_INVALID_ARGUMENT and what in capi.lib().cc_last_error().decode()
    with pytest.raises(ValueError):
        montecarlo.product_sr_simulation(pc, (), backend=object())


def test_simulation_log_name_ladder_and_sharding(tmp_path, monkeypatch):
    pc = cc.product_code(bch(6, 3), bch(6, 3), extended=True)
    stub = StubBackend()
    sim = montecarlo.product_sr_simulation(pc, RISING, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    start, _ = montecarlo.ladder(pc.rate, 0.5)
    hard = montecarlo.product_hard_simulation(pc, 8, backend=StubBackend())
    assert sim.start == start == hard.start and sim.points() == hard.points() and sim.halves == 8
    res = sim()
    path = tmp_path / "(63, 45, 7)-BMx(63, 45, 7)-BM-ext-sr8.log"
    assert path.exists()
    assert len(res) == len(sim.points()) == len(stub.calls)
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["mean_last"] == 3.5
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["ebno", "wer", "mean_last"] and len(lines) == 1 + len(res)
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
    sim2 = montecarlo.product_sr_simulation(pc, RISING, backend=stub2)
    monkeypatch.setattr(sim2, "_dist", lambda: Dist())
    sim2.run_point(3.0, 1000, 2)
    lo, count = montecarlo.shard(1000, 1, 3)
    assert stub2.calls == [(3.0, 0, (2 << 40) + lo, count)]


def test_benchmark_options():
    assert "--weights" in benchmark.usage_text()
    base = ["--simulation", "product", "--k", "6", "--dmin", "7"]
    assert benchmark.main(base + ["--weights", "0.5,x"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,-1"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,nan"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,inf", "--halves", "2"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,inf", "--alpha", "0,0.3"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,inf", "--beta", "0.2,0.2"]) == 1
    assert benchmark.main(["--simulation", "product", "--weights", "0.5,inf"]) == 1
    assert benchmark.main(base + ["--weights", "0.5,inf", "--cols-dmin", "4"]) == 1

    def parsed(extra):
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("--simulation")
        for name in ("--k", "--dmin"):
            ap.add_argument(name, action="append")
        for name in ("--cols-k", "--cols-dmin", "--chase", "--halves"):
            ap.add_argument(name, type=int, default=None)
        for name in ("--alpha", "--beta", "--weights"):
            ap.add_argument(name)
        return benchmark.product_sr_arguments(ap.parse_args(base + extra))

    assert parsed(["--weights", "0.6,1,inf"]) == ((6, 7), (6, 7), [0.6, 1.0, INF])
    assert parsed(["--weights", "0", "--cols-k", "4", "--cols-dmin", "3"]) == ((6, 7), (4, 3), [0.0])
    assert isinstance(parsed(["--weights", "1", "--halves", "6"]), str)


# ---- what the GPU batches hold ----
def test_model_batches_are_not_degenerate():
    right = stuck = reverted = fallback = clean_changed = 0
    for name in sorted(CASES):
        rows, cols, extended, sent, y = case(name)
        for schedule in sorted(SCHEDULES):
            got = model_outputs(name, schedule)
            _, trace = model_steps(name, schedule)
            correct = (got["out"] == sent).all(axis=(1, 2))
            ok = got["status"] == SR.FRAME_OK
            rv, fb, cl = (sum(t[k] for t in trace) for k in ("reverted", "fallback", "clean_changed"))
            print(name, schedule, "blocks", y.shape[0], "right", int(correct.sum()), "not converged", int((~ok).sum()), "last",
                  sorted(set(got["last"].tolist())), "reverted", rv, "fallback lines", fb, "clean lines changed", cl)
            right, stuck = right + int(correct.sum()), stuck + int((~ok).sum())
            reverted, fallback = reverted + rv, fallback + fb
            if schedule == "nonmonotone":
                clean_changed += cl
            if schedule == "late":
                assert ((got["last"] >= 3) | (got["last"] == 0)).all() and (got["last"] != 0).any(), name
        rising = model_outputs(name, "rising")
        assert (SR.hard(y) != sent).any() and rising["nflip"].max() > 0, name
        if name not in ("e256_239xe256_239", "255_131x15_11"):  # two and four blocks
            assert ((rising["out"] == sent).all(axis=(1, 2))).any() and (rising["out"] != sent).any(), name
    assert right > 0 and stuck > 0 and reverted > 0 and fallback > 0 and clean_changed > 0


def test_special_values_follow_the_comparisons():
    """-0.0 decides as 0, a NaN decides as 0 and is never weak, +-inf is weak under no weight, and |y| equal to the
    weight is strong: a candidate's flip there reverts"""
    dec = SR.decoder(4, 1)
    y = np.ones((1, 15, 15), np.float32)
    y[0, 0, 3] = -1.0     # one error in row 0: the candidate flips it
    y[0, 1, 4] = -0.5     # the same, at exactly the weight: reverted
    y[0, 2, 5] = -0.25    # weak: corrected
    y[0, 3, 0], y[0, 3, 1], y[0, 3, 2], y[0, 3, 6] = -0.0, np.nan, np.inf, -np.inf
    z = SR.hard(y)
    assert z[0, 3].tolist() == [0, 0, 0, 0, 0, 0, 1] + [0] * 8
    x1 = SR.steps(dec, dec, y, (0.5,), False)[0]
    assert x1[0, 0, 3] == 1 and x1[0, 1, 4] == 1 and x1[0, 2, 5] == 0 and x1[0, 3, 6] == 1
    xinf = SR.steps(dec, dec, y, (INF,), False)[0]
    assert xinf[0, 0, 3] == 0 and xinf[0, 1, 4] == 0 and xinf[0, 3, 6] == 1  # -inf is not below inf


def test_the_gain_over_plain_ibdd():
    """eBCH(64,51)^2 at 4.0 dB, 512 all-zero blocks: fewer than half as many wrong blocks as iBDD at 8 half-iterations
    (measured: 16 against 115)"""
    dec = SR.decoder(6, 2)
    rng = np.random.default_rng(1)
    s = SR.sigma(dec, dec, True, 4.0)
    y = (1 + s * rng.standard_normal((512, 64, 64))).astype(np.float32)
    sr = int(SR.decode(dec, dec, y, RISING, True)["out"].any(axis=(1, 2)).sum())
    hard = int(PH.decode(dec, dec, SR.hard(y), 8, True)["out"].any(axis=(1, 2)).sum())
    print("wrong blocks: iBDD-SR", sr, "iBDD", hard)
    assert hard > 0 and 2 * sr < hard
