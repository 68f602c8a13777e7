"""CPU-side checks of the product-code calls on CC_DEVICE_NONE handles: the symbols are declared, bound and
exported; every refusal of cc_product_decode(_dev) and its relatives in the order the header states; product_code's
attributes, shapes and TypeErrors; cc_product_sigma against the formula; product_simulation's ladder, log name and
sharding over a stub backend; the benchmark's options; what the ragged-tile batches of tests/test_gpu_product.py are chosen
for, decoded by the model alone."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi, montecarlo
from channelcoding_amd.montecarlo import product_simulation

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_product_decode", "cc_product_decode_dev", "cc_product_encode_batch", "cc_product_encode_batch_dev",
         "cc_product_extract_batch", "cc_product_extract_batch_dev", "cc_awgn_product_dev", "cc_mc_run_product_dev")


def bch(q, t, **kw):
    return cc.primitive_bch(q, cc.errors(t), BM(), **dict(NONE, **kw))


def vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Call:
    """one cc_product_decode(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, rows, cols, extended=False, p=2, alpha=(0.0, 0.5), beta=(0.2, 0.4), B=2):
        self.pc = cc.product_code(rows, cols, extended)
        self.desc = self.pc._pc(p, alpha, beta)
        N = self.pc.n
        self.B = B
        self.y = np.ones(B * N, np.float32)
        self.out = np.zeros(B * N, np.uint8)
        self.ext = np.zeros(B * N, np.float32)
        self.status = np.zeros(B * max(self.pc.n1, self.pc.n2), np.int32)

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), y=vp(self.y), out=vp(self.out), ext=vp(self.ext), status=vp(self.status))
        a.update(replace)
        lib = capi.lib()
        if dev:
            return lib.cc_product_decode_dev(a["desc"], a["y"], a["out"], a["ext"], a["status"], self.B, None)
        return lib.cc_product_decode(a["desc"], a["y"], a["out"], a["ext"], a["status"], self.B)


def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    assert re.search(r"\bdouble cc_product_sigma\(", header) and "cc_product_sigma" in capi.exported_symbols()
    assert "typedef struct cc_product {" in header
    # the struct the binding passes is the header's: two pointers, int, two uint32, two pointers
    assert C.sizeof(capi.Product) == 2 * C.sizeof(C.c_void_p) + 4 + 4 + 4 + 4 + 2 * C.sizeof(C.c_void_p)
    for name in ("product_code", "product_decode"):
        assert name in cc.__all__ and callable(getattr(cc, name))
    assert callable(montecarlo.ProductBackend) and callable(product_simulation)


def test_refusals_and_their_order():
    lib = capi.lib()
    rows, cols = bch(4, 1), bch(4, 2)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    good = Call(rows, cols)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check, with and without ext
        assert good(dev) == capi.ERR_NO_DEVICE and good(dev, ext=None) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        bad = Call(rs, ms, p=99, alpha=(float("inf"),), beta=(-1.0,))
        bad.desc.halves = 0
        for call in (good, bad):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("y", "out", "status"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        for field in ("rows", "cols"):
            c = Call(rows, cols)
            setattr(c.desc, field, None)
            assert c(dev) == capi.ERR_INVALID_ARGUMENT
        for field in ("alpha", "beta"):
            c = Call(rs, cols, p=99)
            setattr(c.desc, field, C.POINTER(C.c_float)())
            assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. no half-iteration: before the handles are looked at
        c = Call(rs, ms, p=99)
        c.desc.halves = 0
        assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 3. what the Chase call refuses for rows, then for cols, before the schedule and the buffers are looked at
        nan = dict(alpha=(float("nan"), 0.0), beta=(-1.0, 0.0))
        for r, c_, p, text in ((rs, ms, 2, "Reed-Solomon"), (ms, rs, 2, "min-sum"), (rows, rs, 2, "Reed-Solomon"),
                               (rows, ms, 2, "min-sum"), (rows, ms, 99, "CC_CHASE_MAX_P"), (rs, cols, 99, "Reed-Solomon"),
                               (rows, cols, 7, "CC_CHASE_MAX_P"),
                               (bch(3, 1, n=5), cols, 6, "frame length"), (rows, bch(3, 1, n=5), 6, "frame length"),
                               (bch(8, 17), cols, 2, "2t <= 32")):
            c = Call(r, c_, p=p, **nan)
            assert c(dev, ext=c.y.ctypes.data_as(C.c_void_p)) == capi.ERR_UNSUPPORTED, text
            assert text in lib.cc_last_error().decode(), text
        matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
        c = Call(rows, cols, **nan)
        c.desc.cols = matrix._h
        assert c(dev) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in lib.cc_last_error().decode()
        # 5. the schedule, before the buffers
        for alpha, beta in (((0.0, float("inf")), (0.2, 0.4)), ((float("nan"), 0.0), (0.2, 0.4)),
                            ((0.0, 0.5), (0.2, -0.1)), ((0.0, 0.5), (float("nan"), 0.4)), ((0.0, 0.5), (0.2, float("inf")))):
            c = Call(rows, cols, alpha=alpha, beta=beta)
            assert c(dev, out=c.y.ctypes.data_as(C.c_void_p)) == capi.ERR_INVALID_ARGUMENT, (alpha, beta)
        for alpha in ((-3.0, 0.0), (0.0, -0.0)):  # a negative alpha is a schedule
            assert Call(rows, cols, alpha=alpha)(dev) == capi.ERR_NO_DEVICE
        # 6. ext or out overlapping y, by any byte
        c = Call(rows, cols)
        N = c.pc.n
        whole = np.ones(4 * c.B * N + 8, np.float32)
        y, far = whole[: c.B * N], whole[2 * c.B * N + 2:]
        for ext in (whole[c.B * N - 1:], whole[:1], y):
            assert c(dev, y=vp(y), ext=vp(ext)) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(y), out=vp(whole[c.B * N - 1:])) == capi.ERR_INVALID_ARGUMENT
        assert c(dev, y=vp(y), ext=vp(whole[c.B * N:]), out=vp(far)) == capi.ERR_NO_DEVICE  # adjacent is not overlapping
    # the other calls: null pointers, the handles in the same order, then the device
    pc, msg, cw = good.pc, np.zeros(2 * 7 * 11, np.uint8), np.zeros(2 * 225, np.uint8)
    for name, a, b in (("cc_product_encode_batch", msg, cw), ("cc_product_extract_batch", cw, msg)):
        for suffix, tail in (("", ()), ("_dev", (None,))):
            fn = getattr(lib, name + suffix)
            assert fn(C.byref(good.desc), vp(a), vp(b), 2, *tail) == capi.ERR_NO_DEVICE
            assert fn(None, vp(a), vp(b), 2, *tail) == capi.ERR_INVALID_ARGUMENT
            assert fn(C.byref(good.desc), None, vp(b), 2, *tail) == capi.ERR_INVALID_ARGUMENT
            assert fn(C.byref(good.desc), vp(a), None, 2, *tail) == capi.ERR_INVALID_ARGUMENT
            assert fn(C.byref(Call(rs, cols).desc), vp(a), vp(b), 2, *tail) == capi.ERR_UNSUPPORTED
    counters = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    run = lambda desc, c: lib.cc_mc_run_product_dev(desc, 3.0, 1, 0, 16, 1, vp(c), None)
    assert run(C.byref(good.desc), counters) == capi.ERR_NO_DEVICE
    worst = Call(rs, ms, p=99, alpha=(float("inf"),), beta=(-1.0,))
    assert run(None, counters) == capi.ERR_INVALID_ARGUMENT and run(C.byref(worst.desc), None) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), counters) == capi.ERR_UNSUPPORTED
    worst.desc.halves = 0
    assert run(C.byref(worst.desc), counters) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(Call(rows, cols, beta=(0.2, -1.0)).desc), counters) == capi.ERR_INVALID_ARGUMENT
    y = np.zeros(16 * 225, np.float32)
    awgn = lambda desc, y_: lib.cc_awgn_product_dev(desc, 3.0, 1, 0, 16, 1, vp(y_), None, None)
    assert awgn(C.byref(good.desc), y) == capi.ERR_NO_DEVICE and awgn(C.byref(good.desc), None) == capi.ERR_INVALID_ARGUMENT
    assert awgn(None, y) == capi.ERR_INVALID_ARGUMENT and awgn(C.byref(Call(rows, ms).desc), y) == capi.ERR_UNSUPPORTED


def test_product_code_attributes_shapes_and_type_errors():
    rows, cols = bch(4, 1), bch(3, 1)
    pc = cc.product_code(rows, cols)
    assert (pc.n1, pc.n2, pc.k1, pc.k2, pc.n, pc.l) == (15, 7, 11, 4, 105, 44) and pc.rate == 44 / 105
    assert pc.to_string() == "(15, 11, 3)-BMx(7, 4, 3)-BM"
    ext = cc.product_code(bch(6, 3), bch(6, 3), extended=True)
    assert (ext.n1, ext.n2, ext.k1, ext.k2, ext.n, ext.l) == (64, 64, 45, 45, 4096, 2025)
    assert ext.to_string() == "(63, 45, 7)-BMx(63, 45, 7)-BM-ext"
    with pytest.raises(TypeError):
        cc.product_code(rows, object())
    y = np.ones((2, 7, 15), np.float32)
    for call in (pc.correct_batch, pc.decode_batch):
        with pytest.raises(cc.CcError) as e:
            call(y, 2, (0.0,), (0.5,))
        assert e.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(cc.CcError) as e:
            call(np.ones((2, 15, 7), np.float32), 2, (0.0,), (0.5,))
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="float32"):
            call(np.ones((2, 7, 15), np.uint8), 2, (0.0,), (0.5,))
        with pytest.raises(ValueError):
            call(y, 2, (0.0, 0.1), (0.5,))
        with pytest.raises(ValueError):
            call(y, 2, (), ())
        with pytest.raises(cc.CcError) as e:
            call(y, 7, (0.0,), (0.5,))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(cc.CcError) as e:
            call(y, 2, (0.0,), (1e39,))  # +inf as a float32
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError) as e:
        pc.correct_batch(y, 2, (0.0,), (0.5,), ext=False)
    assert e.value.status == capi.ERR_NO_DEVICE
    for call, good, bad in ((pc.encode_batch, (2, 4, 11), (2, 11, 4)), (pc.extract_batch, (2, 7, 15), (2, 15, 7))):
        with pytest.raises(cc.CcError) as e:
            call(np.zeros(good, np.uint8))
        assert e.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(cc.CcError) as e:
            call(np.zeros(bad, np.uint8))
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="uint8"):
            call(np.zeros(good, np.float32))
    # product_decode on two codes of the package is that call
    with pytest.raises(cc.CcError) as e:
        cc.product_decode(rows, cols, y, 2, (0.0,), (0.5,))
    assert e.value.status == capi.ERR_NO_DEVICE


def test_sigma_is_the_formula_at_the_rate_of_the_product():
    for r, c, extended in ((bch(4, 1), bch(3, 1), False), (bch(6, 3), bch(6, 2), True), (bch(8, 2), bch(8, 2), True)):
        pc = cc.product_code(r, c, extended)
        e = 1 if extended else 0
        rate = r.l * c.l / ((r.n + e) * (c.n + e))
        assert pc.rate == rate
        for ebno in (-1.0, 0.0, 3.0, 7.5):
            assert abs(pc.sigma(ebno) - 1.0 / np.sqrt(2.0 * rate * 10.0 ** (ebno / 10.0))) < 1e-12
    assert capi.lib().cc_product_sigma(None, 3.0) == 0.0


class StubBackend:
    """counts what it is asked for: one block error in a hundred"""

    def __init__(self):
        self.calls = []

    def run(self, point, seed, first, blocks):
        self.calls.append((point, seed, first, blocks))
        c = np.zeros(capi.MC_NCOUNTERS, np.int64)
        c[capi.MC_FRAMES], c[capi.MC_WORD_ERRORS], c[capi.MC_BIT_ERRORS] = blocks, blocks // 100, blocks // 50
        return c


def test_simulation_ladder_log_name_and_sharding(tmp_path, monkeypatch):
    pc = cc.product_code(bch(6, 3), bch(6, 3), extended=True)
    alpha, beta = (0.0, 0.2, 0.3), (0.2, 0.4, 0.6)
    stub = StubBackend()
    sim = product_simulation(pc, 4, alpha, beta, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    start, _ = montecarlo.ladder(pc.rate, 0.5)
    assert sim.start == start and sim.points()[0] == start and sim.points()[1] == start + 0.5
    res = sim()
    assert (tmp_path / "(63, 45, 7)-BMx(63, 45, 7)-BM-ext-chase4-h3.log").exists()
    assert len(res) == len(sim.points()) == len(stub.calls)
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["ber"] == 20 / (1000 * 4096)
    # every point draws from its own stretch of the global block sequence
    assert [c[2] for c in stub.calls[:3]] == [0, 1 << 40, 2 << 40] and all(c[1] == 0 for c in stub.calls)
    with pytest.raises(RuntimeError, match="already exists"):
        sim()
    with pytest.raises(ValueError):
        product_simulation(pc, 4, (), (), backend=stub)
    with pytest.raises(ValueError):
        product_simulation(pc, 4, (0.0, 0.1), (0.2,), backend=stub)

    # sharding is by block: rank 1 of 3 owns the middle third of the blocks of a point
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
    sim2 = product_simulation(pc, 4, alpha, beta, backend=stub2)
    monkeypatch.setattr(sim2, "_dist", lambda: Dist())
    sim2.run_point(3.0, 1000, 2)
    lo, count = montecarlo.shard(1000, 1, 3)
    assert stub2.calls == [(3.0, 0, (2 << 40) + lo, count)]


def test_benchmark_options():
    assert "--cols-k" in benchmark.usage_text() and "product" in benchmark.usage_text()
    base = ["--simulation", "product", "--k", "6", "--dmin", "7"]
    assert benchmark.main(base) == 1  # no default schedule
    assert benchmark.main(base + ["--alpha", "0,0.3", "--beta", "0.2"]) == 1
    assert benchmark.main(base + ["--alpha", "0,0.3", "--beta", "0.2,0.4", "--chase", "7"]) == 1
    assert benchmark.main(["--simulation", "product", "--alpha", "0", "--beta", "0.2"]) == 1
    ap = lambda extra: benchmark.product_arguments(benchmark_args(base + extra))
    assert ap(["--alpha", "0,0.3", "--beta", "0.2,0.4"]) == ((6, 7), (6, 7), 4, [0.0, 0.3], [0.2, 0.4])
    assert ap(["--alpha", "0", "--beta", "1", "--cols-k", "4", "--cols-dmin", "3", "--chase", "2"]) == ((6, 7), (4, 3), 2, [0.0], [1.0])
    pc = benchmark.build_product((6, 7), (4, 3), True, device=capi.DEVICE_NONE)
    assert pc.to_string() == "(63, 45, 7)-BMx(15, 11, 3)-BM-ext"


@pytest.mark.parametrize("name", ["255_239x63_57", "63_57x255_239"])
def test_ragged_tile_batches_hold_what_they_are_chosen_for(name):
    """the two cases of tests/test_gpu_product.py with a short last tile, by the model alone: the conditions of its
    test_model_batches_are_not_degenerate, and a tiling with R % TR != 0 in every shape"""
    import test_gpu_product as G
    assert name in G.RAGGED
    G.test_model_batches_are_not_degenerate(name)
    for shape, rows in G.tilings(name).items():
        assert len(rows) == 2 and 0 < rows[-1] < rows[0], (shape, rows)


def benchmark_args(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--simulation")
    for name in ("--k", "--dmin"):
        ap.add_argument(name, action="append")
    for name in ("--cols-k", "--cols-dmin", "--chase"):
        ap.add_argument(name, type=int, default=None)
    ap.add_argument("--alpha")
    ap.add_argument("--beta")
    return ap.parse_args(argv)
