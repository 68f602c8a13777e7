"""GPU tests of iBDD with scaled reliability of product codes (cc_product_decode_sr): out, nflip, last and
status byte for byte and int for int against tests/product_sr_model.py.

The batches and schedules are those of tests/test_product_sr_host.py (CASES and SCHEDULES there say what each is for;
test_model_batches_are_not_degenerate holds it).  Every case runs every schedule; the rising schedule also runs under the
buffer contract of tests/guarded_buffers.py (guards around every output, poison around y, each subset of nflip, last and
status NULL, least alignment).  Further: special values planted in y, prefixes of the schedule, more half-iterations
than the kernel's arguments hold, B = 0, B no multiple of four, more blocks than the grid holds workgroups (wavefronts),
host pointers against device pointers, a tensor on a stream of its own, and the Monte-Carlo counters against channel +
model + count, split and chunked."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import ProductSrBackend
import guarded_buffers as GB
import product_sr_model as SR
from test_gpu_product_hard import counted
from test_product_hard_host import encode_blocks
from test_product_sr_host import CASES, INF, RISING, SCHEDULES, case, model_outputs, noisy

pytestmark = pytest.mark.gpu
KEYS = ("out", "nflip", "last", "status")


def handle(q, t, N=None):
    kw = {} if N is None else {"n": N}
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw)


def product_of(name):
    r, c, extended = CASES[name][:3]
    return cc.product_code(handle(*r), handle(*c), extended=extended)


def same(got, want, what):
    assert set(got) >= set(KEYS), what
    for k in KEYS:
        g = got[k].cpu().numpy() if hasattr(got[k], "cpu") else got[k]
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), (what, k)


def on_device(pc, y, weights):
    import torch
    return pc.correct_sr_batch(torch.from_numpy(np.array(y)).cuda(), weights)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model_under_every_schedule(name):
    y = case(name)[4]
    pc = product_of(name)
    for schedule in sorted(SCHEDULES):
        same(on_device(pc, y, SCHEDULES[schedule]), model_outputs(name, schedule), (name, schedule))


@pytest.mark.parametrize("name", sorted(CASES))
def test_buffer_contract(name):
    y = case(name)[4]
    B = min(y.shape[0], 33)
    y = y[:B]
    pc = product_of(name)
    w = np.array(RISING, np.float32)
    desc = pc._pc_hard(len(RISING))
    want = {k: np.array(v) for k, v in model_outputs(name, "rising", blocks=slice(0, B)).items()}

    def call(p):
        return capi.lib().cc_product_decode_sr_dev(C.byref(desc), w.ctypes.data_as(C.c_void_p), p["y"], p["out"], p["nflip"],
                                                   p["last"], p["status"], B, p["stream"])

    GB.check_call(call, {"y": y}, {"out": (np.uint8, y.size), "nflip": (np.int32, B), "last": (np.int32, B),
                                   "status": (np.int32, B)}, want, optional=("nflip", "last", "status"), what=name)


@pytest.mark.parametrize("name", ["15_7x15_11", "e64_51xe64_51", "127_113x7_4"])
def test_prefixes_of_the_schedule(name):
    y = case(name)[4][:37]
    pc = product_of(name)
    for H in range(1, 9):
        same(on_device(pc, y, RISING[:H]), model_outputs(name, "rising", H, slice(0, 37)), (name, H))


@pytest.mark.parametrize("B", [0, 1, 2, 3, 5])
def test_few_blocks_and_none(B):
    import torch
    for name in ("15_7x15_11", "e64_51xe64_51", "127_113x7_4"):
        y = case(name)[4][:B]
        got = on_device(product_of(name), y, RISING)
        assert got["out"].shape == y.shape and got["last"].shape == (B,)
        same(got, model_outputs(name, "rising", blocks=slice(0, B)), (name, B))
    desc = product_of("15_7x15_11")._pc_hard(2)
    w = (C.c_float * 2)(0.5, 1.0)
    assert capi.lib().cc_product_decode_sr_dev(C.byref(desc), w, None, None, None, None, None, 0, None) == capi.OK
    assert capi.lib().cc_product_decode_sr(C.byref(desc), w, None, None, None, None, None, 0) == capi.OK
    counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    assert capi.lib().cc_mc_run_product_sr_dev(C.byref(desc), w, 3.0, 1, 0, 0, 1, C.c_void_p(counters.data_ptr()), None) == capi.OK
    assert not counters.any()


@pytest.mark.parametrize("name", ["15_7x15_11", "e16_11xe32_26", "127_113x7_4"])
def test_special_values(name):
    """-0.0, NaN, +inf and -inf planted in y, and |y| set to exactly the weight at a fiftieth of the positions: ties that
    candidates flip revert (the host test shows one such position in the model)"""
    rows, cols, extended, sent, y = case(name)
    y = np.array(y[:64])
    rng = np.random.default_rng(5)
    for value in (-0.0, np.nan, np.inf, -np.inf):
        y[rng.random(y.shape) < 0.003] = value
    tie = rng.random(y.shape) < 0.02
    y[tie] = np.where(y[tie] < 0, np.float32(-1.0), np.float32(1.0))
    assert np.isnan(y).any() and np.isinf(y).any() and (np.abs(y) == 1.0).sum() > 50
    pc = product_of(name)
    for weights in ((1.0, 1.0, 1.0, 1.0), (0.5, 1.0, 1.5, INF), (INF, 0.0, INF)):
        trace = []
        xs = SR.steps(rows, cols, y, weights, extended, trace)
        assert sum(t["reverted"] for t in trace) > 0
        same(on_device(pc, y, weights), SR.outputs(rows, cols, y, xs, len(weights), extended), (name, weights))


def test_more_half_iterations_than_the_arguments_hold():
    """131 half-iterations whose levels do not repeat with a short period: the levels past the 128th come from the
    workspace; against the model and against the 128-prefix"""
    rows, cols, extended, sent, y = case("15_7x15_11")
    y = y[:48]
    rng = np.random.default_rng(9)
    weights = tuple(float(v) for v in rng.choice([0.3, 0.7, 1.1, 1.6], 131))
    xs = SR.steps(rows, cols, y, weights, extended)
    pc = product_of("15_7x15_11")
    for H in (131, 129, 128):
        want = SR.outputs(rows, cols, y, xs, H, extended)
        same(on_device(pc, y, weights[:H]), want, H)
    assert want["last"].max() > 100


def trips(rows_qt, cols_qt, per_cu, ebno):
    """2 * capacity + 77 blocks: every workgroup (wavefront) of the largest grid decodes a second and a third block over
    the planes, states and ctl of the one before; the model decodes a prefix, a stretch around an odd cut, the suffix"""
    import torch
    rows, cols = SR.decoder(*rows_qt), SR.decoder(*cols_qt)
    pc = cc.product_code(handle(*rows_qt), handle(*cols_qt))
    cap = per_cu * torch.cuda.get_device_properties(0).multi_processor_count
    B = 2 * cap + 77
    rng = np.random.default_rng(77)
    few = encode_blocks(rows, cols, rng.integers(0, 2, (64, cols.l, rows.l)).astype(np.uint8), False)
    sent = few[rng.integers(0, 64, B)]
    y = noisy(rows, cols, False, sent, ebno, rng)
    cut = (cap + cap // 3) | 1
    pick = np.unique(np.concatenate([np.arange(40), np.arange(cut - 20, cut + 20), np.arange(B - 40, B)]))
    want = SR.decode(rows, cols, y[pick], RISING, False)
    assert len(set(want["last"].tolist())) >= 3 and len(set(want["status"].tolist())) == 2
    yd = torch.from_numpy(y).cuda()
    whole = {k: v.cpu().numpy() for k, v in pc.correct_sr_batch(yd, RISING).items()}
    same({k: v[pick] for k, v in whole.items()}, want, "whole")
    for lo, hi in ((0, cut), (cut, B)):
        same(pc.correct_sr_batch(yd[lo:hi], RISING), {k: v[lo:hi] for k, v in whole.items()}, lo)


def test_second_and_third_block_of_a_wavefront():
    trips((4, 2), (4, 1), 32, 3.0)


def test_second_and_third_block_of_a_workgroup():
    trips((7, 2), (3, 1), 8, 4.5)


def test_host_pointers_and_a_stream_of_its_own():
    import torch
    name = "e16_11xe32_26"
    y = case(name)[4]
    pc = product_of(name)
    want = model_outputs(name, "rising")
    host = pc.correct_sr_batch(y, RISING)
    assert list(host) == list(KEYS) and all(isinstance(v, np.ndarray) for v in host.values())
    same(host, want, "host")
    dec = pc.decode_sr_batch(y, RISING)
    assert list(dec) == list(KEYS) + ["msg"] and np.array_equal(dec["msg"], pc.extract_batch(want["out"]))
    stream = torch.cuda.Stream()
    yd = torch.from_numpy(np.array(y)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        got = pc.correct_sr_batch(yd, RISING)
    stream.synchronize()
    same(got, want, "stream")


# ---- Monte-Carlo ----
def mc(pc, weights, ebno, seed, first, blocks, random_codewords):
    return ProductSrBackend(pc, weights, random_codewords).run(ebno, seed, first, blocks).cpu().numpy()


@pytest.mark.parametrize("q,t,extended,ebno,blocks", [(4, 1, False, 4.0, 512), (5, 1, True, 3.5, 128)],
                         ids=["15_11x15_11", "e32_26xe32_26"])
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_against_channel_model_and_count(q, t, extended, ebno, blocks, random_codewords):
    pc = cc.product_code(handle(q, t), handle(q, t), extended=extended)
    dec = SR.decoder(q, t)
    seed, first = 2026, (1 << 33) + 5
    ch = pc.channel(ebno, seed, first, blocks, random_codewords)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    xs = SR.steps(dec, dec, y, RISING, extended)
    for halves in (8, 3):
        expect = counted(SR.outputs(dec, dec, y, xs, halves, extended), sent, y)
        got = mc(pc, RISING[:halves], ebno, seed, first, blocks, random_codewords)
        assert np.array_equal(got, expect), (halves, got, expect)
        assert expect[capi.MC_WORD_ERRORS] > 0 and expect[capi.MC_ITER_SUM] > 0 and expect[capi.MC_FAILURES] > 0
        assert expect[capi.MC_ITER_HIST:].sum() == blocks
        assert halves < 8 or np.count_nonzero(expect[capi.MC_ITER_HIST:]) >= 3
    cut = blocks // 3
    parts = mc(pc, RISING, ebno, seed, first, cut, random_codewords) + mc(pc, RISING, ebno, seed, first + cut, blocks - cut, random_codewords)
    assert np.array_equal(parts, mc(pc, RISING, ebno, seed, first, blocks, random_codewords))


def test_mc_across_a_chunk_boundary_equals_the_composition():
    """chunks of 100 blocks (the value is read once, so in a process of its own): 512 blocks cross five boundaries"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here)) +
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import ProductSrBackend\n"
        "from test_gpu_product_hard import counted\n"
        "W = (0.6, 1.0, 1.4, 2.0, float('inf'))\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "pc = cc.product_code(mk(5, 3), mk(5, 3))\n"
        "for rc in (True, False):\n"
        "    got = ProductSrBackend(pc, W, rc).run(3.5, 31, 7, 512).cpu().numpy()\n"
        "    ch = pc.channel(3.5, 31, 7, 512, rc)\n"
        "    res = {k: v.cpu().numpy() for k, v in pc.correct_sr_batch(ch['y'], W).items()}\n"
        "    want = counted(res, ch['sent'].cpu().numpy(), ch['y'].cpu().numpy())\n"
        "    assert np.array_equal(got, want), (got, want)\n"
        "    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_ITER_SUM] > 0\n"
        "print('PRODUCT SR MC OK')\n")
    out = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, CC_AMD_PRODUCT_MC_CHUNK_VALUES=str(100 * 961)),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "PRODUCT SR MC OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
