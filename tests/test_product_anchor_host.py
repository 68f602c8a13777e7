"""CPU-side checks of anchor decoding of product codes (cc_product_decode_anchor) on CC_DEVICE_NONE handles:
the symbols are declared, bound and exported; every refusal in the order the header states, delta == 0 with its text
right behind halves == 0; product_code's TypeErrors and ValueErrors; product_anchor_simulation's log name over a stub; the
benchmark's options; the model of tests/product_anchor_model.py -- nothing is backtracked under a delta above the number
of lines, an anchor's line is a word at every pass boundary, the model against a line-by-line transcription of the
contract over exhaustive enumeration on BCH(7,4)^2 and eBCH(8,4)^2, a hand-built block that shows the sit-out rule -- and
what the batches of tests/test_gpu_product_anchor.py are chosen for, decoded by the model alone.

The batches are those of tests/test_product_hard_host.py (CASES, TRIPS, LONG there) under delta = 1, 2, 3 and 2^31 and up
to 16 half-iterations."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import benchmark, capi, montecarlo
import product_anchor_model as PA
import product_hard_model as PH
from shortened_model import Shortened
from test_product_hard_host import (CASES, LONG, StubBackend, TRIPS, bch, case, encode_blocks, nearest_word_rule, vp)

NONE = dict(device=capi.DEVICE_NONE)
BM = cc.berlekamp_massey_tag
NAMES = ("cc_product_decode_anchor", "cc_product_decode_anchor_dev", "cc_mc_run_product_anchor_dev")
DELTAS = (1, 2, 3, 1 << 31)
HALVES = (1, 2, 3, 8, 16)
SMALL = ("nflip", "last", "status", "nback", "nconf")


@functools.lru_cache(maxsize=None)
def anchor_case(name, delta):
    """the model's run of 16 half-iterations over the batch `name` of CASES, with what every pass saw and the state
    after it, made once"""
    rows, cols, extended, sent, z, _, _ = case(name)
    trace, states = [], []
    run = PA.steps(rows, cols, z, max(HALVES), delta, extended, trace, states=states)
    for a in run[0]:
        a.setflags(write=False)
    return run, trace, states


def model_outputs(name, delta, halves, blocks=slice(None)):
    rows, cols, extended, sent, z, _, _ = case(name)
    xs, nback, nconf = anchor_case(name, delta)[0]
    return PA.outputs(rows, cols, z[blocks], ([x[blocks] for x in xs], nback[:, blocks], nconf[:, blocks]), halves, extended)


# ---- batches past the first trip of a workgroup ----
TRIP_HALVES = 8
TRIP_DELTA = 1


def trips_batch(name, cus):
    """test_product_hard_host.trips_batch for the anchor decoder: 2 * capacity + 77 blocks, so that every workgroup
    (wavefront) of the largest grid decodes a second and a third block over the flags, counters and records of the one
    before.  The blocks of the first trip are drawn from those of a pool that the model backtracks in: each leaves anchor
    flags, hold flags and records behind.  The model's outputs on a picked subset: a prefix, a stretch around an odd cut
    past the capacity, the suffix."""
    (rq, rt), (cq, ct), flips, per_cu = TRIPS[name]
    rows, cols = PH.decoder(rq, rt), PH.decoder(cq, ct)
    cap = per_cu * cus
    B = 2 * cap + 77
    rng = np.random.default_rng(77)
    few = encode_blocks(rows, cols, rng.integers(0, 2, (256, cols.l, rows.l)).astype(np.uint8), False)
    z = few[rng.integers(0, 256, B)]
    z ^= rng.integers(0, 256, z.shape, dtype=np.uint8) < flips
    pool = z[cap: cap + 600]
    busy = pool[PA.decode(rows, cols, pool, TRIP_HALVES, TRIP_DELTA, False)["nback"] > 0]
    assert len(busy) >= 8, len(busy)
    z[:cap] = busy[rng.integers(0, len(busy), cap)]
    cut = (cap + cap // 3) | 1
    pick = np.unique(np.concatenate([np.arange(50), np.arange(cut - 25, cut + 25), np.arange(B - 50, B)]))
    want = PA.decode(rows, cols, z[pick], TRIP_HALVES, TRIP_DELTA, False)
    return dict(rows=rows, cols=cols, z=z, cap=cap, cut=cut, pick=pick, want=want)


def trips_batch_is_not_degenerate(name, batch):
    """the picked blocks of the first trip all backtrack; among those that are no workgroup's first, `last` takes three
    values, both statuses occur, and the counts of backtracks and of refusals take three values each"""
    late = batch["pick"] >= batch["cap"]
    want = batch["want"]
    print(name, "blocks", batch["z"].shape[0], "picked", late.size, "past the first trip", int(late.sum()), "last",
          sorted(set(want["last"][late].tolist())), "not converged", int((want["status"][late] != PH.FRAME_OK).sum()),
          "nback > 0", int((want["nback"][late] > 0).sum()), "nconf > 0", int((want["nconf"][late] > 0).sum()))
    assert late.sum() >= 100 and late.size <= 150
    assert (want["nback"][~late] > 0).all()
    assert len(set(want["last"][late].tolist())) >= 3
    assert set(want["status"][late].tolist()) == {PH.FRAME_OK, PH.FRAME_NOT_CONVERGED}
    for k in ("nback", "nconf"):
        assert (want[k][late] > 0).any() and len(set(want[k][late].tolist())) >= 3, k


# ---- many half-iterations ----
LONG_HALVES = (56, 57)
LONG_DELTA = 2


@functools.lru_cache(maxsize=None)
def long_case():
    """BCH(15,11)^2 at p = 0.06 (LONG of tests/test_product_hard_host.py): the received blocks and the model's full run
    of 57 half-iterations, made once"""
    (q, t), p, blocks, seed = LONG
    dec = PH.decoder(q, t)
    rng = np.random.default_rng(seed)
    sent = encode_blocks(dec, dec, rng.integers(0, 2, (blocks, dec.l, dec.l)).astype(np.uint8), False)
    z = sent ^ (rng.random(sent.shape) < p).astype(np.uint8)
    states = []
    run = PA.steps(dec, dec, z, max(LONG_HALVES), LONG_DELTA, False, states=states)
    return dec, z, run, states


# ---- symbols and refusals ----
def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    raw = C.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.exported_symbols() and hasattr(capi.lib(), name) and hasattr(raw, name)
    # delta is a call argument: the struct is what it was
    assert C.sizeof(capi.Product) == 2 * C.sizeof(C.c_void_p) + 4 + 4 + 4 + 4 + 2 * C.sizeof(C.c_void_p)
    assert callable(montecarlo.ProductAnchorBackend) and callable(montecarlo.product_anchor_simulation)
    for name in ("correct_anchor_batch", "decode_anchor_batch"):
        assert callable(getattr(cc.product_code, name))


def test_the_header_states_the_contract_of_the_model():
    """the sentences of the contract that the model's docstring and the header share"""
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "channelcoding_amd.h")).read()
    flat = " ".join(header.replace("*", " ").split())
    for sentence in ("An anchor is skipped.", "A held line clears its hold flag and is otherwise skipped.",
                     "every crossing anchor with at least `delta` conflicts in this pass is backtracked",
                     "so it sits out its next pass", "Conflict counts do not survive the pass.",
                     "This counts bits, not flags.", "A quiet pass can still turn clean lines into anchors or consume a hold."):
        assert sentence in flat, sentence


class Call:
    """one cc_product_decode_anchor(_dev) call on host arrays, every piece of it replaceable"""

    def __init__(self, rows, cols, extended=False, halves=4, B=2, delta=2):
        self.pc = cc.product_code(rows, cols, extended)
        self.desc = capi.Product(rows._h, cols._h, int(bool(extended)), 99, halves, None, None)
        self.B, self.delta, N = B, delta, self.pc.n
        self.inp, self.out = np.zeros(B * N, np.uint8), np.zeros(B * N, np.uint8)
        self.small = {k: np.zeros(B, np.int32) for k in SMALL}

    def __call__(self, dev=False, **replace):
        a = dict(desc=C.byref(self.desc), delta=self.delta, inp=vp(self.inp), out=vp(self.out), B=self.B)
        a.update({k: vp(v) for k, v in self.small.items()})
        a.update(replace)
        lib = capi.lib()
        args = [a["desc"], a["delta"], a["inp"], a["out"]] + [a[k] for k in SMALL] + [a["B"]]
        return lib.cc_product_decode_anchor_dev(*args, None) if dev else lib.cc_product_decode_anchor(*args)


def test_refusals_and_their_order():
    lib = capi.lib()
    text = lambda: lib.cc_last_error().decode()
    rows, cols = bch(4, 1), bch(4, 2)
    rs = cc.rs(8, cc.errors(16), BM(), **NONE)
    ms = cc.primitive_bch(5, cc.errors(2), cc.min_sum_tag(10), **NONE)
    matrix = cc.min_sum_decoder(ms.H(), cc.min_sum_tag(10), **NONE)
    good = Call(rows, cols)
    counters = np.zeros(capi.MC_NCOUNTERS, np.uint64)
    run = lambda desc, c, delta=2: lib.cc_mc_run_product_anchor_dev(desc, delta, 3.0, 1, 0, 16, 1, vp(c), None)
    for dev in (False, True):
        # a call with nothing wrong reaches the device check; the five per-block outputs may be NULL, out == in is allowed,
        # and delta may be as large as the type allows
        assert good(dev) == capi.ERR_NO_DEVICE
        assert good(dev, **{k: None for k in SMALL}) == capi.ERR_NO_DEVICE
        assert good(dev, out=vp(good.inp)) == capi.ERR_NO_DEVICE
        assert good(dev, delta=1) == good(dev, delta=(1 << 32) - 1) == capi.ERR_NO_DEVICE
        # 1. null pointers, whatever else is wrong with the call
        bad = Call(rs, ms, halves=0, delta=0)
        for call in (good, bad):
            assert call(dev, desc=None) == capi.ERR_INVALID_ARGUMENT
            for name in ("inp", "out"):
                assert call(dev, **{name: None}) == capi.ERR_INVALID_ARGUMENT, name
        for field in ("rows", "cols"):
            c = Call(rs, ms, halves=0, delta=0)
            setattr(c.desc, field, None)
            assert c(dev) == capi.ERR_INVALID_ARGUMENT
        # 2. no half-iteration: before delta and before the handles are looked at
        assert Call(rows, rs)(dev) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in text()
        assert Call(rs, ms, halves=0, delta=0)(dev) == capi.ERR_INVALID_ARGUMENT and "delta" not in text()
        # 2a. delta == 0, with a text: before the handles are looked at
        assert Call(rs, ms, delta=0)(dev) == capi.ERR_INVALID_ARGUMENT and "delta is 0" in text()
        assert good(dev, delta=0) == capi.ERR_INVALID_ARGUMENT and "delta is 0" in text()
        # 3. what the Chase call refuses at p = 0 for rows, then for cols, before the buffers are looked at
        for r, c_, what in ((rs, ms, "Reed-Solomon"), (ms, rs, "min-sum"), (rows, rs, "Reed-Solomon"), (rows, ms, "min-sum"),
                            (bch(8, 17), ms, "2t <= 32"), (rows, bch(8, 17), "2t <= 32")):
            c = Call(r, c_)
            assert c(dev, out=vp(c.inp[1:])) == capi.ERR_UNSUPPORTED, what
            assert what in text(), what
        c = Call(rows, cols)
        c.desc.cols = matrix._h
        assert c(dev, out=vp(c.inp[1:])) == capi.ERR_INVALID_ARGUMENT and "cc_minsum_create" in text()
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
        assert good(dev, B=0, inp=None, out=None, delta=0) == capi.ERR_INVALID_ARGUMENT
    # a value that is no bit is looked at only once a device is there: the device check comes first
    c = Call(rows, cols)
    c.inp[5] = 2
    assert c(False) == capi.ERR_NO_DEVICE
    # the Monte-Carlo call: NULL pc / counters first, then the same order
    assert run(C.byref(good.desc), counters) == capi.ERR_NO_DEVICE
    worst = Call(rs, ms, halves=0)
    assert run(None, counters) == capi.ERR_INVALID_ARGUMENT and run(C.byref(worst.desc), None, 0) == capi.ERR_INVALID_ARGUMENT
    assert run(C.byref(worst.desc), counters) == capi.ERR_INVALID_ARGUMENT
    worst.desc.halves = 3
    assert run(C.byref(worst.desc), counters, 0) == capi.ERR_INVALID_ARGUMENT and "delta is 0" in text()
    assert run(C.byref(worst.desc), counters) == capi.ERR_UNSUPPORTED and "Reed-Solomon" in text()
    assert not counters.any()


# ---- the Python layer ----
def test_product_code_type_and_value_errors():
    pc = cc.product_code(bch(4, 1), bch(3, 1))
    z = np.zeros((2, 7, 15), np.uint8)
    for call in (pc.correct_anchor_batch, pc.decode_anchor_batch):
        with pytest.raises(cc.CcError) as e:
            call(z, 2, 4)
        assert e.value.status == capi.ERR_NO_DEVICE
        with pytest.raises(cc.CcError) as e:
            call(np.zeros((2, 15, 7), np.uint8), 2, 4)
        assert e.value.status == capi.ERR_LENGTH
        with pytest.raises(TypeError, match="uint8"):
            call(np.zeros((2, 7, 15), np.float32), 2, 4)
        for halves in (0, -1):
            with pytest.raises(ValueError):
                call(z, 2, halves)
        for delta in (0, -1, 1 << 32):
            with pytest.raises(ValueError, match="delta"):
                call(z, delta, 4)
        for delta in (1.5, True, "2"):
            with pytest.raises((TypeError, ValueError)):
                call(z, delta, 4)
        with pytest.raises(TypeError):
            call(z, halves=4)  # delta has no default
    with pytest.raises(ValueError):
        montecarlo.product_anchor_simulation(pc, 0, 4, backend=object())
    with pytest.raises(ValueError):
        montecarlo.product_anchor_simulation(pc, 2, 0, backend=object())


def test_simulation_log_name_and_ladder(tmp_path):
    pc = cc.product_code(bch(6, 3), bch(6, 3), extended=True)
    stub = StubBackend()
    sim = montecarlo.product_anchor_simulation(pc, 2, 6, backend=stub, max_samples=1000, log_dir=str(tmp_path))
    hard = montecarlo.product_hard_simulation(pc, 6, backend=StubBackend())
    assert sim.start == hard.start and sim.points() == hard.points() and (sim.delta, sim.halves) == (2, 6)
    res = sim()
    path = tmp_path / "(63, 45, 7)-BMx(63, 45, 7)-BM-ext-anchor2-h6.log"
    assert path.exists() and len(res) == len(sim.points()) == len(stub.calls)
    assert res[0]["frames"] == 1000 and res[0]["wer"] == 0.01 and res[0]["mean_last"] == 3.5
    lines = path.read_text().splitlines()
    assert lines[0].split() == ["ebno", "wer", "mean_last"] and len(lines) == 1 + len(res)
    assert [c[2] for c in stub.calls[:3]] == [0, 1 << 40, 2 << 40]


def test_benchmark_options():
    assert "--anchor" in benchmark.usage_text()
    base = ["--simulation", "product", "--k", "6", "--dmin", "7"]
    assert benchmark.main(base + ["--anchor", "2"]) == 1  # no --halves
    assert benchmark.main(base + ["--halves", "4", "--anchor", "0"]) == 1
    assert benchmark.main(base + ["--halves", "0", "--anchor", "2"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--anchor", "2", "--alpha", "0"]) == 1
    assert benchmark.main(base + ["--halves", "4", "--anchor", "2", "--weights", "1,1,1,1"]) == 1

    def parsed(extra):
        import argparse
        ap = argparse.ArgumentParser()
        ap.add_argument("--simulation")
        for name in ("--k", "--dmin"):
            ap.add_argument(name, action="append")
        for name in ("--cols-k", "--cols-dmin", "--chase", "--halves", "--anchor"):
            ap.add_argument(name, type=int, default=None)
        for name in ("--alpha", "--beta", "--weights"):
            ap.add_argument(name)
        return benchmark.product_anchor_arguments(ap.parse_args(base + extra))

    assert parsed(["--halves", "6", "--anchor", "2"]) == ((6, 7), (6, 7), 6, 2)
    assert parsed(["--halves", "1", "--anchor", "1", "--cols-k", "4", "--cols-dmin", "3"]) == ((6, 7), (4, 3), 1, 1)
    assert isinstance(parsed(["--anchor", "2"]), str) and isinstance(parsed(["--halves", "6", "--anchor", "0"]), str)


# ---- the model ----
def test_nothing_is_backtracked_under_a_delta_above_the_number_of_lines():
    """a crossing anchor collects at most one conflict per line of the pass"""
    for name in ("15_11x15_7", "e16_11xe32_26", "s40_22x15_7"):
        rows, cols, extended, sent, z, _, _ = case(name)
        w2, w1 = z.shape[1:]
        _, nback, nconf = PA.steps(rows, cols, z, 8, max(w1, w2) + 1, extended)
        assert not nback.any() and nconf.any(), name
        assert nback.sum() == 0 == anchor_case(name, 1 << 31)[0][1].sum()
        assert anchor_case(name, 1)[0][1].any(), name


def test_an_anchor_is_a_word_at_every_pass_boundary_and_records_belong_to_anchors():
    for name, delta in (("15_11x15_7", 1), ("e16_11xe32_26", 2), ("s40_22x15_7", 1), ("63_45x63_45", 3)):
        rows, cols, extended, sent, z, _, _ = case(name)
        (xs, _, _), _, states = anchor_case(name, delta)
        B, w2, w1 = z.shape
        for x, st in zip(xs, states):
            for code, lines, d in ((rows, x.reshape(B * w2, w1), 0), (cols, PH.turn(x).reshape(B * w1, w2), 1)):
                word = PH.is_word(code, lines, extended).reshape(st.A[d].shape)
                assert word[st.A[d]].all(), (name, d)
                assert not st.R[d][~st.A[d]].any() and not (st.A[d] & st.H[d]).any(), (name, d)
                assert (st.R[d].sum(axis=2) <= code.t).all()


def contract_by_enumeration(words, t, z, halves, delta, w):
    """the contract of the header line by line, one block at a time, with sets and loops; bounded-distance decoding by
    enumeration of the code"""
    B = z.shape[0]
    x = z.copy()
    xs, nback, nconf = [], np.zeros((halves, B), np.int32), np.zeros((halves, B), np.int32)
    flags = [{"A": [[False] * w, [False] * w], "H": [[False] * w, [False] * w], "R": [[set() for _ in range(w)] for _ in range(2)]}
             for _ in range(B)]
    for h in range(halves):
        d, o = h % 2, 1 - h % 2
        for b in range(B):
            s = flags[b]
            blk = x[b] if d == 0 else x[b].T  # a view: lines of the pass are its rows
            taken = nearest_word_rule(words, t, np.ascontiguousarray(blk))
            d_near = (blk[:, None, :] != words[None, :, :]).sum(axis=2).min(axis=1)
            A0, H0, Ac = list(s["A"][d]), list(s["H"][d]), list(s["A"][o])
            count = [0] * w
            flips = []
            for i in range(w):
                if A0[i]:
                    continue
                if H0[i]:
                    s["H"][d][i] = False
                    continue
                if d_near[i] > t:
                    continue
                E = set(np.flatnonzero(taken[i] != blk[i]).tolist())
                hits = [k for k in E if Ac[k]]
                if not hits:
                    flips += [(i, k) for k in E]
                    s["A"][d][i], s["R"][d][i] = True, E
                else:
                    nconf[h, b] += 1
                    for k in hits:
                        count[k] += 1
            for i, k in flips:
                blk[i, k] ^= 1
            for k in range(w):
                if Ac[k] and count[k] >= delta:
                    for i in s["R"][o][k]:
                        blk[i, k] ^= 1
                        s["A"][d][i], s["R"][d][i] = False, set()
                    s["A"][o][k], s["R"][o][k], s["H"][o][k] = False, set(), True
                    nback[h, b] += 1
        xs.append(x.copy())
    return xs, nback, nconf, flags


@pytest.mark.parametrize("delta", [1, 2, 3])
@pytest.mark.parametrize("extended", [False, True], ids=["7_4", "e8_4"])
def test_model_against_the_contract_by_enumeration(extended, delta):
    dec = PH.decoder(3, 1)
    msgs = ((np.arange(16)[:, None] >> np.arange(4)[None, :]) & 1).astype(np.uint8)
    words = np.asarray(dec.encode(msgs), np.uint8)
    if extended:
        words = np.concatenate([words, (words.sum(axis=1, keepdims=True) & 1).astype(np.uint8)], axis=1)
    w = 8 if extended else 7
    rng = np.random.default_rng(21)
    sent = encode_blocks(dec, dec, rng.integers(0, 2, (120, 4, 4)).astype(np.uint8), extended)
    z = sent ^ (rng.random(sent.shape) < 0.09).astype(np.uint8)
    z[0] = 0
    z[1] = sent[1]
    halves = 8
    states = []
    xs, nback, nconf = PA.steps(dec, dec, z, halves, delta, extended, states=states)
    exs, eback, econf, flags = contract_by_enumeration(words, 1, z, halves, delta, w)
    for h in range(halves):
        assert np.array_equal(xs[h], exs[h]), h
    assert np.array_equal(nback, eback) and np.array_equal(nconf, econf)
    for b in range(120):
        for d in range(2):
            assert states[-1].A[d][b].tolist() == flags[b]["A"][d] and states[-1].H[d][b].tolist() == flags[b]["H"][d]
            assert [set(np.flatnonzero(r).tolist()) for r in states[-1].R[d][b]] == flags[b]["R"][d]
    assert nback.any() and nconf.any() and (nconf.sum(axis=0) > nback.sum(axis=0)).any()
    # a code block comes back unchanged, with every line an anchor after two passes
    for b in (0, 1):
        assert np.array_equal(xs[-1][b], z[b]) and not nback[:, b].any() and not nconf[:, b].any()
        assert states[0].A[0][b].all() and not states[0].A[1][b].any() and states[1].A[0][b].all() and states[1].A[1][b].all()
    got = PA.outputs(dec, dec, z, (xs, nback, nconf), halves, extended)
    assert got["last"][0] == 0 == got["nflip"][0] and got["status"][0] == PH.FRAME_OK
    assert got["nback"].dtype == got["nconf"].dtype == np.int32


def test_the_sit_out_rule_on_a_hand_built_block():
    """BCH(7,4)^2, the zero block with two errors in row 3: the row is miscorrected into a word of weight 3 and becomes an
    anchor; its three columns are refused, the row is backtracked and sits out, and the columns decode the block.  Without
    the hold flag the row miscorrects again in the very next row pass, because the columns that voted it out have not
    moved yet, and the block cycles."""
    dec = PH.decoder(3, 1)
    z = np.zeros((1, 7, 7), np.uint8)
    z[0, 3, 1] = z[0, 3, 4] = 1
    for delta in (1, 2, 3):
        trace = []
        xs, nback, nconf = PA.steps(dec, dec, z, 8, delta, False, trace)
        assert xs[0][0, 3].sum() == 3 and xs[0].sum() == 3            # the miscorrection
        assert nconf[1, 0] == 3 and nback[1, 0] == 1                   # three columns refused, the row backtracked
        assert np.array_equal(xs[1], z)                                # its flip is taken back
        assert trace[2]["held"][0, 3] and np.array_equal(xs[2], z)     # the row sits out
        assert not xs[3].any() and nback.sum() == 1                    # the columns decode
        got = PA.outputs(dec, dec, z, (xs, nback, nconf), 8, False)
        assert got["status"][0] == PH.FRAME_OK and got["last"][0] == 4 and got["nflip"][0] == 2
        ys, yback, _ = PA.steps(dec, dec, z, 8, delta, False, sit_out=False)
        assert all(np.array_equal(ys[h], xs[0] if h % 2 == 0 else z) for h in range(8)) and yback.sum() == 4
    # with more conflicts asked for than the row collects it stays, and the columns finish the miscorrection's word
    xs, nback, nconf = PA.steps(dec, dec, z, 8, 4, False)
    assert nback.sum() == 0 and nconf[1, 0] == 3 and xs[-1].sum() == 3


# ---- what the GPU batches hold ----
def test_model_batches_are_not_degenerate():
    seen = dict(back=0, refused_only=0, lost=0, held=0, clean_back=0, parity_conflict=0, virtual=0,
                better=0)
    statuses = set()
    for name in sorted(CASES):
        rows, cols, extended, sent, z, hard_xs, _ = case(name)
        B = z.shape[0]
        hard_right = (PH.outputs(rows, cols, z, hard_xs, 8, extended)["out"] == sent).all(axis=(1, 2))
        for delta in DELTAS:
            (xs, nback, nconf), trace, states = anchor_case(name, delta)
            got = PA.outputs(rows, cols, z, (xs, nback, nconf), 8, extended)
            right = (got["out"] == sent).all(axis=(1, 2))
            print(name, "delta", delta, "blocks", B, "right", int(right.sum()), "iBDD right", int(hard_right.sum()), "nback",
                  got["nback"].tolist()[:8], "nconf", got["nconf"].tolist()[:8], "last", sorted(set(got["last"].tolist())))
            statuses |= set(got["status"].tolist())
            seen["back"] += int((got["nback"] > 0).sum())
            seen["refused_only"] += int(((got["nconf"] > 0) & (got["nback"] == 0)).sum())
            if right.sum() > hard_right.sum() and not np.array_equal(got["out"], PH.outputs(rows, cols, z, hard_xs, 8, extended)["out"]):
                seen["better"] += 1
            for tr in trace:
                seen["lost"] += int(tr["lost"].sum())
                seen["held"] += int(tr["held"].sum())
                empty = tr["back"] & ~tr["undo"].any(axis=2)
                seen["clean_back"] += int(empty.sum())
                code = cols if tr["column"] else rows
                if extended:
                    seen["parity_conflict"] += int(tr["conflict"][:, :, code.n].sum())
                if isinstance(code, Shortened):
                    L = tr["before"].shape[1]
                    virtual = PH.rejected_for_a_virtual_root(code, tr["before"].reshape(B * L, -1)).reshape(B, L)
                    seen["virtual"] += int((virtual & tr["active"]).sum())
    print(seen, statuses)
    assert statuses == {PH.FRAME_OK, PH.FRAME_NOT_CONVERGED}
    for k, v in seen.items():
        assert v > 0, k


@pytest.mark.parametrize("name", sorted(TRIPS))
def test_trip_batches_are_not_degenerate(name):
    """at the 256 compute units of an MI355X; the GPU test asserts the same at the count of the device it runs on"""
    trips_batch_is_not_degenerate(name, trips_batch(name, 256))


def test_long_batch_shows_an_early_stop_that_no_bit_change_alone_would_get_wrong():
    """BCH(15,11)^2 at p = 0.06 through 56 and 57 half-iterations: blocks that change up to the last pass, blocks that
    settle early, and blocks with a pass that changes no bit but a flag -- after which bits change again, so a stop on
    two passes without a bit change would show"""
    dec, z, (xs, nback, nconf), states = long_case()
    chain = [z] + xs
    quiet_bits = np.array([~(chain[h + 1] != chain[h]).any(axis=(1, 2)) for h in range(len(xs))])
    start = PA.State(*z.shape)
    quiet_state = np.array([quiet_bits[h] & (states[h - 1] if h else start).same(states[h]) for h in range(len(xs))])
    trap = np.zeros(z.shape[0], bool)
    for h in range(1, len(xs) - 1):
        fixed = quiet_state[h - 1] & quiet_state[h]
        assert quiet_state[h + 1:, fixed].all()  # the fixed point the device may stop at
        trap |= quiet_bits[h - 1] & quiet_bits[h] & ~quiet_bits[h + 1:].all(axis=0)
    for halves in LONG_HALVES:
        got = PA.outputs(dec, dec, z, (xs, nback, nconf), halves, False)
        print(halves, "last", sorted(set(got["last"].tolist())), "nback > 0", int((got["nback"] > 0).sum()))
        assert (got["last"] <= 8).sum() >= 5 and set(got["status"].tolist()) == {PH.FRAME_OK, PH.FRAME_NOT_CONVERGED}
    print("blocks where two passes without a bit change are no fixed point:", int(trap.sum()))
    assert trap.any()
