"""GPU tests of product codes on the device: cc_product_decode(_dev) bit for bit against the model loops of
chase_soft_model / chase_ext_model after 1 .. 4 half-iterations (ext compared as u32), with guard elements around every
output; signed zeros; the hard output of ext == NULL; buffers at odd offsets; host against device pointers in small
staging chunks; the encoder and its inverse; the channel against awgn_model; the Monte-Carlo counters against channel +
model + count, sharded, chunked and over the number of half-iterations.

What the batches are chosen for, and where a condition cannot hold (test_model_batches_are_not_degenerate):
- a component word fails: asserted for BCH(63,45), where 16 % of the syndromes are decodable and a word without a
  candidate among 16 patterns is common.  A full-length t = 1 code is perfect and has a candidate for every pattern; of
  BCH(255,239) half the syndromes are decodable, so a word whose 16 patterns all fail is one in tens of thousands: the
  batches of those codes have no failed word, and none is asserted.
- positions with a competitor and positions with +-beta: a code of length 7 or 8 has 16 words and p = 4 gives 16 test
  patterns, whose candidates differ from the winner at every position; +-beta is asserted for the longer components.
- the block errors fall from the first half-iteration to the last: every case.

Which case gives which tiling of mix_turn_kernel and of the byte turn (rows per tile = 8448 // (C | 1), capped at R;
tilings() computes them, test_tilings_of_the_cases holds them):
- one tile, the whole block: 7_4x15_11, 63_45x63_45 (134 rows would fit), e256_239xe8_4 and its turn, the models' own two
  cases, every Monte-Carlo code;
- eight even tiles of 32 rows: e256_239xe256_239;
- two tiles, the last one short: 255_239x63_57 (63 x 255) has 33 + 30 rows of y in a column pass and in the byte turn,
  134 + 121 in a row pass and in the turn of `ext`; 63_57x255_239 (255 x 63) has them the other way round;
- more tiles than the largest grid has workgroups, two a block: test_grid_stride_over_the_tiles_of_a_block;
- more blocks than the largest grid has workgroups, a tile each: test_grid_stride_trips_of_the_small_kernels."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import ProductBackend
import awgn_model
import chase_ext_model as E
import chase_model as M
import chase_soft_model as S
from checkers import awgn_llr
from test_chase_ext_host import extended_product_batch
from test_chase_soft_host import ALPHA, BETA, P, product_batch
from test_discrete_host import bch_message_bits
from test_gpu_chase_soft import GUARD, SENTINEL, guarded, guards_intact
from test_gpu_mc import tau

pytestmark = pytest.mark.gpu

# name: rows (q, t), cols (q, t), extended, Eb/N0 chosen with the model on the CPU (test_model_batches_are_not_degenerate
# holds what it was chosen for), blocks, seed
CASES = {
    "7_4x15_11": ((3, 1), (4, 1), False, 2.0, 67, 11),           # 15 x 7: narrower than any tile, odd, non-square
    "63_45x63_45": ((6, 3), (6, 3), False, 2.5, 8, 12),          # one tile of 63 odd rows, eight blocks, t = 3: words fail
    "e256_239xe8_4": ((8, 2), (3, 1), True, 3.5, 16, 13),        # 8 x 256: the 256 side along the rows
    "e8_4xe256_239": ((3, 1), (8, 2), True, 3.5, 16, 14),        # 256 x 8: its turn
    "e256_239xe256_239": ((8, 2), (8, 2), True, 4.5, 2, 15),     # a full block, 64 Ki values: eight even tiles
    "255_239x63_57": ((8, 2), (6, 1), False, 4.0, 3, 21),        # 63 x 255: two ragged tiles in every shape
    "63_57x255_239": ((6, 1), (8, 2), False, 4.0, 3, 22),        # 255 x 63: its turn
}
RAGGED = ("255_239x63_57", "63_57x255_239")
HALVES = (1, 2, 3, 4)
TILE = 8448  # values of a tile in LDS, of mix_turn_kernel and of the byte turn alike


def tiles_of(R, C):
    """the rows of the tiles a source array [R][C] is cut into: 8448 // (C | 1) rows a tile, capped at R, the rest last"""
    TR = min(TILE // (C | 1), R)
    return [TR] * (R // TR) + ([R % TR] if R % TR else [])


def tilings(name):
    """the tiles of a block in the three shapes of a decode: X of a column pass from y [w2][w1], X of a row pass and a last
    `ext` from the column-oriented [w1][w2], and the byte turn of a last column pass's `out`, w2 positions of w1"""
    (rq, _), (cq, _), extended = CASES[name][:3]
    e = 1 if extended else 0
    w1, w2 = (1 << rq) - 1 + e, (1 << cq) - 1 + e
    return dict(mix_column=tiles_of(w2, w1), mix_row_and_turn=tiles_of(w1, w2), byte_turn=tiles_of(w2, w1))


def can_fail(qt):
    return qt[1] > 2  # (see the head of the file)


def has_plain(qt):
    return qt[0] > 3  # components longer than 8


def encode_blocks(rows, cols, info, extended):
    """the helper construction of product_batch / extended_product_batch: rows encoded (and extended), then columns"""
    blocks = info.shape[0]
    ext = E.extend if extended else (lambda w: w)
    e = 1 if extended else 0
    wide = ext(rows.encode(info.reshape(-1, rows.l))).reshape(blocks, cols.l, rows.n + e)
    tall = ext(cols.encode(np.ascontiguousarray(wide.transpose(0, 2, 1)).reshape(-1, cols.l)))
    return np.ascontiguousarray(tall.reshape(blocks, rows.n + e, cols.n + e).transpose(0, 2, 1))


def model_steps(rows, cols, y, extended, p=P, alpha=ALPHA, beta=BETA):
    return (E if extended else S).product_decode(rows, cols, y, p, alpha, beta)


@functools.lru_cache(maxsize=None)
def case(name):
    """model decoders, the blocks sent, y and the model's outputs after each of the four half-iterations, made once"""
    (rq, rt), (cq, ct), extended, ebno, blocks, seed = CASES[name]
    rows, cols = M.decoder(rq, rt), M.decoder(cq, ct)
    rng = np.random.default_rng(seed)
    sent = encode_blocks(rows, cols, rng.integers(0, 2, (blocks, cols.l, rows.l)).astype(np.uint8), extended)
    y = awgn_llr(rng, sent, rows.l * cols.l / sent[0].size, ebno)
    y.setflags(write=False)
    return rows, cols, sent, y, model_steps(rows, cols, y, extended)


def handles(rq_rt, cq_ct):
    make = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
    return make(*rq_rt), make(*cq_ct)


def product_of(name):
    rq_rt, cq_ct, extended = CASES[name][:3]
    return cc.product_code(*handles(rq_rt, cq_ct), extended=extended)


def ptr(a):
    return None if a is None else C.c_void_p(a.data_ptr())


def decode_dev(pc, y, halves, want_ext=True, p=P, alpha=ALPHA, beta=BETA):
    """cc_product_decode_dev itself on a device tensor y (B, n2, n1), every output between guard elements"""
    import torch
    desc = pc._pc(p, alpha[:halves], beta[:halves])
    B, lines = y.shape[0], pc.n2 if halves % 2 else pc.n1
    wo, out = guarded(torch, B * pc.n, torch.uint8)
    we, ext = guarded(torch, B * pc.n, torch.float32)
    ws, status = guarded(torch, B * lines, torch.int32)
    rc = capi.lib().cc_product_decode_dev(C.byref(desc), ptr(y), ptr(out), ptr(ext) if want_ext else None, ptr(status), B, None)
    capi.check(rc, "cc_product_decode_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wo) and guards_intact(torch, we) and guards_intact(torch, ws)
    if not want_ext:
        assert bool((we.view(torch.uint8) == SENTINEL).all())
    return dict(out=out.cpu().numpy().reshape(B, pc.n2, pc.n1), ext=ext.cpu().numpy().reshape(B, pc.n2, pc.n1),
                status=status.cpu().numpy().reshape(B, lines))


def same(got, want, what, ext=True):
    assert np.array_equal(got["out"], want["out"]), what
    assert np.array_equal(got["status"], want["status"]), what
    if ext:
        assert np.array_equal(got["ext"].view(np.uint32), want["ext"].view(np.uint32)), what


@pytest.mark.parametrize("name", sorted(CASES))
def test_model_batches_are_not_degenerate(name):
    rows, cols, sent, y, steps = case(name)
    rq_rt, cq_ct = CASES[name][:2]
    errors = [int((s["out"] != sent).any(axis=(1, 2)).sum()) for s in steps]
    print(name, "block errors after each half-iteration", errors, "of", sent.shape[0])
    assert errors[-1] < errors[0], errors
    for h, s in enumerate(steps):
        if can_fail(cq_ct if h % 2 else rq_rt):
            assert (s["status"] == M.FRAME_LOCATOR).any(), (name, h)
        b = np.float32(BETA[h])
        plain = np.abs(s["ext"]) == b  # +-beta: no competitor (a competitor gives that value by accident at most)
        assert (~plain & (s["ext"] != 0)).any(), (name, h)
        if has_plain(cq_ct if h % 2 else rq_rt):
            assert plain.any(), (name, h)


def test_tilings_of_the_cases():
    """what the head of the file says of the tiles, from the launch arithmetic; the two ragged cases have a short last
    tile in every shape, so a later change of the tile size cannot make them even without this test failing"""
    for name in sorted(CASES):
        t = tilings(name)
        print(name, t)
        if name in RAGGED:
            for shape, rows in t.items():
                assert len(rows) == 2 and 0 < rows[-1] < rows[0], (name, shape, rows)  # R % TR != 0
        elif name == "e256_239xe256_239":
            assert all(rows == [32] * 8 for rows in t.values())
        else:
            assert all(len(rows) == 1 for rows in t.values()), (name, t)
    assert tilings("255_239x63_57") == dict(mix_column=[33, 30], mix_row_and_turn=[134, 121], byte_turn=[33, 30])
    assert tilings("63_57x255_239") == dict(mix_column=[134, 121], mix_row_and_turn=[33, 30], byte_turn=[134, 121])


@pytest.mark.parametrize("halves", HALVES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_model(name, halves):
    import torch
    rows, cols, sent, y, steps = case(name)
    pc = product_of(name)
    got = decode_dev(pc, torch.from_numpy(np.array(y)).cuda(), halves)
    same(got, steps[halves - 1], (name, halves))


@pytest.mark.parametrize("B", [1, 2])
def test_single_blocks_narrower_than_a_tile(B):
    import torch
    rows, cols, sent, y, steps = case("7_4x15_11")
    pc = product_of("7_4x15_11")
    for halves in HALVES:
        got = decode_dev(pc, torch.from_numpy(np.array(y[:B])).cuda(), halves)
        same(got, {k: v[:B] for k, v in steps[halves - 1].items()}, (B, halves))


@pytest.mark.parametrize("which", ["15_7x15_11", "e16_11xe32_26"])
def test_the_models_own_cases_through_the_c_call_with_host_and_device_pointers(which):
    import torch
    if which == "15_7x15_11":
        rows, cols, sent, y = product_batch(which)
        y, extended, qt = y[:100], False, ((4, 2), (4, 1))
    else:
        rows, cols, sent, y = extended_product_batch(4, 1, 5, 1, 3.0, 64, 2017)
        extended, qt = True, ((4, 1), (5, 1))
    steps = model_steps(rows, cols, y, extended)
    pc = cc.product_code(*handles(*qt), extended=extended)
    yh = np.ascontiguousarray(y)
    B = yh.shape[0]
    for halves in HALVES:
        same(decode_dev(pc, torch.from_numpy(yh).cuda(), halves), steps[halves - 1], (which, halves, "device"))
        desc = pc._pc(P, ALPHA[:halves], BETA[:halves])
        lines = pc.n2 if halves % 2 else pc.n1
        out, ext = np.full((B, pc.n2, pc.n1), SENTINEL, np.uint8), np.full((B, pc.n2, pc.n1), np.nan, np.float32)
        status = np.full((B, lines), -7, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        capi.check(capi.lib().cc_product_decode(C.byref(desc), vp(yh), vp(out), vp(ext), vp(status), B), "cc_product_decode")
        same(dict(out=out, ext=ext, status=status), steps[halves - 1], (which, halves, "host"))


def test_grid_stride_trips_of_the_small_kernels():
    """BCH(7,4)^2 with more than 16 times as many blocks as the largest grid the mix kernel is launched with (8 per
    compute unit): every workgroup makes more than 16 trips.  The model decodes a subset; a prefix and the rest, decoded
    on their own, equal the whole."""
    import torch
    pc = cc.product_code(*handles((3, 1), (3, 1)))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * 8 * cus + 77
    rng = np.random.default_rng(77)
    rows = M.decoder(3, 1)
    few = encode_blocks(rows, rows, rng.integers(0, 2, (256, 4, 4)).astype(np.uint8), False)
    sent = few[rng.integers(0, 256, B)]
    y = awgn_llr(rng, sent, 16 / 49, 1.0)
    yd = torch.from_numpy(y).cuda()
    cut = 12345
    pick = np.concatenate([np.arange(40), np.arange(cut - 20, cut + 20), np.arange(B - 40, B)])
    steps = model_steps(rows, rows, y[pick], False)
    for halves in (2, 3):
        whole = pc.correct_batch(yd, P, ALPHA[:halves], BETA[:halves])
        whole = {k: v.cpu().numpy() for k, v in whole.items()}
        same({k: v[pick] for k, v in whole.items()}, steps[halves - 1], halves)
        for lo, hi in ((0, cut), (cut, B)):
            part = pc.correct_batch(yd[lo:hi], P, ALPHA[:halves], BETA[:halves])
            same({k: v.cpu().numpy() for k, v in part.items()}, {k: v[lo:hi] for k, v in whole.items()}, (halves, lo))
    # the model's errors fall here too
    assert (steps[2]["out"] != sent[pick]).any(axis=(1, 2)).sum() < (steps[0]["out"] != sent[pick]).any(axis=(1, 2)).sum()


def test_grid_stride_over_the_tiles_of_a_block():
    """BCH(255,239) x BCH(63,57), two ragged tiles a block in every shape, with 77 more blocks than half the largest grid
    (8 workgroups per compute unit): more tiles than workgroups, so a workgroup comes back for tiles t >= gridDim.x and
    splits those into block t / 2 and tile t % 2, a short tile after a full one in the same LDS.
    The model decodes a prefix, a stretch around an odd cut and the suffix; the blocks before and from the cut, decoded on
    their own, equal the whole."""
    import torch
    name = "255_239x63_57"
    pc = product_of(name)
    rows, cols = M.decoder(8, 2), M.decoder(6, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * cus // 2 + 77
    assert all(len(t) == 2 for t in tilings(name).values()) and 2 * B > 8 * cus
    rng = np.random.default_rng(78)
    few = encode_blocks(rows, cols, rng.integers(0, 2, (16, cols.l, rows.l)).astype(np.uint8), False)
    sent = few[rng.integers(0, 16, B)]
    y = awgn_llr(rng, sent, rows.l * cols.l / sent[0].size, CASES[name][3])
    yd = torch.from_numpy(y).cuda()
    cut = (B // 2) | 1
    pick = np.concatenate([np.arange(6), np.arange(cut - 4, cut + 4), np.arange(B - 6, B)])
    steps = model_steps(rows, cols, y[pick], False, alpha=ALPHA[:3], beta=BETA[:3])
    wrong = [int((s["out"] != sent[pick]).sum()) for s in steps]
    print("blocks", B, "picked", pick.size, "bit errors of the model after each half-iteration", wrong)
    assert wrong[2] < wrong[0]
    for halves in (2, 3):
        whole = pc.correct_batch(yd, P, ALPHA[:halves], BETA[:halves])
        whole = {k: v.cpu().numpy() for k, v in whole.items()}
        same({k: v[pick] for k, v in whole.items()}, steps[halves - 1], halves)
        for lo, hi in ((0, cut), (cut, B)):
            part = pc.correct_batch(yd[lo:hi], P, ALPHA[:halves], BETA[:halves])
            same({k: v.cpu().numpy() for k, v in part.items()}, {k: v[lo:hi] for k, v in whole.items()}, (halves, lo))


def test_handles_on_different_devices_are_refused_and_an_empty_batch_is_fine():
    """refusal 4 of the header needs a handle with a device, so it is tested here: after what the Chase call refuses for
    either handle, before the schedule"""
    import torch
    on, off = handles((4, 1), (4, 1))[0], cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag(), device=capi.DEVICE_NONE)
    y = torch.ones((2, 15, 15), dtype=torch.float32, device="cuda")
    for rows, cols in ((on, off), (off, on)):
        pc = cc.product_code(rows, cols)
        with pytest.raises(cc.CcError) as e:
            pc.correct_batch(y, 2, (0.0,), (float("nan"),))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
        with pytest.raises(cc.CcError) as e:
            pc.correct_batch(y, 7, (0.0,), (0.5,))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(cc.CcError) as e:
            pc.correct_batch(y, 2, (0.0,), (0.5,))
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    pc = cc.product_code(on, on)
    desc = pc._pc(2, (0.0,), (0.5,))
    assert capi.lib().cc_product_decode_dev(C.byref(desc), None, None, None, None, 0, None) == capi.OK
    assert capi.lib().cc_product_decode(C.byref(desc), None, None, None, None, 0) == capi.OK
    assert capi.lib().cc_product_encode_batch_dev(C.byref(desc), None, None, 0, None) == capi.OK
    counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device="cuda")
    assert capi.lib().cc_mc_run_product_dev(C.byref(desc), 3.0, 1, 0, 0, 1, ptr(counters), None) == capi.OK
    assert not counters.any()


@pytest.mark.parametrize("alpha0", [-0.5, 0.0])
def test_signed_zeros_in_y_with_a_negative_and_a_zero_first_alpha(alpha0):
    """X = y + (alpha * 0.0f): with alpha >= 0 a -0.0f of y becomes +0.0f, with alpha < 0 it stays -0.0f.  Four in ten
    values of y are zeros of either sign, so candidates that differ at zeros alone tie (K - M = 0) and the sign of the
    zero of X is the sign of ext = s (K - M) - X there: the two values of alpha[0] give different ext, and a copy in
    place of the sum gives that of the negative alpha for both."""
    import torch
    rows, cols, sent, y, _ = case("7_4x15_11")
    rng = np.random.default_rng(3)
    y = np.array(y[:40])
    zero = rng.random(y.shape) < 0.4
    y[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    schedule = lambda a0: (a0, 0.3, -0.25, 0.0)
    steps = S.product_decode(rows, cols, y, P, schedule(alpha0), BETA)
    other = S.product_decode(rows, cols, y, P, schedule(-0.5 if alpha0 == 0.0 else 0.0), BETA)
    for a, b in zip(steps, other):  # what a copy would get wrong, after every half-iteration
        assert (a["ext"].view(np.uint32) != b["ext"].view(np.uint32)).any()
        assert (np.signbit(a["ext"]) & (a["ext"] == 0)).any()
    pc = product_of("7_4x15_11")
    for halves in HALVES:
        got = decode_dev(pc, torch.from_numpy(y).cuda(), halves, alpha=schedule(alpha0), beta=BETA)
        same(got, steps[halves - 1], (alpha0, halves))


@pytest.mark.parametrize("name", ["7_4x15_11", "63_45x63_45", "e8_4xe256_239", "255_239x63_57", "63_57x255_239"])
def test_without_ext_the_hard_output_call_gives_the_same_out_and_status(name):
    import torch
    rows, cols, sent, y, steps = case(name)
    pc = product_of(name)
    for halves in HALVES:
        got = decode_dev(pc, torch.from_numpy(np.array(y)).cuda(), halves, want_ext=False)
        same(got, steps[halves - 1], (name, halves), ext=False)
        res = pc.correct_batch(torch.from_numpy(np.array(y)).cuda(), P, ALPHA[:halves], BETA[:halves], ext=False)
        assert sorted(res) == ["out", "status"]


def test_buffers_at_odd_offsets():
    import torch
    name = "7_4x15_11"
    rows, cols, sent, y, steps = case(name)
    pc = product_of(name)
    B, N = 5, pc.n
    base_y = torch.zeros(B * N + 3, dtype=torch.float32, device="cuda")
    yd = base_y[3:]
    yd.copy_(torch.from_numpy(np.array(y[:B])).cuda().reshape(-1))
    for halves in (3, 4):
        lines = pc.n2 if halves % 2 else pc.n1
        wo, out = guarded(torch, B * N + 1, torch.uint8)
        we, ext = guarded(torch, B * N + 1, torch.float32)
        ws, status = guarded(torch, B * lines + 1, torch.int32)
        desc = pc._pc(P, ALPHA[:halves], BETA[:halves])
        rc = capi.lib().cc_product_decode_dev(C.byref(desc), ptr(yd), ptr(out[1:]), ptr(ext[1:]), ptr(status[1:]), B, None)
        capi.check(rc, "cc_product_decode_dev")
        torch.cuda.synchronize()
        assert guards_intact(torch, wo) and guards_intact(torch, we) and guards_intact(torch, ws)
        assert int(out[0]) == SENTINEL
        got = dict(out=out[1:].cpu().numpy().reshape(B, pc.n2, pc.n1), ext=ext[1:].cpu().numpy().reshape(B, pc.n2, pc.n1),
                   status=status[1:].cpu().numpy().reshape(B, lines))
        same(got, {k: v[:B] for k, v in steps[halves - 1].items()}, halves)


def run_child(script, env, marker):
    here = os.path.dirname(os.path.abspath(__file__))
    head = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n" % (here, os.path.dirname(here))
    out = subprocess.run([sys.executable, "-c", head + script], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0 and marker in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_host_pointers_equal_device_pointers_in_small_staging_chunks():
    """the staging chunk forced small in a process of its own (the value is read once): 70 blocks of 63 x 63 in chunks
    of 16, pageable and page-locked memory, with and without ext, and the Python calls on both sides"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(8)\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "for pc, B in ((cc.product_code(mk(6, 3), mk(6, 3)), 70), (cc.product_code(mk(4, 1), mk(5, 1), extended=True), 300)):\n"
        "    y = (1.0 + 0.7 * rng.standard_normal((B, pc.n2, pc.n1))).astype(np.float32)\n"
        "    pinned = torch.from_numpy(y).pin_memory().numpy()\n"
        "    for halves in (1, 4):\n"
        "        a, b = (0.0, 0.3, 0.5, 0.7)[:halves], (0.2, 0.4, 0.6, 0.8)[:halves]\n"
        "        dev = {k: v.cpu().numpy() for k, v in pc.correct_batch(torch.from_numpy(y.copy()).cuda(), 4, a, b).items()}\n"
        "        assert (dev['status'] != 0).any() or pc.rows.t == 1\n"
        "        assert (dev['ext'] != 0).any() and dev['out'].any()\n"
        "        for src in (y, pinned):\n"
        "            host = pc.correct_batch(src, 4, a, b)\n"
        "            assert list(host) == ['out', 'status', 'ext']\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape, (halves, k)\n"
        "                assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (halves, k)\n"
        "            hard = pc.correct_batch(src, 4, a, b, ext=False)\n"
        "            assert list(hard) == ['out', 'status']\n"
        "            assert np.array_equal(hard['out'], dev['out']) and np.array_equal(hard['status'], dev['status'])\n"
        "        dec = pc.decode_batch(y, 4, a, b)\n"
        "        assert np.array_equal(dec['msg'], pc.extract_batch(dev['out'])) and dec['msg'].shape == (B, pc.k2, pc.k1)\n"
        "        old = cc.product_decode(pc.rows, pc.cols, y, 4, a, b, extended=pc.extended)\n"
        "        assert np.array_equal(old['ext'].view(np.uint32), dev['ext'].view(np.uint32))\n"
        "    m = rng.integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8)\n"
        "    cw = pc.encode_batch(m)\n"
        "    assert np.array_equal(cw, pc.encode_batch(torch.from_numpy(m).cuda()).cpu().numpy())\n"
        "    assert np.array_equal(pc.extract_batch(cw), m)\n"
        "print('PRODUCT HOST OK')\n", {"CC_AMD_HOST_CHUNK_BYTES": str(16 * 63 * 63 * 4)}, "PRODUCT HOST OK")


# ---- encode and extract ----
ENCODE = [((3, 1), (4, 1), False), ((6, 3), (4, 2), False), ((4, 1), (5, 1), True), ((8, 2), (3, 1), True),
          ((8, 2), (8, 2), True)]


def syndromes_vanish(code, words, extended):
    H = np.asarray(code.H(), np.int64)
    inner = words[:, : code.n].astype(np.int64)
    ok = not (inner @ H.T % 2).any()
    return ok and (not extended or not (words.astype(np.int64).sum(axis=1) % 2).any())


@pytest.mark.parametrize("rq_rt,cq_ct,extended", ENCODE)
def test_encode_equals_the_helper_construction_and_extract_inverts_it(rq_rt, cq_ct, extended):
    import torch
    r, c = handles(rq_rt, cq_ct)
    pc = cc.product_code(r, c, extended=extended)
    rows, cols = M.decoder(*rq_rt), M.decoder(*cq_ct)
    B = 37 if pc.n < 4096 else 3
    msg = np.random.default_rng(5).integers(0, 2, (B, pc.k2, pc.k1)).astype(np.uint8)
    want = encode_blocks(rows, cols, msg, extended)
    wm, m = guarded(torch, msg.size, torch.uint8)
    m.copy_(torch.from_numpy(msg).cuda().reshape(-1))
    wc, cw = guarded(torch, B * pc.n, torch.uint8)
    desc = pc._pc()
    capi.check(capi.lib().cc_product_encode_batch_dev(C.byref(desc), ptr(m), ptr(cw), B, None), "cc_product_encode_batch_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc)
    got = cw.cpu().numpy().reshape(B, pc.n2, pc.n1)
    assert np.array_equal(got, want)
    # every row and every column, the parity row and column among them
    assert syndromes_vanish(r, got.reshape(-1, pc.n1), extended)
    assert syndromes_vanish(c, np.ascontiguousarray(got.transpose(0, 2, 1)).reshape(-1, pc.n2), extended)
    wb, back = guarded(torch, msg.size, torch.uint8)
    capi.check(capi.lib().cc_product_extract_batch_dev(C.byref(desc), ptr(cw), ptr(back), B, None), "cc_product_extract_batch_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wb) and np.array_equal(back.cpu().numpy().reshape(msg.shape), msg)
    assert torch.equal(pc.extract_batch(pc.encode_batch(torch.from_numpy(msg).cuda())).cpu(), torch.from_numpy(msg))


def test_encode_and_extract_over_several_trips_of_the_row_kernel():
    """eBCH(8,4)^2 with an odd number of blocks, three times 32 per compute unit and 77 more: the row kernel that appends
    (encode) or drops (extract) the parity bit walks 4 B and then 8 B rows, 16 rows a workgroup and at most 8 workgroups per
    compute unit, so both launches make more than two trips and the last is partial -- rows that are not live next to
    rows that shuffle.  Every block against the helper construction of one of 256 distinct messages."""
    import torch
    r, c = handles((3, 1), (3, 1))
    pc = cc.product_code(r, c, extended=True)
    rows = M.decoder(3, 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 3 * 32 * cus + 77
    per_trip = 16 * 8 * cus
    assert B % 2 == 1 and 4 * B > 2 * per_trip and (4 * B) % per_trip and (8 * B) % per_trip
    rng = np.random.default_rng(79)
    few_msg = ((rng.choice(1 << 16, 256, replace=False)[:, None] >> np.arange(16)[None, :]) & 1).astype(np.uint8).reshape(256, 4, 4)
    few = encode_blocks(rows, rows, few_msg, True)
    idx = rng.integers(0, 256, B)
    msg, want = few_msg[idx], few[idx]
    wm, m = guarded(torch, msg.size, torch.uint8)
    m.copy_(torch.from_numpy(msg).cuda().reshape(-1))
    wc, cw = guarded(torch, B * pc.n, torch.uint8)
    desc = pc._pc()
    capi.check(capi.lib().cc_product_encode_batch_dev(C.byref(desc), ptr(m), ptr(cw), B, None), "cc_product_encode_batch_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc) and guards_intact(torch, wm)
    got = cw.cpu().numpy().reshape(B, pc.n2, pc.n1)
    differ = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert differ.size == 0, ("blocks that differ", differ[:8], differ.size)
    assert syndromes_vanish(r, got.reshape(-1, pc.n1), True)
    assert syndromes_vanish(c, np.ascontiguousarray(got.transpose(0, 2, 1)).reshape(-1, pc.n2), True)
    wb, back = guarded(torch, msg.size, torch.uint8)
    capi.check(capi.lib().cc_product_extract_batch_dev(C.byref(desc), ptr(cw), ptr(back), B, None), "cc_product_extract_batch_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wb) and guards_intact(torch, wc)
    assert np.array_equal(back.cpu().numpy().reshape(msg.shape), msg)


# ---- channel ----
CHANNEL =[((3, 1), (4, 1), False, 300), ((6, 2), (6, 2), True, 40)]  # 15 x 7 and 64 x 64 blocks


@pytest.mark.parametrize("rq_rt,cq_ct,extended,blocks", CHANNEL)
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_channel_against_the_float64_model(rq_rt, cq_ct, extended, blocks, random_codewords):
    pc = cc.product_code(*handles(rq_rt, cq_ct), extended=extended)
    seed, first, ebno = 0x1234567890, (1 << 33) + 5, 3.0
    got = pc.channel(ebno, seed, first, blocks, random_codewords)
    y, sent = got["y"].cpu().numpy(), got["sent"].cpu().numpy()
    # the blocks sent: the message bits of frame g of a code with l = k1 k2, through the helper construction
    if random_codewords:
        msg = bch_message_bits(seed, first, blocks, pc.l).reshape(blocks, pc.k2, pc.k1)
        want = encode_blocks(M.decoder(*rq_rt), M.decoder(*cq_ct), msg, extended)
        assert want.any()
    else:
        want = np.zeros((blocks, pc.n2, pc.n1), np.uint8)
    assert np.array_equal(sent, want)
    sigma = float(np.float32(pc.sigma(ebno)))
    rate = pc.k1 * pc.k2 / pc.n
    assert abs(pc.sigma(ebno) - 1.0 / np.sqrt(2.0 * rate * 10.0 ** (ebno / 10.0))) < 1e-12
    ref = awgn_model.awgn_reference(pc.n, sigma, seed, first, blocks, want.reshape(blocks, -1))
    worst = float(np.abs(y.reshape(blocks, -1) - ref).max())
    print("channel", pc.to_string(), "max |y - ref|", worst, "tau", tau(sigma))
    assert worst <= tau(sigma)
    # a sharded draw equals the whole
    cut = blocks // 3
    a, b = pc.channel(ebno, seed, first, cut, random_codewords), pc.channel(ebno, seed, first + cut, blocks - cut, random_codewords)
    assert np.array_equal(np.concatenate([a["y"].cpu().numpy(), b["y"].cpu().numpy()]).view(np.uint32), y.view(np.uint32))
    assert np.array_equal(np.concatenate([a["sent"].cpu().numpy(), b["sent"].cpu().numpy()]), sent)


# ---- Monte-Carlo ----
def counted(out, status, sent, y):
    """the counters of the blocks given, by the definitions of the header"""
    B = out.shape[0]
    wrong = (out != sent).reshape(B, -1).sum(axis=1)
    failed = (status != M.FRAME_OK).any(axis=1)
    c = np.zeros(capi.MC_NCOUNTERS, np.int64)
    c[capi.MC_FRAMES] = B
    c[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    c[capi.MC_BIT_ERRORS] = int(wrong.sum())
    c[capi.MC_FAILURES] = int(failed.sum())
    c[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    c[capi.MC_CHANNEL_BIT_ERRORS] = int(((y < 0) != (sent != 0)).sum())
    return c


def mc(pc, halves, ebno, seed, first, blocks, random_codewords=True, p=P):
    return ProductBackend(pc, p, ALPHA[:halves], BETA[:halves], random_codewords).run(ebno, seed, first, blocks).cpu().numpy()


@pytest.mark.parametrize("rq_rt,cq_ct,ebno,blocks", [((4, 1), (4, 1), 3.0, 512), ((5, 3), (5, 3), 2.0, 64)],
                         ids=["15_11x15_11", "31_16x31_16"])
@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_counters_against_channel_model_and_count(rq_rt, cq_ct, ebno, blocks, random_codewords):
    """BCH(15,11)^2 is the issue's case; a perfect code never fails, so BCH(31,16)^2 (t = 3) is there for the failures"""
    pc = cc.product_code(*handles(rq_rt, cq_ct))
    seed = 2026
    ch = pc.channel(ebno, seed, 0, blocks, random_codewords)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    steps = model_steps(M.decoder(*rq_rt), M.decoder(*cq_ct), y, False)
    for halves in (4, 3):
        last = steps[halves - 1]
        expect = counted(last["out"], last["status"], sent, y)
        got = mc(pc, halves, ebno, seed, 0, blocks, random_codewords)
        assert np.array_equal(got, expect), (halves, got[:8], expect[:8])
        assert expect[capi.MC_WORD_ERRORS] > 0 and got[capi.MC_ITER_SUM] == 0 and not got[capi.MC_ITER_HIST:].any()
        assert expect[capi.MC_FAILURES] > 0 or rq_rt[1] == 1
    cut = blocks // 3
    shards = mc(pc, 4, ebno, seed, 0, cut, random_codewords) + mc(pc, 4, ebno, seed, cut, blocks - cut, random_codewords)
    assert np.array_equal(shards, mc(pc, 4, ebno, seed, 0, blocks, random_codewords))


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_count_walks_more_than_64_status_entries_of_a_block(random_codewords):
    """BCH(127,120) x BCH(15,7) at p = 0: after two half-iterations a block has 127 status entries, the columns decoded
    with the t = 2 code, which does fail -- the count kernel's second trip over a block's entries, a partial one of 63.
    After one half-iteration there are 15.  Eb/N0 and seed were chosen with the model on the CPU so that some blocks fail
    at entries >= 64 alone and some at entries < 64 alone (13 and 17 of 64 on awgn_model's channel values); a count that
    stops after the first 64 entries gets CC_MC_FAILURES and CC_MC_UNDETECTED wrong."""
    rq_rt, cq_ct, ebno, seed, blocks = (7, 1), (4, 2), 5.0, 2027, 64
    pc = cc.product_code(*handles(rq_rt, cq_ct))
    ch = pc.channel(ebno, seed, 0, blocks, random_codewords)
    y, sent = ch["y"].cpu().numpy(), ch["sent"].cpu().numpy()
    assert bool(sent.any()) == random_codewords
    steps = model_steps(M.decoder(*rq_rt), M.decoder(*cq_ct), y, False, p=0, alpha=ALPHA[:2], beta=BETA[:2])
    assert steps[0]["status"].shape == (blocks, 15) and steps[1]["status"].shape == (blocks, 127)
    bad = steps[1]["status"] != M.FRAME_OK
    early, late = bad[:, :64].any(axis=1), bad[:, 64:].any(axis=1)
    print("blocks failing at entries >= 64 alone", int((late & ~early).sum()), "at entries < 64 alone", int((early & ~late).sum()))
    assert (late & ~early).any() and (early & ~late).any()
    for halves in (2, 1):
        last = steps[halves - 1]
        expect = counted(last["out"], last["status"], sent, y)
        got = mc(pc, halves, ebno, seed, 0, blocks, random_codewords, p=0)
        assert np.array_equal(got, expect), (halves, got[:8], expect[:8])
    assert expect[capi.MC_FAILURES] == 0  # (one half-iteration: a full-length t = 1 code decodes every word)


@pytest.mark.parametrize("random_codewords", [True, False], ids=["random", "zero"])
def test_mc_count_of_several_blocks_per_wavefront(random_codewords):
    """BCH(7,4)^2 with three times as many blocks as the count kernel's largest grid has wavefronts (8 workgroups of four
    per compute unit) and 77 more, one chunk: every wavefront sums three or four blocks in registers before its atomics.
    Want = the composition on the device (the decode call is held to the model by the tests above): channel, the decode
    call without ext, the counter definitions.  A perfect code has no failed word, so CC_MC_FAILURES is zero here and
    every wrong block undetected.  Three shards of unequal size sum to the whole."""
    import torch
    pc = cc.product_code(*handles((3, 1), (3, 1)))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    blocks = 3 * 32 * cus + 77
    assert blocks * pc.n < 1 << 24  # one chunk
    seed, first, ebno, halves = 2028, (1 << 33) + 5, 2.0, 3
    ch = pc.channel(ebno, seed, first, blocks, random_codewords)
    assert bool(ch["sent"].any()) == random_codewords
    res = pc.correct_batch(ch["y"], P, ALPHA[:halves], BETA[:halves], ext=False)
    wrong = (res["out"] != ch["sent"]).reshape(blocks, -1).sum(dim=1)
    failed = (res["status"] != 0).any(dim=1)
    want = np.zeros(capi.MC_NCOUNTERS, np.int64)
    want[capi.MC_FRAMES] = blocks
    want[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())
    want[capi.MC_BIT_ERRORS] = int(wrong.sum())
    want[capi.MC_FAILURES] = int(failed.sum())
    want[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())
    want[capi.MC_CHANNEL_BIT_ERRORS] = int(((ch["y"] < 0) != (ch["sent"] != 0)).sum())
    print("counters", want[:7])
    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_UNDETECTED] > 0 and want[capi.MC_BIT_ERRORS] > want[capi.MC_WORD_ERRORS]
    wc, counters = guarded(torch, capi.MC_NCOUNTERS, torch.int64)
    counters.zero_()
    desc = pc._pc(P, ALPHA[:halves], BETA[:halves])
    rc = capi.lib().cc_mc_run_product_dev(C.byref(desc), ebno, seed, first, blocks, int(random_codewords), ptr(counters), None)
    capi.check(rc, "cc_mc_run_product_dev")
    torch.cuda.synchronize()
    assert guards_intact(torch, wc)
    assert np.array_equal(counters.cpu().numpy(), want), (counters.cpu().numpy()[:8], want[:8])
    a, b = blocks // 5, blocks // 2 + 1
    shards = sum(mc(pc, halves, ebno, seed, first + lo, hi - lo, random_codewords) for lo, hi in ((0, a), (a, b), (b, blocks)))
    assert np.array_equal(shards, want)


def test_mc_across_a_chunk_boundary_equals_the_composition():
    """chunks of 100 blocks (the value is read once, so in a process of its own): 512 blocks cross five boundaries"""
    run_child(
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "from channelcoding_amd import capi\n"
        "from channelcoding_amd.montecarlo import ProductBackend\n"
        "mk = lambda q, t: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())\n"
        "pc = cc.product_code(mk(5, 3), mk(5, 3))\n"
        "a, b = (0.0, 0.3, 0.5), (0.2, 0.4, 0.6)\n"
        "for rc in (True, False):\n"
        "    got = ProductBackend(pc, 4, a, b, rc).run(2.0, 31, 7, 512).cpu().numpy()\n"
        "    ch = pc.channel(2.0, 31, 7, 512, rc)\n"
        "    res = pc.correct_batch(ch['y'], 4, a, b, ext=False)\n"
        "    wrong = (res['out'] != ch['sent']).reshape(512, -1).sum(dim=1)\n"
        "    failed = (res['status'] != 0).any(dim=1)\n"
        "    want = np.zeros(capi.MC_NCOUNTERS, np.int64)\n"
        "    want[capi.MC_FRAMES] = 512\n"
        "    want[capi.MC_WORD_ERRORS] = int((failed | (wrong > 0)).sum())\n"
        "    want[capi.MC_BIT_ERRORS] = int(wrong.sum())\n"
        "    want[capi.MC_FAILURES] = int(failed.sum())\n"
        "    want[capi.MC_UNDETECTED] = int((~failed & (wrong > 0)).sum())\n"
        "    want[capi.MC_CHANNEL_BIT_ERRORS] = int(((ch['y'] < 0) != (ch['sent'] != 0)).sum())\n"
        "    assert np.array_equal(got, want), (got[:8], want[:8])\n"
        "    assert want[capi.MC_WORD_ERRORS] > 0 and want[capi.MC_FAILURES] > 0\n"
        "print('PRODUCT MC OK')\n", {"CC_AMD_PRODUCT_MC_CHUNK_VALUES": str(100 * 961)}, "PRODUCT MC OK")


def test_mc_four_half_iterations_beat_one_on_the_same_channel():
    pc = cc.product_code(*handles((6, 3), (6, 3)))
    one, four = mc(pc, 1, 2.5, 9, 0, 1024), mc(pc, 4, 2.5, 9, 0, 1024)
    assert one[capi.MC_FRAMES] == four[capi.MC_FRAMES] == 1024
    assert one[capi.MC_CHANNEL_BIT_ERRORS] == four[capi.MC_CHANNEL_BIT_ERRORS] > 0
    print("block errors after one half-iteration", one[capi.MC_WORD_ERRORS], "after four", four[capi.MC_WORD_ERRORS])
    assert four[capi.MC_WORD_ERRORS] < one[capi.MC_WORD_ERRORS]
