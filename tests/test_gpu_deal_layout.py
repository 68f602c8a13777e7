"""Which LDS address serves an edge, and which do not need serving, in the diagonal min-sum kernel (minsum_diag_impl.hpp):
row 0 of an iteration takes the constant +0.0f for the column sums it continues instead of reading cs' (ROW0_FRESH: it is
the first contributor of every column it touches), and on the geometries of 16 lanes per frame the stop scan reads the
check masks of a lane's 16 columns with four 16-byte reads from a per-lane table (CB128).  What that can get wrong: a
column of row 0 that is not fresh after all (a frame that follows another on the same lane group, either frame parity of
a half-wave, an erased position 0 or 254); a mask that belongs to another column or lane (the stop test then ends a
frame too early or too late: iters and status); the sign of a zero message of row 0; and the geometries that keep the
old paths.
Bar: bit for bit in out, L, iters and status against the generic kernel (a process of its own) and the oracle."""
import numpy as np
import pytest

from checkers import BCH, O0, O1, O2, Oracle, awgn_llr
from test_gpu_frame_switch import ALL_TAGS, _check_any, _generic_any, _mixed

pytestmark = pytest.mark.gpu

TAGS6 = dict(ALL_TAGS, SCMS1=("self_correcting_1_min_sum_tag", {}))
SIZES = (1, 2, 3, 5, 67)


def _batch(name, q, t, iterations, stop, yk, erasures=None):
    """test_gpu_frame_switch._batch over all six variants"""
    return {"tag": TAGS6[name][0], "kw": TAGS6[name][1], "q": q, "t": t, "iterations": iterations, "stop": stop,
            "y": yk, "erasures": erasures}


def _gaps(y, B):
    """B frames in a call of their own leave the other lane groups empty; with B = 1, 2, 3 and 5 each frame parity of a
    half-wave (lane groups 0 / 1 and 2 / 3 of a wavefront) is occupied and left empty in turn"""
    return y[:B]


@pytest.mark.parametrize("name", sorted(TAGS6))
def test_every_variant_every_occupancy(tmp_path, name):
    """BCH(255,231), all six variants, stop rules O1 and O2, B = 1, 2, 3, 5 and 67 frames of 3.5 dB and 6 dB mixed, 20
    iterations, with L requested and without."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(2600 + len(name) + ord(name[0]))
    y67 = _mixed(rng, o, 67)
    ys = {"y%d" % B: _gaps(y67, B) for B in SIZES}
    cases = [(B, stop) for B in SIZES for stop in (O1, O2)]
    spec = [_batch(name, 8, 3, 20, stop, "y%d" % B) for B, stop in cases]
    gen = _generic_any(tmp_path, spec, ys)
    seen = set()
    for k, (B, stop) in enumerate(cases):
        for want_L in (True, False):
            res = _check_any(o, spec[k], ys["y%d" % B], gen, k, want_L, (name, B, stop, want_L))
            seen.update(np.asarray(res["iters"]).tolist())
    assert 1 in seen and 20 in seen, sorted(seen)


@pytest.mark.parametrize("iterations,stop", [(20, O0), (1, O2)])
def test_message_free_kernel(tmp_path, iterations, stop):
    """The message-free kernel under the as-shipped rule (no scan) and as the one-iteration pass under O2 (the scan with
    the per-lane mask table), at the same batch sizes."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(2610 + iterations + stop)
    y67 = _mixed(rng, o, 67)
    ys = {"y%d" % B: _gaps(y67, B) for B in SIZES}
    spec = [_batch("MS", 8, 3, iterations, stop, "y%d" % B) for B in SIZES]
    gen = _generic_any(tmp_path, spec, ys)
    for k, B in enumerate(SIZES):
        _check_any(o, spec[k], ys["y%d" % B], gen, k, True, ("single", iterations, stop, B))


def test_erased_ends_on_both_frame_parities(tmp_path):
    """Six frames at 4 dB, MS<5>, O1 and O2: erasure lists with position 0 (the column only row 0 touches), position 254,
    both, and both among others, on frames of even and odd index -- the two frame parities of a half-wave."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(2620)
    y = awgn_llr(rng, np.zeros((6, o.n), np.uint8), o.l / o.n, 4.0)
    more = sorted(rng.choice(np.arange(1, 254), 5, replace=False).tolist())
    erasures = [[0], [0], [254], [254], [0, 254], sorted([0, 254] + more)]
    for turn, e in enumerate((erasures, erasures[1:] + erasures[:1])):  # every list on the other parity too
        for stop in (O1, O2):
            d = tmp_path / ("%d_%d" % (turn, stop))
            d.mkdir()
            spec = [_batch("MS", 8, 3, 5, stop, "y", e)]
            gen = _generic_any(d, spec, {"y": y})
            _check_any(o, spec[0], y, gen, 0, True, ("erased ends", turn, stop))


def test_second_frame_on_a_lane_group(tmp_path):
    """16 x 2 x CUs + 1040 frames of 6 dB, every eighth at 3.5 dB, MS<20>, O2: lane groups take a second frame, whose
    row 0 must find cs' = 0 where the frame before left its last column sums to the stop scan."""
    import torch
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(2630)
    B = 16 * 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1040
    y = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 6.0)
    y[::8] = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 3.5)[::8]
    spec = [_batch("MS", 8, 3, 20, O2, "y")]
    gen = _generic_any(tmp_path, spec, {"y": y})
    _check_any(o, spec[0], y, gen, 0, True, "second frame")


def _minus_zero_frames(o, rng, B):
    """Frames whose row 0 sends -0.0f into column 0, which no other row touches: channel value 0.0 at two positions of
    row 0's support (the row's two minima are zero, so every message of the row is a zero) and an odd number of
    negative values among the others, column 0 positive: the message to column 0 carries the product of the other
    edges' signs (a zero counts by its sign bit, as in the kernel)."""
    H = o.H()
    sup = np.flatnonzero(H[0])
    assert sup[0] == 0 and H[1:, 0].sum() == 0  # column 0 belongs to row 0 alone
    y = np.abs(awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 5.0)) + np.float32(0.25)
    for f in range(B):
        zeros = rng.choice(sup[1:], 2, replace=False)
        rest = np.setdiff1d(sup[1:], zeros)
        neg = rng.choice(rest, 1 + 2 * int(rng.integers(0, 3)), replace=False)
        y[f, neg] = -y[f, neg]
        y[f, zeros] = 0.0
    return y.astype(np.float32), sup


def test_minus_zero_from_row_0(tmp_path):
    """+0.0f + (-0.0f) is +0.0f, not the message: row 0 keeps its addition.  MS<1> and MS<3>, L compared by bit pattern."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(2640)
    y, sup = _minus_zero_frames(o, rng, 5)
    # first iteration on the CPU: q = y, row 0's message to column 0 = (product of the other edges' signs) x (minimum of
    # the other magnitudes); a zero edge contributes the sign bit of +0.0f
    for f in range(len(y)):
        others = y[f, sup[1:]]
        r0 = np.float32(np.abs(others).min()) * (np.float32(-1.0) if (np.signbit(others).sum() & 1) else np.float32(1.0))
        assert r0 == 0.0 and np.signbit(r0), (f, r0)
    spec = [_batch("MS", 8, 3, it, O2, "y") for it in (1, 3)]
    gen = _generic_any(tmp_path, spec, {"y": y})
    for k, it in enumerate((1, 3)):
        res = _check_any(o, spec[k], y, gen, k, True, ("minus zero", it))
        _, oL, _, _ = o.minsum(0, it, y, stop=O2, fast=True)
        assert np.array_equal(np.asarray(res["L"]).view(np.uint32), oL.view(np.uint32)), ("L bit pattern", it)


@pytest.mark.parametrize("q,t", [(6, 2), (5, 1), (7, 2)])
def test_other_geometries(tmp_path, q, t):
    """BCH(63,51) (empty slots: row 0 keeps its read), BCH(31,26) and BCH(127,113) (8 lanes per frame: the column-linear
    mask table), B = 5 and 67 mixed frames, MS<20>, O1 and O2."""
    o = Oracle(BCH, q, t)
    rng = np.random.default_rng(2650 + q)
    ys = {"y%d" % B: _mixed(rng, o, B) for B in (5, 67)}
    cases = [(yk, stop) for yk in sorted(ys) for stop in (O1, O2)]
    spec = [_batch("MS", q, t, 20, stop, yk) for yk, stop in cases]
    gen = _generic_any(tmp_path, spec, ys)
    for k, (yk, stop) in enumerate(cases):
        _check_any(o, spec[k], ys[yk], gen, k, True, ("geometry", q, yk, stop))
