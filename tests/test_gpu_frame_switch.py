"""The frame switch of the diagonal min-sum kernel (minsum_diag_impl.hpp, the tail of the iteration loop): a lane group
whose frame has ended makes the frame's result from the registers the stop scan left (cs' and y of its owned columns)
instead of reading the cells back, and sets the next frame up from the staged channel values in one batch behind one
wait.  What that can get wrong: a result taken from the wrong iteration's registers when the groups of a wavefront end
their frames in different iterations or together; the branch without L; the column beyond the frame (lane 15, c = 15 for
n = 255); an erased position, whose zero must reach the cell at set-up and the scan's y of the next frame; the
message-free kernel, which runs the switch every iteration, with the stop scan and without it.
Bar: bit for bit in out, L, iters and status against the generic kernel (a process of its own) and the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from checkers import BCH, O0, O1, O2, Oracle, awgn_llr
from test_gpu_row_groups import TAGS, _check, _generic

import channelcoding_amd as cc
from channelcoding_amd import _capi as capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL_TAGS = dict(TAGS, SCMS2=("self_correcting_2_min_sum_tag", {}))

# test_gpu_row_groups._CHILD for any primitive BCH code: a batch names q and t too
_CHILD = """
import json, sys
import numpy as np
import channelcoding_amd as cc
spec = json.load(open(sys.argv[1]))
data = np.load(sys.argv[2])
out = {}
for k, b in enumerate(spec):
    tag = getattr(cc, b["tag"])(b["iterations"], **{a: tuple(v) for a, v in b["kw"].items()})
    code = cc.primitive_bch(b["q"], cc.errors(b["t"]), tag, stop_rule=b["stop"])
    res = code.correct_batch(data[b["y"]], erasures=b["erasures"], want_L=True)
    out["kernel%d" % k] = code.kernel_info()["kernel"]
    for key in ("out", "L", "iters", "status"):
        out["%s%d" % (key, k)] = res[key]
np.savez(sys.argv[3], **out)
"""


def _generic_any(tmp_path, spec, data):
    sp, dp, op = tmp_path / "spec.json", tmp_path / "in.npz", tmp_path / "out.npz"
    sp.write_text(json.dumps(spec))
    np.savez(dp, **data)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(sp), str(dp), str(op)], cwd=ROOT,
                       env=dict(os.environ, CC_AMD_FORCE_GENERIC="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = np.load(op)
    for k in range(len(spec)):
        assert str(out["kernel%d" % k]).startswith("minsum_generic_kernel")
    return out


def _batch(name, q, t, iterations, stop, yk, erasures=None):
    return {"tag": ALL_TAGS[name][0], "kw": ALL_TAGS[name][1], "q": q, "t": t, "iterations": iterations, "stop": stop,
            "y": yk, "erasures": erasures}


def _check_any(o, b, y, gen, k, want_L, what):
    """Batch b (a _batch) through the diagonal kernel, with L or without: against batch k of the generic kernel's
    results and against the oracle."""
    tag = getattr(cc, b["tag"])(b["iterations"], **b["kw"])
    code = cc.primitive_bch(b["q"], cc.errors(b["t"]), tag, stop_rule=b["stop"])
    assert code.kernel_info()["kernel"].startswith("minsum_diag_kernel"), code.kernel_info()["kernel"]
    res = code.correct_batch(y, erasures=b["erasures"], want_L=want_L)
    ye = y.copy()  # an erased position enters the decoder as channel value 0 (cyclic.h:259-262)
    for f, e in enumerate(b["erasures"] or ()):
        ye[f, e] = 0.0
    ob, oL, oit, ost = o.minsum(tag.alg - capi.ALG_MS, b["iterations"], ye, alpha=tag.alpha, beta=tag.beta, stop=b["stop"],
                                fast=True)
    for key, want in (("out", ob), ("L", oL), ("iters", oit), ("status", ost)):
        if key == "L" and not want_L:
            assert res.get("L") is None
            continue
        got = np.asarray(res[key])
        assert np.array_equal(got.astype(want.dtype), want), (what, key, "oracle")
        assert np.array_equal(got, gen["%s%d" % (key, k)]), (what, key, "generic kernel")
    return res


def _mixed(rng, o, B):
    """B frames, 3.5 dB and 6 dB in turn: neighbours in a wavefront end their frames after 1 .. 20 iterations"""
    y = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 3.5)
    y[1::2] = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 6.0)[1::2]
    return y


@pytest.mark.parametrize("name", sorted(ALL_TAGS))
def test_groups_end_apart_and_together(tmp_path, name):
    """BCH(255,231), B = 1, 3, 5 and 67 frames of 3.5 dB and 6 dB mixed in one batch, 20 iterations, stop rules O1 and
    O2, with L requested and without (both instantiations of the result path)."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(4800 + len(name))
    ys = {"y%d" % B: _mixed(rng, o, B) for B in (1, 3, 5, 67)}
    cases = [(yk, stop) for yk in sorted(ys) for stop in (O1, O2)]
    spec = [_batch(name, 8, 3, 20, stop, yk) for yk, stop in cases]
    gen = _generic_any(tmp_path, spec, ys)
    seen = set()
    for k, (yk, stop) in enumerate(cases):
        for want_L in (True, False):
            res = _check_any(o, spec[k], ys[yk], gen, k, want_L, (name, yk, stop, want_L))
            seen.update(np.asarray(res["iters"]).tolist())
    assert 1 in seen and 20 in seen, sorted(seen)


@pytest.mark.parametrize("iterations,stop", [(1, O1), (1, O2), (20, O0)])
def test_message_free_kernel(tmp_path, iterations, stop):
    """One iteration per frame (Iterations = 1: with the stop scan; stop rule O0 "as shipped" with 20 iterations: without
    it), B = 5 and 67, L requested: the switch runs every iteration for every lane group."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(4810 + iterations + stop)
    ys = {"y%d" % B: _mixed(rng, o, B) for B in (5, 67)}
    spec = [_batch("MS", 8, 3, iterations, stop, yk) for yk in sorted(ys)]
    gen = _generic_any(tmp_path, spec, ys)
    for k, yk in enumerate(sorted(ys)):
        _check_any(o, spec[k], ys[yk], gen, k, True, ("single", iterations, stop, yk))


def test_erasures_reach_the_cell(tmp_path):
    """16 frames at 4 dB, MS<3>, eight of them with 1 .. 64 erased positions, position 254 among them; then the same 16
    frames three times over with the lists moved to the frames 32 .. 47 (48 frames, B >= 33: three workgroups' worth), so
    that frames with erasures come behind frames without.  (The launcher starts a workgroup per 16 frames while compute
    units are free, so here every lane group still has one frame; a frame with erasures that FOLLOWS one without on the
    same lane group is in test_next_frame_set_up.)"""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(480)
    y = awgn_llr(rng, np.zeros((16, o.n), np.uint8), o.l / o.n, 4.0)
    erasures = [sorted(rng.choice(o.n - 1, 2 ** (f // 2) - 1, replace=False).tolist() + [254]) if f % 2 == 0 and f < 14 else []
                for f in range(16)]
    erasures[15] = sorted(rng.choice(o.n - 1, 3, replace=False).tolist())
    assert [len(e) for e in erasures if e] == [1, 2, 4, 8, 16, 32, 64, 3] and erasures[0] == [254]
    y3 = np.tile(y, (3, 1))
    er3 = [[] for _ in range(32)] + erasures
    for stop_k, stop in enumerate((O1, O2)):
        spec = [{"tag": TAGS["MS"][0], "kw": {}, "iterations": 3, "stop": stop, "y": "y", "erasures": erasures},
                {"tag": TAGS["MS"][0], "kw": {}, "iterations": 3, "stop": stop, "y": "y3", "erasures": er3}]
        (tmp_path / str(stop_k)).mkdir()
        gen = _generic(tmp_path / str(stop_k), spec, {"y": y, "y3": y3})
        _check(o, "MS", 3, stop, y, erasures, gen, 0, ("erasures", stop))
        _check(o, "MS", 3, stop, y3, er3, gen, 1, ("erasures behind none", stop))


def _last_column_negative(rng, o, B):
    """frames whose last real column n - 1 carries the only negative channel value, small enough to be corrected or not"""
    y = np.abs(awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 5.0)) + np.float32(0.25)
    y[:, o.n - 1] = -np.abs(y[:, o.n - 1]) * np.exp2(rng.integers(-3, 4, B)).astype(np.float32)
    return y.astype(np.float32)


@pytest.mark.parametrize("q,t", [(8, 3), (6, 2), (5, 1)])
def test_the_column_beyond_the_frame(tmp_path, q, t):
    """n = 255, 63 and 31 are one short of the lanes' columns: the last lane's last column lies beyond the frame and must
    neither be stored nor disturb the stop test.  Frames whose last real column n - 1 carries the only negative channel
    value, over seven binades, B = 9 and 67; one iteration (where two frames in three leave with a negative L in column
    n - 1 alone), three, and 20.  BCH(63,51) is a
    geometry of 8 lanes per frame with an empty last slot in some lanes, BCH(31,26) stages its frames dword by dword."""
    o = Oracle(BCH, q, t)
    rng = np.random.default_rng(4820 + q)
    ys = {"y%d" % B: _last_column_negative(rng, o, B) for B in (9, 67)}
    cases = [(yk, it) for yk in sorted(ys) for it in (1, 3, 20)]
    spec = [_batch("MS", q, t, it, O2, yk) for yk, it in cases]
    gen = _generic_any(tmp_path, spec, ys)
    for k, (yk, it) in enumerate(cases):
        res = _check_any(o, spec[k], ys[yk], gen, k, True, ("beyond", q, yk, it))
        if it == 1:  # most of these frames leave with column n - 1 as their only negative L
            L = np.asarray(res["L"])
            only = (L[:, o.n - 1] < 0) & (L[:, : o.n - 1] > 0).all(axis=1)
            assert 2 * int(only.sum()) > len(L), (q, yk, int(only.sum()))


def test_next_frame_set_up(tmp_path):
    """A lane group takes a second frame only in a call of more frames than the resident workgroups hold at once (16 per
    workgroup, two workgroups per compute unit for BCH(255,231)): 16 x 2 x CUs + 1040 frames of 6 dB, every eighth at
    3.5 dB, MS<20>, stop rule O2, with L and without.  The frames behind the first wave carry erasure lists (1 .. 8
    positions, every fourth frame), so a frame with erasures follows one without on the same lane group."""
    import torch
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(4830)
    first = 16 * 2 * torch.cuda.get_device_properties(0).multi_processor_count
    B = first + 1040
    y = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 6.0)
    y[::8] = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 3.5)[::8]
    erasures = [[] for _ in range(B)]
    for f in range(first, B, 4):
        erasures[f] = sorted(rng.choice(o.n, 1 + (f // 4) % 8, replace=False).tolist())
    spec = [_batch("MS", 8, 3, 20, O2, "y", erasures)]
    gen = _generic_any(tmp_path, spec, {"y": y})
    for want_L in (True, False):
        _check_any(o, spec[0], y, gen, 0, want_L, ("second frame", want_L))
