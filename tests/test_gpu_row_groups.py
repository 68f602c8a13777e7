"""The four-row body of the diagonal min-sum kernel (minsum_diag_impl.hpp, DIAG_ROWS_FOUR*): four rows share one
transposed reduction that leaves row b's (min1, min2, parity) in bank b of the frame's 16 lanes, and each row's back
fetches its bank's values with a row_newbcast move.  The stages treat the four banks and the four rows of a group
differently, so every edge must be its row's unique minimum once, the second minimum must be found with its multiplicity
wherever its holders sit, and zeros must keep their sign through Y = (m1 ^ m2) | parity << 31; lane groups of a wavefront
switch frames in the middle of each other's iterations.  Bar: bit for bit in out, L, iters and status against the generic
kernel (CC_AMD_FORCE_GENERIC=1, a process of its own) and against the oracle on every frame."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from checkers import BCH, O1, O2, Oracle, awgn_llr

import channelcoding_amd as cc
from channelcoding_amd import _capi as capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# variants that take the four-row body on the headline geometry (diag_row_body in csrc/cc_internal.hpp), with their
# usual parameters: name -> (tag class, keyword arguments besides the iterations)
TAGS = {
    "MS": ("min_sum_tag", {}),
    "NMS": ("normalized_min_sum_tag", {"ratio": (4, 5)}),
    "OMS": ("offset_min_sum_tag", {"ratio": (1, 100)}),
    "2DNMS": ("normalized_2d_min_sum_tag", {"alpha": (8, 10), "beta": (9, 10)}),
}

# decodes the batches of spec.json in a child process (argv: spec.json in.npz out.npz); a batch: tag, iterations, stop
# rule, key of its channel values in in.npz, per-frame erasure lists or null
_CHILD = """
import json, sys
import numpy as np
import channelcoding_amd as cc
spec = json.load(open(sys.argv[1]))
data = np.load(sys.argv[2])
out = {}
for k, b in enumerate(spec):
    tag = getattr(cc, b["tag"])(b["iterations"], **{a: tuple(v) for a, v in b["kw"].items()})
    code = cc.primitive_bch(8, cc.errors(3), tag, stop_rule=b["stop"])
    res = code.correct_batch(data[b["y"]], erasures=b["erasures"], want_L=True)
    out["kernel%d" % k] = code.kernel_info()["kernel"]
    for key in ("out", "L", "iters", "status"):
        out["%s%d" % (key, k)] = res[key]
np.savez(sys.argv[3], **out)
"""


def _tag(name, iterations):
    cls, kw = TAGS[name]
    return getattr(cc, cls)(iterations, **kw)


def _generic(tmp_path, spec, data):
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


def _check(o, name, iterations, stop, y, erasures, gen, k, what):
    """One batch through the four-row body: against batch k of the generic kernel's results and against the oracle."""
    tag = _tag(name, iterations)
    code = cc.primitive_bch(8, cc.errors(3), tag, stop_rule=stop)
    assert "four-row" in code.kernel_info()["kernel"], code.kernel_info()["kernel"]
    res = code.correct_batch(y, erasures=erasures, want_L=True)
    ye = y.copy()  # an erased position enters the decoder as channel value 0 (cyclic.h:259-262)
    for f, e in enumerate(erasures or ()):
        ye[f, e] = 0.0
    ob, oL, oit, ost = o.minsum(tag.alg - capi.ALG_MS, iterations, ye, alpha=tag.alpha, beta=tag.beta, stop=stop, fast=True)
    for key, want in (("out", ob), ("L", oL), ("iters", oit), ("status", ost)):
        got = np.asarray(res[key])
        assert np.array_equal(got.astype(want.dtype), want), (what, key, "oracle")
        assert np.array_equal(got, gen["%s%d" % (key, k)]), (what, key, "generic kernel")
    return res


def test_where_the_minimum_sits(tmp_path):
    """BCH(255,231) MS<3>.  255 frames: frame c has |y| = 1 everywhere except 0.25 in column c, so every edge of column c
    is its row's unique minimum in the first iteration -- each (row of a group, bank, lane, slot) once.  64 frames with
    two equal smallest magnitudes in random columns: the second minimum with multiplicity, its holders in one lane, in
    two lanes of a bank, in two banks.  16 frames quantised to multiples of 0.25 with exact zeros, and 8 frames with
    erasure lists: m1 = m2 = 0 and the sign of zero through Y."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(46)
    n = o.n
    sign = lambda shape: np.where(rng.integers(0, 2, shape) == 1, -1.0, 1.0)
    y_one = sign((n, n))
    y_one[np.arange(n), np.arange(n)] *= 0.25
    y_two = sign((64, n)) * rng.uniform(1.0, 2.0, (64, n))
    for f in range(64):
        y_two[f, rng.choice(n, 2, replace=False)] = sign(2) * 0.5
    y_q = np.round((1.0 + 0.8 * rng.standard_normal((16, n))) * 4.0) / 4.0 + 0.0
    assert (y_q == 0.0).sum() >= 16
    y_e = awgn_llr(rng, np.zeros((8, n), np.uint8), o.l / o.n, 4.0)
    y = np.concatenate([y_one, y_two, y_q, y_e]).astype(np.float32)
    erasures = [[] for _ in range(len(y) - 8)] + [sorted(rng.choice(n, 1 + f, replace=False).tolist()) for f in range(8)]
    spec = [{"tag": TAGS["MS"][0], "kw": {}, "iterations": 3, "stop": O2, "y": "y", "erasures": erasures}]
    gen = _generic(tmp_path, spec, {"y": y})
    _check(o, "MS", 3, O2, y, erasures, gen, 0, "minimum")


@pytest.mark.parametrize("name", sorted(TAGS))
def test_groups_out_of_phase(tmp_path, name):
    """257 frames (17 workgroups, the last one ragged) at 3.5 dB and at 6 dB, 20 iterations, stop rules O1 and O2:
    iteration counts spread from 1 to 20, so the lane groups of a wavefront start their frames in the middle of each
    other's iterations -- the row groups of one frame meet every phase of the other three."""
    o = Oracle(BCH, 8, 3)
    rng = np.random.default_rng(4600 + len(name))
    ys = {"y%d" % k: awgn_llr(rng, np.zeros((257, o.n), np.uint8), o.l / o.n, e) for k, e in enumerate((3.5, 6.0))}
    cases = [(yk, stop) for yk in sorted(ys) for stop in (O1, O2)]
    spec = [{"tag": TAGS[name][0], "kw": TAGS[name][1], "iterations": 20, "stop": stop, "y": yk, "erasures": None}
            for yk, stop in cases]
    gen = _generic(tmp_path, spec, ys)
    seen = set()
    for k, (yk, stop) in enumerate(cases):
        res = _check(o, name, 20, stop, ys[yk], None, gen, k, (name, yk, stop))
        seen.update(np.asarray(res["iters"]).tolist())
    assert min(seen) <= 1 and max(seen) == 20 and len(seen) >= 8, sorted(seen)
