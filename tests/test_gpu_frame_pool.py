"""The general diagonal min-sum kernel of the 16-lanes-per-frame geometries draws its frames from one pool per call
(sharded counters in the call's workspace, minsum_diag_impl.hpp); the others keep a per-workgroup deal.  Whatever
order the lane groups draw in, every frame must be decoded exactly once and written at its own index: batch sizes
below and around the number of lane groups, calls back to back on one handle (each call's counters start from zero),
calls on two streams at once, and the operating points where iteration counts spread the most.  Bar: bit for bit against the generic kernel (CC_AMD_FORCE_GENERIC=1, a process of its own) and
against the oracle on a sample."""
import os
import subprocess
import sys

import numpy as np
import pytest

from checkers import BCH, O2, Oracle, awgn_llr

import channelcoding_amd as cc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# decodes y.npy in a child process and saves out / iters / status / L (argv: q t iterations y.npy out.npz)
_CHILD = """
import sys
import numpy as np
import channelcoding_amd as cc
q, t, iters = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
code = cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(iters))
res = code.correct_batch(np.load(sys.argv[4]), want_L=True)
np.savez(sys.argv[5], kernel=code.kernel_info()["kernel"], **res)
"""


def _generic(tmp_path, q, t, iters, y, tag):
    yp, op = tmp_path / ("y_%s.npy" % tag), tmp_path / ("out_%s.npz" % tag)
    np.save(yp, y)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(q), str(t), str(iters), str(yp), str(op)], cwd=ROOT,
                       env=dict(os.environ, CC_AMD_FORCE_GENERIC="1"), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(np.load(op))
    assert str(out.pop("kernel")).startswith("minsum_generic_kernel")
    return out


def _same(a, b, tag):
    for key in ("out", "iters", "status", "L"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), (tag, key)


def _oracle(o, iters, y, res, idx, tag):
    ob, oL, oit, ost = o.minsum(0, iters, y[idx], stop=O2, fast=True)
    assert np.array_equal(res["out"][idx], ob), tag
    assert np.array_equal(res["L"][idx], oL), tag
    assert np.array_equal(res["iters"][idx].astype(np.uint32), oit), tag
    assert np.array_equal(res["status"][idx], ost), tag


@pytest.mark.parametrize("q,t,iters", [(8, 3, 20), (6, 3, 10)])  # 16 lanes per frame (pool), 8 (per-workgroup deal)
def test_pool_ragged_batches(tmp_path, q, t, iters):
    """Batches smaller than one workgroup's lane groups (16 / 32), not a multiple of them, and grids of fewer
    workgroups than shards: every frame against the oracle, and all of them against the generic kernel."""
    o = Oracle(BCH, q, t)
    code = cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(iters))
    assert code.kernel_info()["kernel"].startswith("minsum_diag_kernel")
    rng = np.random.default_rng(q * 10 + t)
    sizes = (1, 3, 7, 15, 17, 31, 33, 100, 257, 1001)
    ys = [awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, 3.5) for B in sizes]
    allres = []
    for B, y in zip(sizes, ys):
        res = code.correct_batch(y, want_L=True)
        _oracle(o, iters, y, res, np.arange(B), ("B", B))
        allres.append(res)
    gen = _generic(tmp_path, q, t, iters, np.concatenate(ys), "ragged")
    at = 0
    for B, res in zip(sizes, allres):
        _same(res, {k: v[at:at + B] for k, v in gen.items()}, ("B", B))
        at += B


@pytest.mark.parametrize("ebno", [2.0, 4.0, 6.0])
@pytest.mark.parametrize("log2b", [16, 18])  # 2^18 frames take the two-pass route (a pool per kernel launch)
def test_pool_operating_points(tmp_path, ebno, log2b):
    """The headline code at 2 / 4 / 6 dB (every frame 20 iterations / the headline point / the widest spread of
    iteration counts): bit for bit against the generic kernel, and a strided sample against the oracle."""
    o = Oracle(BCH, 8, 3)
    code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
    rng = np.random.default_rng(int(ebno * 10) + log2b)
    B = 1 << log2b
    y = awgn_llr(rng, np.zeros((B, o.n), np.uint8), o.l / o.n, ebno)
    res = code.correct_batch(y, want_L=True)
    _same(res, _generic(tmp_path, 8, 3, 20, y, "op"), ("ebno", ebno))
    _oracle(o, 20, y, res, np.arange(0, B, B // 256), ("ebno", ebno))


def _dev_call(code, ty):
    import torch
    r = code.correct_batch(ty, want_L=True)
    return {k: v for k, v in r.items() if isinstance(v, torch.Tensor)}


def _host(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def test_pool_back_to_back_and_concurrent_calls():
    """Calls enqueued back to back on one handle and one stream (each call's counters are zeroed on the stream, so a
    later call must not see an earlier call's draws), then two handles and one handle on two streams at once: each
    result equals the one of a call made alone."""
    import torch
    rng = np.random.default_rng(5)
    codes = [cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20)), cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))]
    sizes = (5000, 777, 20000, 64)
    ys = [torch.from_numpy(awgn_llr(rng, np.zeros((B, 255), np.uint8), 231 / 255, e)).cuda()
          for B, e in zip(sizes, (4.0, 3.0, 5.0, 6.0))]
    alone = []
    for y in ys:
        alone.append(_host(_dev_call(codes[0], y)))
        torch.cuda.synchronize()
    # back to back, one handle, one stream, no synchronisation in between
    outs = [_dev_call(codes[0], y) for y in ys]
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(alone, outs)):
        _same(a, _host(b), ("back to back", k))
    # two streams at once: two handles, then one handle
    for pair in ((codes[0], codes[1]), (codes[0], codes[0])):
        s = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        got = [None] * len(ys)
        for k, y in enumerate(ys):
            with torch.cuda.stream(s[k % 2]):
                got[k] = _dev_call(pair[k % 2], y)
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(alone, got)):
            _same(a, _host(b), ("two streams", k))
