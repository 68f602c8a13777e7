"""The batch API on a side stream for the two layouts no other test runs there: 16-bit symbols (BCH over GF(2^10),
n = 1023, t = 2) and symbol-interleaved blocks (RS(15,11), interleave=4).  Eight frames each, 0 .. t symbol errors at
positions drawn from a fixed seed, per-frame erasure lists of which two name symbols in error and the others are
empty.  encode, correct, correct in place (blocks), extract and decode_batch on device tensors inside
torch.cuda.stream(...) against the same calls on host arrays, bit for bit, and against what was sent.

decode_batch on host arrays of 16-bit symbols without interleave= hands them to the byte call, which refuses them; the
device result is compared with correct_batch + extract_batch on the host there, which is what decode_batch is."""
import numpy as np
import pytest
import torch

import channelcoding_amd as cc

pytestmark = pytest.mark.gpu
B, I = 8, 4
ERRORS = (0, 2, 1, 2, 0, 1, 2, 1)  # symbol errors of frame f, 0 .. t
ERASED = {1: 2, 6: 1}  # frame -> how many of its symbols in error its erasure list names; the other lists are empty


def frames(code, seed, hi, dtype):
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, hi, (B, code.l)).astype(dtype)
    cw = code.encode_batch(msg)
    rx, per = cw.copy(), []
    for f in range(B):
        pos = sorted(int(p) for p in rng.choice(code.n, ERRORS[f], replace=False))
        for p in pos:
            rx[f, p] ^= 1 if hi == 2 else int(rng.integers(1, hi))
        per.append(pos[:ERASED.get(f, 0)])
    assert (rx != cw).sum(axis=1).tolist() == list(ERRORS)
    return msg, cw, rx, per


def to_device(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def to_host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def same(dev, host):
    if isinstance(host, dict):
        assert sorted(dev) == sorted(host)  # (the fused host decode orders its keys otherwise)
        return all(same(dev[k], host[k]) for k in host)
    a = to_host(dev)
    return a.dtype == host.dtype and a.shape == host.shape and np.array_equal(a, host)


def run(code, seed, hi, dtype, layout, kw, in_place, host_decode):
    msg, cw, rx, per = frames(code, seed, hi, dtype)
    m, c, r = layout(msg), layout(cw), layout(rx)
    host_cw, host_cor, host_msg = code.encode_batch(m, **kw), code.correct_batch(r, erasures=per, **kw), \
        code.extract_batch(c, **kw)
    host_dec = host_decode(r, per)
    dm, dr = to_device(m), to_device(r)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev_cw = code.encode_batch(dm, **kw)
        dev_cor = code.correct_batch(dr, erasures=per, **kw)
        if in_place:
            again = dr.clone()
            dev_again = code.correct_batch(again, erasures=per, out=again, **kw)
        dev_msg = code.extract_batch(dev_cw, **kw)
        dev_dec = code.decode_batch(dr, erasures=per, **kw)
    side.synchronize()
    assert same(dev_cw, host_cw) and np.array_equal(host_cw, c)
    assert same(dev_cor, host_cor) and np.array_equal(host_cor["out"], c)
    assert not host_cor["status"].any() and host_cor["nerr"].tolist() == list(ERRORS)
    if in_place:
        assert dev_again["out"] is again and same(dev_again, host_cor) and same(dr, r)
    assert same(dev_msg, host_msg) and np.array_equal(host_msg, m)
    assert same(dev_dec, host_dec) and np.array_equal(host_dec["out"], c) and np.array_equal(host_dec["msg"], m)
    assert not host_dec["status"].any() and host_dec["nerr"].tolist() == list(ERRORS)


def test_16_bit_symbols_on_a_side_stream():
    code = cc.primitive_bch(10, cc.errors(2), cc.berlekamp_massey_tag(), modular_polynomial=0x409)
    assert code.n == 1023 and code.wide

    def correct_then_extract(r, per):
        res = code.correct_batch(r, erasures=per)
        res["msg"] = code.extract_batch(res["out"])
        return res
    run(code, 1023, 2, np.uint16, lambda a: a, {}, False, correct_then_extract)


def test_interleaved_blocks_on_a_side_stream():
    code = cc.rs(4, cc.errors(2), cc.berlekamp_massey_tag())
    assert (code.n, code.l) == (15, 11)
    run(code, 1511, 16, np.uint8, lambda a: cc.interleave(a, I), dict(interleave=I), True,
        lambda r, per: code.decode_batch(r, erasures=per, interleave=I))
