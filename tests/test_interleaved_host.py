"""Symbol-interleaved blocks on the host: the Python helpers against the numpy model of the layout, the
new refusals of the interleaved entry points, the refusals of the plain calls reproduced with status and text on
CC_DEVICE_NONE handles (no device is asked for), the route queries where they refuse, and the export of every
interleaved symbol of the header.  (A route query answers CC_ERR_NO_DEVICE on such a handle before it names a route, as
cc_packed_route does: "0 with erasures" and "0 under CC_AMD_INTERLEAVED_NATIVE=0" are asserted where a device is,
tests/test_gpu_interleaved.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from interleave_model import deinterleave, interleave

NONE = capi.DEVICE_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BM = cc.berlekamp_massey_tag


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("n", [7, 204, 255, 1023])
@pytest.mark.parametrize("I", [1, 2, 5, 16, 256])
def test_helpers_equal_the_model(I, n, dtype):
    rng = np.random.default_rng(1000 * I + n)
    x = rng.integers(0, 1 << (8 * np.dtype(dtype).itemsize), (3 * I, n)).astype(dtype)
    y = cc.interleave(x, I)
    assert y.dtype == dtype and y.shape == (3, n, I) and y.flags.c_contiguous
    assert np.array_equal(y, interleave(x, I))
    # the sentence of the header: symbol p of frame b I + j at index b I n + p I + j
    for f, p in ((0, 0), (I - 1, n - 1), (2 * I + I // 2, n // 2)):
        assert y.reshape(-1)[(f // I) * I * n + p * I + f % I] == x[f, p]
    back = cc.deinterleave(y, I)
    assert back.dtype == dtype and np.array_equal(back, x) and np.array_equal(deinterleave(y, I), x)
    # highest power first = this layout read backwards
    assert np.array_equal(y.reshape(-1)[::-1].reshape(3, n, I), interleave(x[::-1, ::-1], I))


def test_helpers_check_their_arguments():
    x = np.zeros((6, 7), np.uint8)
    for bad in (0, 257, 4):
        with pytest.raises(cc.CcError) as e:
            cc.interleave(x, bad)
        assert e.value.status == capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError):
        cc.deinterleave(np.zeros((2, 7, 3), np.uint8), 2)


def _handles():
    return {
        "bch": cc.primitive_bch(8, cc.errors(3), BM(), device=NONE),
        "rs": cc.rs(8, cc.errors(16), BM(), device=NONE),
        "short": cc.rs(8, cc.errors(8), BM(), device=NONE, n=204, mu=0),
        "wide": cc.rs(10, cc.errors(4), BM(), device=NONE, modular_polynomial=0x409),
    }


def _buffers(B):
    buf = [np.zeros(B * 2048, np.uint16) for _ in range(3)]
    nerr, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    return [C.c_void_p(b.ctypes.data) for b in buf], C.c_void_p(nerr.ctypes.data), C.c_void_p(status.ctypes.data), buf


def _call_all(code, B, I, wide):
    """status of every interleaved entry point of the handle's symbol width on host buffers"""
    lib = capi.lib()
    p, ne, st, keep = _buffers(max(B, 1))
    h, sfx = code._h, "_u16" if wide else ""
    neg = lambda r: -r if r < 0 else capi.OK  # noqa: E731
    g = lambda name: getattr(lib, name)  # noqa: E731
    res = {
        "route": neg(lib.cc_interleaved_route(h, B, I, 0)),
        "encode": g("cc_encode_interleaved_batch" + sfx)(h, p[0], p[1], B, I),
        "encode_dev": g("cc_encode_interleaved_batch%s_dev" % sfx)(h, p[0], p[1], B, I, None),
        "correct": g("cc_correct_hard_interleaved_batch" + sfx)(h, p[0], None, None, p[1], ne, st, B, I),
        "correct_dev": g("cc_correct_hard_interleaved_batch%s_dev" % sfx)(h, p[0], None, None, p[1], ne, st, B, I, None),
        "extract": g("cc_extract_interleaved_batch" + sfx)(h, p[0], p[1], B, I),
        "extract_dev": g("cc_extract_interleaved_batch%s_dev" % sfx)(h, p[0], p[1], B, I, None),
    }
    if not wide:
        res["decode"] = lib.cc_decode_hard_interleaved_batch(h, p[0], None, None, p[1], p[2], ne, st, B, I)
    del keep
    return res


@pytest.mark.parametrize("B,I", [(4, 0), (257, 257), (7, 2), (10, 4)])
def test_depth_and_batch_size_are_checked(B, I):
    for name, code in _handles().items():
        for fn, rc in _call_all(code, B, I, name == "wide").items():
            assert rc == capi.ERR_INVALID_ARGUMENT, (name, fn, rc)
            assert "interleaving depth" in capi.lib().cc_last_error().decode(), (name, fn)
        for which in (0, 1):  # (the map query has no B: a depth in range gets as far as the device)
            want = capi.ERR_NO_DEVICE if 1 <= I <= 256 else capi.ERR_INVALID_ARGUMENT
            assert capi.lib().cc_interleaved_map_route(code._h, which, I) == -want, (name, which)


@pytest.mark.parametrize("I", [1, 2, 5, 16, 256])
def test_a_call_that_would_run_answers_no_device(I):
    for name, code in _handles().items():
        for fn, rc in _call_all(code, 2 * I, I, name == "wide").items():
            assert rc == capi.ERR_NO_DEVICE, (name, fn, rc)
        assert capi.lib().cc_interleaved_map_route(code._h, 0, I) == -capi.ERR_NO_DEVICE


def _plain_and_interleaved(code, wide, erasures):
    """(status, text) of the plain hard-decode call and of the interleaved one, host and _dev forms"""
    lib = capi.lib()
    p, ne, st, keep = _buffers(4)
    er = np.zeros(4, np.uint16)
    off = np.arange(5, dtype=np.uint32)
    pe, po = (C.c_void_p(er.ctypes.data), C.c_void_p(off.ctypes.data)) if erasures else (None, None)
    sfx = "_u16" if wide else ""
    out = []
    for dev in ("", "_dev"):
        tail = (None,) if dev else ()
        a = getattr(lib, "cc_correct_hard_batch" + sfx + dev)(code._h, p[0], pe, po, p[1], ne, st, 4, *tail)
        ta = lib.cc_last_error().decode()
        b = getattr(lib, "cc_correct_hard_interleaved_batch" + sfx + dev)(code._h, p[0], pe, po, p[1], ne, st, 4, 2, *tail)
        tb = lib.cc_last_error().decode()
        out.append(((a, ta), (b, tb)))
    del keep
    return out


def test_refusals_of_the_plain_call_come_first_with_their_text():
    H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1]], np.uint8)
    rs8 = cc.rs(8, cc.errors(16), cc.peterson_gorenstein_zierler_tag(), device=NONE)
    wrapped = cc.rs(8, cc.errors(16), BM(), device=NONE, mu=112, step=11)  # 112 + 31 * 11 > 254: the exponents wrap
    wide = cc.rs(10, cc.errors(4), BM(), device=NONE, modular_polynomial=0x409)
    widepgz = cc.rs(10, cc.errors(4), cc.peterson_gorenstein_zierler_tag(), device=NONE, modular_polynomial=0x409)
    minsum = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(10), device=NONE)
    cases = [
        ("rs+pgz+erasures", rs8, False, True, capi.ERR_UNSUPPORTED, "PGZ"),
        ("rs16+pgz+erasures", widepgz, True, True, capi.ERR_UNSUPPORTED, "PGZ"),
        ("wrapped mu/step", wrapped, False, False, capi.ERR_UNSUPPORTED, "wrap"),
        ("byte call on a 16-bit handle", wide, False, False, capi.ERR_UNSUPPORTED, "_u16"),
        ("16-bit call on a byte handle", rs8, True, False, capi.ERR_UNSUPPORTED, "_u16"),
        ("min-sum handle", minsum, False, False, capi.ERR_INVALID_ARGUMENT, "min-sum"),
    ]
    for name, code, wide_call, erasures, status, word in cases:
        for (a, ta), (b, tb) in _plain_and_interleaved(code, wide_call, erasures):
            assert a == b == status, (name, a, b)
            assert ta == tb and word in tb, (name, ta, tb)
        r = capi.lib().cc_interleaved_route(code._h, 4, 2, int(erasures))
        if wide_call == code.wide:  # (the query has no symbol width: it answers for the handle's own)
            assert r == -status, (name, r)
    # a handle of cc_minsum_create: refused by the interleaved calls themselves
    matrix = cc.min_sum_decoder(H, cc.min_sum_tag(5), device=NONE)
    for fn, rc in _call_all(matrix, 4, 2, False).items():
        assert rc == capi.ERR_INVALID_ARGUMENT, (fn, rc)
        assert "cc_minsum_create" in capi.lib().cc_last_error().decode()
    # the Python layer: the same statuses as exceptions; packed and interleaved do not combine
    blocks = np.zeros((2, 255, 2), np.uint8)
    with pytest.raises(cc.CcError) as e:
        rs8.correct_batch(blocks, [[0]] * 4, interleave=2)
    assert e.value.status == capi.ERR_UNSUPPORTED and "PGZ" in str(e.value)
    with pytest.raises(cc.CcError) as e:
        rs8.correct_batch(blocks, interleave=2)
    assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        rs8.correct_batch(np.zeros((2, 254, 2), np.uint8), interleave=2)
    assert e.value.status == capi.ERR_LENGTH
    bch = cc.primitive_bch(8, cc.errors(3), BM(), device=NONE)
    for call in (lambda: bch.correct_batch(np.zeros((2, 32), np.uint8), packed=True, interleave=2),
                 lambda: bch.encode_batch(np.zeros((2, 29), np.uint8), packed=True, interleave=2),
                 lambda: bch.extract_batch(np.zeros((2, 32), np.uint8), packed=True, interleave=2),
                 lambda: bch.decode_batch(np.zeros((2, 32), np.uint8), packed=True, interleave=2)):
        with pytest.raises(TypeError):
            call()


def test_route_queries():
    lib = capi.lib()
    rs8 = cc.rs(8, cc.errors(16), BM(), device=NONE)
    assert lib.cc_interleaved_route(None, 4, 2, 0) == -capi.ERR_INVALID_ARGUMENT
    assert lib.cc_interleaved_route(rs8._h, 5, 2, 0) == -capi.ERR_INVALID_ARGUMENT
    assert lib.cc_interleaved_map_route(rs8._h, 2, 2) == -capi.ERR_INVALID_ARGUMENT
    with pytest.raises(cc.CcError) as e:
        rs8.interleaved_route(4, 2)
    assert e.value.status == capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        rs8.interleaved_map_route(1, 300)
    assert e.value.status == capi.ERR_INVALID_ARGUMENT


def test_null_pointers_and_erasure_pairs():
    code = cc.rs(8, cc.errors(16), BM(), device=NONE)
    lib = capi.lib()
    z = np.zeros(2048, np.uint8)
    p = C.c_void_p(z.ctypes.data)
    assert lib.cc_correct_hard_interleaved_batch(code._h, None, None, None, p, None, None, 2, 2) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_correct_hard_interleaved_batch(code._h, p, p, None, p, None, None, 2, 2) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_correct_hard_interleaved_batch_dev(code._h, p, None, p, p, None, None, 2, 2, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_encode_interleaved_batch(None, p, p, 2, 2) == capi.ERR_INVALID_ARGUMENT
    q = C.c_void_p(z.ctypes.data + 1024)
    assert lib.cc_interleave_dev(p, 3, 8, 2, q, 2, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_interleave_dev(p, 1, 8, 0, q, 2, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_deinterleave_dev(p, 1, 8, 2, q, 3, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_deinterleave_dev(p, 1, 8, 2, p, 2, None) == capi.ERR_INVALID_ARGUMENT  # in place
    assert lib.cc_interleave_dev(p, 1, 8, 2, q, 0, None) == capi.OK  # nothing to do: no device is touched


def test_every_interleaved_symbol_of_the_header_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "channelcoding_amd.h")).read()
    names = set(re.findall(r"\bint (cc_\w*interleave\w*)\(", header))
    want = {"cc_interleaved_route", "cc_interleaved_map_route", "cc_interleave_dev", "cc_deinterleave_dev",
            "cc_decode_hard_interleaved_batch"}
    for op in ("encode", "correct_hard", "extract"):
        for sfx in ("", "_dev", "_u16", "_u16_dev"):
            want.add("cc_%s_interleaved_batch%s" % (op, sfx))
    assert names == want
    assert names <= set(capi.exported_symbols())
    lib = capi.lib()  # (raises if the library lacks a declared symbol)
    for name in names:
        assert getattr(lib, name) is not None
