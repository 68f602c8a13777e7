"""Packed-bit interface on the host: the container format of pack_bits / unpack_bits against
numpy.packbits(bitorder="little"), cc_packed_bytes and the refusals of the packed entry points on CC_DEVICE_NONE handles
(no device is asked for), and the export of every packed symbol of the header."""
import ctypes as C
import re
import os

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi

NONE = capi.DEVICE_NONE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 7, 8, 9, 31, 200, 255, 1023, 3000)


@pytest.mark.parametrize("n", LENGTHS)
def test_pack_unpack_equal_numpy(n):
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2, (37, n)).astype(np.uint8)
    packed = cc.pack_bits(bits)
    assert packed.dtype == np.uint8 and packed.shape == (37, (n + 7) // 8)
    assert np.array_equal(packed, np.packbits(bits, axis=-1, bitorder="little"))
    # the coefficient of x^p is bit p & 7 of byte p >> 3
    for p in (0, n // 2, n - 1):
        assert np.array_equal((packed[:, p >> 3] >> (p & 7)) & 1, bits[:, p])
    # pad bits are zero on output ...
    pad = np.unpackbits(packed, axis=-1, bitorder="little")[:, n:]
    assert pad.shape == (37, 8 * ((n + 7) // 8) - n) and not pad.any()
    # ... and ignored on input; round trip
    dirty = packed.copy()
    if n % 8:
        dirty[:, -1] |= (0xFF << (n % 8)) & 0xFF
    back = cc.unpack_bits(dirty, n)
    assert back.dtype == np.uint8 and np.array_equal(back, bits)
    assert np.array_equal(back, np.unpackbits(packed, axis=-1, count=n, bitorder="little"))
    assert np.array_equal(cc.pack_bits(cc.unpack_bits(packed, n)), packed)
    # only bit 0 of a symbol counts (16-bit symbols of the q > 8 codes too)
    assert np.array_equal(cc.pack_bits(bits.astype(np.uint16) | 0x100), packed)
    assert np.array_equal(cc.unpack_bits(packed, n, np.uint16), bits.astype(np.uint16))


def test_unpack_checks_the_width():
    with pytest.raises(cc.CcError):
        cc.unpack_bits(np.zeros((2, 4), np.uint8), 40)


def test_packed_bytes():
    a = cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=NONE)
    assert (a.n, a.l) == (255, 231) and (a.packed_bytes, a.packed_message_bytes) == (32, 29)
    b = cc.primitive_bch(8, cc.errors(3), cc.peterson_gorenstein_zierler_tag(), device=NONE, n=200)
    assert (b.n, b.l) == (200, 176) and (b.packed_bytes, b.packed_message_bytes) == (25, 22)
    c = cc.primitive_bch(14, cc.errors(12), cc.euklid_tag(), device=NONE, modular_polynomial=0x402B, n=3000)
    assert c.n == 3000 and c.packed_bytes == 375 and c.packed_message_bytes == (c.l + 7) // 8
    d = cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=NONE, coding="multiplication", n=100)
    assert (d.packed_bytes, d.packed_message_bytes) == (13, 10)
    lib = capi.lib()
    assert lib.cc_packed_bytes(a._h, 2) == -capi.ERR_INVALID_ARGUMENT
    assert lib.cc_packed_bytes(None, 0) == -capi.ERR_INVALID_ARGUMENT


def _refused_handles():
    H = np.array([[1, 1, 0, 1, 0, 0], [0, 1, 1, 0, 1, 0], [1, 0, 1, 0, 0, 1]], np.uint8)
    return [
        ("rs", cc.rs(8, cc.errors(8), cc.berlekamp_massey_tag(), device=NONE)),
        ("rs16", cc.rs(10, cc.errors(4), cc.berlekamp_massey_tag(), device=NONE, modular_polynomial=0x409)),
        ("minsum", cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(10), device=NONE)),
        ("matrix", cc.min_sum_decoder(H, cc.min_sum_tag(5), device=NONE)),
    ]


def _call_all(code, B=2):
    """status of every packed entry point on host buffers large enough for any code of the tests"""
    lib = capi.lib()
    buf = [np.zeros(B * 512, np.uint8) for _ in range(3)]
    nerr, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    p = [C.c_void_p(b.ctypes.data) for b in buf]
    ne, st = C.c_void_p(nerr.ctypes.data), C.c_void_p(status.ctypes.data)
    h = code._h
    neg = lambda r: -r if r < 0 else capi.OK  # noqa: E731  (cc_packed_bytes / cc_packed_route: a negative status)
    return {
        "cc_packed_bytes": neg(lib.cc_packed_bytes(h, 0)),
        "cc_packed_bytes(msg)": neg(lib.cc_packed_bytes(h, 1)),
        "cc_packed_route": neg(lib.cc_packed_route(h, B)),
        "cc_packed_map_route": neg(lib.cc_packed_map_route(h, 0)),
        "cc_packed_map_route(extract)": neg(lib.cc_packed_map_route(h, 1)),
        "cc_encode_packed_batch": lib.cc_encode_packed_batch(h, p[0], p[1], B),
        "cc_encode_packed_batch_dev": lib.cc_encode_packed_batch_dev(h, p[0], p[1], B, None),
        "cc_correct_hard_packed_batch": lib.cc_correct_hard_packed_batch(h, p[0], None, None, p[1], ne, st, B),
        "cc_correct_hard_packed_batch_dev": lib.cc_correct_hard_packed_batch_dev(h, p[0], None, None, p[1], ne, st, B, None),
        "cc_extract_packed_batch": lib.cc_extract_packed_batch(h, p[0], p[1], B),
        "cc_extract_packed_batch_dev": lib.cc_extract_packed_batch_dev(h, p[0], p[1], B, None),
        "cc_decode_hard_packed_batch": lib.cc_decode_hard_packed_batch(h, p[0], None, None, p[1], p[2], ne, st, B),
    }


def test_handles_without_a_packed_form_are_refused():
    for name, code in _refused_handles():
        for fn, rc in _call_all(code).items():
            assert rc == capi.ERR_UNSUPPORTED, (name, fn, rc)
            assert "packed" in capi.lib().cc_last_error().decode(), (name, fn)
        with pytest.raises(cc.CcError) as e:
            code.packed_bytes
        assert e.value.status == capi.ERR_UNSUPPORTED and "packed" in str(e.value)
        for call in (lambda: code.correct_batch(np.zeros((1, 32), np.uint8), packed=True),
                     lambda: code.encode_batch(np.zeros((1, 32), np.uint8), packed=True),
                     lambda: code.extract_batch(np.zeros((1, 32), np.uint8), packed=True),
                     lambda: code.decode_batch(np.zeros((1, 32), np.uint8), packed=True)):
            with pytest.raises(cc.CcError) as e:
                call()
            assert e.value.status == capi.ERR_UNSUPPORTED


def test_the_reason_is_named():
    lib = capi.lib()
    want = {"rs": "RS", "rs16": "RS", "minsum": "min-sum", "matrix": "cc_minsum_create"}
    for name, code in _refused_handles():
        assert lib.cc_packed_bytes(code._h, 0) == -capi.ERR_UNSUPPORTED
        text = lib.cc_last_error().decode()
        assert "packed" in text and want[name] in text, (name, text)


@pytest.mark.parametrize("kw", [dict(q=8, t=3), dict(q=8, t=3, n=200), dict(q=6, t=3), dict(q=10, t=2, modular_polynomial=0x409)])
def test_no_device_as_the_byte_calls(kw):
    kw = dict(kw)
    q, t = kw.pop("q"), kw.pop("t")
    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), device=NONE, **kw)
    res = _call_all(code)
    assert res.pop("cc_packed_bytes") == capi.OK and res.pop("cc_packed_bytes(msg)") == capi.OK
    for fn, rc in res.items():
        assert rc == capi.ERR_NO_DEVICE, (fn, rc)
    lib = capi.lib()
    z = np.zeros(4 * code.n, np.uint16)
    p = C.c_void_p(z.ctypes.data)
    byte_rc = (lib.cc_correct_hard_batch_u16 if q > 8 else lib.cc_correct_hard_batch)(code._h, p, None, None, p, None, None, 1)
    assert byte_rc == capi.ERR_NO_DEVICE


def test_null_pointers_and_erasure_pairs():
    code = cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag(), device=NONE)
    lib = capi.lib()
    z = np.zeros(64, np.uint8)
    p = C.c_void_p(z.ctypes.data)
    assert lib.cc_correct_hard_packed_batch(code._h, None, None, None, p, None, None, 1) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_correct_hard_packed_batch(code._h, p, p, None, p, None, None, 1) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_correct_hard_packed_batch_dev(code._h, p, None, p, p, None, None, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_encode_packed_batch(None, p, p, 1) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_pack_bits_dev(p, 3, 8, p, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_unpack_bits_dev(p, 8, p, 0, 1, None) == capi.ERR_INVALID_ARGUMENT
    assert lib.cc_pack_bits_dev(p, 1, 8, p, 0, None) == capi.OK  # nothing to do: no device is touched


def test_every_packed_symbol_of_the_header_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "channelcoding_amd.h")).read()
    names = set(re.findall(r"\bint (cc_\w*pack\w*)\(", header))
    assert names == {"cc_packed_bytes", "cc_packed_route", "cc_packed_map_route", "cc_pack_bits_dev", "cc_unpack_bits_dev",
                     "cc_encode_packed_batch", "cc_encode_packed_batch_dev", "cc_correct_hard_packed_batch",
                     "cc_correct_hard_packed_batch_dev", "cc_extract_packed_batch", "cc_extract_packed_batch_dev",
                     "cc_decode_hard_packed_batch"}
    assert names <= set(capi.exported_symbols())
    lib = capi.lib()  # (raises if the library lacks a declared symbol)
    for name in names:
        assert getattr(lib, name) is not None
