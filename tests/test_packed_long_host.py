"""The native packed route of the 16-bit handles changes no refusal: on CC_DEVICE_NONE handles every
packed entry point of a q > 8 code answers what it answered before -- CC_ERR_NO_DEVICE before a route is named, for the
tags and sizes the native route serves (BM, PGZ) and for those it leaves alone (Euklid, t = 32), CC_ERR_UNSUPPORTED for
RS -- and cc_packed_bytes needs no device."""
import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi

from test_packed_host import _call_all

NONE = capi.DEVICE_NONE
TAGS = {"PGZ": cc.peterson_gorenstein_zierler_tag, "BM": cc.berlekamp_massey_tag, "EUKLID": cc.euklid_tag}
# (q, t, N, polynomial): the codes of tests/test_gpu_packed_long.py, and t = 32, beyond the native route's lanes
CODES = [(9, 3, None, 0x211), (10, 2, None, 0x409), (14, 12, 3000, 0x402B), (13, 31, 1000, 0x201B), (15, 2, None, 0x8003),
         (11, 4, 70, 0x805), (10, 32, None, 0x409)]


@pytest.mark.parametrize("tag", ["BM", "PGZ", "EUKLID"])
@pytest.mark.parametrize("q,t,N,poly", CODES)
def test_no_device_before_a_route_is_named(q, t, N, poly, tag):
    code = cc.primitive_bch(q, cc.errors(t), TAGS[tag](), device=NONE, modular_polynomial=poly, n=N)
    assert code.packed_bytes == (code.n + 7) // 8 and code.packed_message_bytes == (code.l + 7) // 8
    lib = capi.lib()
    for B in (1, 700, 1024, 4096, 1 << 20):
        assert lib.cc_packed_route(code._h, B) == -capi.ERR_NO_DEVICE
    with pytest.raises(cc.CcError) as e:
        code.packed_route(4096)
    assert e.value.status == capi.ERR_NO_DEVICE
    res = _call_all(code) if code.packed_bytes <= 512 else {}
    assert res.pop("cc_packed_bytes", capi.OK) == capi.OK and res.pop("cc_packed_bytes(msg)", capi.OK) == capi.OK
    for fn, rc in res.items():
        assert rc == capi.ERR_NO_DEVICE, (fn, rc)
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(np.zeros((2, code.packed_bytes), np.uint8), packed=True)
    assert e.value.status == capi.ERR_NO_DEVICE


def test_rs_over_a_16_bit_field_has_no_packed_form():
    lib = capi.lib()
    for tag in TAGS.values():
        code = cc.rs(10, cc.errors(4), tag(), device=NONE, modular_polynomial=0x409)
        for B in (1, 1024, 4096):
            assert lib.cc_packed_route(code._h, B) == -capi.ERR_UNSUPPORTED
            assert "packed" in lib.cc_last_error().decode() and "RS" in lib.cc_last_error().decode()
        for fn, rc in _call_all(code).items():
            assert rc == capi.ERR_UNSUPPORTED, (fn, rc)
