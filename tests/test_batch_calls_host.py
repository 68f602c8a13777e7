"""What the Python batch API (encode_batch, extract_batch, correct_batch, decode_batch of channelcoding_amd/codes.py) hands
to the C library, call by call, and what it gives back or raises -- on host arrays and, with CPU tensors standing in for
device tensors, on the device branches too.  No device is asked for: the handles are CC_DEVICE_NONE ones, capi._lib is a
proxy that forwards every query to the real library and records the batch calls instead of making them (answering
CC_OK), and codes._stream_handle returns a marker.

Recorded per C call: its name and, per argument after the handle, "null", the number, "stream", "in" (the caller's own
buffer), the name of another buffer of the caller's, the key of the returned array it points to, or "staged:<dtype>" for
a copy the wrapper made; the erasure list read back through its two pointers.  Recorded per case, as one line: the calls, then
the result (keys in order, dtype, shape, z for a host array that is all zero, =in for the caller's input) or the
exception (type, CcError.status, the text, which begins with `where`).

The expected records are tests/golden/batch_calls.json, written by running this module as a script.  They were made with
the wrapper as it stood before its layouts got one call helper, except the cases of HAND_WRITTEN: byte-symbol
extract_batch checks width and dtype as encode_batch does, which it did not before."""
import contextlib
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import channelcoding_amd as cc
from channelcoding_amd import capi, codes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_calls.json")
BATCH_CALL = re.compile(r"cc_(encode|extract|correct|decode)_\w*batch\w*")
TAKES_ERASURES = re.compile(r"cc_(correct_(hard|soft)|decode_(hard|soft))_\w*")
STREAM = 0x5EED0
SIDES = ("numpy", "torch")
BM = cc.berlekamp_massey_tag
NONE = capi.DEVICE_NONE

# (case, side) whose expected record is written by hand, to the rule that byte-symbol extract_batch raises
# CcError(ERR_LENGTH, "extract_batch") for a last dimension other than n and for a tensor that is not uint8
_LENGTH = "!! CcError %d: extract_batch: sequence has the wrong length" % capi.ERR_LENGTH
HAND_WRITTEN = {
    ("refuse/width/extract/bch/plain", "numpy"): _LENGTH,
    ("refuse/width/extract/bch/plain", "torch"): _LENGTH,
    ("refuse/width/extract/bch/plain-two-frames-wide", "numpy"): _LENGTH,
    ("refuse/width/extract/bch/plain-two-frames-wide", "torch"): _LENGTH,
    ("refuse/width/extract/rs/plain", "numpy"): _LENGTH,
    ("refuse/width/extract/rs/plain", "torch"): _LENGTH,
    ("refuse/dtype/extract/bch/plain-int16", "torch"): _LENGTH,
    ("refuse/dtype/extract/bch/plain-float32", "torch"): _LENGTH,
}


class NonContiguous:
    """the array as a strided view"""
    def __init__(self, a):
        self.a = a


class OtherSide:
    """the array on the side the case does not run on"""
    def __init__(self, a):
        self.a = a


class ReadOnly:
    def __init__(self, a):
        self.a = a


SAME = "the input itself"  # out is b


def _tensor(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def to_side(v, side):
    if isinstance(v, NonContiguous):
        base = to_side(np.repeat(v.a, 2, axis=-1), side)
        return base[..., ::2]
    if isinstance(v, OtherSide):
        return to_side(v.a, SIDES[1 - SIDES.index(side)])
    if isinstance(v, ReadOnly):
        a = to_side(v.a, side)
        if side == "numpy":
            a.flags.writeable = False
        return a
    if isinstance(v, np.ndarray):
        return np.array(v) if side == "numpy" else _tensor(v)
    return v


def _is_array(a):
    return isinstance(a, np.ndarray) or codes._is_torch(a)


def _address(a):
    return a.data_ptr() if codes._is_torch(a) else a.ctypes.data


def _dtype(a):
    return str(a.dtype).replace("torch.", "")


class Proxy:
    """capi._lib with the batch calls recorded instead of made"""

    def __init__(self, real):
        self.real, self.calls, self.kept = real, [], []

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not BATCH_CALL.fullmatch(name):
            return fn

        def record(*args):
            call = dict(name=name, args=list(args))
            if TAKES_ERASURES.fullmatch(name) and args[3] is not None and args[3].value:
                B = args[[t is C.c_size_t for t in capi._SIGNATURES[name][1]].index(True)]
                off = list((C.c_uint32 * (B + 1)).from_address(args[3].value))
                call["erasure_offsets"] = off
                call["erasures"] = list((C.c_uint16 * off[-1]).from_address(args[2].value)) if off[-1] else []
            self.calls.append(call)
            return capi.OK
        return record

    def ptr(self, a):
        """codes._ptr, keeping the array alive so that no later buffer takes its address"""
        if a is not None:
            self.kept.append(a)
        return self.real_ptr(a)


@contextlib.contextmanager
def swapped():
    """capi._lib, codes._stream_handle and codes._ptr replaced; restored on the way out"""
    real_lib, real_stream, real_ptr = capi.lib(), codes._stream_handle, codes._ptr
    p = Proxy(real_lib)
    p.real_ptr = real_ptr
    capi._lib, codes._stream_handle, codes._ptr = p, lambda t: C.c_void_p(STREAM), p.ptr
    try:
        yield p
    finally:
        capi._lib, codes._stream_handle, codes._ptr = real_lib, real_stream, real_ptr


@pytest.fixture
def proxy():
    with swapped() as p:
        yield p


def _describe_arg(a, code, named, result, kept):
    if a is None or (isinstance(a, C.c_void_p) and not a.value):
        return "null"
    if not isinstance(a, C.c_void_p):
        return a if isinstance(a, float) else int(a)
    if a.value == STREAM:
        return "stream"
    for label, obj in list(named.items()) + list(result.items()):
        if _is_array(obj) and _address(obj) == a.value:
            return label
    for obj in kept:
        if _address(obj) == a.value:
            return "staged:" + _dtype(obj)
    return "staged"


def _describe_result(res, x, side):
    """key:dtype[shape], then z for a host array that is all zero and =in for the caller's input itself"""
    return " ".join("%s:%s%s%s%s" % (key, _dtype(a), list(a.shape), "z" if side == "numpy" and not a.any() else "",
                                     "=in" if a is x else "") for key, a in res.items()).replace(", ", ",")


def run_case(case, side, proxy):
    """The record of one case on one side, one line: the C calls, then `-> result` or `!! exception`."""
    _name, handle, method, x, kw = case
    code = HANDLES[handle]
    x = to_side(x, side)
    kw = {k: (x if v is SAME else to_side(v, side)) for k, v in kw.items()}
    named = {"in": x}
    named.update((k, v) for k, v in kw.items() if _is_array(v) and v is not x and k != "out")
    result = {}
    try:
        res = getattr(code, method)(x, **kw)
        result = res if isinstance(res, dict) else {"return": res}
        end = "-> " + _describe_result(result, x, side)
    except Exception as e:  # noqa: BLE001 -- whatever the wrapper raises is the record
        text = str(e)  # (for a CcError it begins with `where`)
        detail = capi.lib().cc_last_error().decode()
        if detail and text.endswith(" (" + detail + ")"):  # (the library's last message: whatever call came before)
            text = text[:-len(detail) - 3]
        if "unexpected keyword argument" in text:  # (the interpreter's own wording)
            text = "unexpected keyword argument" + text.split("unexpected keyword argument")[1]
        end = "!! %s%s: %s" % (type(e).__name__, " %d" % e.status if isinstance(e, cc.CcError) else "", text)
    calls = []
    for call in proxy.calls:
        assert call["args"][0].value == code._h.value  # (the handle comes first, always)
        args = ",".join(str(_describe_arg(a, code, named, result, proxy.kept)) for a in call["args"][1:])
        lists = ""
        if "erasures" in call:
            lists = " erasures %s at %s" % (call["erasures"], call["erasure_offsets"])
        calls.append("%s(%s)%s" % (call["name"], args, lists.replace(", ", ",")))
    return " ; ".join(calls + [end])


# ---- the handles and the cases ----
HANDLES = {
    "bch": cc.primitive_bch(4, cc.errors(2), BM(), device=NONE),  # BCH(15,7)
    "rs": cc.rs(4, cc.errors(2), BM(), device=NONE),  # RS(15,11)
    "ms": cc.primitive_bch(4, cc.errors(2), cc.min_sum_tag(5), device=NONE),
    "wide": cc.primitive_bch(10, cc.errors(2), BM(), device=NONE, modular_polynomial=0x409),  # n = 1023, 16-bit symbols
    "widems": cc.primitive_bch(10, cc.errors(2), cc.min_sum_tag(5), device=NONE, modular_polynomial=0x409),
}
B, I, BI = 3, 4, 8
LAYOUTS = {"bch": ("plain", "packed", "interleave"), "rs": ("plain", "interleave"), "wide": ("plain", "interleave")}
METHODS = ("encode_batch", "extract_batch", "correct_batch", "decode_batch")


def sym(shape, dtype=np.uint8):
    return (np.arange(int(np.prod(shape))) % 2).astype(dtype).reshape(shape)


def val(shape, dtype=np.float32):
    return (1 - 2 * sym(shape).astype(np.int32)).astype(dtype)


def _cases():
    cases = []

    def add(name, handle, method, x, **kw):
        cases.append((name, handle, method, x, kw))

    def per_frame(frames):
        return [[7 + f % 3] if f != 1 else [] for f in range(frames)]

    for h, layouts in LAYOUTS.items():
        code = HANDLES[h]
        for layout in layouts:
            dt = np.uint16 if h == "wide" and layout != "packed" else np.uint8
            other = np.uint8 if dt == np.uint16 else np.uint16  # (tensors: int16)
            n, l = (code.packed_bytes, code.packed_message_bytes) if layout == "packed" else (code.n, code.l)
            lk = {"packed": dict(packed=True), "interleave": dict(interleave=I), "plain": {}}[layout]
            frames = BI if layout == "interleave" else B

            def shaped(w):
                return (BI // I, w, I) if layout == "interleave" else (B, w)
            tag = "%s/%s" % (h, layout)
            for method in METHODS:  # every method in every layout, and its refusal of a wrong width
                m, w = method[:-6], l if method == "encode_batch" else n
                add("%s/%s" % (m, tag), h, method, sym(shaped(w), dt), **lk)
                add("refuse/width/%s/%s" % (m, tag), h, method, sym(shaped(w + 1), dt), **lk)
            x = sym(shaped(n), dt)
            for form, er in (("empty", []), ("flat", [2]), ("per-frame", per_frame(frames))):
                add("correct/%s/erasures-%s" % (tag, form), h, "correct_batch", x, erasures=er, **lk)
            add("decode/%s/erasures-per-frame" % tag, h, "decode_batch", x, erasures=per_frame(frames), **lk)
            add("correct/%s/non-contiguous" % tag, h, "correct_batch", NonContiguous(x), **lk)
            add("refuse/erasures/correct/%s/a-list-too-few" % tag, h, "correct_batch", x, erasures=[[1]] * (frames - 1),
                **lk)
            add("refuse/erasures/decode/%s/position-n" % tag, h, "decode_batch", x, erasures=[code.n], **lk)
            add("refuse/dtype/correct/%s/other-width" % tag, h, "correct_batch", x.astype(other), **lk)
            add("refuse/dtype/encode/%s/other-width" % tag, h, "encode_batch", sym(shaped(l), other), **lk)
            add("refuse/dtype/correct/%s/float32" % tag, h, "correct_batch", val(shaped(n)), **lk)
            if layout == "plain":
                add("refuse/out/%s" % tag, h, "correct_batch", x, out=np.ones_like(x))
                continue
            add("out/%s/fresh" % tag, h, "correct_batch", x, out=np.ones_like(x), erasures=[1], **lk)
            add("out/%s/in-place" % tag, h, "correct_batch", x, out=SAME, **lk)
            add("refuse/out/%s/in-place-non-contiguous" % tag, h, "correct_batch", NonContiguous(x), out=SAME, **lk)
            add("refuse/out/%s/shape" % tag, h, "correct_batch", x, out=np.ones_like(x)[:1], **lk)
            add("refuse/out/%s/dtype" % tag, h, "correct_batch", x, out=np.ones(x.shape, other), **lk)
            add("refuse/out/%s/read-only" % tag, h, "correct_batch", x, out=ReadOnly(np.ones_like(x)), **lk)
            add("refuse/out/%s/non-contiguous" % tag, h, "correct_batch", x, out=NonContiguous(np.ones_like(x)), **lk)
            add("refuse/out/%s/decode" % tag, h, "decode_batch", x, out=np.ones_like(x), **lk)
    add("encode/bch/plain/non-contiguous", "bch", "encode_batch", NonContiguous(sym((B, 7))))
    add("extract/bch/plain/one-dimension", "bch", "extract_batch", sym((15,)))
    add("correct/bch/plain/three-dimensions", "bch", "correct_batch", sym((B, 1, 15)), erasures=per_frame(B))
    add("refuse/width/extract/bch/plain-two-frames-wide", "bch", "extract_batch", sym((B, 30)))
    add("refuse/width/correct/bch/interleave-other-depth", "bch", "correct_batch", sym((BI // I, 15, I - 1)), interleave=I)
    add("refuse/dtype/extract/bch/plain-int16", "bch", "extract_batch", sym((B, 15), np.uint16))
    add("refuse/dtype/extract/bch/plain-float32", "bch", "extract_batch", val((B, 15)))
    add("refuse/packed/rs", "rs", "correct_batch", sym((B, 2)), packed=True)
    # channel values: the soft call, a hard handle on float and on int input
    for h in ("ms", "widems", "bch"):
        n = HANDLES[h].n
        y = val((B, n))
        add("correct/%s/float32" % h, h, "correct_batch", y)
        add("correct/%s/float32/want_L" % h, h, "correct_batch", y, want_L=True, erasures=per_frame(B))
        add("correct/%s/float32/non-contiguous" % h, h, "correct_batch", NonContiguous(y))
        add("decode/%s/float32" % h, h, "decode_batch", y, erasures=[0, 3])
        for dt in (np.float64, np.int32, np.uint8):
            add("refuse/dtype/correct/%s/values-%s" % (h, np.dtype(dt).name), h, "correct_batch", val((B, n), dt))
        add("decode/%s/int32" % h, h, "decode_batch", val((B, n), np.int32))
        add("decode/%s/symbols" % h, h, "decode_batch", sym((B, n)))
        add("refuse/width/correct/%s/values" % h, h, "correct_batch", val((B, n - 1)))
        add("refuse/erasures/correct/%s/values/position-n" % h, h, "correct_batch", y, erasures=[[1], [n], []])
    # Chase, Chase with soft output, GMD
    y, w, rel = val((B, 15)), sym((B, 15)), np.abs(val((B, 15))) * 0.5
    for method in ("correct_batch", "decode_batch"):
        m = method[:-6]
        add("%s/bch/chase" % m, "bch", method, y, chase=4)
        add("%s/bch/chase-soft" % m, "bch", method, y, chase=4, soft=0.5)
        add("%s/rs/gmd-all" % m, "rs", method, w, gmd=True, reliability=rel)
        add("%s/rs/gmd-2" % m, "rs", method, w, gmd=2, reliability=rel)
        # the keyword combinations that are refused
        packed_x, blocks = sym((B, 2)), sym((BI // I, 15, I))
        add("refuse/keywords/%s/soft-alone" % m, "bch", method, y, soft=0.5)
        add("refuse/keywords/%s/soft+gmd" % m, "bch", method, y, soft=0.5, chase=4, gmd=2)
        add("refuse/keywords/%s/soft+reliability" % m, "bch", method, y, soft=0.5, chase=4, reliability=rel)
        add("refuse/keywords/%s/soft+erasures" % m, "bch", method, y, soft=0.5, chase=4, erasures=[1])
        add("refuse/keywords/%s/gmd-alone" % m, "rs", method, w, gmd=2)
        add("refuse/keywords/%s/reliability-alone" % m, "rs", method, w, reliability=rel)
        add("refuse/keywords/%s/gmd+erasures" % m, "rs", method, w, gmd=2, reliability=rel, erasures=[1])
        add("refuse/keywords/%s/gmd+packed" % m, "rs", method, w, gmd=2, reliability=rel, packed=True)
        add("refuse/keywords/%s/gmd+interleave" % m, "rs", method, w, gmd=2, reliability=rel, interleave=I)
        add("refuse/keywords/%s/gmd+chase" % m, "rs", method, w, gmd=2, reliability=rel, chase=4)
        add("refuse/keywords/%s/chase+erasures" % m, "bch", method, y, chase=4, erasures=[1])
        add("refuse/keywords/%s/chase+packed" % m, "bch", method, packed_x, chase=4, packed=True)
        add("refuse/keywords/%s/chase+interleave" % m, "bch", method, blocks, chase=4, interleave=I)
        add("refuse/keywords/%s/interleave+packed" % m, "bch", method, packed_x, interleave=I, packed=True)
    add("correct/bch/chase-soft/non-contiguous", "bch", "correct_batch", NonContiguous(y), chase=2, soft=1)
    add("correct/rs/gmd/non-contiguous-reliability", "rs", "correct_batch", w, gmd=2, reliability=NonContiguous(rel))
    add("refuse/value/chase-negative", "bch", "correct_batch", y, chase=-1)
    add("refuse/value/gmd-0", "rs", "correct_batch", w, gmd=0, reliability=rel)
    add("refuse/value/soft-true", "bch", "correct_batch", y, chase=4, soft=True)
    add("refuse/width/chase", "bch", "correct_batch", val((B, 14)), chase=4)
    add("refuse/width/gmd", "rs", "correct_batch", sym((B, 14)), gmd=2, reliability=np.abs(val((B, 14))))
    add("refuse/width/gmd-reliability-shape", "rs", "correct_batch", w, gmd=2, reliability=rel[:2])
    add("refuse/side/gmd-reliability", "rs", "correct_batch", w, gmd=2, reliability=OtherSide(rel))
    add("refuse/dtype/chase-int32", "bch", "correct_batch", val((B, 15), np.int32), chase=4)
    add("refuse/dtype/chase-float64", "bch", "correct_batch", val((B, 15), np.float64), chase=4, soft=0.5)
    add("refuse/dtype/gmd-symbols-float32", "rs", "correct_batch", w.astype(np.float32), gmd=2, reliability=rel)
    add("refuse/dtype/gmd-reliability-int32", "rs", "correct_batch", w, gmd=2, reliability=rel.astype(np.int32))
    add("refuse/keywords/encode/interleave+packed", "bch", "encode_batch", sym((B, 1)), interleave=I, packed=True)
    add("refuse/keywords/extract/interleave+packed", "bch", "extract_batch", sym((B, 2)), interleave=I, packed=True)
    add("refuse/keywords/encode/out", "bch", "encode_batch", sym((B, 7)), out=np.ones((B, 15), np.uint8))
    add("refuse/keywords/extract/out", "bch", "extract_batch", sym((B, 15)), out=np.ones((B, 7), np.uint8))
    add("refuse/keywords/correct/gmd+want_L", "rs", "correct_batch", w, gmd=2, reliability=rel, want_L=True)
    add("refuse/keywords/correct/gmd+out", "rs", "correct_batch", w, gmd=2, reliability=rel, out=np.ones_like(w))
    add("refuse/keywords/correct/chase+want_L", "bch", "correct_batch", y, chase=4, want_L=True)
    add("refuse/keywords/correct/chase+out", "bch", "correct_batch", y, chase=4, out=np.ones((B, 15), np.uint8))
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


CASES = _cases()


@pytest.fixture(scope="module")
def golden():
    """case -> the record of both sides, or [on numpy arrays, on tensors]"""
    with open(GOLDEN) as f:
        return {k: dict(zip(SIDES, v if isinstance(v, list) else (v, v))) for k, v in json.load(f).items()}


def test_the_golden_file_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES)
    for (name, side), record in HAND_WRITTEN.items():
        assert golden[name][side] == record


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_batch_call(case, side, proxy, golden):
    assert run_case(case, side, proxy) == golden[case[0]][side]


def test_the_proxy_is_gone_afterwards():
    assert isinstance(capi.lib(), C.CDLL) and codes._stream_handle.__module__ == codes.__name__
    assert codes._ptr.__module__ == codes.__name__


if __name__ == "__main__":  # writes the golden file from the wrapper as it stands, one case per line
    lines = []
    for case in CASES:
        both = []
        for side in SIDES:
            with swapped() as p:
                both.append(HAND_WRITTEN.get((case[0], side)) or run_case(case, side, p))
        lines.append("%s: %s" % (json.dumps(case[0]), json.dumps(both[0] if both[0] == both[1] else both)))
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(sorted(lines)) + "\n}\n")
    print("%d cases written to %s" % (len(lines), GOLDEN))
