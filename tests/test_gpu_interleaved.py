"""GPU tests of the symbol-interleaved interface.  The checker is the contract: for every frame,
de-interleaving (tests/interleave_model.py) the output of an interleaved call gives symbol for symbol what the plain
call returns for the de-interleaved input, with identical nerr and status -- on the native route (the bit-plane chain
addressing the blocks itself) and on the generic one (de-interleave, plain router, interleave).  Every comparison is
exact equality over all frames and all outputs; the plain calls are pinned to the oracle and the reference by the rest
of the suite.
The suite runs with CC_AMD_PLANES_MIN_WORK=0, so every GF(2^8) call of the bit-plane codes is native at I = 2 .. 16;
RS(255,223) at I = 7 therefore takes the generic route where the switch forces it (the child process of
test_native_against_generic_in_a_child_process), at I = 33 by its depth."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import channelcoding_amd as cc
from channelcoding_amd import capi
from interleave_model import deinterleave, interleave

pytestmark = pytest.mark.gpu

TAGS = {"PGZ": cc.peterson_gorenstein_zierler_tag, "BM": cc.berlekamp_massey_tag, "EUKLID": cc.euklid_tag}
# name -> (family, q, t, tag, keywords)
CODES = {
    "RS(255,223) BM mu=1": ("rs", 8, 16, "BM", {}),
    "RS(255,239) Euklid mu=0": ("rs", 8, 8, "EUKLID", dict(mu=0)),
    "RS(204,188) BM mu=0": ("rs", 8, 8, "BM", dict(mu=0, n=204)),
    "BCH(255,231) BM": ("bch", 8, 3, "BM", {}),
    "BCH(255,231) PGZ": ("bch", 8, 3, "PGZ", {}),
    "RS(15,9)": ("rs", 4, 3, "BM", {}),
    "RS(7,3)": ("rs", 3, 2, "EUKLID", {}),
    "BCH(63,45)": ("bch", 6, 3, "BM", {}),
    "BCH(63,45) PGZ": ("bch", 6, 3, "PGZ", {}),
    "BCH(255,9)": ("bch", 8, 63, "BM", {}),
    "RS(1023,1015)": ("rs", 10, 4, "BM", dict(modular_polynomial=0x409)),
    "BCH(511,484)": ("bch", 9, 3, "BM", dict(modular_polynomial=0x211)),
}
NATIVE = list(CODES)[:5]
# (I, m): B = I m frames with 64 and 32 not dividing B -- blocks straddle the 32-frame groups and the 64-frame chunks, the
# last group is partial; and one size below one group
DEPTHS = [(2, 67), (3, 43), (4, 35), (5, 27), (8, 13), (16, 5), (5, 1)]


def make(name):
    fam, q, t, tag, kw = CODES[name]
    ctor = cc.rs if fam == "rs" else cc.primitive_bch
    return ctor(q, cc.errors(t), TAGS[tag](), **kw)


def received(code, rng, B, emax, emin=0):
    """random codewords with emin .. emax symbol errors per frame (uniform); frame-major"""
    dt = np.uint16 if code.wide else np.uint8
    top = 2 if code.family == capi.FAMILY_BCH else 1 << code.q
    cw = code.encode_batch(rng.integers(0, top, (B, code.l)).astype(dt))
    ne = rng.integers(emin, emax + 1, B)
    order = rng.random((B, code.n)).argsort(axis=1)
    hit = np.zeros((B, code.n), bool)
    np.put_along_axis(hit, order, np.arange(code.n)[None, :] < ne[:, None], axis=1)
    val = rng.integers(1, top, (B, code.n)).astype(dt)
    return cw, cw ^ np.where(hit, val, 0).astype(dt)


def check_equal(code, rx, I, erasures=None, route=None):
    """interleaved call (host and device pointers, out of place and in place) against the plain call on the same frames"""
    B = rx.shape[0]
    if route is not None:
        assert code.interleaved_route(B, I, erasures is not None) == route
    want = code.correct_batch(rx, erasures)
    blocks = interleave(rx, I)
    got = code.correct_batch(blocks, erasures, interleave=I)
    dev = code.correct_batch(torch.from_numpy(blocks).cuda(), erasures, interleave=I)
    again = torch.from_numpy(blocks).cuda()
    inplace = code.correct_batch(again, erasures, interleave=I, out=again)
    assert inplace["out"] is again
    for res in (got, dev, inplace):
        res = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in res.items()}
        assert res["out"].shape == blocks.shape and res["out"].dtype == rx.dtype
        assert np.array_equal(res["status"], want["status"])
        assert np.array_equal(res["nerr"], want["nerr"])
        assert np.array_equal(deinterleave(res["out"], I), want["out"])
    return want


@pytest.mark.parametrize("name", NATIVE)
def test_native_decode_equals_the_plain_call(name):
    code = make(name)
    t = code.t
    rng = np.random.default_rng(len(name) + 7 * t)
    seen = {"clean": 0, "corrected": 0, "failed": 0}
    for I, m in DEPTHS:
        B = I * m
        assert m == 1 or (B % 32 and B % 64)
        rx = np.concatenate([received(code, rng, B, 0)[1][: B // 4], received(code, rng, B, t, 1)[1][: B // 2],
                             received(code, rng, B, t + 3, t + 1)[1]])[:B]
        rx = rx[rng.permutation(B)]
        res = check_equal(code, rx, I, route=1)
        seen["clean"] += int(((res["status"] == 0) & (res["nerr"] == 0)).sum())
        seen["corrected"] += int(((res["status"] == 0) & (res["nerr"] > 0)).sum())
        seen["failed"] += int((res["status"] != 0).sum())
    assert all(seen.values()), seen


def test_native_decode_of_many_chunks():
    """2 051 blocks of depth 5: more than one workgroup of every kernel of the chain, blocks across every boundary"""
    code = make("RS(255,223) BM mu=1")
    rng = np.random.default_rng(5)
    _, rx = received(code, rng, 5 * 2051, code.t + 2)
    res = check_equal(code, rx, 5, route=1)
    assert (res["status"] == 0).any() and (res["status"] != 0).any()


@pytest.mark.parametrize("name,I", [(n, i) for n in list(CODES)[5:] for i in (3, 16)] + [("RS(255,223) BM mu=1", 33)])
def test_generic_decode_equals_the_plain_call(name, I):
    code = make(name)
    rng = np.random.default_rng(len(name) + I)
    for B in (I, 9 * I):
        _, rx = received(code, rng, B, code.t + 3)
        check_equal(code, rx, I, route=0)


@pytest.mark.parametrize("name", ["RS(255,223) BM mu=1", "BCH(63,45) PGZ"])
def test_erasures_go_the_generic_way(name):
    """Erasure lists per frame f (the CSR of the plain call): Berlekamp-Massey with erasures on RS(255,223), the two-trial
    PGZ rule of bch.h:97-149 on BCH(63,45); 0 .. 2t + 1 erasures per frame (beyond 2t: CC_FRAME_ERASURES)."""
    code = make(name)
    t, I, B = code.t, 5, 35
    rng = np.random.default_rng(11 * t)
    _, rx = received(code, rng, B, 2)
    ers = []
    for f in range(B):
        er = sorted(rng.choice(code.n, int(rng.integers(0, 2 * t + 2)), replace=False).tolist())
        rx[f, er] = 0
        ers.append(er)
    ers[0] = []
    ers[1] = sorted(rng.choice(code.n, 2 * t + 1, replace=False).tolist())
    res = check_equal(code, rx, I, ers, route=0)
    assert res["status"][1] == capi.FRAME_ERASURES and (res["status"] == 0).any()


ENCODE = [("RS(255,223) BM mu=1", 1), ("RS(255,239) Euklid mu=0", 1), ("RS(204,188) BM mu=0", 0), ("BCH(255,231) BM", 0),
          ("RS(1023,1015)", 0)]


@pytest.mark.parametrize("name,native_encode", ENCODE)
def test_encode_extract_decode(name, native_encode):
    code = make(name)
    rng = np.random.default_rng(len(name))
    dt = np.uint16 if code.wide else np.uint8
    top = 2 if code.family == capi.FAMILY_BCH else 1 << code.q
    for I, m in ((16, 5), (5, 27), (3, 1)):
        B = I * m
        assert code.interleaved_map_route(0, I) == native_encode and code.interleaved_map_route(1, I) == 1
        msg = rng.integers(0, top, (B, code.l)).astype(dt)
        cw = code.encode_batch(msg)
        mb = interleave(msg, I)
        for src in (mb, torch.from_numpy(mb.view(np.int16) if code.wide else mb).cuda()):
            got = code.encode_batch(src, interleave=I)
            got = got.cpu().numpy().view(dt) if torch.is_tensor(got) else got
            assert got.shape == (m, code.n, I) and np.array_equal(deinterleave(got, I), cw)
        _, rx = received(code, rng, B, code.t + 3)
        want = code.extract_batch(rx)
        rb = interleave(rx, I)
        for src in (rb, torch.from_numpy(rb.view(np.int16) if code.wide else rb).cuda()):
            got = code.extract_batch(src, interleave=I)
            got = got.cpu().numpy().view(dt) if torch.is_tensor(got) else got
            assert got.shape == (m, code.l, I) and np.array_equal(deinterleave(got, I), want)
        corr = code.correct_batch(rx)
        dec = dict(corr, msg=code.extract_batch(corr["out"]))
        for src in (rb, torch.from_numpy(rb.view(np.int16) if code.wide else rb).cuda()):
            got = code.decode_batch(src, interleave=I)
            got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
            assert np.array_equal(got["status"], dec["status"]) and np.array_equal(got["nerr"], dec["nerr"])
            assert np.array_equal(deinterleave(got["out"].view(dt), I), dec["out"])
            assert np.array_equal(deinterleave(got["msg"].view(dt), I), dec["msg"])


def test_decode_without_words_and_round_trip():
    """cc_decode_hard_interleaved_batch with words = NULL; encode -> corrupt -> decode -> message at I = 16"""
    code = make("RS(255,239) Euklid mu=0")
    lib = capi.lib()
    rng = np.random.default_rng(16)
    I, B = 16, 80
    msg = rng.integers(0, 256, (B, code.l)).astype(np.uint8)
    blocks = code.encode_batch(interleave(msg, I), interleave=I)
    hit = rng.random(blocks.shape) < 6.0 / 255  # about six symbol errors per word, bursts spread over the 16 decoders
    rx = blocks ^ np.where(hit, rng.integers(1, 256, blocks.shape), 0).astype(np.uint8)
    res = code.decode_batch(rx, interleave=I)
    ok = res["status"] == 0
    assert ok.sum() > B // 2
    assert np.array_equal(deinterleave(res["msg"], I)[ok], msg[ok])
    assert np.array_equal(deinterleave(res["out"], I)[ok], deinterleave(blocks, I)[ok])
    out_msg = np.zeros((B // I, code.l, I), np.uint8)
    nerr, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
    p = lambda a: a.ctypes.data_as(capi.C.c_void_p)  # noqa: E731
    capi.check(lib.cc_decode_hard_interleaved_batch(code._h, p(rx), None, None, p(out_msg), None, p(nerr), p(status), B, I),
               "cc_decode_hard_interleaved_batch")
    assert np.array_equal(out_msg, res["msg"]) and np.array_equal(status, res["status"]) and np.array_equal(nerr, res["nerr"])


CHILD = (
    "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
    "import numpy as np\n"
    "import channelcoding_amd as cc\n"
    "from interleave_model import interleave\n"
    "from test_gpu_interleaved import make, received\n"
    "want = int(sys.argv[1])\n"
    "code = make('RS(255,223) BM mu=1')\n"
    "res = {}\n"
    "for I, B in ((5, 135), (7, 133)):\n"
    "    rng = np.random.default_rng(I)\n"
    "    _, rx = received(code, rng, B, code.t + 3)\n"
    "    assert code.interleaved_route(B, I) == want, (I, code.interleaved_route(B, I))\n"
    "    assert code.interleaved_route(B, I, True) == 0\n"
    "    assert code.interleaved_map_route(0, I) == want and code.interleaved_map_route(1, I) == want\n"
    "    r = code.correct_batch(interleave(rx, I), interleave=I)\n"
    "    for k in ('out', 'nerr', 'status'):\n"
    "        res['%%d_%%s' %% (I, k)] = r[k]\n"
    "    res['%%d_enc' %% I] = code.encode_batch(interleave(rx[:, :code.l], I), interleave=I)\n"
    "    res['%%d_ext' %% I] = code.extract_batch(interleave(rx, I), interleave=I)\n"
    "np.savez(sys.argv[2], **res)\n"
    "print('ROUTE OK')\n")


def test_native_against_generic_in_a_child_process(tmp_path):
    """CC_AMD_INTERLEAVED_NATIVE (read once per process): one fresh child per setting runs the same seeded RS(255,223)
    calls -- I = 5, B = 135 and I = 7, B = 133 -- and writes the outputs; identical bytes, and the route queries name
    the route each process took (0 with erasures in both)."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = CHILD % (here, os.path.dirname(here))
    files = []
    for native in (1, 0):
        f = str(tmp_path / ("route%d.npz" % native))
        env = dict(os.environ, CC_AMD_INTERLEAVED_NATIVE=str(native))
        out = subprocess.run([sys.executable, "-c", script, str(native), f], env=env, capture_output=True, text=True,
                             timeout=300)
        assert out.returncode == 0 and "ROUTE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        files.append(np.load(f))
    a, b = files
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 10
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
@pytest.mark.parametrize("I,n", [(1, 255), (2, 7), (5, 204), (16, 255), (33, 255), (256, 1023), (3, 9000)])
def test_device_helpers_equal_the_model(I, n, dtype):
    rng = np.random.default_rng(I * n)
    np_dt = np.uint8 if dtype == torch.uint8 else np.int16
    x = rng.integers(0, 127, (3 * I, n)).astype(np_dt)
    y = cc.interleave(torch.from_numpy(x).cuda(), I)
    assert tuple(y.shape) == (3, n, I) and y.dtype == dtype
    assert np.array_equal(y.cpu().numpy(), interleave(x, I))
    assert np.array_equal(cc.deinterleave(y, I).cpu().numpy(), x)


def test_host_pointers_in_small_chunks(tmp_path):
    """CC_AMD_HOST_CHUNK_BYTES forced small (a process of its own: the value is read once): a staged chunk holds whole
    blocks, whatever the chunk size asks for."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import channelcoding_amd as cc\n"
        "from interleave_model import deinterleave, interleave\n"
        "from test_gpu_interleaved import make, received\n"
        "for name, I, B in (('RS(255,223) BM mu=1', 5, 135), ('RS(255,223) BM mu=1', 33, 99), ('RS(1023,1015)', 3, 51)):\n"
        "    code = make(name)\n"
        "    rng = np.random.default_rng(B)\n"
        "    _, rx = received(code, rng, B, code.t + 3)\n"
        "    want = code.correct_batch(rx)\n"
        "    got = code.decode_batch(interleave(rx, I), interleave=I)\n"
        "    assert np.array_equal(got['status'], want['status']) and np.array_equal(got['nerr'], want['nerr'])\n"
        "    assert np.array_equal(deinterleave(got['out'], I), want['out'])\n"
        "    assert np.array_equal(deinterleave(got['msg'], I), code.extract_batch(want['out']))\n"
        "    enc = code.encode_batch(interleave(rx[:, :code.l], I), interleave=I)\n"
        "    assert np.array_equal(deinterleave(enc, I), code.encode_batch(rx[:, :code.l]))\n"
        "print('CHUNKS OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="6000")  # 23 frames of 255 bytes: not a multiple of 5
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHUNKS OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_python_buffers_are_checked():
    code = make("RS(255,223) BM mu=1")
    x = torch.zeros((2, 255, 4), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((2, 255, 2), dtype=torch.uint8, device="cuda"), torch.zeros((2, 255, 4), dtype=torch.int8, device="cuda"),
                torch.zeros((2, 255, 4), dtype=torch.uint8), np.zeros((2, 255, 4), np.uint8)):
        with pytest.raises(TypeError):
            code.correct_batch(x, interleave=4, out=bad)
    with pytest.raises(cc.CcError) as e:
        code.correct_batch(x, interleave=2)
    assert e.value.status == capi.ERR_LENGTH
    with pytest.raises(TypeError):
        code.correct_batch(np.zeros((2, 255, 4), np.float32), interleave=4)
    empty = code.correct_batch(torch.zeros((0, 255, 4), dtype=torch.uint8, device="cuda"), interleave=4)
    assert tuple(empty["out"].shape) == (0, 255, 4) and empty["status"].shape[0] == 0
