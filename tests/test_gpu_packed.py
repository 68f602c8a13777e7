"""GPU tests of the packed-bit interface: for every frame, unpacking the output of a packed call gives byte
for byte what the byte (or 16-bit) call returns for the unpacked input, with identical nerr and status -- on the native
route (GF(2^8), n <= 255, no erasures: packed_syndrome_kernel / packed_fix_kernel around the unchanged Berlekamp-Massey
and root-search stages) and on the generic one (unpack, byte route, pack).  Plus a truth that needs no reference: the
bounded-distance guarantee and H out^T = 0.  No frame is excluded from any comparison."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import shortened_model as S
from checkers import BCH, BM, EUKLID, PGZ, WideOracle

import channelcoding_amd as cc
from channelcoding_amd import capi

pytestmark = pytest.mark.gpu

TAGS = {"PGZ": cc.peterson_gorenstein_zierler_tag, "BM": cc.berlekamp_massey_tag, "EUKLID": cc.euklid_tag}
SIZES = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4161)
# (q, t, N): BCH(255,231), BCH(255,139), BCH(255,247), shortened BCH(200,176) and BCH(100,76) (P = 13: odd pitch)
NATIVE = [(8, 3, None), (8, 15, None), (8, 1, None), (8, 3, 200), (8, 3, 100)]
# the generic route's reach: q = 5, 6, 7, the 16-bit handles BCH(511,484), BCH(1023,1003), and GF(2^14), t = 12, N = 3000
GENERIC = [(5, 2, None, None), (6, 3, None, None), (7, 3, None, None), (9, 3, None, 0x211), (10, 2, None, 0x409),
           (14, 12, 3000, 0x402B)]


def make(q, t, n=None, tag="BM", poly=None, coding="division"):
    return cc.primitive_bch(q, cc.errors(t), TAGS[tag](), coding=coding, n=n, modular_polynomial=poly)


def sym_dtype(code):
    return np.uint16 if code.wide else np.uint8


def received(code, rng, B, emax, emin=0):
    """random codewords and the same with emin .. emax bit errors per frame (uniform), error counts"""
    cw = code.encode_batch(rng.integers(0, 2, (B, code.l)).astype(sym_dtype(code)))
    ne = rng.integers(emin, emax + 1, B)
    order = rng.random((B, code.n)).argsort(axis=1)
    flips = np.zeros((B, code.n), cw.dtype)
    np.put_along_axis(flips, order, (np.arange(code.n)[None, :] < ne[:, None]).astype(cw.dtype), axis=1)
    return cw, cw ^ flips, ne


def pad_bits(packed, n):
    return np.unpackbits(np.ascontiguousarray(packed), axis=-1, bitorder="little")[:, n:]


def check_equal(code, rx, erasures=None, dirty_pad=False):
    """packed call against the byte call on the same frames; returns the byte call's result"""
    want = code.correct_batch(rx, erasures)
    pk = cc.pack_bits(rx)
    if dirty_pad and code.n % 8:
        pk[:, -1] |= (0xFF << (code.n % 8)) & 0xFF
    got = code.correct_batch(pk, erasures, packed=True)
    assert got["out"].shape == (rx.shape[0], code.packed_bytes) and got["out"].dtype == np.uint8
    assert np.array_equal(got["status"], want["status"])
    assert np.array_equal(got["nerr"], want["nerr"])
    assert np.array_equal(cc.unpack_bits(got["out"], code.n, sym_dtype(code)), want["out"])
    assert not pad_bits(got["out"], code.n).any()
    return want


@pytest.mark.parametrize("tag", ["PGZ", "BM", "EUKLID"])
@pytest.mark.parametrize("q,t,N", NATIVE)
def test_equal_to_the_byte_route_at_layout_boundaries(q, t, N, tag):
    code = make(q, t, N, tag)
    rng = np.random.default_rng(1000 * t + (N or 0) + len(tag))
    seen = {"corrected": 0, "clean": 0, "failed": 0, "locator": 0}
    for B in SIZES:
        assert code.packed_route(B) == 1  # (the suite runs with CC_AMD_PLANES_MIN_WORK=0)
        _, rx, _ = received(code, rng, B, t + 3)
        res = check_equal(code, rx, dirty_pad=B in (33, 2049))
        seen["corrected"] += int(((res["status"] == 0) & (res["nerr"] > 0)).sum())
        seen["clean"] += int(((res["status"] == 0) & (res["nerr"] == 0)).sum())
        seen["failed"] += int((res["status"] != 0).sum())
        seen["locator"] += int((res["status"] == capi.FRAME_LOCATOR).sum())
    assert seen["corrected"] > 0 and seen["clean"] > 0, seen
    # BCH(255,247) at full length is a perfect code (every non-zero syndrome is alpha^p of one position p < 255): it has
    # no failing frame; every other code of the list must show some
    if (t, N) != (1, None):
        assert seen["failed"] > 0, seen
    if N is not None:  # shortened: t + 1 or more errors bring locators with a root at a position >= N
        _, rx, _ = received(code, rng, 4161, t + 3, t + 1)
        res = check_equal(code, rx)
        assert (res["status"] == capi.FRAME_LOCATOR).any()


@pytest.mark.parametrize("q,t,N", NATIVE)
def test_torch_inputs_side_stream_and_in_place(q, t, N):
    code = make(q, t, N, "BM")
    rng = np.random.default_rng(77 + t + (N or 0))
    for B in (65, 2049):
        _, rx, _ = received(code, rng, B, t + 3)
        want = code.correct_batch(rx)
        pk = torch.from_numpy(cc.pack_bits(rx)).cuda()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = code.correct_batch(pk, packed=True)
            unp = cc.unpack_bits(got["out"], code.n)
            again = pk.clone()
            inplace = code.correct_batch(again, packed=True, out=again)  # out is in
        side.synchronize()
        assert inplace["out"] is again
        for res in (got, inplace):
            assert np.array_equal(res["status"].cpu().numpy(), want["status"])
            assert np.array_equal(res["nerr"].cpu().numpy(), want["nerr"])
            assert np.array_equal(cc.unpack_bits(res["out"].cpu().numpy(), code.n), want["out"])
        assert np.array_equal(unp.cpu().numpy(), want["out"])  # the device unpack kernel
        assert np.array_equal(cc.pack_bits(torch.from_numpy(rx).cuda()).cpu().numpy(), cc.pack_bits(rx))  # and pack


@pytest.mark.parametrize("tag", ["PGZ", "BM", "EUKLID"])
@pytest.mark.parametrize("q,t,N", NATIVE)
def test_bounded_distance_guarantee_and_parity(q, t, N, tag):
    """Nothing here is compared with the code under test: a codeword with e <= t flipped bits comes back as the
    codeword with nerr = e, status 0; and every frame with status 0 satisfies H out^T = 0 over GF(2)."""
    code = make(q, t, N, tag)
    rng = np.random.default_rng(5 * t + (N or 0))
    H = code.H().astype(np.int64)
    for e in range(t + 1):
        cw, rx, ne = received(code, rng, 4096, e, e)
        assert (ne == e).all() and ((cw ^ rx).sum(axis=1) == e).all()
        assert code.packed_route(4096) == 1
        res = code.correct_batch(cc.pack_bits(rx), packed=True)
        assert (res["status"] == 0).all() and (res["nerr"] == e).all(), e
        assert np.array_equal(cc.unpack_bits(res["out"], code.n), cw), e
    _, rx, _ = received(code, rng, 4096, t + 3)
    res = code.correct_batch(cc.pack_bits(rx), packed=True)
    out = cc.unpack_bits(res["out"], code.n).astype(np.int64)
    ok = res["status"] == 0
    assert ok.any() and not ((out[ok] @ H.T) & 1).any()


def test_native_against_generic_in_a_child_process(tmp_path):
    """CC_AMD_PACKED_NATIVE=0 (read once per process): the same calls through unpack / byte route / pack give
    identical bytes, and cc_packed_route says which route each process took."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import channelcoding_amd as cc\n"
        "from test_gpu_packed import GENERIC, NATIVE, make, received\n"
        "want = int(sys.argv[1])\n"
        "res = {}\n"
        "for q, t, N in NATIVE:\n"
        "    for tag in ('PGZ', 'BM', 'EUKLID'):\n"
        "        code = make(q, t, N, tag)\n"
        "        rng = np.random.default_rng(3 * t + (N or 0))\n"
        "        for B in (1, 65, 2049, 4161):\n"
        "            assert code.packed_route(B) == want, (q, t, N, B, code.packed_route(B))\n"
        "            _, rx, _ = received(code, rng, B, t + 3)\n"
        "            r = code.correct_batch(cc.pack_bits(rx), packed=True)\n"
        "            for k in ('out', 'nerr', 'status'):\n"
        "                res['%%d_%%d_%%s_%%s_%%d_%%s' %% (q, t, N, tag, B, k)] = r[k]\n"
        "for q, t, N, poly in [(q, t, N, None) for q, t, N in NATIVE] + GENERIC:\n"
        "    code = make(q, t, N, 'BM', poly)\n"
        "    assert code.packed_map_route(0) == (want if code.k <= 32 and q <= 8 else 0), (q, t, N)\n"
        "    assert code.packed_map_route(1) == want, (q, t, N)\n"
        "    rng = np.random.default_rng(7 * t + q)\n"
        "    for B in (1, 65, 2049):\n"
        "        pm = rng.integers(0, 256, (B, code.packed_message_bytes), dtype=np.uint8)\n"
        "        pc = rng.integers(0, 256, (B, code.packed_bytes), dtype=np.uint8)\n"
        "        res['enc_%%d_%%d_%%s_%%d' %% (q, t, N, B)] = code.encode_batch(pm, packed=True)\n"
        "        res['ext_%%d_%%d_%%s_%%d' %% (q, t, N, B)] = code.extract_batch(pc, packed=True)\n"
        "np.savez(sys.argv[2], **res)\n"
        "print('ROUTE OK')\n" % (here, os.path.dirname(here)))
    files = []
    for native in (1, 0):
        f = str(tmp_path / ("route%d.npz" % native))
        env = dict(os.environ, CC_AMD_PACKED_NATIVE=str(native))
        out = subprocess.run([sys.executable, "-c", script, str(native), f], env=env, capture_output=True, text=True,
                             timeout=900)
        assert out.returncode == 0 and "ROUTE OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
        files.append(np.load(f))
    a, b = files
    assert sorted(a.files) == sorted(b.files) and len(a.files) == len(NATIVE) * 3 * 4 * 3 + (len(NATIVE) + len(GENERIC)) * 3 * 2
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k
    assert make(8, 3).packed_route(64) == 1  # (this process: native)


@pytest.mark.parametrize("tag", ["PGZ", "BM", "EUKLID"])
@pytest.mark.parametrize("q,t,N,poly", GENERIC)
def test_generic_route_reach(q, t, N, poly, tag):
    code = make(q, t, N, tag, poly)
    rng = np.random.default_rng(100 * q + t)
    model = None
    if poly is not None:  # the 16-bit handles: the same frames against the 16-bit oracle as well
        model = WideOracle(BCH, q, t, poly)
        model = S.Shortened(model, N) if N else model
    for B in (1, 33, 700):
        assert code.packed_route(B) == 0
        _, rx, _ = received(code, rng, B, t + 3)
        want = check_equal(code, rx, dirty_pad=B == 33)
        if model is not None:
            alg = {"PGZ": PGZ, "BM": BM, "EUKLID": EUKLID}[tag]
            m_out, m_nerr, m_st = model.correct_hard(alg, rx)[:3]
            assert np.array_equal(want["status"] == 0, m_st == 0)
            assert np.array_equal(want["out"], np.where((m_st == 0)[:, None], m_out, rx))
            assert np.array_equal(want["nerr"], np.where(m_st == 0, m_nerr, -1))
            if alg == BM:
                assert np.array_equal(want["status"], S.native_status(m_st, want["status"]) if N else m_st)
    # torch: int16 symbols on the 16-bit handles
    _, rx, _ = received(code, rng, 65, t + 3)
    want = code.correct_batch(rx)
    got = code.correct_batch(torch.from_numpy(cc.pack_bits(rx)).cuda(), packed=True)
    assert np.array_equal(got["status"].cpu().numpy(), want["status"]) and np.array_equal(got["nerr"].cpu().numpy(), want["nerr"])
    sym = cc.unpack_bits(got["out"], code.n, torch.int16 if code.wide else torch.uint8)
    assert np.array_equal(sym.cpu().numpy().astype(rx.dtype), want["out"])


@pytest.mark.parametrize("tag", ["BM", "PGZ"])
@pytest.mark.parametrize("q,t", [(6, 3), (8, 3)])
def test_erasures_go_the_generic_way(q, t, tag):
    """Berlekamp-Massey with erasures and the two-trial PGZ rule (bch.h:97-149), against the byte call: 0 .. 2t + 1
    erasures per frame (beyond 2t: CC_FRAME_ERASURES), errors up to and beyond what is left of the capability."""
    code = make(q, t, None, tag)
    rng = np.random.default_rng(9 * q + t)
    for B in (1, 65, 333):
        cw, rx, _ = received(code, rng, B, 2)
        ers = []
        for f in range(B):
            er = sorted(rng.choice(code.n, int(rng.integers(0, 2 * t + 2)), replace=False).tolist())
            rx[f, er] = rng.integers(0, 2, len(er))
            ers.append(er)
        ers[0] = []
        res = check_equal(code, rx, ers)
        if B == 333:
            assert (res["status"] == 0).any() and (res["status"] != 0).any()
        # and through torch / the _dev call
        got = code.correct_batch(torch.from_numpy(cc.pack_bits(rx)).cuda(), ers, packed=True)
        assert np.array_equal(got["status"].cpu().numpy(), res["status"]) and np.array_equal(got["nerr"].cpu().numpy(), res["nerr"])
        assert np.array_equal(cc.unpack_bits(got["out"].cpu().numpy(), code.n), res["out"])


def test_refusals_of_the_16_bit_route_stay():
    """A 16-bit Euklid handle at t = 32 is refused by the packed call exactly as by its _u16 call."""
    code = cc.primitive_bch(10, cc.errors(32), cc.euklid_tag(), modular_polynomial=0x409)
    rx = np.zeros((2, code.n), np.uint16)
    with pytest.raises(cc.CcError) as a:
        code.correct_batch(rx)
    with pytest.raises(cc.CcError) as b:
        code.correct_batch(cc.pack_bits(rx), packed=True)
    assert a.value.status == b.value.status == capi.ERR_UNSUPPORTED
    assert str(a.value).split(":", 1)[1] == str(b.value).split(":", 1)[1]
    with pytest.raises(cc.CcError) as c:
        code.packed_route(2)
    assert c.value.status == capi.ERR_UNSUPPORTED


# every code of the two lists with division coding; multiplication coding where the library builds it (q <= 8)
ENCODE_CASES = [(q, t, N, None, c) for q, t, N in NATIVE for c in ("division", "multiplication")] + \
               [(q, t, N, poly, c) for q, t, N, poly in GENERIC for c in ("division", "multiplication") if c == "division" or q <= 8]


@pytest.mark.parametrize("q,t,N,poly,coding", ENCODE_CASES)
def test_encode_extract_decode(q, t, N, poly, coding):
    code = make(q, t, N, "BM", poly, coding)
    rng = np.random.default_rng(q + 10 * t)
    dt = sym_dtype(code)
    # which calls work on the packed words themselves: division coding; the encoder up to 32 parity bits, q <= 8
    assert code.packed_map_route(0) == int(coding == "division" and code.k <= 32 and q <= 8)
    assert code.packed_map_route(1) == int(coding == "division")
    for B in (1, 33, 2049):
        msg = rng.integers(0, 2, (B, code.l)).astype(dt)
        msg[0] = 0
        msg[-1] = 1
        cw = code.encode_batch(msg)
        pm = cc.pack_bits(msg)
        dirty = pm.copy()
        if code.l % 8:
            dirty[:, -1] |= (0xFF << (code.l % 8)) & 0xFF  # pad bits set to 1 change nothing
        for src in (pm, dirty, torch.from_numpy(dirty).cuda()):
            pcw = code.encode_batch(src, packed=True)
            pcw = pcw.cpu().numpy() if torch.is_tensor(pcw) else pcw
            assert pcw.shape == (B, code.packed_bytes)
            assert np.array_equal(cc.unpack_bits(pcw, code.n, dt), cw) and not pad_bits(pcw, code.n).any()
        _, rx, _ = received(code, rng, B, t + 3)
        want = code.extract_batch(rx)
        prx = cc.pack_bits(rx)
        if code.n % 8:
            prx[:, -1] |= (0xFF << (code.n % 8)) & 0xFF
        for src in (prx, torch.from_numpy(prx).cuda()):
            got = code.extract_batch(src, packed=True)
            got = got.cpu().numpy() if torch.is_tensor(got) else got
            assert got.shape == (B, code.packed_message_bytes)
            assert np.array_equal(cc.unpack_bits(got, code.l, dt), want) and not pad_bits(got, code.l).any()
        if code.wide:
            corr = code.correct_batch(rx)
            dec = dict(corr, msg=code.extract_batch(corr["out"]))
        else:
            dec = code.decode_batch(rx)
        for src in (prx, torch.from_numpy(prx).cuda()):
            got = code.decode_batch(src, packed=True)
            got = {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}
            assert np.array_equal(got["status"], dec["status"]) and np.array_equal(got["nerr"], dec["nerr"])
            assert np.array_equal(cc.unpack_bits(got["out"], code.n, dt), dec["out"])
            assert np.array_equal(cc.unpack_bits(got["msg"], code.l, dt), dec["msg"])
            assert not pad_bits(got["out"], code.n).any() and not pad_bits(got["msg"], code.l).any()


@pytest.mark.parametrize("q,t,N", NATIVE)
def test_empty_batches_and_exact_allocations(q, t, N):
    """B = 0 returns empty outputs.  A batch that ends on the last byte of its allocation: the kernels move whole dwords
    only where they lie inside the frame and the tail of a frame byte by byte (packed_words.hpp: load_word / store_word), so
    B * P bytes from the allocator are all a call needs -- for P = 25 and 13 too."""
    code = make(q, t, N, "BM")
    P = code.packed_bytes
    for empty in (np.zeros((0, P), np.uint8), torch.zeros((0, P), dtype=torch.uint8, device="cuda")):
        res = code.correct_batch(empty, packed=True)
        assert tuple(res["out"].shape) == (0, P) and res["status"].shape[0] == 0 and res["nerr"].shape[0] == 0
        assert tuple(code.extract_batch(empty, packed=True).shape) == (0, code.packed_message_bytes)
    assert tuple(code.encode_batch(np.zeros((0, code.packed_message_bytes), np.uint8), packed=True).shape) == (0, P)
    rng = np.random.default_rng(P)
    for B in (1, 37, 2051):
        _, rx, _ = received(code, rng, B, t + 3)
        want = code.correct_batch(rx)
        flat = torch.empty(B * P, dtype=torch.uint8, device="cuda")  # exactly B * P bytes
        flat.copy_(torch.from_numpy(cc.pack_bits(rx).reshape(-1)))
        out = torch.empty(B * P, dtype=torch.uint8, device="cuda")
        res = code.correct_batch(flat.view(B, P), packed=True, out=out.view(B, P))
        assert np.array_equal(res["status"].cpu().numpy(), want["status"])
        assert np.array_equal(cc.unpack_bits(out.view(B, P).cpu().numpy(), code.n), want["out"])
        sym = torch.empty(B * code.n, dtype=torch.uint8, device="cuda")
        sym.copy_(torch.from_numpy(rx.reshape(-1)))
        assert np.array_equal(cc.pack_bits(sym.view(B, code.n)).cpu().numpy(), cc.pack_bits(rx))
        assert np.array_equal(cc.unpack_bits(flat.view(B, P), code.n).cpu().numpy(), rx)


def test_long_locators_and_rechecks_reach_the_corrector():
    """The two rare branches of packed_fix_kernel, which stand in for chunk_fix_kernel, reached on purpose.
    Long locators (BM tag): a word of the t = 14 code plus w <= 12 errors has the 28 syndromes of a w-error pattern and a
    29th that does not fit, so Berlekamp-Massey on the 30 syndromes of BCH(255,139) jumps to L = 29 - w >= 17 at the
    last odd syndrome -- beyond the 17 coefficients of the plane search.
    Re-checks: a binary word without erasures never has L != deg lambda (every discrepancy at an even-indexed syndrome
    is zero, so the top coefficient of lambda never cancels: packed.hip, packed_fix_kernel), which is why no received
    word can be built for that class and why no CC_FRAME_RECHECK shows here; twelve batches of 2^16 words beyond the
    capability of short codes, whose low-degree locators often split in the field, are compared frame by frame and
    must agree on that too."""
    inner = make(8, 14)
    assert inner.k < make(8, 15).k
    rng = np.random.default_rng(2024)
    cw, _, _ = received(inner, rng, 8192, 0)
    w = rng.integers(0, 13, 8192)
    order = rng.random((8192, 255)).argsort(axis=1)
    flips = np.zeros((8192, 255), np.uint8)
    np.put_along_axis(flips, order, (np.arange(255)[None, :] < w[:, None]).astype(np.uint8), axis=1)
    for tag in ("BM", "PGZ", "EUKLID"):
        code = make(8, 15, None, tag)
        assert code.packed_route(8192) == 1
        res = check_equal(code, cw ^ flips)
        assert (res["status"] != 0).any()
    for t, N in ((2, None), (3, None), (3, 200), (2, 100)):
        for tag in ("BM", "PGZ", "EUKLID"):
            code = make(8, t, N, tag)
            _, rx, _ = received(code, rng, 1 << 16, t + 4, t + 1)
            assert code.packed_route(1 << 16) == 1
            res = check_equal(code, rx)
            assert (res["status"] != 0).any() and not (res["status"] == capi.FRAME_RECHECK).any()


def test_small_and_large_calls_at_default_settings():
    """Without CC_AMD_PLANES_MIN_WORK (the suite sets 0) a small GF(2^8) call takes the generic route -- unpack, one
    wavefront per frame in place, pack -- and a large one the native chain: the byte call's answers on both sides."""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "import channelcoding_amd as cc\n"
        "from test_gpu_packed import check_equal, make, received\n"
        "rng = np.random.default_rng(21)\n"
        "for t, N, sizes in ((3, None, ((1, 0), (33, 0), (65535, 0), (65536, 1))), (15, None, ((700, 0), (13107, 0), (13108, 1))),\n"
        "                    (3, 100, ((2049, 0), (65536, 1)))):\n"
        "    for tag in ('BM', 'PGZ'):\n"
        "        code = make(8, t, N, tag)\n"
        "        for B, route in sizes:\n"
        "            assert code.packed_route(B) == route, (t, N, B, code.packed_route(B))\n"
        "            _, rx, _ = received(code, rng, B, t + 3)\n"
        "            check_equal(code, rx, dirty_pad=True)\n"
        "print('DEFAULT OK')\n" % (here, os.path.dirname(here)))
    env = {k: v for k, v in os.environ.items() if k != "CC_AMD_PLANES_MIN_WORK"}
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "DEFAULT OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


def test_python_buffers_are_checked():
    code = make(8, 3)
    P = code.packed_bytes
    pk = torch.zeros((4, P), dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros((3, P), dtype=torch.uint8, device="cuda"), torch.zeros((4, P), dtype=torch.int8, device="cuda"),
                torch.zeros((4, P), dtype=torch.uint8), torch.zeros((4, 2 * P), dtype=torch.uint8, device="cuda")[:, ::2],
                np.zeros((4, P), np.uint8)):
        with pytest.raises(TypeError):
            code.correct_batch(pk, packed=True, out=bad)
    strided = torch.zeros((4, 2 * P), dtype=torch.uint8, device="cuda")[:, ::2]
    with pytest.raises(TypeError):
        code.correct_batch(strided, packed=True, out=strided)
    with pytest.raises(TypeError):
        code.correct_batch(np.zeros((4, P), np.uint8), packed=True, out=np.zeros((4, P + 1), np.uint8))
    with pytest.raises(TypeError):
        cc.pack_bits(torch.zeros((2, 16), dtype=torch.float16, device="cuda"))
    with pytest.raises(TypeError):
        cc.unpack_bits(pk, code.n, torch.bfloat16)
