"""Every host-pointer entry point across staging chunk boundaries, against its _dev twin.

The test starts this file as a process of its own with CC_AMD_HOST_CHUNK_BYTES=1 (the value is read once per process;
chunk_frames has a floor of 16 frames), so every host-pointer call below is cut into chunks of 16 frames, or of 15 at
interleaving depth 5.  The child reads include/channelcoding_amd.h: every cc_X for which cc_X_dev is declared too is a
host-pointer call, and the child fails for one it has not driven.  Each is made through ctypes on B = 37 frames, blocks
or streams (16 + 16 + 5: the third chunk reuses the first one's staging slot, a call of more than two chunks starts on
fresh streams, the last chunk is ragged; 35 = 15 + 15 + 5 at depth 5) and its outputs must equal, bit for bit, those
of the _dev twin on the same inputs in one launch -- with every optional output present, with every optional output
NULL and, where L or ext exists, with that alone NULL.  Calls that take erasure lists get ragged ones, none in the
first chunk and some in the later ones (the lists of a chunk are indexed by their global offsets), and run without
lists too.  cc_correct_hard_batch also runs in place.  The four cc_decode_*_batch calls, which have no _dev twin, are
checked against correct followed by extract.

The expected values come from the _dev twins, which the other suites pin to the models and the oracle.  Half of every
decoder's batch is lightly and half heavily disturbed, and the _dev result must hold both a decoded and a failed
frame.  Three decoders cannot fail on the codes used here, and the condition is another one: ordered-statistics
decoding and cc_product_decode on BCH(7,4)^2 and eBCH(8,4)^2 (a perfect code and its extension) must both leave frames
as they are and change frames, and GMD on RS(15,11) must hold both outcomes under one trial (under all t + 1 trials the
last one erases n - l positions, after which any word of an MDS code decodes; that run is compared all the same).

Shapes, the smallest that reach every call site: BCH(15,7), t = 2, under the BM and PGZ tags for the byte, f32, packed,
interleaved, Chase, Chase soft-output, extended Chase and OSD calls; min-sum on BCH(15,7); RS(15,11) for GMD;
BCH(511,493) for the 16-bit calls; BCH(7,4)^2 and eBCH(8,4)^2 for the product calls; the staircase of eBCH(16,11), 6
blocks, window 4, 2 iterations."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
B, I = 37, 5
BI = 35


def test_every_host_pointer_call_in_three_chunks_equals_its_dev_twin():
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "HOST CALLS OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def host_pointer_symbols():
    with open(os.path.join(ROOT, "include", "channelcoding_amd.h")) as f:
        names = set(re.findall(r"\b(cc_\w+)\s*\(", f.read()))
    return {n for n in names if n + "_dev" in names}


# ---- the child ----
def child():
    sys.path.insert(0, HERE)
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from interleave_model import interleave

    lib = capi.lib()
    rng = np.random.default_rng(2031)
    done, one_outcome = set(), []
    INF = float("inf")

    def host_ptr(a):
        return None if a is None else C.c_void_p(a.ctypes.data)

    def dev_copy(a):  # any dtype travels as its bytes
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    def dev_ptr(t):
        return None if t is None else C.c_void_p(t.data_ptr())

    def IN(a):
        return ("in", None if a is None else np.ascontiguousarray(a))

    def OUT(name, dtype, count, kind="must"):  # kind: must / opt (NULL allowed, buffer anyway) / drop (NULL: another kernel)
        return ("out", name, dtype, int(count), kind)

    def VAL(v):
        return ("val", v)

    def pair(sym, first, items, n, absent=()):
        """sym on host pointers and sym_dev on device pointers, the same inputs; returns the _dev outputs"""
        hargs, dargs, outs, keep = [first], [first], {}, []
        for it in items:
            if it == "B":
                hargs.append(n), dargs.append(n)
            elif it[0] == "val":
                hargs.append(it[1]), dargs.append(it[1])
            elif it[0] == "in":
                t = None if it[1] is None else dev_copy(it[1])
                keep.append(t)
                hargs.append(host_ptr(it[1])), dargs.append(dev_ptr(t))
            elif it[4] in absent:
                hargs.append(None), dargs.append(None)
            else:
                h = np.full(it[3] * np.dtype(it[2]).itemsize, 0xA5, np.uint8).view(it[2])  # both sides start from one poison
                t = dev_copy(h)
                outs[it[1]] = (h, t)
                hargs.append(host_ptr(h)), dargs.append(dev_ptr(t))
        capi.check(getattr(lib, sym + "_dev")(*dargs, None), sym + "_dev")
        torch.cuda.synchronize()
        capi.check(getattr(lib, sym)(*hargs), sym)
        res = {}
        for name, (h, t) in outs.items():
            res[name] = t.cpu().numpy().view(h.dtype)
            assert np.array_equal(h.view(np.uint8), res[name].view(np.uint8)), (sym, name, absent)
        done.add(sym)
        return res

    def variants(sym, first, items, n, mixed=None):
        kinds = {it[4] for it in items if it != "B" and it[0] == "out"}
        res = pair(sym, first, items, n)
        if mixed is not None and not mixed(res):  # (collected, so that one run names them all)
            one_outcome.append((sym, {k: v[:40] for k, v in res.items() if k in ("nerr", "status")}))
        if kinds & {"opt", "drop"}:
            pair(sym, first, items, n, ("opt", "drop"))
        if "drop" in kinds:
            pair(sym, first, items, n, ("drop",))
        return res

    def both_status(res):
        return bool((res["status"] == 0).any() and (res["status"] != 0).any())

    def ragged(frames, n, first):
        """erasure CSR: no erasure in frames < first, two in frame `first`, 0 .. 3 in the later ones"""
        er, off = [], [0]
        for f in range(frames):
            k = 0 if f < first else 2 if f == first else int(rng.integers(0, 4))
            er += sorted(rng.choice(n, k, replace=False).tolist())
            off.append(len(er))
        return np.array(er, np.uint16), np.array(off, np.uint32)

    def disturbed(cw, top, few, many):
        """codewords with 0 .. few symbol errors in the even frames and `many` in the odd ones"""
        rx = cw.copy()
        for f in range(rx.shape[0]):
            k = int(rng.integers(0, few + 1)) if f % 2 == 0 else many
            pos = rng.choice(rx.shape[1], k, replace=False)
            rx[f, pos] ^= rng.integers(1, top + 1, k).astype(rx.dtype)
        return rx

    def values(cw, quiet=0.35, loud=1.6):
        """BPSK values of code bits: sigma = quiet in the even frames, loud in the odd ones"""
        sigma = np.where(np.arange(cw.shape[0]) % 2 == 0, quiet, loud).reshape((-1,) + (1,) * (cw.ndim - 1))
        return ((1.0 - 2.0 * cw) + sigma * rng.standard_normal(cw.shape)).astype(np.float32)

    def hard_items(x, csr, dtype, count, frames, tail=()):
        return [IN(x), IN(csr[0]), IN(csr[1]), OUT("out", dtype, count), OUT("nerr", np.int32, frames, "opt"),
                OUT("status", np.int32, frames, "opt"), "B"] + [VAL(v) for v in tail]

    def map_items(x, dtype, count, tail=()):
        return [IN(x), OUT("out", dtype, count), "B"] + [VAL(v) for v in tail]

    NONE = (None, None)

    # ---- BCH(15,7), t = 2, under two tags: byte, f32, packed, interleaved, Chase, OSD ----
    for tag in (cc.berlekamp_massey_tag(), cc.peterson_gorenstein_zierler_tag()):
        code = cc.primitive_bch(4, cc.errors(2), tag)
        n, l, h = code.n, code.l, code._h
        assert (n, l) == (15, 7)
        msg = rng.integers(0, 2, (B, l)).astype(np.uint8)
        cw = variants("cc_encode_batch", h, map_items(msg, np.uint8, B * n), B)["out"].reshape(B, n)
        assert np.array_equal(variants("cc_extract_batch", h, map_items(cw, np.uint8, B * l), B)["out"].reshape(B, l), msg)
        rx = disturbed(cw, 1, 2, 4)
        y = ((1.0 - 2.0 * rx) * rng.uniform(0.5, 1.5, rx.shape)).astype(np.float32)
        pw = np.packbits(rx, axis=-1, bitorder="little")
        for csr in (ragged(B, n, 16), NONE):
            first = variants("cc_correct_hard_batch", h, hard_items(rx, csr, np.uint8, B * n, B), B, both_status)
            f32 = variants("cc_correct_hard_f32_batch", h, hard_items(y, csr, np.uint8, B * n, B), B, both_status)
            assert all(np.array_equal(first[k], f32[k]) for k in first)
            variants("cc_correct_hard_packed_batch", h, hard_items(pw, csr, np.uint8, B * 2, B), B, both_status)
            # in place: out == in on the host side
            work, nerr, status = rx.copy(), np.zeros(B, np.int32), np.zeros(B, np.int32)
            capi.check(lib.cc_correct_hard_batch(h, host_ptr(work), host_ptr(csr[0]), host_ptr(csr[1]), host_ptr(work), host_ptr(nerr),
                                                 host_ptr(status), B), "cc_correct_hard_batch in place")
            assert np.array_equal(work.reshape(-1), first["out"]) and np.array_equal(nerr, first["nerr"])
            assert np.array_equal(status, first["status"])
            # decode = correct + extract
            want_msg = variants("cc_extract_batch", h, map_items(first["out"], np.uint8, B * l), B)["out"]
            for sym, x in (("cc_decode_hard_batch", rx), ("cc_decode_hard_packed_batch", pw)):
                packed = sym.endswith("packed_batch")
                m = np.zeros(B * (1 if packed else l), np.uint8)
                w, ne, st = np.zeros((2 if packed else n) * B, np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32)
                capi.check(getattr(lib, sym)(h, host_ptr(x), host_ptr(csr[0]), host_ptr(csr[1]), host_ptr(m), host_ptr(w), host_ptr(ne),
                                             host_ptr(st), B), sym)
                assert np.array_equal(ne, first["nerr"]) and np.array_equal(st, first["status"]), sym
                if packed:
                    assert np.array_equal(np.unpackbits(w.reshape(B, 2), axis=-1, count=n, bitorder="little").reshape(-1), first["out"])
                    assert np.array_equal(np.unpackbits(m.reshape(B, 1), axis=-1, count=l, bitorder="little").reshape(-1), want_msg)
                else:
                    assert np.array_equal(w, first["out"]) and np.array_equal(m, want_msg), sym
        pm = np.packbits(msg, axis=-1, bitorder="little")
        pcw = variants("cc_encode_packed_batch", h, map_items(pm, np.uint8, B * 2), B)["out"]
        assert np.array_equal(pcw, np.packbits(cw, axis=-1, bitorder="little").reshape(-1))
        assert np.array_equal(variants("cc_extract_packed_batch", h, map_items(pcw, np.uint8, B), B)["out"], pm.reshape(-1))
        # interleaved, depth 5: 35 frames in chunks of 15
        imsg, icw, irx = interleave(msg[:BI], I), interleave(cw[:BI], I), interleave(rx[:BI], I)
        got = variants("cc_encode_interleaved_batch", h, map_items(imsg, np.uint8, BI * n, (I,)), BI)["out"]
        assert np.array_equal(got, icw.reshape(-1))
        got = variants("cc_extract_interleaved_batch", h, map_items(icw, np.uint8, BI * l, (I,)), BI)["out"]
        assert np.array_equal(got, imsg.reshape(-1))
        for csr in (ragged(BI, n, 15), NONE):
            res = variants("cc_correct_hard_interleaved_batch", h, hard_items(irx, csr, np.uint8, BI * n, BI, (I,)), BI, both_status)
            m, w, ne, st = np.zeros(BI * l, np.uint8), np.zeros(BI * n, np.uint8), np.zeros(BI, np.int32), np.zeros(BI, np.int32)
            capi.check(lib.cc_decode_hard_interleaved_batch(h, host_ptr(irx), host_ptr(csr[0]), host_ptr(csr[1]), host_ptr(m), host_ptr(w),
                                                            host_ptr(ne), host_ptr(st), BI, I), "cc_decode_hard_interleaved_batch")
            want = variants("cc_extract_interleaved_batch", h, map_items(res["out"], np.uint8, BI * l, (I,)), BI)["out"]
            assert np.array_equal(w, res["out"]) and np.array_equal(m, want)
            assert np.array_equal(ne, res["nerr"]) and np.array_equal(st, res["status"])
        # Chase-II (p = 1), its soft output, the extended code, OSD (order 1)
        llr = values(cw)
        soft = [OUT("out", np.uint8, B * n), OUT("nerr", np.int32, B, "opt"), OUT("metric", np.float32, B, "opt"),
                OUT("status", np.int32, B, "opt"), "B"]
        variants("cc_correct_chase_batch", h, [IN(llr), VAL(1)] + soft, B, both_status)
        variants("cc_correct_chase_soft_batch", h, [IN(llr), VAL(1), VAL(0.5), soft[0], OUT("ext", np.float32, B * n)] + soft[1:], B,
                 both_status)
        parity = cw.sum(axis=1, keepdims=True).astype(np.uint8) & 1
        ellr = values(np.concatenate([cw, parity], axis=1))
        variants("cc_correct_chase_extended_batch", h,
                 [IN(ellr), VAL(1), VAL(0.5), OUT("out", np.uint8, B * (n + 1)), OUT("ext", np.float32, B * (n + 1), "drop")] + soft[1:],
                 B, both_status)
        variants("cc_correct_osd_batch", h, [IN(llr), VAL(1)] + soft, B, lambda r: bool((r["nerr"] == 0).any() and (r["nerr"] > 0).any()))

    # ---- min-sum on BCH(15,7) ----
    ms = cc.primitive_bch(4, cc.errors(2), cc.min_sum_tag(5))
    cw = cc.primitive_bch(4, cc.errors(2), cc.berlekamp_massey_tag()).encode_batch(rng.integers(0, 2, (B, 7)).astype(np.uint8))
    llr = values(cw, 0.35, 1.2)
    for csr in (ragged(B, 15, 16), NONE):
        items = [IN(llr), IN(csr[0]), IN(csr[1]), OUT("hard", np.uint8, B * 15), OUT("L", np.float32, B * 15, "drop"),
                 OUT("iters", np.uint16, B, "opt"), OUT("status", np.int32, B, "opt"), "B"]
        res = variants("cc_correct_soft_batch", ms._h, items, B, both_status)
        m, w, it, st = np.zeros(B * 7, np.uint8), np.zeros(B * 15, np.uint8), np.zeros(B, np.uint16), np.zeros(B, np.int32)
        capi.check(lib.cc_decode_soft_batch(ms._h, host_ptr(llr), host_ptr(csr[0]), host_ptr(csr[1]), host_ptr(m), host_ptr(w),
                                            host_ptr(it), host_ptr(st), B), "cc_decode_soft_batch")
        want = variants("cc_extract_batch", ms._h, map_items(res["hard"], np.uint8, B * 7), B)["out"]
        assert np.array_equal(w, res["hard"]) and np.array_equal(m, want)
        assert np.array_equal(it, res["iters"]) and np.array_equal(st, res["status"])

    # ---- GMD on RS(15,11) ----
    rs = cc.rs(4, cc.errors(2), cc.berlekamp_massey_tag())
    assert (rs.n, rs.l) == (15, 11)
    cw = rs.encode_batch(rng.integers(0, 16, (B, 11)).astype(np.uint8))
    rx = disturbed(cw, 15, 3, 6)
    rel = np.where(rx == cw, rng.uniform(0.6, 1.0, rx.shape), rng.uniform(0.0, 0.7, rx.shape)).astype(np.float32)
    # one trial is bounded-distance decoding, which fails on most words with six errors.  With all t + 1 = 3 trials the
    # last one erases n - l = 4 positions, and any 11 symbols of an MDS word fix a codeword: no frame of this code can
    # fail, so that run is compared without the two-outcome condition
    for trials, mixed in ((1, both_status), (capi.GMD_ALL, None)):
        variants("cc_correct_gmd_batch", rs._h,
                 [IN(rx), IN(rel), VAL(trials), OUT("out", np.uint8, B * 15), OUT("nerr", np.int32, B, "opt"),
                  OUT("metric", np.float32, B, "opt"), OUT("status", np.int32, B, "opt"), "B"], B, mixed)

    # ---- 16-bit symbols: BCH(511, .), t = 2 ----
    wide = cc.primitive_bch(9, cc.errors(2), cc.berlekamp_massey_tag(), modular_polynomial=0x211)  # x^9 + x^4 + 1
    n, l, h = wide.n, wide.l, wide._h
    msg = rng.integers(0, 2, (B, l)).astype(np.uint16)
    cw = variants("cc_encode_batch_u16", h, map_items(msg, np.uint16, B * n), B)["out"].reshape(B, n)
    assert np.array_equal(variants("cc_extract_batch_u16", h, map_items(cw, np.uint16, B * l), B)["out"].reshape(B, l), msg)
    rx = disturbed(cw, 1, 2, 5)
    imsg, icw, irx = interleave(msg[:BI], I), interleave(cw[:BI], I), interleave(rx[:BI], I)
    assert np.array_equal(variants("cc_encode_interleaved_batch_u16", h, map_items(imsg, np.uint16, BI * n, (I,)), BI)["out"], icw.reshape(-1))
    assert np.array_equal(variants("cc_extract_interleaved_batch_u16", h, map_items(icw, np.uint16, BI * l, (I,)), BI)["out"], imsg.reshape(-1))
    for first in (16, None):
        variants("cc_correct_hard_batch_u16", h, hard_items(rx, ragged(B, n, first) if first else NONE, np.uint16, B * n, B), B, both_status)
        variants("cc_correct_hard_interleaved_batch_u16", h,
                 hard_items(irx, ragged(BI, n, first - 1) if first else NONE, np.uint16, BI * n, BI, (I,)), BI, both_status)

    # ---- product codes: BCH(7,4)^2 and eBCH(8,4)^2 ----
    comp = cc.primitive_bch(3, cc.errors(1), cc.berlekamp_massey_tag())
    for extended in (False, True):
        pc = cc.product_code(comp, comp, extended=extended)
        N, K = pc.n, pc.l
        plain, hard2, hard4 = pc._pc(), pc._pc_hard(2), pc._pc_hard(4)
        msg = rng.integers(0, 2, (B, K)).astype(np.uint8)
        cw = variants("cc_product_encode_batch", C.byref(plain), map_items(msg, np.uint8, B * N), B)["out"].reshape(B, N)
        assert np.array_equal(variants("cc_product_extract_batch", C.byref(plain), map_items(cw, np.uint8, B * K), B)["out"].reshape(B, K), msg)
        y = values(cw, 0.4, 1.3)
        z = (y < 0).astype(np.uint8)
        # an odd number of half-iterations ends on the rows.  BCH(7,4) is perfect and the extended decoder sets the parity
        # bit of what it finds: no line of either code can fail, whatever p.  The two outcomes of this call are blocks that
        # come back as the hard decisions of y and blocks the decoder changed
        lines = pc.n2
        turbo = pc._pc(2, (0.3, 0.5, 0.7), (0.2, 0.4, 0.6))

        def changed_and_unchanged(r):
            changed = (r["out"].reshape(B, N) != z.reshape(B, N)).any(axis=1)
            return bool(changed.any() and (~changed).any() and not r["status"].any())

        variants("cc_product_decode", C.byref(turbo),
                 [IN(y), OUT("out", np.uint8, B * N), OUT("ext", np.float32, B * N, "drop"), OUT("status", np.int32, B * lines), "B"], B,
                 changed_and_unchanged)
        counts = [OUT("nflip", np.int32, B, "opt"), OUT("last", np.int32, B, "opt"), OUT("status", np.int32, B, "opt")]
        variants("cc_product_decode_hard", C.byref(hard4), [IN(z), OUT("out", np.uint8, B * N)] + counts + ["B"], B, both_status)
        variants("cc_product_decode_anchor", C.byref(hard4),
                 [VAL(1), IN(z), OUT("out", np.uint8, B * N)] + counts + [OUT("nback", np.int32, B, "opt"), OUT("nconf", np.int32, B, "opt"), "B"],
                 B, both_status)
        fw = (C.c_float * 2)(0.6, INF)
        variants("cc_product_decode_sr", C.byref(hard2), [VAL(fw), IN(y), OUT("out", np.uint8, B * N)] + counts + ["B"], B, both_status)

    # ---- the staircase of eBCH(16,11): 6 blocks, window 4, 2 iterations ----
    sc = cc.staircase_code(cc.primitive_bch(4, cc.errors(1), cc.berlekamp_massey_tag()), 6, 4, 2, extended=True)
    desc = sc._sc()
    msg = rng.integers(0, 2, (B, sc.l)).astype(np.uint8)
    cw = variants("cc_staircase_encode_batch", C.byref(desc), map_items(msg, np.uint8, B * sc.n), B)["out"].reshape(B, sc.n)
    assert np.array_equal(variants("cc_staircase_extract_batch", C.byref(desc), map_items(cw, np.uint8, B * sc.l), B)["out"].reshape(B, sc.l), msg)
    y = values(cw, 0.35, 0.9)
    counts = [OUT("nflip", np.int32, B, "opt"), OUT("status", np.int32, B, "opt"), "B"]
    variants("cc_staircase_decode", C.byref(desc), [IN((y < 0).astype(np.uint8)), OUT("out", np.uint8, B * sc.n)] + counts, B, both_status)
    fw = (C.c_float * 4)(0.5, 0.9, 1.3, INF)
    variants("cc_staircase_decode_sr", C.byref(desc), [VAL(fw), IN(y), OUT("out", np.uint8, B * sc.n)] + counts, B, both_status)

    assert not one_outcome, ("a decoder's batch holds one outcome only", one_outcome)
    symbols = host_pointer_symbols()
    assert len(symbols) >= 32 and symbols == done, ("no driver for", sorted(symbols - done), "not in the header", sorted(done - symbols))
    print("HOST CALLS OK: %d host-pointer entry points" % len(done))


if __name__ == "__main__":
    child()
