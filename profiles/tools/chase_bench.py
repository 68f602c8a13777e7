"""Chase-II (cc_correct_chase_batch_dev, cc_mc_run_chase_dev) on one MI355X: decode rates next to the hard
decoder and to min-sum on the same values, and word error rates next to min-sum.

    python profiles/tools/chase_bench.py rates      BCH(255,231), BCH(127,106), BCH(63,45): 2^20 frames of AWGN values
                                                    resident in HBM at 4 and 6 dB; legs chase p = 0, 2, 4, 6, the BM tag's
                                                    cc_correct_hard_f32_batch_dev and MS<20> on the same buffer.  Three runs
                                                    per leg, the legs alternating inside one process (run 1 of every leg,
                                                    then run 2, ..), device events around each call after one warm-up
                                                    call per leg; slowest - fastest reported.
    python profiles/tools/chase_bench.py wer        BCH(255,231), BCH(63,45) at 4, 5 and 6 dB, 2^22 frames per point,
                                                    random codewords, one seed: chase p = 0, 4, 6 against MS<20> and
                                                    NMS<20> (alpha = 8/10)
    python profiles/tools/chase_bench.py soft       the soft output (cc_correct_chase_soft_batch_dev) on the
                                                    codes, p values and noise points of `rates`: legs soft p, chase p of
                                                    this build and, with --parent-lib, chase p of the parent commit's
                                                    library loaded next to it; alternation and timing as in `rates`, the
                                                    legs of a p taking turns at going first;
                                                    then the soft leg's time as a ratio to the chase leg of the same p
    python profiles/tools/chase_bench.py product    BCH(63,45) x BCH(63,45) at 3.0 dB, 2^12 blocks from numpy seed 1:
                                                    block errors of cc.product_decode (p = 4, Pyndiah's alpha and beta
                                                    of six half-iterations) after every half-iteration, against hard
                                                    decoding of rows then columns
    python profiles/tools/chase_bench.py extended   the extended call (cc_correct_chase_extended_batch_dev)
                                                    on the codes and p values of `rates` at 4 dB: legs ext-hard p (ext
                                                    NULL) and ext-soft p on rows of n + 1 values -- the parity value of
                                                    the transmitted word plus noise of the same sigma appended to every
                                                    frame -- next to chase p and soft p of this build on the n inner
                                                    values and, with --parent-lib, chase p and soft p of the parent
                                                    commit's library loaded next to it; alternation and timing as in
                                                    `soft`; then the ratios extended / plain with F of both, and the
                                                    existing calls against the parent's spread
    python profiles/tools/chase_bench.py product-ext  eBCH(64,51) x eBCH(64,51) against BCH(63,51) x BCH(63,51) at the
                                                    same Eb/N0 (--ebno, default 3.0 dB; each code's own rate in the noise
                                                    variance), 2^12 blocks from numpy seed 1, the same information bits:
                                                    block errors of cc.product_decode (p = 4, the alpha and beta of
                                                    `product`) after every half-iteration
    --parent-lib PATH                               soft, extended: libchannelcoding_amd.so built from the parent commit
    --ebno DB                                       product-ext: the noise point
    --frames-log2 K                                 another number of frames per leg / point
    --only p6                                       rates: only the p = 6 leg of BCH(255,231) at 4 dB, five calls (for a
                                                    rocprofv3 run of its own)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

RATE_CODES = [(8, 3), (7, 3), (6, 3)]
WER_CODES = [(8, 3), (6, 3)]
PS = (0, 2, 4, 6)


def channel(code, ebno, frames):
    import torch
    from channelcoding_amd import capi
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, float(ebno), 1, 0, frames, 1, C.c_void_p(llr.data_ptr()), None, None),
               "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr


def legs_of(q, t, llr):
    """name -> (call, buffers kept alive); every leg writes buffers of its own"""
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    B, n = llr.shape
    bm = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
    ms = cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(20))
    out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    nerr = torch.empty(B, dtype=torch.int32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    iters = torch.empty(B, dtype=torch.int16, device="cuda")
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    legs = {}
    for p in PS:
        legs["chase p=%d" % p] = lambda p=p: capi.check(lib.cc_correct_chase_batch_dev(
            bm._h, ptr(llr), p, ptr(out), ptr(nerr), ptr(metric), ptr(status), B, stream), "chase")
    legs["hard BM"] = lambda: capi.check(lib.cc_correct_hard_f32_batch_dev(
        bm._h, ptr(llr), None, None, ptr(out), ptr(nerr), ptr(status), B, stream), "hard")
    legs["MS<20>"] = lambda: capi.check(lib.cc_correct_soft_batch_dev(
        ms._h, ptr(llr), None, None, ptr(out), None, ptr(iters), ptr(status), B, stream), "soft")
    return legs, (bm, ms, out, nerr, status, metric, iters), status


def timed_ms(call):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rates(frames, only):
    import torch
    for q, t in RATE_CODES[:1] if only else RATE_CODES:
        for ebno in (4.0,) if only else (4.0, 6.0):
            import channelcoding_amd as cc
            code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
            llr = channel(code, ebno, frames)
            legs, keep, status = legs_of(q, t, llr)
            if only:
                legs = {k: v for k, v in legs.items() if k == "chase p=6"}
            times = {k: [] for k in legs}
            failed = {}
            for k, call in legs.items():  # warm-up: code objects, workspaces
                call()
                torch.cuda.synchronize()
                failed[k] = int((status != 0).sum())
            for _ in range(5 if only else 3):
                for k, call in legs.items():
                    times[k].append(timed_ms(call))
            print("%s  %d frames at %.0f dB" % (code.to_string(), frames, ebno), flush=True)
            for k, ts in times.items():
                print("  %-10s ms %8.3f - %8.3f   M frames/s %8.2f - %8.2f   ns/frame %8.2f   frames not decoded %d" % (
                    k, max(ts), min(ts), frames / max(ts) / 1e3, frames / min(ts) / 1e3, 1e6 * min(ts) / frames, failed[k]),
                    flush=True)
            if "hard BM" in times:
                per_frame, hard = 1e6 * min(times["chase p=6"]) / frames, 1e6 * min(times["hard BM"]) / frames
                print("  p = 6: %.2f ns per frame = %.3f ns per test pattern; hard decoding %.2f ns per frame" % (
                    per_frame, per_frame / 64, hard), flush=True)
            del legs, keep, llr


def frames_per_wave(code, p, soft):
    """F of launch_chase_soft (soft) or launch_chase at p, asked of the library"""
    from channelcoding_amd import capi
    return capi.lib().cc_chase_frames_per_wavefront(code._h, p, int(soft))


def parent_chase(path, code, soft=False):
    """cc_correct_chase_batch_dev (soft: cc_correct_chase_soft_batch_dev) of the library at `path`, on a handle that
    library creates from the code's descriptor"""
    lib = C.CDLL(path)
    h = C.c_void_p()
    lib.cc_code_create.restype = C.c_int
    lib.cc_code_create.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.cc_code_create(C.byref(code._desc), C.byref(h)) == 0
    fn = lib.cc_correct_chase_soft_batch_dev if soft else lib.cc_correct_chase_batch_dev
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + ([C.c_float] if soft else []) + [C.c_void_p] * (5 if soft else 4) \
        + [C.c_size_t, C.c_void_p]
    return lib, h, fn


def soft(frames, parent_lib):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    for q, t in RATE_CODES:
        for ebno in (4.0, 6.0):
            code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
            llr = channel(code, ebno, frames)
            B, n = llr.shape
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            bufs = {}
            for leg in ("soft", "chase", "parent"):
                bufs[leg] = dict(out=torch.empty((B, n), dtype=torch.uint8, device="cuda"),
                                 nerr=torch.empty(B, dtype=torch.int32, device="cuda"),
                                 status=torch.empty(B, dtype=torch.int32, device="cuda"),
                                 metric=torch.empty(B, dtype=torch.float32, device="cuda"))
            ext = torch.empty((B, n), dtype=torch.float32, device="cuda")
            parent = parent_chase(parent_lib, code) if parent_lib else None
            legs = {}
            for p in PS:
                b = bufs["soft"]
                legs["soft p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_soft_batch_dev(
                    code._h, ptr(llr), p, 0.5, ptr(b["out"]), ptr(ext), ptr(b["nerr"]), ptr(b["metric"]), ptr(b["status"]), B,
                    stream), "soft")
                b = bufs["chase"]
                legs["chase p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_batch_dev(
                    code._h, ptr(llr), p, ptr(b["out"]), ptr(b["nerr"]), ptr(b["metric"]), ptr(b["status"]), B, stream), "chase")
                if parent:
                    b = bufs["parent"]
                    legs["parent p=%d" % p] = lambda p=p, b=b: capi.check(parent[2](
                        parent[1], ptr(llr), p, ptr(b["out"]), ptr(b["nerr"]), ptr(b["metric"]), ptr(b["status"]), B, stream),
                        "parent")
            times = {k: [] for k in legs}
            for k, call in legs.items():  # warm-up: code objects
                call()
                torch.cuda.synchronize()
                if not k.startswith("soft"):  # the three legs of a p agree on the four outputs
                    for name, v in bufs[k.split()[0]].items():
                        assert torch.equal(v.view(torch.uint8), bufs["soft"][name].view(torch.uint8)), (k, name)
            names = list(legs)
            per_p = len(names) // len(PS)
            for run in range(3):  # the legs of a p take turns at going first, so that no leg always follows the same one
                for g in range(0, len(names), per_p):
                    for i in range(per_p):
                        k = names[g + (i + run) % per_p]
                        times[k].append(timed_ms(legs[k]))
            print("%s  %d frames at %.0f dB" % (code.to_string(), frames, ebno), flush=True)
            for k, ts in times.items():
                p = int(k.split("=")[1])
                print("  %-11s ms %8.3f - %8.3f   ns/frame %8.2f   F %2d" % (
                    k, max(ts), min(ts), 1e6 * min(ts) / frames, frames_per_wave(code, p, k.startswith("soft"))),
                    flush=True)
            for p in PS:
                s_, c_ = times["soft p=%d" % p], times["chase p=%d" % p]
                line = "  p = %d: soft / chase = %.2f - %.2f (fastest / fastest %.2f)" % (
                    p, min(s_) / max(c_), max(s_) / min(c_), min(s_) / min(c_))
                if parent:
                    a_ = times["parent p=%d" % p]
                    inside = min(a_) <= min(c_) <= max(a_) or min(a_) <= max(c_) <= max(a_) or (min(c_) <= min(a_) and max(c_) >= max(a_))
                    line += "; chase %.3f - %.3f ms against the parent's %.3f - %.3f ms: %s" % (
                        max(c_), min(c_), max(a_), min(a_), "within its spread" if inside else (
                            "FASTER than its fastest" if max(c_) < min(a_) else "SLOWER than its slowest"))
                print(line, flush=True)
            del legs, bufs, ext, llr


def spread(ts):
    return "%.3f - %.3f" % (max(ts), min(ts))


def against(mine, theirs):
    inside = min(theirs) <= min(mine) <= max(theirs) or min(theirs) <= max(mine) <= max(theirs) or (
        min(mine) <= min(theirs) and max(mine) >= max(theirs))
    return "within its spread" if inside else ("FASTER than its fastest" if max(mine) < min(theirs) else "SLOWER than its slowest")


def extended(frames, parent_lib):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    ebno = 4.0
    for q, t in RATE_CODES:
        code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        B, n = frames, code.n
        llr = torch.empty((B, n), dtype=torch.float32, device="cuda")
        sent = torch.empty((B, n), dtype=torch.uint8, device="cuda")
        capi.check(lib.cc_awgn_llr_dev(code._h, ebno, 1, 0, B, 1, ptr(llr), ptr(sent), None), "cc_awgn_llr_dev")
        gen = torch.Generator(device="cuda").manual_seed(1)
        parity = (sent.sum(dim=1, dtype=torch.int32) & 1).to(torch.float32)
        yn = (1.0 - 2.0 * parity) + lib.cc_sigma(code._h, ebno) * torch.randn(B, generator=gen, device="cuda")
        wide = torch.cat([llr, yn[:, None]], dim=1).contiguous()
        del sent, parity, yn
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        kinds = ["ext-hard", "chase", "ext-soft", "soft"] + (["parent-chase", "parent-soft"] if parent_lib else [])
        bufs = {}
        for leg in kinds:
            w = n + 1 if leg.startswith("ext") else n
            bufs[leg] = dict(out=torch.empty((B, w), dtype=torch.uint8, device="cuda"),
                             nerr=torch.empty(B, dtype=torch.int32, device="cuda"),
                             status=torch.empty(B, dtype=torch.int32, device="cuda"),
                             metric=torch.empty(B, dtype=torch.float32, device="cuda"))
            if leg.endswith("soft"):
                bufs[leg]["ext"] = torch.empty((B, w), dtype=torch.float32, device="cuda")
        parents = (parent_chase(parent_lib, code), parent_chase(parent_lib, code, True)) if parent_lib else None
        four = lambda b: (ptr(b["nerr"]), ptr(b["metric"]), ptr(b["status"]), B, stream)
        legs = {}
        for p in PS:
            b = bufs["ext-hard"]
            legs["ext-hard p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_extended_batch_dev(
                code._h, ptr(wide), p, 0.5, ptr(b["out"]), None, *four(b)), "ext-hard")
            b = bufs["chase"]
            legs["chase p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_batch_dev(
                code._h, ptr(llr), p, ptr(b["out"]), *four(b)), "chase")
            if parents:
                b = bufs["parent-chase"]
                legs["parent-chase p=%d" % p] = lambda p=p, b=b: capi.check(parents[0][2](
                    parents[0][1], ptr(llr), p, ptr(b["out"]), *four(b)), "parent-chase")
            b = bufs["ext-soft"]
            legs["ext-soft p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_extended_batch_dev(
                code._h, ptr(wide), p, 0.5, ptr(b["out"]), ptr(b["ext"]), *four(b)), "ext-soft")
            b = bufs["soft"]
            legs["soft p=%d" % p] = lambda p=p, b=b: capi.check(lib.cc_correct_chase_soft_batch_dev(
                code._h, ptr(llr), p, 0.5, ptr(b["out"]), ptr(b["ext"]), *four(b)), "soft")
            if parents:
                b = bufs["parent-soft"]
                legs["parent-soft p=%d" % p] = lambda p=p, b=b: capi.check(parents[1][2](
                    parents[1][1], ptr(llr), p, 0.5, ptr(b["out"]), ptr(b["ext"]), *four(b)), "parent-soft")
        times = {k: [] for k in legs}
        failed = {}
        for k, call in legs.items():  # warm-up: code objects; the legs that must agree do
            call()
            torch.cuda.synchronize()
            kind = k.split()[0]
            failed[k] = int((bufs[kind]["status"] != 0).sum())
            twin = {"ext-soft": "ext-hard", "parent-chase": "chase", "soft": "chase", "parent-soft": "soft"}.get(kind)
            if twin:
                for name, v in bufs[kind].items():
                    if name in bufs[twin]:
                        assert torch.equal(v.view(torch.uint8), bufs[twin][name].view(torch.uint8)), (k, name)
        names = list(legs)
        per_p = len(names) // len(PS)
        for run in range(3):  # the legs of a p take turns at going first
            for g in range(0, len(names), per_p):
                for i in range(per_p):
                    k = names[g + (i + run) % per_p]
                    times[k].append(timed_ms(legs[k]))
        print("%s and its extended code, %d frames at %.0f dB" % (code.to_string(), frames, ebno), flush=True)
        F = lambda k, p: (lib.cc_chase_extended_frames_per_wavefront if k.startswith("ext") else lib.cc_chase_frames_per_wavefront)(
            code._h, p, int(k.split()[0].endswith("soft")))
        for k, ts in times.items():
            p = int(k.split("=")[1])
            print("  %-17s ms %8.3f - %8.3f   ns/frame %8.2f   F %2d   frames not decoded %d" % (
                k, max(ts), min(ts), 1e6 * min(ts) / frames, F(k, p), failed[k]), flush=True)
        for p in PS:
            for e, c in (("ext-hard", "chase"), ("ext-soft", "soft")):
                e_, c_ = times["%s p=%d" % (e, p)], times["%s p=%d" % (c, p)]
                fe, fc = F(e, p), F(c, p)
                line = "  p = %d: %s / %s = %.3f - %.3f (fastest / fastest %.3f; (n + 1) / n = %.3f); F %d against %d: %s" % (
                    p, e, c, min(e_) / max(c_), max(e_) / min(c_), min(e_) / min(c_), (n + 1) / n, fe, fc,
                    "the wider rows alone" if fe == fc else "the wider rows lower F")
                if parents:
                    a_ = times["parent-%s p=%d" % (c, p)]
                    line += "; %s %s ms against the parent's %s ms: %s" % (c, spread(c_), spread(a_), against(c_, a_))
                print(line, flush=True)
        del legs, bufs, llr, wide


def product_ext(blocks, ebno):
    import numpy as np
    import torch
    import channelcoding_amd as cc
    code = cc.primitive_bch(6, cc.errors(2), cc.berlekamp_massey_tag())
    n, l = code.n, code.l
    alpha, beta = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9), (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
    info = np.random.default_rng(1).integers(0, 2, (blocks, l, l)).astype(np.uint8)
    for extended in (False, True):
        w = n + 1 if extended else n
        widen = cc.extend if extended else (lambda a: a)
        wide = widen(code.encode_batch(info.reshape(-1, l))).reshape(blocks, l, w)
        sent = widen(code.encode_batch(np.ascontiguousarray(wide.transpose(0, 2, 1)).reshape(-1, l))).reshape(blocks, w, w)
        sent = np.ascontiguousarray(sent.transpose(0, 2, 1))
        rate = (l / w) ** 2
        sigma = 1.0 / np.sqrt(2.0 * rate * 10.0 ** (ebno / 10.0))
        noise = np.random.default_rng(2).standard_normal(sent.shape).astype(np.float32)
        y = torch.from_numpy(((1.0 - 2.0 * sent.astype(np.float32)) + np.float32(sigma) * noise).astype(np.float32)).cuda()
        truth = torch.from_numpy(sent).cuda()
        errors = lambda out: int((out != truth).any(dim=2).any(dim=1).sum())
        name = "eBCH(%d,%d)" % (w, l) if extended else "BCH(%d,%d)" % (n, l)
        print("%s x %s, rate %.4f, sigma %.4f, %d blocks at %.2f dB, numpy seeds 1 (bits) and 2 (noise): block errors" % (
            name, name, rate, sigma, blocks, ebno))
        print("  channel decisions %d" % errors((y < 0).to(torch.uint8)), flush=True)
        for halves in range(1, len(alpha) + 1):
            res = cc.product_decode(code, code, y, 4, alpha[:halves], beta[:halves], extended=extended)
            print("  product_decode p = 4, %d half-iterations: %d" % (halves, errors(res["out"])), flush=True)


def product(blocks):
    import numpy as np
    import torch
    import channelcoding_amd as cc
    code = cc.primitive_bch(6, cc.errors(3), cc.berlekamp_massey_tag())
    n, l, ebno = code.n, code.l, 3.0
    rng = np.random.default_rng(1)
    info = rng.integers(0, 2, (blocks, l, l)).astype(np.uint8)
    wide = code.encode_batch(info.reshape(-1, l)).reshape(blocks, l, n)
    sent = code.encode_batch(np.ascontiguousarray(wide.transpose(0, 2, 1)).reshape(-1, l)).reshape(blocks, n, n)
    sent = np.ascontiguousarray(sent.transpose(0, 2, 1))
    sigma = 1.0 / np.sqrt(2.0 * (l / n) ** 2 * 10.0 ** (ebno / 10.0))
    y = ((1.0 - 2.0 * sent.astype(np.float32)) + np.float32(sigma) * rng.standard_normal(sent.shape).astype(np.float32))
    y = torch.from_numpy(y.astype(np.float32)).cuda()
    truth = torch.from_numpy(sent).cuda()
    errors = lambda out: int((out != truth).any(dim=2).any(dim=1).sum())
    rows = code.correct_batch(y.reshape(-1, n))["out"].reshape(blocks, n, n)  # hard decoding: rows, then columns
    cols = code.correct_batch(rows.transpose(1, 2).contiguous().reshape(-1, n))["out"].reshape(blocks, n, n).transpose(1, 2)
    alpha, beta = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9), (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
    print("BCH(63,45) x BCH(63,45), rate %.3f, %d blocks at %.1f dB, numpy seed 1: block errors" % ((l / n) ** 2, blocks, ebno))
    print("  channel decisions %d   hard rows %d   hard rows then columns %d" % (
        errors((y < 0).to(torch.uint8)), errors(rows), errors(cols)), flush=True)
    for halves in range(1, len(alpha) + 1):
        res = cc.product_decode(code, code, y, 4, alpha[:halves], beta[:halves])
        print("  product_decode p = 4, %d half-iterations: %d" % (halves, errors(res["out"])), flush=True)


def wer(frames):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ChaseBackend, DeviceBackend
    for q, t in WER_CODES:
        bm = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        decoders = [("chase p=%d" % p, ChaseBackend(bm, p, True)) for p in (0, 4, 6)]
        decoders.append(("MS<20>", DeviceBackend(cc.primitive_bch(q, cc.errors(t), cc.min_sum_tag(20)), True)))
        decoders.append(("NMS<20> 8/10", DeviceBackend(cc.primitive_bch(q, cc.errors(t), cc.normalized_min_sum_tag(20, 8 / 10)), True)))
        print("%s  %d frames per point, random codewords, seed 1: word errors (wer) / undetected" % (
            bm.to_string().split("-")[0], frames), flush=True)
        for ebno in (4.0, 5.0, 6.0):
            row = []
            for name, be in decoders:
                c = be.run(ebno, 1, 0, frames).cpu().numpy()
                assert int(c[capi.MC_FRAMES]) == frames
                row.append("%s %d (%.3e) / %d" % (name, int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_WORD_ERRORS]) / frames,
                                                  int(c[capi.MC_UNDETECTED])))
            print("  %.0f dB  %s" % (ebno, "   ".join(row)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "wer", "soft", "product", "extended", "product-ext"))
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--frames-log2", type=int, default=None)
    ap.add_argument("--only", choices=("p6",))
    ap.add_argument("--ebno", type=float, default=3.0)
    a = ap.parse_args()
    if a.what == "rates":
        rates(1 << (a.frames_log2 if a.frames_log2 is not None else 20), a.only)
    elif a.what == "soft":
        soft(1 << (a.frames_log2 if a.frames_log2 is not None else 20), a.parent_lib)
    elif a.what == "extended":
        extended(1 << (a.frames_log2 if a.frames_log2 is not None else 20), a.parent_lib)
    elif a.what == "product-ext":
        product_ext(1 << (a.frames_log2 if a.frames_log2 is not None else 12), a.ebno)
    elif a.what == "product":
        product(1 << (a.frames_log2 if a.frames_log2 is not None else 12))
    else:
        wer(1 << (a.frames_log2 if a.frames_log2 is not None else 22))


if __name__ == "__main__":
    main()
