"""Ordered-statistics decoding (cc_correct_osd_batch_dev, cc_mc_run_osd_dev) on one MI355X: decode rates
next to Chase-II and the hard decoder on the same values, and word error rates next to them.

    python profiles/tools/osd_bench.py rates    BCH(63,45), BCH(127,106), BCH(255,231): 2^20 frames of AWGN values
                                                resident in HBM at 4 and 6 dB; legs osd order 0, 1, 2, chase p = 4, 6 and
                                                the BM tag's cc_correct_hard_f32_batch_dev on the same buffer.  The order-2
                                                leg decodes the first 2^(--order2-log2) frames (default 2^20: all of
                                                them; the line says how many).  Three runs per leg, the legs alternating
                                                inside one process (run 1 of every leg, then run 2, ..), device events
                                                around each call after one warm-up call per leg; slowest - fastest
                                                reported, and the time per test pattern at order 2
    python profiles/tools/osd_bench.py wer      BCH(255,231), BCH(63,45) at 4, 5 and 6 dB, 2^22 frames per point (order 2:
                                                at most 2^(--order2-log2 + 2)), random codewords, seed 1 (the seed and
                                                points of chase_bench.py wer): osd order 0, 1, 2 against chase p = 6 and
                                                p = 0 (hard), with the undetected share.  One seed, no confidence intervals
    --frames-log2 K                             another number of frames per leg / point
    --order2-log2 K                             frames of the order-2 leg of `rates`
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

RATE_CODES = [(6, 3), (7, 3), (8, 3)]
WER_CODES = [(8, 3), (6, 3)]
ORDERS = (0, 1, 2)
PS = (4, 6)


def channel(code, ebno, frames):
    import torch
    from channelcoding_amd import capi
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, float(ebno), 1, 0, frames, 1, C.c_void_p(llr.data_ptr()), None, None),
               "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr


def timed_ms(call):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rates(frames, frames2):
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
            out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
            nerr = torch.empty(B, dtype=torch.int32, device="cuda")
            status = torch.empty(B, dtype=torch.int32, device="cuda")
            metric = torch.empty(B, dtype=torch.float32, device="cuda")
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            count = {"osd order=2": min(frames, frames2)}
            legs = {}
            for o in ORDERS:
                m = count.get("osd order=%d" % o, B)
                legs["osd order=%d" % o] = lambda o=o, m=m: capi.check(lib.cc_correct_osd_batch_dev(
                    code._h, ptr(llr), o, ptr(out), ptr(nerr), ptr(metric), ptr(status), m, stream), "osd")
            for p in PS:
                legs["chase p=%d" % p] = lambda p=p: capi.check(lib.cc_correct_chase_batch_dev(
                    code._h, ptr(llr), p, ptr(out), ptr(nerr), ptr(metric), ptr(status), B, stream), "chase")
            legs["hard BM"] = lambda: capi.check(lib.cc_correct_hard_f32_batch_dev(
                code._h, ptr(llr), None, None, ptr(out), ptr(nerr), ptr(status), B, stream), "hard")
            times = {k: [] for k in legs}
            for call in legs.values():  # warm-up: code objects, workspaces
                call()
                torch.cuda.synchronize()
            for _ in range(3):
                for k, call in legs.items():
                    times[k].append(timed_ms(call))
            print("%s  %d frames at %.0f dB, F = %d" % (code.to_string(), frames, ebno,
                                                       lib.cc_osd_frames_per_wavefront(code._h, 2)), flush=True)
            for k, ts in times.items():
                m = count.get(k, B)
                print("  %-12s %8d frames   ms %9.3f - %9.3f   M frames/s %8.3f - %8.3f   ns/frame %10.2f" % (
                    k, m, max(ts), min(ts), m / max(ts) / 1e3, m / min(ts) / 1e3, 1e6 * min(ts) / m), flush=True)
            l = code.l
            patterns = 1 + l + l * (l - 1) // 2
            per2 = 1e6 * min(times["osd order=2"]) / count["osd order=2"]
            per0 = 1e6 * min(times["osd order=0"]) / B
            print("  order 2: %.2f ns per frame over %d test patterns = %.4f ns per pattern; without the order-0 frame "
                  "time %.4f ns per pattern" % (per2, patterns, per2 / patterns, (per2 - per0) / (patterns - 1)), flush=True)
            del legs, llr, out, nerr, status, metric


def wer(frames, frames2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ChaseBackend, OsdBackend
    for q, t in WER_CODES:
        bm = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        decoders = [("osd order=%d" % o, OsdBackend(bm, o, True), frames2 if o == 2 else frames) for o in ORDERS]
        decoders += [("chase p=6", ChaseBackend(bm, 6, True), frames), ("hard (chase p=0)", ChaseBackend(bm, 0, True), frames)]
        print("%s  %d frames per point (order 2: %d), random codewords, seed 1: word errors (wer) / undetected" % (
            bm.to_string().split("-")[0], frames, frames2), flush=True)
        for ebno in (4.0, 5.0, 6.0):
            row = []
            for name, be, m in decoders:
                c = be.run(ebno, 1, 0, m).cpu().numpy()
                assert int(c[capi.MC_FRAMES]) == m
                row.append("%s %d (%.3e) / %d" % (name, int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_WORD_ERRORS]) / m,
                                                  int(c[capi.MC_UNDETECTED])))
            print("  %.0f dB  %s" % (ebno, "   ".join(row)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "wer"))
    ap.add_argument("--frames-log2", type=int, default=None)
    ap.add_argument("--order2-log2", type=int, default=20)
    a = ap.parse_args()
    if a.what == "rates":
        rates(1 << (a.frames_log2 if a.frames_log2 is not None else 20), 1 << a.order2_log2)
    else:
        frames = 1 << (a.frames_log2 if a.frames_log2 is not None else 22)
        wer(frames, min(frames, 1 << (a.order2_log2 + 2)))


if __name__ == "__main__":
    main()
