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
    ap.add_argument("what", choices=("rates", "wer"))
    ap.add_argument("--frames-log2", type=int, default=None)
    ap.add_argument("--only", choices=("p6",))
    a = ap.parse_args()
    if a.what == "rates":
        rates(1 << (a.frames_log2 if a.frames_log2 is not None else 20), a.only)
    else:
        wer(1 << (a.frames_log2 if a.frames_log2 is not None else 22))


if __name__ == "__main__":
    main()
