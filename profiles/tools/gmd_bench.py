"""GMD (cc_correct_gmd_batch_dev, cc_mc_run_gmd_dev) on one MI355X: decode rates next to the hard decoder and
to what a caller could do before -- one errors-and-erasures call per trial -- and word error counts against one trial.

    python profiles/tools/gmd_bench.py rates        RS(255,223), RS(255,239), RS(63,47): 2^20 frames of cc_awgn_symbols_dev
                                                    resident in HBM at 5 and 7 dB; legs gmd m = 1, ceil((t + 1) / 2), t + 1,
                                                    (a) the BM tag's cc_correct_hard_batch_dev on the same symbols and
                                                    (b) m calls of cc_correct_hard_batch_dev with the erasure CSR of trial
                                                    tau = 0 .. m - 1 (the lists made beforehand: the selection and the
                                                    metric are not counted).  Three runs per leg, the legs alternating
                                                    inside one process (run 1 of every leg, then run 2, ..), device events
                                                    around each leg after one warm-up per leg; slowest - fastest reported.
    python profiles/tools/gmd_bench.py wer          RS(255,223), RS(255,239) at 5, 6 and 7 dB, 2^22 frames per point,
                                                    random codewords, one seed: m = 1 against all trials
    --frames-log2 K                                 another number of frames per leg / point
    --only all                                      rates: only the m = t + 1 leg of RS(255,223) at 5 dB, five calls (for a
                                                    kernel trace in a run of its own)
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

RATE_CODES = [(8, 16), (8, 8), (6, 8)]
WER_CODES = [(8, 16), (8, 8)]


def channel(code, ebno, frames):
    import torch
    from channelcoding_amd import capi
    w = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    rel = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().cc_awgn_symbols_dev(code._h, float(ebno), 1, 0, frames, 1, C.c_void_p(w.data_ptr()),
                                              C.c_void_p(rel.data_ptr()), None, None), "cc_awgn_symbols_dev")
    torch.cuda.synchronize()
    return w, rel


def erasure_lists(rel, t, trials):
    """the CSR of every trial: (positions int16, offsets int32) with the 2 tau least reliable positions of each frame in
    ascending order"""
    import torch
    B = rel.shape[0]
    keys = rel.view(torch.int32) & 0x7FFFFFFF
    order = torch.sort(keys, dim=1, stable=True).indices[:, : 2 * t]
    lists = []
    for tau in range(trials):
        if tau == 0:
            lists.append((None, None))
            continue
        pos = torch.sort(order[:, : 2 * tau], dim=1).values.to(torch.int16).contiguous()
        off = (torch.arange(B + 1, device="cuda", dtype=torch.int64) * (2 * tau)).to(torch.int32)
        lists.append((pos, off))
    return lists


def legs_of(code, w, rel):
    """name -> call; every leg writes buffers of its own"""
    import torch
    from channelcoding_amd import capi
    lib = capi.lib()
    B, n = w.shape
    t = code.t
    out = torch.empty((B, n), dtype=torch.uint8, device="cuda")
    nerr = torch.empty(B, dtype=torch.int32, device="cuda")
    status = torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    ptr = lambda x: None if x is None else C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ms = sorted({1, (t + 2) // 2, t + 1})
    lists = erasure_lists(rel, t, t + 1)
    legs = {}
    for m in ms:
        legs["gmd m=%d" % m] = lambda m=m: capi.check(lib.cc_correct_gmd_batch_dev(
            code._h, ptr(w), ptr(rel), m, ptr(out), ptr(nerr), ptr(metric), ptr(status), B, stream), "gmd")
    legs["hard BM"] = lambda: capi.check(lib.cc_correct_hard_batch_dev(
        code._h, ptr(w), None, None, ptr(out), ptr(nerr), ptr(status), B, stream), "hard")

    def calls(m):
        for er, off in lists[:m]:
            capi.check(lib.cc_correct_hard_batch_dev(code._h, ptr(w), ptr(er), ptr(off), ptr(out), ptr(nerr), ptr(status), B,
                                                     stream), "hard with erasures")
    for m in ms[1:]:
        legs["%d calls" % m] = lambda m=m: calls(m)
    return legs, (out, nerr, status, metric, lists), status, ms


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
    import channelcoding_amd as cc
    for q, t in RATE_CODES[:1] if only else RATE_CODES:
        for ebno in (5.0,) if only else (5.0, 7.0):
            code = cc.rs(q, cc.errors(t), cc.berlekamp_massey_tag())
            w, rel = channel(code, ebno, frames)
            legs, keep, status, ms = legs_of(code, w, rel)
            if only:
                legs = {k: v for k, v in legs.items() if k == "gmd m=%d" % (t + 1)}
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
                print("  %-10s ms %8.3f - %8.3f   M frames/s %8.2f - %8.2f   ns/frame %8.2f   frames not decoded%s %d" % (
                    k, max(ts), min(ts), frames / max(ts) / 1e3, frames / min(ts) / 1e3, 1e6 * min(ts) / frames,
                    " (last call)" if k.endswith("calls") else "", failed[k]), flush=True)
            if "hard BM" in times:
                hard = 1e6 * min(times["hard BM"]) / frames
                for m in ms:
                    g = 1e6 * min(times["gmd m=%d" % m]) / frames
                    line = "  m = %2d: %.2f ns per frame = %.3f ns per trial; hard decoding %.2f ns per frame" % (m, g, g / m, hard)
                    if "%d calls" % m in times:
                        c = 1e6 * min(times["%d calls" % m]) / frames
                        line += "; %d calls %.2f ns per frame = %.3f ns per call" % (m, c, c / m)
                    print(line, flush=True)
            del legs, keep, w, rel


def wer(frames):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import GmdBackend
    for q, t in WER_CODES:
        code = cc.rs(q, cc.errors(t), cc.berlekamp_massey_tag())
        decoders = [("m=1", GmdBackend(code, 1, True)), ("m=%d" % (t + 1), GmdBackend(code, True, True))]
        print("%s  %d frames per point, random codewords, seed 1 (one seed: the counts carry its sampling error): "
              "word errors (wer) / undetected" % (code.to_string().split("-")[0], frames), flush=True)
        for ebno in (5.0, 6.0, 7.0):
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
    ap.add_argument("--only", choices=("all",))
    a = ap.parse_args()
    if a.what == "rates":
        rates(1 << (a.frames_log2 if a.frames_log2 is not None else 20), a.only)
    else:
        wer(1 << (a.frames_log2 if a.frames_log2 is not None else 22))


if __name__ == "__main__":
    main()
