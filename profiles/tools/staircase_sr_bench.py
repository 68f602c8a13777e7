"""The soft-aided staircase decoder (cc_staircase_decode_sr_dev, cc_mc_run_staircase_sr_dev) on one MI355X.

    python profiles/tools/staircase_sr_bench.py rates   streams/s of cc_staircase_decode_sr_dev next to
                                                        cc_staircase_decode_dev on the same streams resident in HBM, hard-
                                                        decided for the hard call: the AWGN channel
                                                        (cc_awgn_staircase_values_dev, random code streams, seed 17), L =
                                                        32, W = 8, I = 3, weights rising to infinity.  eBCH(256,239) (m =
                                                        128) and BCH(254,238) at 2^8 streams and 4.9 dB, BCH(62,50) (m =
                                                        31) at 2^12 streams and 5.8 dB.  A third leg runs the same kernel
                                                        with every weight infinite: the schedule under which a position
                                                        may stop after two quiet half-passes, as the hard kernel does.
                                                        One warm-up call per leg, device events around 5 calls enqueued
                                                        back to back (ms per call), five such runs per leg, the legs
                                                        taking turns.
    python profiles/tools/staircase_sr_bench.py mc      BER over the counted blocks of the eBCH(256,239) staircase (L = 32,
                                                        W = 8, I = 4) under cc_mc_run_staircase_sr_dev next to
                                                        cc_mc_run_staircase_dev, and the block error rate of
                                                        cc_mc_run_product_sr_dev on eBCH(256,239)^2 with the same eight
                                                        weights, over the Eb/N0 ladder of staircase_bench.py (random code
                                                        words, seed 1; one seed, no intervals), with streams/s: a
                                                        warm-up call per route at the point, then the median of three
                                                        timed calls, the routes taking turns (spread in per cent)
    python profiles/tools/staircase_sr_bench.py pmc     the BCH(62,50) leg of `rates` once per decoder (rising weights,
                                                        every weight infinite, the hard call), no warm-up: the program a
                                                        counter pass of rocprofv3 runs
    python profiles/tools/staircase_sr_bench.py summary DIR
                                                        the counters of the decoder dispatches in the counter_collection
                                                        csv files under DIR, per kernel in the order of `pmc`
    --streams-log2 K                                    another number of streams per leg / point
"""
import argparse
import ctypes as C
import math
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from staircase_bench import BLOCKS, WINDOW, timed_ms  # noqa: E402

ITERS = 3
WEIGHTS = (0.6, 0.95, 1.3, 1.65, 2.0, math.inf)
MC_WEIGHTS = (0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 2.0, math.inf)  # I = 4; those of product_sr_bench.py
# (q, t, n or None), extended, streams log2, Eb/N0
SHAPES = [((8, 2, None), True, 8, 4.9), ((8, 2, 254), False, 8, 4.9), ((6, 2, 62), False, 12, 5.8)]
REPS = 5


def rates(streams_log2, shapes=None, timed=True):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = (C.c_float * len(WEIGHTS))(*WEIGHTS)
    winf = (C.c_float * len(WEIGHTS))(*([math.inf] * len(WEIGHTS)))
    Lc = BLOCKS - WINDOW + 1
    for (q, t, n), extended, log2, ebno in shapes or SHAPES:
        streams = 1 << (streams_log2 if streams_log2 is not None else log2)
        kw = {} if n is None else {"n": n}
        sc = cc.staircase_code(cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **kw), BLOCKS, WINDOW, ITERS,
                               extended=extended)
        ch = sc.channel(ebno, 17, 0, streams, True, values=True)
        y, sent = ch["y"], ch["sent"]
        z = (y < 0).to(torch.uint8)
        out = torch.empty_like(z)
        nflip, status = (torch.empty(streams, dtype=torch.int32, device="cuda") for _ in range(2))
        desc = sc._sc()

        def sr():
            capi.check(lib.cc_staircase_decode_sr_dev(C.byref(desc), w, ptr(y), ptr(out), ptr(nflip), ptr(status), streams, stream), "sr")

        def sr_inf():
            capi.check(lib.cc_staircase_decode_sr_dev(C.byref(desc), winf, ptr(y), ptr(out), ptr(nflip), ptr(status), streams, stream), "sr")

        def hard():
            capi.check(lib.cc_staircase_decode_dev(C.byref(desc), ptr(z), ptr(out), ptr(nflip), ptr(status), streams, stream), "hard")

        print("%s  %d streams, AWGN at %.1f dB (channel BER %.2e), LDS %d bytes per workgroup (hard: %d)" % (
            sc.to_string(), streams, ebno, float((z != sent).float().mean()), sc.lds_bytes(WEIGHTS), sc.lds_bytes()), flush=True)
        legs = {"iBDD-SR": sr, "SR w=inf": sr_inf, "hard": hard}
        for name, call in legs.items():
            call()
            torch.cuda.synchronize()
            right = int((out[:, :Lc] == sent[:, :Lc]).flatten(1).all(dim=1).sum())
            print("  %-8s converged %d, right in the counted blocks %d of %d, mean nflip %.1f" % (
                name, int((status == 0).sum()), right, streams, float(nflip.float().mean())), flush=True)
        if not timed:
            continue
        times = {k: [] for k in legs}
        for _ in range(5):
            for k, call in legs.items():
                times[k].append(timed_ms(call, REPS))
        med = {}
        for k, ts in times.items():
            med[k] = statistics.median(ts)
            print("  %-8s ms %9.3f - %9.3f  median %9.3f   k streams/s %9.2f   coded Gbit/s %7.2f" % (
                k, min(ts), max(ts), med[k], streams / med[k], streams * BLOCKS * sc.m * sc.m / med[k] / 1e6), flush=True)
        print("  iBDD-SR / hard = %.2f in time, with every weight infinite %.2f" % (
            med["iBDD-SR"] / med["hard"], med["SR w=inf"] / med["hard"]), flush=True)


def mc(streams_log2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ProductSrBackend, StaircaseBackend, StaircaseSrBackend
    streams = 1 << (streams_log2 if streams_log2 is not None else 8)
    mk = lambda: cc.primitive_bch(8, cc.errors(2), cc.berlekamp_massey_tag())
    sc = cc.staircase_code(mk(), BLOCKS, WINDOW, 4, extended=True)
    pc = cc.product_code(mk(), mk(), extended=True)
    Lc = BLOCKS - WINDOW + 1
    blocks = streams * Lc // 4  # about as many counted bits on both sides: a product block is four staircase blocks
    backends = (("staircase iBDD-SR", StaircaseSrBackend(sc, MC_WEIGHTS, True), streams, streams * Lc * sc.m * sc.m),
                ("staircase hard", StaircaseBackend(sc, True), streams, streams * Lc * sc.m * sc.m),
                ("product iBDD-SR", ProductSrBackend(pc, MC_WEIGHTS, True), blocks, blocks * pc.n))
    print("%s (R = %.3f), %d streams per point; %s sr8 (R = %.3f), %d blocks per point; random code words, seed 1" % (
        sc.to_string(), sc.rate, streams, pc.to_string(), pc.rate, blocks), flush=True)
    for _, be, _, _ in backends:
        be.run(5.0, 1, 0, 16).cpu()  # warm-up
    for ebno in (4.25, 4.5, 4.625, 4.75, 4.875, 5.0, 5.25):
        row, times, holder = [], {name: [] for name, _, _, _ in backends}, {}
        for name, be, frames, _ in backends:
            holder[name] = be.run(ebno, 1, 0, frames).cpu().numpy()  # warm-up at the point; the counters do not depend on the call
        for _ in range(3):
            for name, be, frames, _ in backends:
                times[name].append(timed_ms(lambda: be.run(ebno, 1, 0, frames)))
        for name, be, frames, bits in backends:
            c, ts = holder[name], times[name]
            ms = statistics.median(ts)
            assert int(c[capi.MC_FRAMES]) == frames
            row.append("%s ber %.3e (%d bits, %d failed) %6.2f k/s (+-%.1f %%)" % (
                name, int(c[capi.MC_BIT_ERRORS]) / bits, int(c[capi.MC_BIT_ERRORS]), int(c[capi.MC_FAILURES]), frames / ms,
                50 * (max(ts) - min(ts)) / ms))
        print("  %.3f dB  %s" % (ebno, "   ".join(row)), flush=True)


def summary(root):
    import csv
    import glob
    rows = {}  # (kernel, occurrence) -> counter -> value
    for path in sorted(glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True)):
        seen = {}
        for r in csv.DictReader(open(path)):
            found = re.search(r"staircase(_sr)?_kernel<\d>", r["Kernel_Name"])
            if not found:
                continue
            name = found.group(0)
            occ = seen.setdefault(name, {}).setdefault(r["Dispatch_Id"], len(seen[name]))
            rows.setdefault((name, occ), {})[r["Counter_Name"]] = float(r["Counter_Value"])
    legs = {("sr", 0): "iBDD-SR, rising weights", ("sr", 1): "iBDD-SR, every weight infinite", ("hard", 0): "hard window"}
    for (name, occ), counters in sorted(rows.items()):
        leg = legs.get(("sr" if "staircase_sr" in name else "hard", occ), "?")
        print("%s  [%s]" % (name, leg))
        for k in sorted(counters):
            print("   %-24s %.6g" % (k, counters[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "mc", "pmc", "summary"))
    ap.add_argument("dir", nargs="?", default=None)
    ap.add_argument("--streams-log2", type=int, default=None)
    a = ap.parse_args()
    if a.what == "summary":
        summary(a.dir)
    elif a.what == "pmc":
        rates(a.streams_log2, SHAPES[2:], False)
    else:
        (rates if a.what == "rates" else mc)(a.streams_log2)


if __name__ == "__main__":
    main()
