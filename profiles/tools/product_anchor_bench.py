"""Anchor decoding of product codes (cc_product_decode_anchor_dev, cc_mc_run_product_anchor_dev) on one
MI355X, by the method of product_hard_bench.py.

    python profiles/tools/product_anchor_bench.py rates   BCH(63,45)^2 at 2^12 blocks (BSC p = 0.04) and eBCH(256,239)^2 at
                                                          2^8 blocks (p = 0.008), random code blocks resident in HBM, 6
                                                          and 8 half-iterations.  Legs: cc_product_decode_hard_dev (its
                                                          object is that of the parent commit, register for register) and
                                                          cc_product_decode_anchor_dev at delta = 2 on the same inputs.
                                                          One warm-up call per leg, device events around 20 calls enqueued
                                                          back to back (ms per call), three such runs per leg, the legs
                                                          taking turns.
    python profiles/tools/product_anchor_bench.py mc      blocks right and CC_MC_UNDETECTED of anchor decoding at delta =
                                                          1, 2, 3 next to iBDD and iBDD-SR (the schedule of
                                                          product_sr_bench.py), 8 half-iterations, random code blocks, seed
                                                          1: eBCH(64,51)^2 at 3.5 .. 5.0 dB with 2^16 blocks per point,
                                                          eBCH(256,239)^2 at 4.5 .. 5.25 dB with 2^12.  One seed, no
                                                          intervals: the points place the waterfalls.
    --blocks-log2 K                                       another number of blocks per leg / point
"""
import argparse
import ctypes as C
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from product_hard_bench import REPS, received, timed_ms  # noqa: E402

# (q, t), extended, blocks log2, BSC p
RATES = [((6, 3), False, 12, 0.04), ((8, 2), True, 8, 0.008)]
HALVES = (6, 8)
DELTA = 2
WEIGHTS = (0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 2.0, math.inf)
# (q, t), blocks log2, Eb/N0 points
LADDERS = [((6, 2), 16, (3.5, 4.0, 4.5, 5.0)), ((8, 2), 12, (4.5, 4.75, 5.0, 5.25))]


def rates(blocks_log2):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (q, t), extended, log2, p in RATES:
        blocks = 1 << (blocks_log2 if blocks_log2 is not None else log2)
        mk = lambda: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        pc = cc.product_code(mk(), mk(), extended=extended)
        sent, z = received(pc, blocks, p, 17)
        out = torch.empty_like(z)
        small = [torch.empty(blocks, dtype=torch.int32, device="cuda") for _ in range(5)]

        def hard(halves):
            desc = pc._pc_hard(halves)
            capi.check(lib.cc_product_decode_hard_dev(C.byref(desc), ptr(z), ptr(out), ptr(small[0]), ptr(small[1]),
                                                      ptr(small[2]), blocks, stream), "hard")

        def anchor(halves):
            desc = pc._pc_hard(halves)
            capi.check(lib.cc_product_decode_anchor_dev(C.byref(desc), DELTA, ptr(z), ptr(out), ptr(small[0]), ptr(small[1]),
                                                        ptr(small[2]), ptr(small[3]), ptr(small[4]), blocks, stream), "anchor")

        print("%s  %d blocks, BSC p = %g, delta = %d" % (pc.to_string(), blocks, p, DELTA), flush=True)
        legs = {}
        for halves in HALVES:
            for name, call in (("iBDD", hard), ("anchor", anchor)):
                small[3].zero_()
                small[4].zero_()
                call(halves)
                torch.cuda.synchronize()
                right = int((out == sent).all(dim=2).all(dim=1).sum())
                print("  %-6s h = %d: converged %d, right %d of %d, mean last %.2f, backtracks %d, refusals %d" % (
                    name, halves, int((small[2] == 0).sum()), right, blocks, float(small[1].float().mean()),
                    int(small[3].sum()), int(small[4].sum())), flush=True)
                legs["%s h=%d" % (name, halves)] = lambda call=call, halves=halves: call(halves)
        times = {k: [] for k in legs}
        for call in legs.values():
            call()
            torch.cuda.synchronize()
        for _ in range(3):
            for k, call in legs.items():
                times[k].append(timed_ms(call, REPS))
        for halves in HALVES:
            med = {}
            for name in ("iBDD", "anchor"):
                ts = times["%s h=%d" % (name, halves)]
                med[name] = statistics.median(ts)
                print("  %-12s ms %9.3f - %9.3f  median %9.3f   k blocks/s %9.2f" % ("%s h=%d" % (name, halves), min(ts), max(ts),
                                                                                    med[name], blocks / med[name]), flush=True)
            ts, th = times["anchor h=%d" % halves], times["iBDD h=%d" % halves]
            print("  h = %d: anchor / iBDD = %.2f (spread of anchor %.1f %%, of iBDD %.1f %%)" % (
                halves, med["anchor"] / med["iBDD"], 100 * (max(ts) - min(ts)) / med["anchor"],
                100 * (max(th) - min(th)) / med["iBDD"]), flush=True)


def mc(blocks_log2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ProductAnchorBackend, ProductHardBackend, ProductSrBackend
    halves = len(WEIGHTS)
    for (q, t), log2, ladder in LADDERS:
        blocks = 1 << (blocks_log2 if blocks_log2 is not None else log2)
        mk = lambda: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        pc = cc.product_code(mk(), mk(), extended=True)
        backends = [("iBDD", ProductHardBackend(pc, halves, True)), ("iBDD-SR", ProductSrBackend(pc, WEIGHTS, True))]
        backends += [("anchor d=%d" % d, ProductAnchorBackend(pc, d, halves, True)) for d in (1, 2, 3)]
        print("%s  %d blocks per point, random code blocks, seed 1, %d half-iterations" % (pc.to_string(), blocks, halves),
              flush=True)
        for _, be in backends:
            be.run(ladder[0], 1, 0, min(blocks, 64)).cpu()  # warm-up
        for ebno in ladder:
            for name, be in backends:
                holder = {}
                ms = timed_ms(lambda: holder.update(c=be.run(ebno, 1, 0, blocks)))
                c = holder["c"].cpu().numpy()
                assert int(c[capi.MC_FRAMES]) == blocks
                print("  %.2f dB  %-11s right %6d  wrong or failed %6d  undetected %5d  bler %.3e  mean last %.2f  %8.2f k blocks/s" % (
                    ebno, name, blocks - int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_UNDETECTED]),
                    int(c[capi.MC_WORD_ERRORS]) / blocks, int(c[capi.MC_ITER_SUM]) / blocks, blocks / ms), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "mc"))
    ap.add_argument("--blocks-log2", type=int, default=None)
    a = ap.parse_args()
    (rates if a.what == "rates" else mc)(a.blocks_log2)


if __name__ == "__main__":
    main()
