"""iBDD with scaled reliability of product codes (cc_product_decode_sr_dev, cc_mc_run_product_sr_dev) on one
MI355X.

    python profiles/tools/product_sr_bench.py rates   blocks/s of cc_product_decode_sr_dev next to
                                                      cc_product_decode_hard_dev, 8 half-iterations each, on the same
                                                      blocks resident in HBM: the AWGN channel at 4 dB
                                                      (cc_awgn_product_dev, random code blocks, seed 17), hard-decided
                                                      for the hard call.  eBCH(64,51)^2 at 2^12 and 2^16 blocks,
                                                      BCH(63,45)^2 at 2^12, eBCH(256,239)^2 at 2^8.  One warm-up call
                                                      per leg, device events around 20 calls enqueued back to back (ms
                                                      per call), five such runs per leg, the legs taking turns.
    python profiles/tools/product_sr_bench.py mc      eBCH(64,51)^2, 8 half-iterations, 3.5 .. 4.5 dB in steps of 0.25:
                                                      block error rate and blocks/s of iBDD-SR, iBDD and the
                                                      Chase-Pyndiah decoder at p = 4 through their Monte-Carlo calls,
                                                      the same seed and block count (random code blocks, seed 1; one
                                                      seed, no intervals)
    --blocks-log2 K                                   another number of blocks per leg / point
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

from product_hard_bench import ALPHA, BETA, REPS, timed_ms  # noqa: E402

WEIGHTS = (0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 2.0, math.inf)
HALVES = len(WEIGHTS)
# (q, t), extended, blocks log2
SHAPES = [((6, 2), True, 12), ((6, 2), True, 16), ((6, 3), False, 12), ((8, 2), True, 8)]
EBNO = 4.0


def rates(blocks_log2):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    w = (C.c_float * HALVES)(*WEIGHTS)
    for (q, t), extended, log2 in SHAPES:
        blocks = 1 << (blocks_log2 if blocks_log2 is not None else log2)
        mk = lambda: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        pc = cc.product_code(mk(), mk(), extended=extended)
        ch = pc.channel(EBNO, 17, 0, blocks, True)
        y, sent = ch["y"], ch["sent"]
        z = (y < 0).to(torch.uint8)
        out = torch.empty_like(z)
        small = [torch.empty(blocks, dtype=torch.int32, device="cuda") for _ in range(3)]
        desc = pc._pc_hard(HALVES)

        def sr():
            capi.check(lib.cc_product_decode_sr_dev(C.byref(desc), w, ptr(y), ptr(out), ptr(small[0]), ptr(small[1]),
                                                    ptr(small[2]), blocks, stream), "sr")

        def hard():
            capi.check(lib.cc_product_decode_hard_dev(C.byref(desc), ptr(z), ptr(out), ptr(small[0]), ptr(small[1]),
                                                      ptr(small[2]), blocks, stream), "hard")

        print("%s  %d blocks, AWGN at %.1f dB, %d half-iterations" % (pc.to_string(), blocks, EBNO, HALVES), flush=True)
        legs = {"iBDD-SR": sr, "iBDD": hard}
        for name, call in legs.items():
            call()
            torch.cuda.synchronize()
            right = int((out == sent).all(dim=2).all(dim=1).sum())
            print("  %-8s converged %d, right %d of %d, mean last %.2f" % (name, int((small[2] == 0).sum()), right, blocks,
                                                                         float(small[1].float().mean())), flush=True)
        times = {k: [] for k in legs}
        for _ in range(5):
            for k, call in legs.items():
                times[k].append(timed_ms(call, REPS))
        med = {}
        for k, ts in times.items():
            med[k] = statistics.median(ts)
            print("  %-8s ms %9.3f - %9.3f  median %9.3f   k blocks/s %9.2f" % (k, min(ts), max(ts), med[k], blocks / med[k]),
                  flush=True)
        print("  iBDD-SR / iBDD = %.2f in time" % (med["iBDD-SR"] / med["iBDD"]), flush=True)


def mc(blocks_log2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ProductBackend, ProductHardBackend, ProductSrBackend
    blocks = 1 << (blocks_log2 if blocks_log2 is not None else 16)
    mk = lambda: cc.primitive_bch(6, cc.errors(2), cc.berlekamp_massey_tag())
    pc = cc.product_code(mk(), mk(), extended=True)
    backends = (("iBDD-SR", ProductSrBackend(pc, WEIGHTS, True)), ("iBDD", ProductHardBackend(pc, HALVES, True)),
                ("turbo p=4", ProductBackend(pc, 4, ALPHA, BETA, True)))
    print("%s  %d blocks per point, random code blocks, seed 1, %d half-iterations" % (pc.to_string(), blocks, HALVES), flush=True)
    for _, be in backends:
        be.run(3.5, 1, 0, min(blocks, 4096)).cpu()  # warm-up
    for ebno in (3.5, 3.75, 4.0, 4.25, 4.5):
        row = []
        for name, be in backends:
            holder = {}
            ms = timed_ms(lambda: holder.update(c=be.run(ebno, 1, 0, blocks)))
            c = holder["c"].cpu().numpy()
            assert int(c[capi.MC_FRAMES]) == blocks
            row.append("%s bler %.3e (%d, %d undetected) %8.2f k blocks/s" % (
                name, int(c[capi.MC_WORD_ERRORS]) / blocks, int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_UNDETECTED]), blocks / ms))
        print("  %.2f dB  %s" % (ebno, "   ".join(row)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "mc"))
    ap.add_argument("--blocks-log2", type=int, default=None)
    a = ap.parse_args()
    (rates if a.what == "rates" else mc)(a.blocks_log2)


if __name__ == "__main__":
    main()
