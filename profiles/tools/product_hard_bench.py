"""Iterated hard-decision decoding of product codes (cc_product_decode_hard_dev, cc_mc_run_product_hard_dev)
on one MI355X.

    python profiles/tools/product_hard_bench.py rates   BCH(63,45)^2 at 2^12 blocks (BSC p = 0.04) and BCH(255,239)^2 at
                                                        2^8 blocks (p = 0.006: the model converges on most blocks), random
                                                        code blocks resident in HBM, 6 and 8 half-iterations.  Legs: the
                                                        fused call, and the loop that does the same work without it --
                                                        cc_correct_hard_batch_dev on the rows, then
                                                        cc_correct_hard_interleaved_batch_dev at depth w1 on the columns,
                                                        PGZ handles (bounded distance) -- whose `out` is asserted equal
                                                        before anything is timed.  Then the extended products
                                                        eBCH(64,51)^2 and eBCH(256,239)^2, which have no such loop: the
                                                        fused call alone.  One warm-up call per leg, device events
                                                        around 20 calls enqueued back to back (ms per call), three
                                                        such runs per leg, the legs taking turns.
    python profiles/tools/product_hard_bench.py mc      blocks/s of cc_mc_run_product_hard_dev (8 half-iterations) next
                                                        to cc_mc_run_product_dev (Chase p = 4, 8 half-iterations) on the
                                                        same codes, and the block error rates of both over one Eb/N0
                                                        ladder (random code blocks, seed 1; one seed, no intervals)
    --blocks-log2 K                                     another number of blocks per leg / point
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# (q, t), blocks log2, BSC p
PLAIN = [((6, 3), 12, 0.04), ((8, 2), 8, 0.006)]
EXTENDED = [((6, 2), 12, 0.035), ((8, 2), 8, 0.008)]
HALVES = (6, 8)
ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0, 1.0)
BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0, 1.0, 1.0)


REPS = 20  # calls per timed window: one call of a fraction of a millisecond would measure the launch path


def timed_ms(call, reps=1):
    """ms per call, `reps` calls enqueued back to back between two device events"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def received(pc, blocks, p, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    msg = torch.randint(0, 2, (blocks, pc.k2, pc.k1), dtype=torch.uint8, device="cuda", generator=g)
    sent = pc.encode_batch(msg)
    flips = (torch.rand(sent.shape, device="cuda", generator=g) < p).to(torch.uint8)
    return sent, sent ^ flips


def report(name, times, blocks):
    ts = times[name]
    med = statistics.median(ts)
    print("  %-22s ms %9.3f - %9.3f  median %9.3f   k blocks/s %9.2f" % (name, min(ts), max(ts), med, blocks / med), flush=True)
    return med


def rates(blocks_log2):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for extended, cases in ((False, PLAIN), (True, EXTENDED)):
        for (q, t), log2, p in cases:
            blocks = 1 << (blocks_log2 if blocks_log2 is not None else log2)
            mk = lambda tag: cc.primitive_bch(q, cc.errors(t), tag())
            pc = cc.product_code(mk(cc.berlekamp_massey_tag), mk(cc.berlekamp_massey_tag), extended=extended)
            pgz = mk(cc.peterson_gorenstein_zierler_tag)
            sent, z = received(pc, blocks, p, 17)
            out = torch.empty_like(z)
            a, b = torch.empty_like(z), torch.empty_like(z)
            small = [torch.empty(blocks, dtype=torch.int32, device="cuda") for _ in range(3)]
            lines = torch.empty(blocks * max(pc.n1, pc.n2), dtype=torch.int32, device="cuda")
            lines2 = torch.empty_like(lines)

            def fused(halves):
                desc = pc._pc_hard(halves)
                capi.check(lib.cc_product_decode_hard_dev(C.byref(desc), ptr(z), ptr(out), ptr(small[0]), ptr(small[1]),
                                                          ptr(small[2]), blocks, stream), "fused")

            def loop(halves):
                src = z
                for h in range(halves):
                    dst = a if src is not a else b
                    if h % 2 == 0:
                        capi.check(lib.cc_correct_hard_batch_dev(pgz._h, ptr(src), None, None, ptr(dst), ptr(lines), ptr(lines2),
                                                                 blocks * pc.n2, stream), "rows")
                    else:
                        capi.check(lib.cc_correct_hard_interleaved_batch_dev(pgz._h, ptr(src), None, None, ptr(dst), ptr(lines),
                                                                             ptr(lines2), blocks * pc.n1, pc.n1, stream), "columns")
                    src = dst
                return src

            print("%s  %d blocks, BSC p = %g" % (pc.to_string(), blocks, p), flush=True)
            legs = {}
            for halves in HALVES:
                fused(halves)
                torch.cuda.synchronize()
                right = int((out == sent).all(dim=2).all(dim=1).sum())
                ok = int((small[2] == 0).sum())
                print("  h = %d: converged %d, right %d of %d, mean last %.2f" % (halves, ok, right, blocks,
                                                                                 float(small[1].float().mean())), flush=True)
                legs["fused h=%d" % halves] = lambda halves=halves: fused(halves)
                if not extended:
                    same = bool((loop(halves) == out).all())
                    torch.cuda.synchronize()
                    assert same, "the loop of component calls and the fused call differ"
                    legs["loop h=%d" % halves] = lambda halves=halves: loop(halves)
            times = {k: [] for k in legs}
            for call in legs.values():
                call()
                torch.cuda.synchronize()
            for _ in range(3):
                for k, call in legs.items():
                    times[k].append(timed_ms(call, REPS))
            for halves in HALVES:
                f = report("fused h=%d" % halves, times, blocks)
                if not extended:
                    ts = times["loop h=%d" % halves]
                    l = report("loop h=%d" % halves, times, blocks)
                    print("  h = %d: loop / fused = %.2f (spread of the loop %.1f %%)" % (halves, l / f,
                                                                                       100 * (max(ts) - min(ts)) / l), flush=True)


def mc(blocks_log2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ProductBackend, ProductHardBackend
    for (q, t), log2, ladder in (((6, 2), 12, (3.0, 3.5, 4.0, 4.5, 5.0)), ((8, 2), 7, (3.5, 4.0, 4.5, 5.0))):
        blocks = 1 << (blocks_log2 if blocks_log2 is not None else log2)
        mk = lambda: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
        pc = cc.product_code(mk(), mk(), extended=True)
        hard, soft = ProductHardBackend(pc, 8, True), ProductBackend(pc, 4, ALPHA, BETA, True)
        print("%s  %d blocks per point, random code blocks, seed 1: iBDD h = 8 against Chase-Pyndiah p = 4, h = 8" % (
            pc.to_string(), blocks), flush=True)
        for be in (hard, soft):
            be.run(ladder[0], 1, 0, min(blocks, 64)).cpu()  # warm-up
        for ebno in ladder:
            row = []
            for name, be in (("hard", hard), ("turbo", soft)):
                holder = {}
                ms = timed_ms(lambda: holder.update(c=be.run(ebno, 1, 0, blocks)))
                c = holder["c"].cpu().numpy()
                assert int(c[capi.MC_FRAMES]) == blocks
                extra = "  mean last %.2f" % (int(c[capi.MC_ITER_SUM]) / blocks) if name == "hard" else ""
                row.append("%s bler %.3e (%d wrong or failed, %d undetected) %8.2f k blocks/s%s" % (
                    name, int(c[capi.MC_WORD_ERRORS]) / blocks, int(c[capi.MC_WORD_ERRORS]), int(c[capi.MC_UNDETECTED]),
                    blocks / ms, extra))
            print("  %.1f dB  %s" % (ebno, "   ".join(row)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "mc"))
    ap.add_argument("--blocks-log2", type=int, default=None)
    a = ap.parse_args()
    (rates if a.what == "rates" else mc)(a.blocks_log2)


if __name__ == "__main__":
    main()
