"""Staircase codes under the sliding-window decoder (cc_staircase_decode_dev, cc_mc_run_staircase_dev) on one
MI355X.

    python profiles/tools/staircase_bench.py rates   BCH(62,50) (m = 31) at 2^12 streams (BSC p = 0.015) and BCH(254,238)
                                                     (m = 127) at 2^8 streams (p = 0.004), L = 32 blocks, W = 8, I = 3,
                                                     random code streams resident in HBM.  Legs: the fused call, and the
                                                     loop that does the same work without it -- per half-pass a torch
                                                     gather of the lines into [B m steps][2m], cc_correct_hard_batch_dev
                                                     on a PGZ handle (bounded distance), the B_0 mask and a scatter back
                                                     -- whose `out` is asserted equal before anything is timed.  Then
                                                     eBCH(256,239) (m = 128, p = 0.004), which has no such loop: the fused
                                                     call alone, in streams/s and coded Gbit/s.  One warm-up call per leg,
                                                     device events around the calls of a run (ms per call), three runs
                                                     per leg, the legs taking turns.
    python profiles/tools/staircase_bench.py mc      BER over the counted blocks of the eBCH(256,239) staircase (R = 0.867,
                                                     L = 32, W = 8, I = 4) next to cc_mc_run_product_hard_dev on
                                                     eBCH(256,239)^2 (R = 0.872, eight half-iterations) over one Eb/N0
                                                     ladder (random code words, seed 1; one seed, no intervals)
    --streams-log2 K                                 another number of streams per leg / point
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

BLOCKS, WINDOW, ITERS = 32, 8, 3
# (q, t, n or None), extended, streams log2, BSC p, fused calls per timed run
CASES = [((6, 2, 62), False, 12, 0.015, 5), ((8, 2, 254), False, 8, 0.004, 5), ((8, 2, None), True, 8, 0.004, 5)]


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


def received(sc, streams, p, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    msg = torch.randint(0, 2, (streams, sc.blocks, sc.m, sc.k_b), dtype=torch.uint8, device="cuda", generator=g)
    sent = sc.encode_batch(msg)
    flips = (torch.rand(sent.shape, device="cuda", generator=g) < p).to(torch.uint8)
    return sent, sent ^ flips


def report(name, ts, streams, bits):
    med = statistics.median(ts)
    print("  %-8s ms %9.3f - %9.3f  median %9.3f   k streams/s %9.2f   coded Gbit/s %7.2f" % (
        name, min(ts), max(ts), med, streams / med, streams * bits / med / 1e6), flush=True)
    return med


def loop_decode(lib, pgz, z, m, W, I, scratch, stream):
    """the schedule of the header with one component call per half-pass; plain codes only"""
    import torch
    from channelcoding_amd import capi
    ptr = lambda x: C.c_void_p(x.data_ptr())
    B, L = z.shape[0], z.shape[1]
    full = torch.cat([torch.zeros_like(z[:, :1]), z], dim=1)
    b_last = max(0, L - W + 1)
    for b in range(b_last + 1):
        top = min(b + W - 1, L)
        for h in range(2 * I):
            steps = [i for i in range(b + 1, top + 1) if (top - i) % 2 == h % 2]
            if not steps:
                continue
            idx = torch.tensor(steps, device=z.device)
            lines = torch.cat([full[:, idx], full[:, idx - 1].transpose(2, 3)], dim=3).contiguous()  # [B][steps][m][2m]
            out = scratch["out"][: lines.numel()].view(lines.shape)
            capi.check(lib.cc_correct_hard_batch_dev(pgz._h, ptr(lines), None, None, ptr(out), ptr(scratch["nerr"]),
                                                     ptr(scratch["status"]), B * len(steps) * m, stream), "lines")
            if 1 in steps:  # the zero block stays zero: such a line keeps its bits
                k = steps.index(1)
                reaches = (out[:, k, :, m:] != lines[:, k, :, m:]).any(dim=2, keepdim=True)
                out[:, k] = torch.where(reaches, lines[:, k], out[:, k])
            full[:, idx] = out[..., :m]
            full[:, idx - 1] = out[..., m:].transpose(2, 3)
    return full[:, 1:]


def rates(streams_log2):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    lib = capi.lib()
    ptr = lambda x: C.c_void_p(x.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (q, t, n), extended, log2, p, reps in CASES:
        streams = 1 << (streams_log2 if streams_log2 is not None else log2)
        kw = {} if n is None else {"n": n}
        mk = lambda tag: cc.primitive_bch(q, cc.errors(t), tag(), **kw)
        sc = cc.staircase_code(mk(cc.berlekamp_massey_tag), BLOCKS, WINDOW, ITERS, extended=extended)
        sent, z = received(sc, streams, p, 17)
        out = torch.empty_like(z)
        nflip, status = (torch.empty(streams, dtype=torch.int32, device="cuda") for _ in range(2))
        desc = sc._sc()

        def fused():
            capi.check(lib.cc_staircase_decode_dev(C.byref(desc), ptr(z), ptr(out), ptr(nflip), ptr(status), streams, stream), "fused")

        print("%s  %d streams, BSC p = %g, LDS %d bytes per workgroup" % (sc.to_string(), streams, p, sc.lds_bytes()), flush=True)
        fused()
        torch.cuda.synchronize()
        Lc = BLOCKS - WINDOW + 1
        right = int((out[:, :Lc] == sent[:, :Lc]).flatten(1).all(dim=1).sum())
        print("  converged %d, right in the counted blocks %d of %d, mean nflip %.1f" % (
            int((status == 0).sum()), right, streams, float(nflip.float().mean())), flush=True)
        legs = {"fused": (lambda: fused(), reps)}
        if not extended:
            pgz = mk(cc.peterson_gorenstein_zierler_tag)
            most = streams * ((WINDOW - 1 + 1) // 2) * sc.m
            scratch = dict(out=torch.empty(most * 2 * sc.m, dtype=torch.uint8, device="cuda"),
                           nerr=torch.empty(most, dtype=torch.int32, device="cuda"),
                           status=torch.empty(most, dtype=torch.int32, device="cuda"))
            loop = lambda: loop_decode(lib, pgz, z, sc.m, WINDOW, ITERS, scratch, stream)
            same = bool((loop() == out).all())
            torch.cuda.synchronize()
            assert same, "the loop of component calls and the fused call differ"
            legs["loop"] = (loop, 1)
        times = {k: [] for k in legs}
        for _ in range(3):
            for k, (call, r) in legs.items():
                times[k].append(timed_ms(call, r))
        bits = BLOCKS * sc.m * sc.m
        f = report("fused", times["fused"], streams, bits)
        if "loop" in legs:
            ts = times["loop"]
            l = report("loop", ts, streams, bits)
            print("  loop / fused = %.2f (spread of the loop %.1f %%, of the fused call %.1f %%)" % (
                l / f, 100 * (max(ts) - min(ts)) / l, 100 * (max(times["fused"]) - min(times["fused"])) / f), flush=True)


def mc(streams_log2):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import ProductHardBackend, StaircaseBackend
    streams = 1 << (streams_log2 if streams_log2 is not None else 8)
    mk = lambda: cc.primitive_bch(8, cc.errors(2), cc.berlekamp_massey_tag())
    sc = cc.staircase_code(mk(), BLOCKS, WINDOW, 4, extended=True)
    pc = cc.product_code(mk(), mk(), extended=True)
    Lc = BLOCKS - WINDOW + 1
    blocks = streams * Lc // 4  # about as many counted bits on both sides: a product block is four staircase blocks
    stair, prod = StaircaseBackend(sc, True), ProductHardBackend(pc, 8, True)
    print("%s (R = %.3f), %d streams per point, against %s iBDD h = 8 (R = %.3f), %d blocks per point; random code words, "
          "seed 1" % (sc.to_string(), sc.rate, streams, pc.to_string(), pc.rate, blocks), flush=True)
    stair.run(5.0, 1, 0, 16).cpu()
    prod.run(5.0, 1, 0, 16).cpu()
    for ebno in (4.25, 4.5, 4.625, 4.75, 4.875, 5.0, 5.25):
        holder = {}
        ms = timed_ms(lambda: holder.update(c=stair.run(ebno, 1, 0, streams)))
        c = holder["c"].cpu().numpy()
        bits = streams * Lc * sc.m * sc.m
        left = "staircase ber %.3e (%d of %d bits, channel %.3e, %d streams failed) %7.2f k streams/s" % (
            int(c[capi.MC_BIT_ERRORS]) / bits, int(c[capi.MC_BIT_ERRORS]), bits, int(c[capi.MC_CHANNEL_BIT_ERRORS]) / bits,
            int(c[capi.MC_FAILURES]), streams / ms)
        ms = timed_ms(lambda: holder.update(c=prod.run(ebno, 1, 0, blocks)))
        c = holder["c"].cpu().numpy()
        bits = blocks * pc.n
        right = "product ber %.3e (%d of %d bits, %d blocks failed) %7.2f k blocks/s" % (
            int(c[capi.MC_BIT_ERRORS]) / bits, int(c[capi.MC_BIT_ERRORS]), bits, int(c[capi.MC_FAILURES]), blocks / ms)
        print("  %.3f dB  %s   %s" % (ebno, left, right), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("rates", "mc"))
    ap.add_argument("--streams-log2", type=int, default=None)
    a = ap.parse_args()
    (rates if a.what == "rates" else mc)(a.streams_log2)


if __name__ == "__main__":
    main()
