"""Throughput of the Monte-Carlo pipeline on packed words (cc_mc_run_bsc_packed_dev: channel -> decode -> count, DESIGN
4.5d) on one MI355X, frames resident nowhere but in the handle's packed workspace.

    python profiles/tools/packed_mc_bench.py                      every workload:
        bch231       BCH(255,231) BM, p = 0.005, random codewords, 2^22 frames per call: the packed route against the byte
                     route (cc_mc_run_discrete_dev) in the same process, alternating
        dvbs2_full   GF(2^14), t = 12, N = 16383     |
        dvbs2_3240   GF(2^14), t = 12, N = 3240      |  2^18 frames per call, BM tag, p = t / (2 n), the all-zero word
        nand_4200    GF(2^13), t = 8,  N = 4200      |  (and once with random codewords: the generic encoder of the long
        bch1003      BCH(1023,1003)                  |  codes), next to the decode-only rate of r10_packed_long_bench.txt
    python profiles/tools/packed_mc_bench.py --only NAME [--legs packed|byte|random]
                                                                  one workload / one leg (for a rocprofv3 run of its own)
    python profiles/tools/packed_mc_bench.py --stats STATS.csv    the share of the channel, word and count kernels in the
                                                                  kernel time of a `rocprofv3 --kernel-trace --stats` run
A call is timed by the host clock around the call and a device synchronise; a warm-up call of the same size first."""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# name -> (q, t, N, polynomial, frames per call, decode-only M frames/s of profiles/r10_packed_long_bench.txt or None)
WORKLOADS = {
    "bch231": (8, 3, None, None, 1 << 22, None),
    "dvbs2_full": (14, 12, None, 0x402B, 1 << 18, 24.3),
    "dvbs2_3240": (14, 12, 3240, 0x402B, 1 << 18, 95.8),
    "nand_4200": (13, 8, 4200, 0x201B, 1 << 18, 117.1),
    "bch1003": (10, 2, None, 0x409, 1 << 18, 548.0),
}
BYTE_YARDSTICK = 698.0  # M frames/s, bch-bm-bsc of profiles/r04_discrete_mc_bench.txt

CHANNEL = ("bsc_packed_kernel", "discrete_kernel")
WORDS = ("random_packed_kernel", "packed_encode_kernel", "random_bits_kernel", "encode", "unpack_bits_kernel<unsigned short>")
COUNT = ("count_packed_kernel", "count_kernel")


def make(name):
    import channelcoding_amd as cc
    q, t, N, poly, frames, decode_only = WORKLOADS[name]
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), n=N, modular_polynomial=poly)


def timed(run, frames, reps):
    import torch
    run(frames)  # code objects, workspace
    torch.cuda.synchronize()
    out, c = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        c = run(frames)
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out, c.cpu().numpy()


def line(leg, frames, times, c):
    from channelcoding_amd import capi
    return "  %-26s ms %s   M frames/s %s   wer=%.4g  channel errors %.4g per frame" % (
        leg, " ".join("%9.3f" % (1e3 * t) for t in times), " ".join("%8.2f" % (frames / t / 1e6) for t in times),
        int(c[capi.MC_WORD_ERRORS]) / frames, int(c[capi.MC_CHANNEL_BIT_ERRORS]) / frames)


def bench(names, legs, reps):
    from channelcoding_amd.montecarlo import DiscreteBackend, PackedBscBackend
    for name in names:
        q, t, N, poly, frames, decode_only = WORKLOADS[name]
        code = make(name)
        print("%s, n = %d, P = %d bytes, %d frames per call, packed_route = %d" % (
            code.to_string(), code.n, code.packed_bytes, frames, code.packed_route(min(frames, 1 << 20))), flush=True)
        if name == "bch231":
            p = 0.005
            packed, byte = PackedBscBackend(code, True), DiscreteBackend(code, "bsc", True)
            best = {}
            for rnd in range(2):  # the two routes alternating
                for leg, be in (("packed", packed), ("byte", byte)):
                    if leg not in legs:
                        continue
                    times, c = timed(lambda f: be.run(p, 0, 0, f), frames, reps)
                    best[leg] = min(best.get(leg, 1e9), min(times))
                    print(line("%s route, p=%g, random" % (leg, p), frames, times, c), flush=True)
            if len(best) == 2:
                print("  best packed %.3f ms = %.1f M frames/s, best byte %.3f ms = %.1f M frames/s (parent commit's byte route: "
                      "%.0f M frames/s): packed / byte = %.2f" % (
                          1e3 * best["packed"], frames / best["packed"] / 1e6, 1e3 * best["byte"],
                          frames / best["byte"] / 1e6, BYTE_YARDSTICK, best["byte"] / best["packed"]), flush=True)
            continue
        p = t / (2.0 * code.n)
        for leg, random_cw in (("packed", False), ("random", True)):
            if leg not in legs:
                continue
            be = PackedBscBackend(code, random_cw)
            times, c = timed(lambda f: be.run(p, 0, 0, f), frames, reps)
            print(line("p=%.3g, %s" % (p, "random codewords" if random_cw else "all-zero word"), frames, times, c), flush=True)
            if not random_cw:
                rate = frames / min(times) / 1e6
                print("  decode only (r10_packed_long_bench.txt): %.1f M frames/s; the pipeline runs at %.2f of it" % (
                    decode_only, rate / decode_only), flush=True)


def stats(path):
    groups = {"channel": 0, "words": 0, "count": 0, "decoder": 0}
    names = {k: [] for k in groups}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], int(row["TotalDurationNs"])
            if name.startswith("__amd_rocclr") or "at::native" in name:
                continue  # fills and copies of the runtime, torch's zeroing of the counters
            g = ("channel" if any(k in name for k in CHANNEL) else "words" if any(k in name for k in WORDS)
                 else "count" if any(k in name for k in COUNT) else "decoder")
            groups[g] += ns
            names[g].append("%s x%s (%.3f ms)" % (name[:56], row["Calls"], ns / 1e6))
    total = sum(groups.values())
    for g, ns in groups.items():
        print("%-8s %9.3f ms  %5.1f %% of kernel time  %s" % (g, ns / 1e6, 100.0 * ns / max(1, total), "; ".join(names[g])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", choices=sorted(WORKLOADS))
    ap.add_argument("--legs", action="append", choices=("packed", "byte", "random"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        bench(a.only or list(WORKLOADS), a.legs or ["packed", "byte", "random"], a.reps)


if __name__ == "__main__":
    main()
