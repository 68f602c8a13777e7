"""Throughput of the burst-channel Monte-Carlo pipeline (cc_mc_run_burst_dev: Gilbert-Elliott channel along interleaved
blocks -> decode -> count) over 2^22 frames, with cc_mc_run_discrete_dev on the same handle at the burst channel's
average symbol error rate as the yardstick of the same session, and the word-error rate at each depth.

    python profiles/tools/burst_mc_bench.py                       all workloads: frames/s of both routes, wer
    python profiles/tools/burst_mc_bench.py --only rs239-I16      one workload (for a rocprofv3 run of its own)
    python profiles/tools/burst_mc_bench.py --only rs239-I16 --route burst
                                                                  the burst route alone (the stage split of one trace)
    python profiles/tools/burst_mc_bench.py --stats STATS.csv     channel / count / decoder split of the kernel time of a
                                                                  `rocprofv3 --kernel-trace --stats` run, and the time of
                                                                  burst_kernel over that of discrete_kernel
    python profiles/tools/burst_mc_bench.py --p-detect 0.9 --p-false-alarm 0.002
                                                                  with a burst detector: cc_mc_run_burst_erasure_dev (the
                                                                  flagged symbols are erasures to the decoder) alternating
                                                                  with cc_mc_run_burst_dev, the errors-only route, on the
                                                                  same handle and channel; --route erasure for the
                                                                  detector route alone; --stats then adds the list stage
"""
import argparse
import csv
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES = 1 << 22
P_GB, P_BG, P_GOOD, P_BAD = 0.005, 0.1, 1e-4, 0.3

# name -> (family, t, interleave); all with Berlekamp-Massey and random codewords
WORKLOADS = {
    "rs239-I1": ("rs", 8, 1),
    "rs239-I16": ("rs", 8, 16),
    "rs223-I5": ("rs", 16, 5),
    "bch231-I8": ("bch", 3, 8),
}

CHANNEL = ("burst_kernel", "discrete_kernel", "random_symbols_kernel", "random_bits_kernel", "encode",
           "bitslice_fused_syndrome_kernel<false, true>", "bitslice_parity_kernel")
COUNT = ("count_kernel",)
LIST = ("flag_count_kernel", "flag_positions_kernel", "discrete_scan_tiles_kernel", "discrete_scan_sums_kernel",
        "discrete_positions_kernel")


def average_error_rate():
    pi_b = P_GB / (P_GB + P_BG)
    return pi_b * P_BAD + (1.0 - pi_b) * P_GOOD


def make(family, t):
    import channelcoding_amd as cc
    cls = cc.rs if family == "rs" else cc.primitive_bch
    return cls(8, cc.errors(t), cc.berlekamp_massey_tag())


def timed(runs, frames, reps):
    """the calls of `runs` alternating, `reps` rounds after a warm-up of each: name -> (times, last counters)"""
    import torch
    for run in runs.values():
        run(1 << 16)  # code objects, workspace
    torch.cuda.synchronize()
    out = {name: ([], None) for name in runs}
    for _ in range(reps):
        for name, run in runs.items():
            t0 = time.perf_counter()
            c = run(frames)
            torch.cuda.synchronize()
            out[name] = (out[name][0] + [time.perf_counter() - t0], c)
    return out


def bench_detector(names, reps, route, p_detect, p_false_alarm):
    """the detector route against the errors-only route of the same handle, channel and session"""
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import BurstBackend
    print("# (p_gb, p_bg, p_good, p_bad) = (%g, %g, %g, %g), detector (p_detect, p_false_alarm) = (%g, %g); %d frames, %d "
          "rounds, the two routes alternating" % (P_GB, P_BG, P_GOOD, P_BAD, p_detect, p_false_alarm, FRAMES, reps),
          flush=True)
    for name in names or WORKLOADS:
        family, t, I = WORKLOADS[name]
        h = make(family, t)
        plain = BurstBackend(h, I, P_GB, P_BG, P_GOOD, random_codewords=True)
        flagged = BurstBackend(h, I, P_GB, P_BG, P_GOOD, random_codewords=True, p_detect=p_detect,
                               p_false_alarm=p_false_alarm)
        runs = {}
        if route in ("both", "erasure"):
            runs["erasure"] = lambda f: flagged.run(P_BAD, 0, 0, f)
        if route in ("both", "burst"):
            runs["burst"] = lambda f: plain.run(P_BAD, 0, 0, f)
        for kind, (times, c) in timed(runs, FRAMES, reps).items():
            best, med = min(times), statistics.median(times)
            print("%-10s %-8s %s I=%d: %8.2f M frames/s best (%.2f ms), %8.2f median  wer=%.4g  channel errors %.4g, "
                  "erasures %.4g per frame" % (name, kind, h.to_string(), I, FRAMES / best / 1e6, best * 1e3,
                                               FRAMES / med / 1e6, int(c[capi.MC_WORD_ERRORS]) / FRAMES,
                                               int(c[capi.MC_CHANNEL_BIT_ERRORS]) / FRAMES,
                                               int(c[capi.MC_CHANNEL_ERASURES]) / FRAMES), flush=True)


def bench(names, reps, route):
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import BurstBackend, DiscreteBackend
    p_avg = average_error_rate()
    print("# (p_gb, p_bg, p_good, p_bad) = (%g, %g, %g, %g): average symbol error rate %.6g; %d frames, %d rounds, the two "
          "routes alternating" % (P_GB, P_BG, P_GOOD, P_BAD, p_avg, FRAMES, reps), flush=True)
    for name in names or WORKLOADS:
        family, t, I = WORKLOADS[name]
        h = make(family, t)
        burst = BurstBackend(h, I, P_GB, P_BG, P_GOOD, random_codewords=True)
        memoryless = DiscreteBackend(h, "bsc", random_codewords=True)
        runs = {}
        if route in ("both", "burst"):
            runs["burst"] = lambda f: burst.run(P_BAD, 0, 0, f)
        if route in ("both", "discrete"):
            runs["discrete"] = lambda f: memoryless.run(p_avg, 0, 0, f)
        for kind, (times, c) in timed(runs, FRAMES, reps).items():
            best, med = min(times), statistics.median(times)
            print("%-10s %-8s %s I=%d: %8.2f M frames/s best (%.2f ms), %8.2f median  wer=%.4g  channel errors %.4g per "
                  "frame" % (name, kind, h.to_string(), I, FRAMES / best / 1e6, best * 1e3, FRAMES / med / 1e6,
                             int(c[capi.MC_WORD_ERRORS]) / FRAMES, int(c[capi.MC_CHANNEL_BIT_ERRORS]) / FRAMES), flush=True)


def stats(path):
    groups = {"channel": 0, "list": 0, "count": 0, "decoder": 0}
    names = {k: [] for k in groups}
    single = {"burst_kernel": 0, "discrete_kernel": 0}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], int(row["TotalDurationNs"])
            if name.startswith("__amd_rocclr") or "at::native" in name:
                continue  # fills and copies of the runtime, torch's zeroing of the counters
            for k in single:
                if k in name:
                    single[k] += ns
            g = ("list" if any(k in name for k in LIST) else "channel" if any(k in name for k in CHANNEL)
                 else "count" if any(k in name for k in COUNT) else "decoder")
            groups[g] += ns
            names[g].append("%s (%.2f ms)" % (name[:60], ns / 1e6))
    total = sum(groups.values())
    for g, ns in groups.items():
        print("%-8s %8.2f ms  %5.1f %% of kernel time  %s" % (g, ns / 1e6, 100.0 * ns / max(1, total),
                                                              "; ".join(names[g])))
    print("channel over decoder: %.3f" % (groups["channel"] / max(1, groups["decoder"])))
    if single["burst_kernel"] and single["discrete_kernel"]:
        print("burst_kernel %.2f ms over discrete_kernel %.2f ms: %.3f" % (
            single["burst_kernel"] / 1e6, single["discrete_kernel"] / 1e6,
            single["burst_kernel"] / single["discrete_kernel"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--route", choices=("both", "burst", "discrete", "erasure"), default="both")
    ap.add_argument("--p-detect", type=float, default=0.0)
    ap.add_argument("--p-false-alarm", type=float, default=0.0)
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    elif a.p_detect or a.p_false_alarm:
        bench_detector(a.only, a.reps, a.route, a.p_detect, a.p_false_alarm)
    else:
        bench(a.only, a.reps, a.route)


if __name__ == "__main__":
    main()
