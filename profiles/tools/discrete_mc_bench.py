"""Throughput of the discrete-channel Monte-Carlo pipeline (cc_mc_run_discrete_dev: channel -> [erasure CSR] -> decode
-> count) over 2^22 frames, with the AWGN hard route at 4 dB (cc_mc_run_dev, profiles/r03_mc_bench.txt) as the yardstick
of the same session.

    python profiles/tools/discrete_mc_bench.py                     all workloads, frames/s
    python profiles/tools/discrete_mc_bench.py --only rs-bm-bec    one workload (for a rocprofv3 run of its own)
    python profiles/tools/discrete_mc_bench.py --only bch-bm-bsc --with-awgn
                                                                   one workload and the AWGN yardstick (the channel
                                                                   kernels of both routes side by side in one trace)
    python profiles/tools/discrete_mc_bench.py --stats STATS.csv   share of the channel and CSR kernels in the kernel
                                                                   time of a `rocprofv3 --kernel-trace --stats` run
"""
import argparse
import csv
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES = 1 << 22

# name -> (code, p_error, p_erasure, random codewords)
WORKLOADS = {
    "bch-bm-bsc": ("bch", "bm", 0.005, 0.0, True),
    "bch-ms-bsc": ("bch", "ms", 0.01, 0.0, False),
    "rs-bm-qsc": ("rs", "bm", 0.03, 0.0, False),
    "rs-bm-bec": ("rs", "bm", 0.0, 0.1, True),
    "rs-bm-bsec": ("rs", "bm", 0.02, 0.04, True),
}
# (the erasure points send random words: for the all-zero word the 0 an erased position receives is the symbol sent,
# and the decoder would see a codeword in every frame without errors)

# kernels of the channel stage (messages, encoder, channel draw, erasure CSR) and of the count; everything else that
# runs is the decoder.  The RS encoder of GF(2^8) runs on bit planes (launch_bitslice_encode): the fused planes kernel in
# its <FLOAT_IN = false, RAW = true> instance, which only the encoder launches, and bitslice_parity_kernel.
CHANNEL = ("discrete_kernel", "random_symbols_kernel", "random_bits_kernel", "encode",
           "bitslice_fused_syndrome_kernel<false, true>", "bitslice_parity_kernel")
CSR = ("discrete_scan_tiles_kernel", "discrete_scan_sums_kernel", "discrete_positions_kernel")
COUNT = ("count_kernel",)


def make(code, alg):
    import channelcoding_amd as cc
    tag = {"bm": cc.berlekamp_massey_tag(), "ms": cc.min_sum_tag(20)}[alg]
    return cc.primitive_bch(8, cc.errors(3), tag) if code == "bch" else cc.rs(8, cc.errors(16), tag)


def timed(run, frames, reps=3):
    import torch
    run(1 << 16)  # code objects, workspace
    torch.cuda.synchronize()
    best, c = None, None
    for _ in range(reps):
        t0 = time.perf_counter()
        c = run(frames)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best, c


def bench(names, reps, with_awgn=False):
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    from channelcoding_amd.montecarlo import DeviceBackend, DiscreteBackend
    if names is None or with_awgn:
        be = DeviceBackend(cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag()), random_codewords=True)
        dt, c = timed(lambda f: be.run(4.0, 0, 0, f), FRAMES, reps)
        print("%-11s BCH(255,231) BM  AWGN 4 dB, random codewords: %8.2f M frames/s  (%.2f ms)  wer=%.4g" % (
            "awgn-hard", FRAMES / dt / 1e6, dt * 1e3, int(c[1]) / int(c[0])), flush=True)
    for name in names or WORKLOADS:
        code, alg, p, e, rcw = WORKLOADS[name]
        h = make(code, alg)
        be = DiscreteBackend(h, "bsec", random_codewords=rcw)
        dt, c = timed(lambda f: be.run((p, e), 0, 0, f), FRAMES, reps)
        print("%-11s %s p=%g eps=%g random codewords=%s: %8.2f M frames/s  (%.2f ms)  wer=%.4g  channel errors %.4g"
              "  erasures %.4g per frame" % (
                  name, h.to_string(), p, e, rcw, FRAMES / dt / 1e6, dt * 1e3, int(c[capi.MC_WORD_ERRORS]) / FRAMES,
                  int(c[capi.MC_CHANNEL_BIT_ERRORS]) / FRAMES, int(c[capi.MC_CHANNEL_ERASURES]) / FRAMES), flush=True)


def stats(path):
    groups = {"channel": 0, "csr": 0, "count": 0, "decoder": 0}
    names = {k: [] for k in groups}
    with open(path) as f:
        for row in csv.DictReader(f):
            name, ns = row["Name"], int(row["TotalDurationNs"])
            if name.startswith("__amd_rocclr") or "at::native" in name:
                continue  # fills and copies of the runtime, torch's zeroing of the counters
            g = ("csr" if any(k in name for k in CSR) else "channel" if any(k in name for k in CHANNEL)
                 else "count" if any(k in name for k in COUNT) else "decoder")
            groups[g] += ns
            names[g].append("%s (%.2f ms)" % (name[:60], ns / 1e6))
    total = sum(groups.values())
    for g, ns in groups.items():
        print("%-8s %8.2f ms  %5.1f %% of kernel time  %s" % (g, ns / 1e6, 100.0 * ns / max(1, total),
                                                              "; ".join(names[g])))
    print("channel + csr over decoder: %.3f" % ((groups["channel"] + groups["csr"]) / max(1, groups["decoder"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", action="append", choices=sorted(WORKLOADS))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--with-awgn", action="store_true", help="with --only: the AWGN yardstick too")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        stats(a.stats)
    else:
        bench(a.only, a.reps, a.with_awgn)


if __name__ == "__main__":
    main()
