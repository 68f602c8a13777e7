#!/usr/bin/env python3
"""Throughput of RS hard decoding and encoding with first root alpha^0 (mu = 0) against the mu = 1 twins.

    python profiles/tools/rs_roots_bench.py [--frames N] [--leg a|b|c] [--runs 3] [--root CHECKOUT]

2^22 frames resident in HBM, Berlekamp-Massey tag, 0 .. t random symbol errors per frame (the mix of rs_bench.py).  Legs:
(a) mu = 1, (b) the same codes with mu = 0 on the bit-plane chain, interleaved run by run in one process; (c) is (b)
with CC_AMD_NO_BITSLICE=1 (the table kernels), which is read once per process: the tool starts a child for it.
Prints M frames/s per run; events around `reps` back-to-back calls, after a warm-up call.  --root names another built
checkout whose package is measured instead of this one's (leg (a) on the parent commit: --leg a --root DIR).
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CODES = (("RS(255,239)", 8, None), ("RS(255,223)", 16, None), ("RS(204,188)", 8, 204))


def rate(fn, frames, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return frames * reps / (a.elapsed_time(b) * 1e-3) / 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 22)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--leg", default="ab")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    import channelcoding_amd as cc
    print("# package: %s" % ("this checkout" if os.path.abspath(args.root) == ROOT else "the checkout given with --root"), flush=True)

    mus = {"ab": (1, 0), "a": (1,), "b": (0,), "c": (0,)}[args.leg]
    label = {1: "a mu=1", 0: "c mu=0 tables" if args.leg == "c" else "b mu=0"}
    rng = np.random.default_rng(5)
    B = args.frames
    for name, t, n in CODES:
        work = {}
        for mu in mus:
            code = cc.rs(8, cc.errors(t), cc.berlekamp_massey_tag(), mu=mu, step=1, n=n)
            msg = torch.from_numpy(rng.integers(0, 256, (4096, code.l)).astype(np.uint8)).cuda()
            cw = code.encode_batch(msg).repeat((B + 4095) // 4096, 1)[:B].contiguous()
            # 0 .. t errors per frame: error e of a frame exists iff e < count
            count = torch.randint(0, t + 1, (B,), device="cuda")
            for e in range(t):
                pos = torch.randint(0, code.n, (B,), device="cuda")
                val = torch.randint(1, 256, (B,), device="cuda", dtype=torch.int32).to(torch.uint8)
                hit = (count > e).to(torch.uint8)
                cw[torch.arange(B, device="cuda"), pos] ^= val * hit
            msgs = msg.repeat((B + 4095) // 4096, 1)[:B].contiguous()
            work[mu] = (code, cw, msgs)
            route = code.hard_route(B) if hasattr(code, "hard_route") else -1  # (the parent commit has no route query)
            print("# %s mu=%d route %d frames %d" % (name, mu, route, B), flush=True)
        for run in range(args.runs):  # legs alternate
            for mu in mus:
                code, rx, msgs = work[mu]
                print("decode %-12s %-14s run %d  %9.1f M frames/s" % (name, label[mu], run, rate(lambda: code.correct_batch(rx), B, args.reps)),
                      flush=True)
        if n is None:
            for run in range(args.runs):
                for mu in mus:
                    code, rx, msgs = work[mu]
                    print("encode %-12s %-14s run %d  %9.1f M frames/s" % (name, label[mu], run, rate(lambda: code.encode_batch(msgs), B, args.reps)),
                          flush=True)
        del work
        torch.cuda.empty_cache()
    if args.leg == "ab":  # leg (c) in a process of its own: the switch is read once
        env = dict(os.environ, CC_AMD_NO_BITSLICE="1")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "c", "--frames", str(args.frames), "--runs",
                        str(args.runs), "--reps", str(args.reps)], env=env, check=True)


if __name__ == "__main__":
    main()
