"""Shortened codes against their mother codes, one session, 2^22 frames each (GF(2^14): 2^16), device-resident data,
best of 3:

    hard   RS(204,188) BM vs RS(255,239) BM, BCH(200,176) BM vs BCH(255,231) BM, BCH over GF(2^14) t = 12 at N = 3000
           vs N = 16383 (cc_correct_hard_batch_dev / _u16_dev on
           received words of the q-ary symmetric channel / AWGN hard decisions near the waterfall)
    soft   BCH(200,176) MS<20> at 4 dB (generic kernel over H[:, :200]) vs BCH(255,231) MS<20> (diagonal kernel)
    mc     cc_mc_run_dev (AWGN, 4 dB) and cc_mc_run_discrete_dev (q-ary SC, p = 0.03) for the two shortened codes

    python profiles/tools/shortened_bench.py               everything, frames/s
    python profiles/tools/shortened_bench.py --only rs204  one workload (for a rocprofv3 run of its own)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES = 1 << 22
WIDE_FRAMES = 1 << 16


def codes():
    import channelcoding_amd as cc
    bm = cc.berlekamp_massey_tag
    return {
        "rs204": lambda: cc.rs(8, cc.errors(8), bm(), n=204),
        "rs255": lambda: cc.rs(8, cc.errors(8), bm()),
        "bch200": lambda: cc.primitive_bch(8, cc.errors(3), bm(), n=200),
        "bch255": lambda: cc.primitive_bch(8, cc.errors(3), bm()),
        "bch200-ms": lambda: cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20), n=200),
        "bch255-ms": lambda: cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20)),
        "bch14-3000": lambda: cc.primitive_bch(14, cc.errors(12), bm(), modular_polynomial=0x402B, n=3000),
        "bch14-16383": lambda: cc.primitive_bch(14, cc.errors(12), bm(), modular_polynomial=0x402B),
    }


def best_of(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def hard(name, code):
    import torch
    from channelcoding_amd import capi
    import ctypes as C
    if code.wide:  # GF(2^14): BCH words with about t channel errors per frame, 2^16 frames (16 KB / 32 KB each)
        frames = WIDE_FRAMES
        g = torch.Generator(device="cuda").manual_seed(5)
        rx = (torch.rand((frames, code.n), device="cuda", generator=g) < 12.0 / code.n).to(torch.int16)
        out = torch.empty_like(rx)
        nerr = torch.empty(frames, dtype=torch.int32, device="cuda")
        st = torch.empty(frames, dtype=torch.int32, device="cuda")
        p = lambda t: C.c_void_p(t.data_ptr())

        def run_w():
            capi.check(capi.lib().cc_correct_hard_batch_u16_dev(code._h, p(rx), None, None, p(out), p(nerr), p(st),
                                                                frames, None), "decode")
        return best_of(run_w), int((st != 0).sum()), frames
    if code.family == capi.FAMILY_RS:
        rx = code.discrete_channel(0.03, 0.0, 1, 0, FRAMES, True)["recv"]
    else:
        y = torch.empty((FRAMES, code.n), dtype=torch.float32, device="cuda")
        capi.check(capi.lib().cc_awgn_llr_dev(code._h, 6.0, 1, 0, FRAMES, 1, C.c_void_p(y.data_ptr()), None, None), "awgn")
        rx = (y < 0).to(torch.uint8)
        del y
    out = torch.empty_like(rx)
    nerr = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    st = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def run():
        capi.check(capi.lib().cc_correct_hard_batch_dev(code._h, p(rx), None, None, p(out), p(nerr), p(st), FRAMES, None),
                   "decode")
    dt = best_of(run)
    return dt, int((st != 0).sum()), FRAMES


def soft(name, code):
    import torch
    from channelcoding_amd import capi
    import ctypes as C
    y = torch.empty((FRAMES, code.n), dtype=torch.float32, device="cuda")
    capi.check(capi.lib().cc_awgn_llr_dev(code._h, 4.0, 2, 0, FRAMES, 0, C.c_void_p(y.data_ptr()), None, None), "awgn")
    hardo = torch.empty((FRAMES, code.n), dtype=torch.uint8, device="cuda")
    st = torch.empty(FRAMES, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def run():
        capi.check(capi.lib().cc_correct_soft_batch_dev(code._h, p(y), None, None, p(hardo), None, None, p(st), FRAMES,
                                                        None), "minsum")
    dt = best_of(run)
    return dt, int((st != 0).sum())


def mc(name, code, discrete):
    import numpy as np
    from channelcoding_amd.montecarlo import DeviceBackend, DiscreteBackend
    if discrete:
        be = DiscreteBackend(code, "bsec", True)
        fn = lambda: be.run((0.03 if code.family else 0.004, 0.0), 3, 0, FRAMES)
    else:
        be = DeviceBackend(code, True)
        fn = lambda: be.run(4.0 if not code.algorithm.soft else 4.0, 3, 0, FRAMES)
    dt = best_of(fn)
    c = fn().cpu().numpy()
    return dt, int(c[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    mk = codes()
    rows = []
    plan = [("hard", "rs204"), ("hard", "rs255"), ("hard", "bch200"), ("hard", "bch255"),
            ("hard", "bch14-3000"), ("hard", "bch14-16383"),
            ("soft", "bch200-ms"), ("soft", "bch255-ms"),
            ("mc-awgn", "bch200"), ("mc-awgn", "bch200-ms"), ("mc-qary", "rs204"), ("mc-bsc", "bch200")]
    for kind, name in plan:
        if a.only and a.only != name and a.only != kind + ":" + name:
            continue
        code = mk[name]()
        frames = FRAMES
        if kind == "hard":
            dt, bad, frames = hard(name, code)
        elif kind == "soft":
            dt, bad = soft(name, code)
        else:
            dt, bad = mc(name, code, kind != "mc-awgn")
        info = code.kernel_info()["kernel"]
        rows.append((kind, code.to_string(), frames / dt / 1e6, dt * 1e3, bad, info[:60]))
        print("%-8s %-22s %9.1f Mframes/s  %8.2f ms  failed/word-errors %8d  %s" % rows[-1], flush=True)
        del code
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
