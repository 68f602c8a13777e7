"""Product codes on the device (cc_product_decode_dev, cc_mc_run_product_dev) on one MI355X.

    python profiles/tools/product_bench.py decode   BCH(63,45)^2 and eBCH(64,51)^2 at 2^12 blocks, eBCH(256,239)^2 at 2^8
                                                    blocks, channel values of cc_awgn_product_dev at 3.0 / 3.0 / 4.5 dB
                                                    resident in HBM; p = 0, 2, 4, six half-iterations.  Legs: `call`, the
                                                    one library call, and `loop`, the loop of cc.product_decode at the
                                                    parent commit kept below as a plain function over the public
                                                    correct_batch(chase=, soft=).  Three runs per leg, the legs taking
                                                    turns at going first, device events around each run after one
                                                    warm-up of every shape; slowest - fastest reported, and loop / call.
    python profiles/tools/product_bench.py mc       cc_mc_run_product_dev at the three codes, p = 4, six half-iterations,
                                                    random codewords: blocks per second of one call of 2^14 / 2^14 / 2^10
                                                    blocks (three runs)
    python profiles/tools/product_bench.py curves   product_simulation at the three codes, p = 4, six half-iterations,
                                                    random codewords, seed 1: block and bit error rates from the first
                                                    point of the ladder in steps of 0.5 dB, a fixed number of blocks per
                                                    point (2^16 / 2^16 / 2^12), to the first point without a block error
    python profiles/tools/product_bench.py trace --case N --p P   five `call` runs of one decode case (for a rocprofv3
                                                    --kernel-trace --stats run of its own)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# Pyndiah's schedule of the first six half-iterations (W is not normalised here: a starting point)
ALPHA = (0.0, 0.2, 0.3, 0.5, 0.7, 0.9)
BETA = (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)
# (q, t, extended, blocks log2 of decode, Eb/N0 of decode, blocks log2 of mc, blocks log2 per point of curves)
CODES = [(6, 3, False, 12, 3.0, 14, 16), (6, 2, True, 12, 3.0, 14, 16), (8, 2, True, 8, 4.5, 10, 12)]


def product(q, t, extended):
    import channelcoding_amd as cc
    make = lambda: cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag())
    return cc.product_code(make(), make(), extended=extended)


def parent_loop(rows, cols, y, p, alpha, beta, extended):
    """cc.product_decode of the parent commit on a device tensor"""
    import torch
    kw = dict(extended=True) if extended else {}
    W = torch.zeros_like(y)
    turn = lambda a: a.transpose(1, 2).contiguous()
    B, n2, n1 = y.shape
    for h, (a, b) in enumerate(zip(alpha, beta)):
        X = y + W * a
        code, lines, length = (rows, n2, n1) if h % 2 == 0 else (cols, n1, n2)
        res = code.correct_batch((X if h % 2 == 0 else turn(X)).reshape(B * lines, length), chase=p, soft=b, **kw)
        out, W = res["out"].reshape(B, lines, length), res["ext"].reshape(B, lines, length)
        if h % 2:
            out, W = turn(out), turn(W)
        status = res["status"].reshape(B, lines)
    return dict(out=out, ext=W, status=status)


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def decode_case(q, t, extended, blocks_log2, ebno):
    pc = product(q, t, extended)
    y = pc.channel(ebno, 1, 0, 1 << blocks_log2, True)["y"]
    return pc, y


def decode():
    import torch
    print("decode: ms per call of six half-iterations; three runs, the legs taking turns; [min .. max]")
    for q, t, extended, blocks_log2, ebno, _, _ in CODES:
        pc, y = decode_case(q, t, extended, blocks_log2, ebno)
        for p in (0, 2, 4):
            legs = {"call": lambda: pc.correct_batch(y, p, ALPHA, BETA),
                    "loop": lambda: parent_loop(pc.rows, pc.cols, y, p, ALPHA, BETA, extended)}
            ref = {k: f() for k, f in legs.items()}  # warm-up of both, and the same bits
            for k in ("out", "status"):
                assert torch.equal(ref["call"][k], ref["loop"][k]), k
            assert torch.equal(ref["call"]["ext"].view(torch.int32), ref["loop"]["ext"].view(torch.int32))
            times = {k: [] for k in legs}
            for run in range(3):
                for k in (("call", "loop") if run % 2 == 0 else ("loop", "call")):
                    times[k].append(timed(legs[k]))
            call, loop = times["call"], times["loop"]
            print("%-34s 2^%d blocks p=%d  call %8.3f [%8.3f .. %8.3f]  loop %8.3f [%8.3f .. %8.3f]  loop/call %5.2f  "
                  "loop spread %6.3f" % (pc.to_string(), blocks_log2, p, sorted(call)[1], min(call), max(call),
                                         sorted(loop)[1], min(loop), max(loop), sorted(loop)[1] / sorted(call)[1],
                                         max(loop) - min(loop)), flush=True)


def mc():
    from channelcoding_amd.montecarlo import ProductBackend
    print("mc: cc_mc_run_product_dev, p = 4, six half-iterations, random codewords, 3.0 dB; blocks per second of one call")
    for q, t, extended, _, _, blocks_log2, _ in CODES:
        pc = product(q, t, extended)
        backend = ProductBackend(pc, 4, ALPHA, BETA, True)
        blocks = 1 << blocks_log2
        backend.run(3.0, 1, 0, blocks)
        ms = [timed(lambda: backend.run(3.0, 1, 0, blocks)) for _ in range(3)]
        print("%-34s 2^%d blocks  %8.2f ms [%8.2f .. %8.2f]  %10.0f blocks/s  %6.1f Mvalues/s" % (
            pc.to_string(), blocks_log2, sorted(ms)[1], min(ms), max(ms), blocks / sorted(ms)[1] * 1e3,
            blocks * pc.n / sorted(ms)[1] * 1e-3), flush=True)


def curves():
    from channelcoding_amd.montecarlo import product_simulation
    for q, t, extended, _, _, _, blocks_log2 in CODES:
        pc = product(q, t, extended)
        sim = product_simulation(pc, 4, ALPHA, BETA, step=0.5, seed=1, random_codewords=True,
                                 samples_per_point=1 << blocks_log2)
        print("%s  rate %.4f  p = 4, six half-iterations, 2^%d blocks per point, seed 1" % (pc.to_string(), pc.rate,
                                                                                           blocks_log2))
        print("%6s %12s %12s %10s %10s" % ("ebno", "block errors", "bler", "ber", "failures"))
        for idx, ebno in enumerate(sim.points()):
            r = sim.run_point(ebno, 1 << blocks_log2, idx)
            print("%6.2f %12d %12.3e %10.3e %10d" % (ebno, r["word_errors"], r["wer"], r["ber"], r["failures"]), flush=True)
            if r["word_errors"] == 0:
                break


def trace(case, p):
    q, t, extended, blocks_log2, ebno, _, _ = CODES[case]
    pc, y = decode_case(q, t, extended, blocks_log2, ebno)
    for _ in range(5):
        pc.correct_batch(y, p, ALPHA, BETA)
    import torch
    torch.cuda.synchronize()
    print("trace: five calls of", pc.to_string(), "2^%d blocks, p = %d" % (blocks_log2, p))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["decode", "mc", "curves", "trace"])
    ap.add_argument("--case", type=int, default=0)
    ap.add_argument("--p", type=int, default=4)
    args = ap.parse_args()
    if args.what == "trace":
        trace(args.case, args.p)
    else:
        {"decode": decode, "mc": mc, "curves": curves}[args.what]()
