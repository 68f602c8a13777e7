"""Command line of the reference's simulation driver (src/simulation/benchmark.c++) on the GPU path.

    python -m channelcoding_amd.benchmark [--simulation awgn|bitflip|bsc|bec|burst|product|staircase] [--algorithm NAME|all]...
                                          [--k 5|6|7|all]... [--dmin 3|5|7|9|11|all]... [--seed N | --seed-time]
                                          [--threads N] [--log-dir DIR] [--p VALUE]... [--max-samples N]
                                          [--interleave I] [--p-gb VALUE] [--p-bg VALUE] [--p-good VALUE]
                                          [--p-detect VALUE] [--p-false-alarm VALUE] [--packed]

Same options, same decoder registry (benchmark.c++:23-166: primitive_bch<k, dmin<d>, A> for k in 5..7,
d in 3,5,7,9 and the nine algorithm tags, min-sum family with 50 iterations, NMS 8/10, OMS 1/100) and the same
selection rule (intersection of the chosen names, powers and distances; an option that is never given selects
everything; an empty selection prints the usage and fails, :430-433).  Each selected decoder runs the chosen
simulation and writes "<to_string()>.log" in the reference's two-column format.

Where the reference spreads the decoders over a pool of CPU threads (--threads, :435-439), every simulation
here is batched on the GPU; launched under torch.distributed.run the frames of each Eb/N0 point are sharded over
the ranks' GPUs (montecarlo.awgn_simulation).  --threads is accepted and ignored.

--simulation bsc / bec is new: the binary symmetric and the binary erasure channel the reference leaves as a TODO
(montecarlo.discrete_simulation), over the points given with --p (default 10^(-k/4), k = 4 .. 16), each decoder
writing "<to_string()>.<bsc|bec>.log".  --simulation bsc --packed runs the BSC on packed words
(montecarlo.discrete_simulation(packed=True)): the same channel, counters and log, an eighth of the bytes.

--simulation burst is new as well: the two-state Gilbert-Elliott channel run along symbol-interleaved blocks of depth
--interleave (montecarlo.burst_simulation), with the transition probabilities --p-gb (good -> bad) and --p-bg (bad ->
good) per transmitted symbol and the symbol error probability --p-good of the good state; the points given with --p are
the error probabilities of the bad state.  Each decoder writes "<to_string()>.burst.log".  --p-detect / --p-false-alarm
add a burst detector: a symbol is flagged with that probability in the bad / good state and handed to the decoder as an
erasure; the default, 0 and 0, is errors-only decoding.

--simulation product is the Eb/N0 ladder of a product code under the iterative Chase-Pyndiah decoder
(montecarlo.product_simulation): --k and --dmin (one value each, k = 3 .. 8) name the row code, --cols-k and --cols-dmin the
column code (default: the row code), --extended takes the two extended codes, --chase P the Chase positions (default 4),
and --alpha a,b,... and --beta a,b,... give the schedule, one value each per half-iteration.  There is no default
schedule.  The log is "<rows>x<cols>[-ext]-chaseP-hH.log".  With --halves H in place of --alpha / --beta the ladder runs
H half-iterations of hard-decision row / column decoding (montecarlo.product_hard_simulation) and the log is
"<rows>x<cols>[-ext]-hard-hH.log", with the mean of the half-iterations a block took next to wer.  With --anchor DELTA next
to --halves H the half-iterations are those of anchor decoding (montecarlo.product_anchor_simulation): a converged line is
taken back after DELTA conflicts in one pass; there is no default, and the log is "<rows>x<cols>[-ext]-anchorDELTA-hH.log".
With --weights a,b,...
in place of all three the ladder runs iBDD with scaled reliability (montecarlo.product_sr_simulation), one weight per
half-iteration (inf is a weight), and the log is "<rows>x<cols>[-ext]-srH.log".

--simulation staircase --blocks L --window W --iters I [--extended] is the Eb/N0 ladder of a staircase code under its
sliding-window hard-decision decoder (montecarlo.staircase_simulation): --k and --dmin (one value each, k = 3 .. 8) name
the component code -- with --extended its extended code, otherwise the code shortened by one position, so that a line has
an even number of bits -- streams of L blocks, a window of W = 2 .. 16 blocks and I iterations per window position.  There
is no default for the three.  ber is taken over the blocks decoded with a full window; the log is
"staircase(<code>[-ext], L=.., W=.., I=..).log".  With --weights a,b,... the ladder runs the window decoder with scaled
reliability (montecarlo.staircase_sr_simulation), exactly 2 I weights, one per half-pass of a window position (inf is a
weight), and the log is "staircase(<code>[-ext], L=.., W=.., I=..)-sr.log".
"""
import argparse
import sys
import time

from . import codes as cc
from .montecarlo import (awgn_simulation, bitflip_simulation, burst_simulation, discrete_simulation,
                         product_anchor_simulation, product_hard_simulation, product_simulation, product_sr_simulation, staircase_simulation,
                         staircase_sr_simulation)

POWERS = (5, 6, 7)
DISTANCES = (3, 5, 7, 9)
ITERATIONS = 50
# to_string() suffix, lower-cased (benchmark.c++:212-216) -> tag factory
ALGORITHMS = {
    "bm": lambda: cc.berlekamp_massey_tag(),
    "pgz": lambda: cc.peterson_gorenstein_zierler_tag(),
    "euklid": lambda: cc.euklid_tag(),
    "ms": lambda: cc.min_sum_tag(ITERATIONS),
    "nms": lambda: cc.normalized_min_sum_tag(ITERATIONS, 8 / 10),
    "oms": lambda: cc.offset_min_sum_tag(ITERATIONS, 1 / 100),
    "scms1": lambda: cc.self_correcting_1_min_sum_tag(ITERATIONS),
    "scms2": lambda: cc.self_correcting_2_min_sum_tag(ITERATIONS),
    "2dnms": lambda: cc.normalized_2d_min_sum_tag(ITERATIONS),
}


_REGISTRY = None


def registry():
    """(name, k, template dmin, reported dmin) of every decoder the reference instantiates, in its order.
    The reference keys --dmin on the distance PRINTED by to_string() (benchmark.c++:224-230), which is the true
    BCH bound of the generator and can exceed the template argument: primitive_bch<5, dmin<9>> reports 11."""
    global _REGISTRY
    if _REGISTRY is None:
        from . import _capi as capi
        reg = []
        for name in ALGORITHMS:
            for k in POWERS:
                for d in DISTANCES:
                    text = cc.primitive_bch(k, cc.dmin(d), ALGORITHMS[name](), device=capi.DEVICE_NONE).to_string()
                    reg.append((name, k, d, int(text[text.rindex(" ") + 1:text.rindex(")")])))
        _REGISTRY = reg
    return _REGISTRY


def reported_distances():
    return sorted({r[3] for r in registry()})


def usage_text():
    lines = ["--simulation [awgn|bitflip|bsc|bec|burst|product|staircase]",
             "                             Choose the simulation to run. The default is AWGN.",
             "--algorithm <name>           Choose algorithm:"]
    lines += ["  " + a for a in ALGORITHMS]
    lines += ["--k <num>                    Choose code length n = 2^k - 1;"] + ["  %d" % k for k in POWERS]
    lines += ["--dmin <num>                 Choose dmin of the code:"] + ["  %d" % d for d in reported_distances()]
    lines += ["--seed <num>                 Set seed of the random number generator. The default is 0.",
              "--seed-time                  Use the current time as seed for the random number generator.",
              "--threads <num>              Accepted for compatibility; simulations are batched on the GPU(s).",
              "--stop-rule <0|1|2>          Min-sum stop rule: 0 as shipped, 1 published, 2 GF(2) parity (default).",
              "--log-dir <dir>              Where the <decoder>.log files go (default: current directory).",
              "--p <value>                  bsc / bec: error / erasure probability of a point (burst: the error",
              "                             probability of the bad state); may be given several times. The default",
              "                             is 10^(-k/4) for k = 4 .. 16.",
              "--interleave <num>           burst: depth of the symbol-interleaved blocks, 1 .. 256. The default is 1.",
              "--p-gb <value>               burst: probability good -> bad per symbol. The default is 0.01.",
              "--p-bg <value>               burst: probability bad -> good per symbol. The default is 0.1.",
              "--p-good <value>             burst: symbol error probability of the good state. The default is 0.",
              "--p-detect <value>           burst: P(symbol flagged | bad state) of a burst detector whose flags are erasures",
              "                             to the decoder. The default is 0.",
              "--p-false-alarm <value>      burst: P(symbol flagged | good state). The default is 0.",
              "--packed                     bsc: channel, decoder and counts on packed words (hard-decision algorithms).",
              "--chase <p>                  awgn: Chase-II over the p least reliable positions, 0 .. 6 (hard-decision",
              "                             algorithms; the log is <decoder>-chase<p>.log).",
              "--osd <order>                awgn: ordered-statistics decoding of order 0 .. 2 (hard-decision algorithms;",
              "                             the log is <decoder>-osd<order>.log). It does not combine with --chase.",
              "--cols-k <num>               product: the column code's k (--k names the row code; default: the row code).",
              "--cols-dmin <num>            product: the column code's dmin (--dmin names the row code's).",
              "--extended                   product: the product of the two extended codes.",
              "--alpha <a,b,...>            product: the factor of W of every half-iteration. There is no default.",
              "--beta <a,b,...>             product: the value of a position without a competitor, per half-iteration.",
              "--halves <num>               product: hard-decision row / column decoding with that many half-iterations,",
              "                             in place of --alpha and --beta.",
              "--anchor <delta>             product: with --halves, anchor decoding: a converged line is taken back after",
              "                             delta >= 1 conflicts in one pass. There is no default.",
              "--weights <a,b,...>          product: iBDD with scaled reliability, one weight per half-iteration (inf is",
              "                             one), in place of --alpha, --beta and --halves.",
              "                             staircase: the window decoder with scaled reliability, exactly 2 * iters",
              "                             weights, one per half-pass of a window position.",
              "--blocks <num>               staircase: blocks per stream. There is no default.",
              "--window <num>               staircase: the decoder's window in blocks, 2 .. 16. There is no default.",
              "--iters <num>                staircase: iterations per window position. There is no default.",
              "--max-samples <num>          awgn / bsc / bec / burst / product / staircase: cap on the frames of one point.",
              "",
              "algorithm, k, and dmin can be specified multiple times.",
              "For all other options, giving them multiple times results in the last value being used."]
    return "\n".join(lines)


def select(algorithms, powers, distances):
    """benchmark.c++:374-428."""
    def chosen(values, reference, what, convert):
        out = set()
        for v in values or ():
            v = str(v).lower()
            if v == "all":
                return set(reference)
            try:
                key = convert(v)
            except ValueError:
                key = None
            if key not in reference:
                raise SystemExit("Unknown %s '%s'\n%s" % (what, v, usage_text()))
            out.add(key)
        return out or set(reference)

    names = chosen(algorithms, set(ALGORITHMS), "algorithm", str)
    ks = chosen(powers, set(POWERS), "k", int)
    ds = chosen(distances, set(reported_distances()), "dmin", int)
    return [(a, k, d) for a, k, d, shown in registry() if a in names and k in ks and shown in ds]


def build(name, k, d, stop_rule, device=None):
    kw = {} if device is None else {"device": device}
    return cc.primitive_bch(k, cc.dmin(d), ALGORITHMS[name](), stop_rule=stop_rule, **kw)


def join_ranks():
    """under torch.distributed.run: this rank's GPU and the process group; None for a single process"""
    import torch
    try:
        import os
        import torch.distributed as tdist
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            local = int(os.environ.get("LOCAL_RANK", "0"))
            torch.cuda.set_device(local)
            tdist.init_process_group("nccl", device_id=torch.device("cuda", local))
            return tdist
    except ImportError:
        pass
    return None


def product_arguments(args):
    """(rows (k, dmin), cols (k, dmin), p, alpha, beta) of --simulation product, or a message saying what is wrong"""
    try:
        if not args.k or len(args.k) != 1 or not args.dmin or len(args.dmin) != 1:
            return "--simulation product takes one --k and one --dmin"
        rows = (int(args.k[0]), int(args.dmin[0]))
        cols = (rows[0] if args.cols_k is None else args.cols_k, rows[1] if args.cols_dmin is None else args.cols_dmin)
        if args.alpha is None or args.beta is None:
            return "--simulation product needs --alpha and --beta: there is no default schedule"
        alpha, beta = ([float(v) for v in text.split(",")] for text in (args.alpha, args.beta))
    except ValueError:
        return "--k, --dmin, --alpha and --beta take numbers"
    p = 4 if args.chase is None else args.chase
    if not 0 <= p <= 6:
        return "--chase <0..6>"
    if len(alpha) != len(beta):
        return "--alpha and --beta take one value each per half-iteration"
    for k, d in (rows, cols):
        if not 3 <= k <= 8 or d < 3 or d % 2 == 0:
            return "--simulation product takes k = 3 .. 8 and an odd dmin >= 3"
    return rows, cols, p, alpha, beta


def product_hard_arguments(args):
    """(rows (k, dmin), cols (k, dmin), halves) of --simulation product --halves H, or a message saying what is wrong"""
    if args.alpha is not None or args.beta is not None:
        return "--halves runs the hard-decision decoder: it does not combine with --alpha or --beta"
    if args.halves < 1:
        return "--halves <1..>"
    try:
        if not args.k or len(args.k) != 1 or not args.dmin or len(args.dmin) != 1:
            return "--simulation product takes one --k and one --dmin"
        rows = (int(args.k[0]), int(args.dmin[0]))
    except ValueError:
        return "--k and --dmin take numbers"
    cols = (rows[0] if args.cols_k is None else args.cols_k, rows[1] if args.cols_dmin is None else args.cols_dmin)
    for k, d in (rows, cols):
        if not 3 <= k <= 8 or d < 3 or d % 2 == 0:
            return "--simulation product takes k = 3 .. 8 and an odd dmin >= 3"
    return rows, cols, args.halves


def product_anchor_arguments(args):
    """(rows (k, dmin), cols (k, dmin), halves, delta) of --simulation product --halves H --anchor DELTA, or a message
    saying what is wrong"""
    if getattr(args, "halves", None) is None:
        return "--anchor goes with --halves: anchor decoding runs that many half-iterations"
    if getattr(args, "weights", None) is not None:
        return "--anchor does not combine with --weights"
    parsed = product_hard_arguments(args)
    if isinstance(parsed, str):
        return parsed
    if not 1 <= args.anchor < 1 << 32:
        return "--anchor <1..>"
    return parsed + (args.anchor,)


def product_sr_arguments(args):
    """(rows (k, dmin), cols (k, dmin), weights) of --simulation product --weights a,b,..., or a message saying what is
    wrong"""
    if args.alpha is not None or args.beta is not None or args.halves is not None:
        return "--weights runs iBDD with scaled reliability: it does not combine with --alpha, --beta or --halves"
    try:
        if not args.k or len(args.k) != 1 or not args.dmin or len(args.dmin) != 1:
            return "--simulation product takes one --k and one --dmin"
        rows = (int(args.k[0]), int(args.dmin[0]))
    except ValueError:
        return "--k and --dmin take numbers"
    try:
        weights = [float(v) for v in args.weights.split(",")]
    except ValueError:
        return "--weights takes numbers, one per half-iteration"
    if any(w != w or w < 0 for w in weights):
        return "--weights takes weights >= 0 (inf is one)"
    cols = (rows[0] if args.cols_k is None else args.cols_k, rows[1] if args.cols_dmin is None else args.cols_dmin)
    for k, d in (rows, cols):
        if not 3 <= k <= 8 or d < 3 or d % 2 == 0:
            return "--simulation product takes k = 3 .. 8 and an odd dmin >= 3"
    return rows, cols, weights


def build_product(rows, cols, extended, device=None):
    kw = {} if device is None else {"device": device}
    make = lambda k, d: cc.primitive_bch(k, cc.dmin(d), cc.berlekamp_massey_tag(), **kw)
    return cc.product_code(make(*rows), make(*cols), extended=extended)


def product_main(args):
    anchor = getattr(args, "anchor", None) is not None
    sr = not anchor and getattr(args, "weights", None) is not None
    hard = not anchor and not sr and getattr(args, "halves", None) is not None
    parsed = product_anchor_arguments(args) if anchor else product_sr_arguments(args) if sr \
        else product_hard_arguments(args) if hard else product_arguments(args)
    if isinstance(parsed, str):
        print(parsed, file=sys.stderr)
        print(usage_text())
        return 1
    seed = time.time_ns() if args.seed_time else args.seed
    dist = join_ranks()
    pc = build_product(parsed[0], parsed[1], args.extended)
    t0 = time.perf_counter()
    if anchor:
        res = product_anchor_simulation(pc, parsed[3], parsed[2], seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    elif sr:
        res = product_sr_simulation(pc, parsed[2], seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    elif hard:
        res = product_hard_simulation(pc, parsed[2], seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    else:
        rows, cols, p, alpha, beta = parsed
        res = product_simulation(pc, p, alpha, beta, seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    if not dist or dist.get_rank() == 0:
        print("%s: %d blocks in %.2f s" % (pc.to_string(), sum(r["frames"] for r in res), time.perf_counter() - t0), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def staircase_arguments(args):
    """(k, dmin, blocks, window, iters) of --simulation staircase, or a message saying what is wrong"""
    if args.alpha is not None or args.beta is not None or args.halves is not None or args.cols_k is not None \
            or args.cols_dmin is not None or args.chase is not None or args.osd is not None:
        return "--simulation staircase takes --k, --dmin, --blocks, --window, --iters and --extended"
    try:
        if not args.k or len(args.k) != 1 or not args.dmin or len(args.dmin) != 1:
            return "--simulation staircase takes one --k and one --dmin"
        k, d = int(args.k[0]), int(args.dmin[0])
    except ValueError:
        return "--k and --dmin take numbers"
    if not 3 <= k <= 8 or d < 3 or d % 2 == 0:
        return "--simulation staircase takes k = 3 .. 8 and an odd dmin >= 3"
    if args.blocks is None or args.window is None or args.iters is None:
        return "--simulation staircase needs --blocks, --window and --iters: there is no default"
    if args.blocks < 1 or not 2 <= args.window <= cc.capi.STAIRCASE_MAX_WINDOW or args.iters < 1:
        return "--blocks <1..> --window <2..%d> --iters <1..>" % cc.capi.STAIRCASE_MAX_WINDOW
    return k, d, args.blocks, args.window, args.iters


def staircase_sr_arguments(args):
    """(k, dmin, blocks, window, iters, weights) of --simulation staircase --weights a,b,..., or a message saying what is
    wrong"""
    parsed = staircase_arguments(args)
    if isinstance(parsed, str):
        return parsed
    try:
        weights = [float(v) for v in args.weights.split(",")]
    except ValueError:
        return "--weights takes numbers, one per half-pass"
    if any(w != w or w < 0 for w in weights):
        return "--weights takes weights >= 0 (inf is one)"
    if len(weights) != 2 * parsed[4]:
        return "--weights takes one weight per half-pass of a window position: 2 * iters = %d" % (2 * parsed[4])
    return parsed + (weights,)


def build_staircase(k, d, blocks, window, iters, extended, device=None):
    """the component shortened by one position where the line would otherwise have an odd number of bits"""
    kw = {} if device is None else {"device": device}
    n = (1 << k) - 1
    if not extended:
        kw["n"] = n - 1
    return cc.staircase_code(cc.primitive_bch(k, cc.dmin(d), cc.berlekamp_massey_tag(), **kw), blocks, window, iters,
                             extended=extended)


def staircase_main(args):
    sr = getattr(args, "weights", None) is not None
    parsed = staircase_sr_arguments(args) if sr else staircase_arguments(args)
    if isinstance(parsed, str):
        print(parsed, file=sys.stderr)
        print(usage_text())
        return 1
    seed = time.time_ns() if args.seed_time else args.seed
    dist = join_ranks()
    try:
        sc = build_staircase(*parsed[:5], args.extended)
    except ValueError as err:
        print("--simulation staircase: %s" % err, file=sys.stderr)
        return 1
    t0 = time.perf_counter()
    if sr:
        res = staircase_sr_simulation(sc, parsed[5], seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    else:
        res = staircase_simulation(sc, seed=seed, log_dir=args.log_dir, max_samples=args.max_samples)()
    if not dist or dist.get_rank() == 0:
        print("%s: %d streams in %.2f s" % (sc.to_string(), sum(r["frames"] for r in res), time.perf_counter() - t0), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="channelcoding_amd.benchmark", add_help=False)
    ap.add_argument("--simulation", "-simulation", default="awgn")
    ap.add_argument("--algorithm", "-algorithm", action="append")
    ap.add_argument("--k", "-k", action="append")
    ap.add_argument("--dmin", "-dmin", action="append")
    ap.add_argument("--seed", "-seed", type=lambda v: int(v, 0), default=0)
    ap.add_argument("--seed-time", "-seed-time", action="store_true")
    ap.add_argument("--threads", "-threads", type=int, default=None)
    ap.add_argument("--stop-rule", type=int, default=2)
    ap.add_argument("--log-dir", default=".")
    ap.add_argument("--errors", type=int, default=0, help="bitflip: largest number of flipped bits")
    ap.add_argument("--max-samples", type=int, default=None, help="awgn / bsc / bec: cap on frames per point")
    ap.add_argument("--p", "-p", type=float, action="append", default=None, help="bsc / bec: channel probability")
    ap.add_argument("--interleave", type=int, default=1, help="burst: depth of the interleaved blocks")
    ap.add_argument("--p-gb", type=float, default=0.01, help="burst: P(good -> bad) per symbol")
    ap.add_argument("--p-bg", type=float, default=0.1, help="burst: P(bad -> good) per symbol")
    ap.add_argument("--p-good", type=float, default=0.0, help="burst: symbol error probability of the good state")
    ap.add_argument("--p-detect", type=float, default=0.0, help="burst: P(flag | bad state) of the burst detector")
    ap.add_argument("--p-false-alarm", type=float, default=0.0, help="burst: P(flag | good state)")
    ap.add_argument("--packed", action="store_true", help="bsc: the route on packed words")
    ap.add_argument("--chase", type=int, default=None, help="awgn: Chase-II with p least reliable positions")
    ap.add_argument("--osd", type=int, default=None, help="awgn: ordered-statistics decoding of this order")
    ap.add_argument("--cols-k", type=int, default=None, help="product: k of the column code")
    ap.add_argument("--cols-dmin", type=int, default=None, help="product: dmin of the column code")
    ap.add_argument("--extended", action="store_true", help="product: the two extended codes")
    ap.add_argument("--alpha", default=None, help="product: a,b,... one per half-iteration")
    ap.add_argument("--beta", default=None, help="product: a,b,... one per half-iteration")
    ap.add_argument("--halves", type=int, default=None, help="product: hard-decision decoding, this many half-iterations")
    ap.add_argument("--anchor", type=int, default=None, help="product: with --halves, anchor decoding at this delta")
    ap.add_argument("--weights", default=None, help="product: iBDD-SR, a,b,... one weight per half-iteration; staircase: the window decoder with scaled "
                         "reliability, exactly 2 * iters weights")
    ap.add_argument("--blocks", type=int, default=None, help="staircase: blocks per stream")
    ap.add_argument("--window", type=int, default=None, help="staircase: window of the decoder in blocks")
    ap.add_argument("--iters", type=int, default=None, help="staircase: iterations per window position")
    ap.add_argument("--help", "-h", action="store_true")
    args, unknown = ap.parse_known_args(argv)
    if args.help or unknown:
        if unknown:
            print("Unkown argument: %s" % " ".join(unknown), file=sys.stderr)
        print(usage_text())
        return 1
    sim = args.simulation.lower()
    if sim == "product":
        return product_main(args)
    if sim == "staircase":
        return staircase_main(args)
    if sim not in ("awgn", "bitflip", "bsc", "bec", "burst"):
        print("Don't know the simulation type '%s'" % sim, file=sys.stderr)
        print(usage_text())
        return 1
    if args.packed and sim != "bsc":
        print("--packed goes with --simulation bsc", file=sys.stderr)
        print(usage_text())
        return 1
    if args.chase is not None and (sim != "awgn" or not 0 <= args.chase <= 6):
        print("--chase <0..6> goes with --simulation awgn", file=sys.stderr)
        print(usage_text())
        return 1
    if args.osd is not None and (sim != "awgn" or not 0 <= args.osd <= 2 or args.chase is not None):
        print("--osd <0..2> goes with --simulation awgn and without --chase", file=sys.stderr)
        print(usage_text())
        return 1
    chosen = select(args.algorithm, args.k, args.dmin)
    if args.chase is not None or args.osd is not None:  # the hard-tag decoders of the registry
        chosen = [c for c in chosen if not ALGORITHMS[c[0]]().soft]
    if not chosen:
        print("The selection is empty")
        print(usage_text())
        return 1
    seed = time.time_ns() if args.seed_time else args.seed

    dist = join_ranks()
    rank = dist.get_rank() if dist else 0
    for name, k, d in chosen:
        code = build(name, k, d, args.stop_rule)
        t0 = time.perf_counter()
        if sim == "awgn":
            res = awgn_simulation(code, seed=seed, log_dir=args.log_dir, max_samples=args.max_samples,
                                  chase=args.chase, osd=args.osd)()
            frames = sum(r["frames"] for r in res)
        elif sim in ("bsc", "bec"):
            packed = dict(packed=True) if args.packed else {}
            res = discrete_simulation(code, sim, points=args.p, seed=seed, log_dir=args.log_dir,
                                      max_samples=args.max_samples, **packed)()
            frames = sum(r["frames"] for r in res)
        elif sim == "burst":
            detector = {}
            if args.p_detect or args.p_false_alarm:
                detector = dict(p_detect=args.p_detect, p_false_alarm=args.p_false_alarm)
            res = burst_simulation(code, interleave=args.interleave, p_gb=args.p_gb, p_bg=args.p_bg,
                                   p_error_good=args.p_good, points=args.p, seed=seed, log_dir=args.log_dir,
                                   max_samples=args.max_samples, **detector)()
            frames = sum(r["frames"] for r in res)
        else:
            if rank == 0:
                res = bitflip_simulation(code, args.errors, log_dir=args.log_dir)()
                frames = sum(r["patterns"] for r in res)
            else:
                frames = 0
        if rank == 0:
            print("%s: %d frames in %.2f s" % (code.to_string(), frames, time.perf_counter() - t0), flush=True)
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
