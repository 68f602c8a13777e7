"""Batched AWGN (and discrete-channel) Monte-Carlo harness, sharded over the GPUs of one node.

Replaces ``awgn_simulation`` (src/simulation/simulation.h:71-83, simulation.c++:83-150 of the
reference).  What is kept: the Eb/N0 ladder (start just above the Shannon limit of the code's rate,
``step`` dB apart, up to max(8, start)), the adaptive sample count ``min(1e6, 5e3 / wer)`` seeded with
wer = 0.5 (simulation.c++:91-93,:110), sigma = 1/sqrt(2 R 10^(EbN0/10)) (:83-85), word-error counting
(:128-135) and the two-column log file "<to_string()>.log" with the reference's field widths (:96-103,
:145-148; an existing file is refused, :72-81).

What is new: frames of one point are independent, so rank r of W decodes the contiguous range
[r*F/W, (r+1)*F/W) of the *global* frame index on its own GPU (cc_mc_run_dev generates the noise on
device from (seed, global frame index)), and ONE all-reduce (RCCL over xGMI for CUDA tensors, gloo on
CPU) of the 64-word counter vector per point gives every rank the totals -- which the adaptive sample
count of the next point needs.  Totals are bit-identical for any number of ranks.

discrete_simulation runs the same harness over the BSC, the BEC or both at once (cc_mc_run_discrete_dev; for RS codes
the q-ary symmetric and the symbol erasure channel), on a ladder of channel probabilities -- with packed=True the BSC on
packed words (cc_mc_run_bsc_packed_dev), which serves the binary BCH codes of every q = 3 .. 15; burst_simulation over the
two-state Gilbert-Elliott channel run along symbol-interleaved blocks (cc_mc_run_burst_dev), sharded in whole blocks;
with a burst detector (p_detect, p_false_alarm) the flagged symbols go to the decoder as erasures
(cc_mc_run_burst_erasure_dev).

The ladder's start point follows the reference's own Shannon-limit look-up ``ebno()`` (simulation.c++:21-70)
including its indexing (see `reference_ebno`), so every "<decoder>.log" starts on the line the reference's does.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _capi as capi

COUNTER_NAMES = {
    "frames": capi.MC_FRAMES, "word_errors": capi.MC_WORD_ERRORS, "bit_errors": capi.MC_BIT_ERRORS,
    "failures": capi.MC_FAILURES, "undetected": capi.MC_UNDETECTED, "iter_sum": capi.MC_ITER_SUM,
    "channel_bit_errors": capi.MC_CHANNEL_BIT_ERRORS,
}


# Shannon limit of the BPSK-AWGN channel (dB) for the code rates of RATES -- the data of simulation.c++:21-52:
# rates 0.01 .. 0.80 in steps of 0.01, then 51 unevenly spaced rates up to 0.999.
RATES = tuple(i / 100.0 for i in range(1, 81)) + (
    0.807, 0.817, 0.827, 0.837, 0.846, 0.855, 0.864, 0.872, 0.880, 0.887, 0.894, 0.900, 0.907, 0.913, 0.918, 0.924,
    0.929, 0.934, 0.938, 0.943, 0.947, 0.951, 0.954, 0.958, 0.961, 0.964, 0.967, 0.970, 0.972, 0.974, 0.976, 0.978,
    0.980, 0.982, 0.983, 0.984, 0.985, 0.986, 0.987, 0.988, 0.989, 0.990, 0.991, 0.992, 0.993, 0.994, 0.995, 0.996,
    0.997, 0.998, 0.999)
LIMITS = (
    -1.548, -1.531, -1.500, -1.470, -1.440, -1.409, -1.378, -1.347, -1.316, -1.285, -1.254, -1.222, -1.190, -1.158,
    -1.126, -1.094, -1.061, -1.028, -0.995, -0.963, -0.928, -0.896, -0.861, -0.827, -0.793, -0.757, -0.724, -0.687,
    -0.651, -0.616, -0.579, -0.544, -0.507, -0.469, -0.432, -0.394, -0.355, -0.314, -0.276, -0.236, -0.198, -0.156,
    -0.118, -0.074, -0.032, 0.010, 0.055, 0.097, 0.144, 0.188, 0.233, 0.279, 0.326, 0.374, 0.424, 0.474, 0.526, 0.574,
    0.628, 0.682, 0.734, 0.791, 0.844, 0.904, 0.960, 1.021, 1.084, 1.143, 1.208, 1.275, 1.343, 1.412, 1.483, 1.554,
    1.628, 1.708, 1.784, 1.867, 1.952, 2.045, 2.108, 2.204, 2.302, 2.402, 2.503, 2.600, 2.712, 2.812, 2.913, 3.009,
    3.114, 3.205, 3.312, 3.414, 3.500, 3.612, 3.709, 3.815, 3.906, 4.014, 4.115, 4.218, 4.304, 4.425, 4.521, 4.618,
    4.725, 4.841, 4.922, 5.004, 5.104, 5.196, 5.307, 5.418, 5.484, 5.549, 5.615, 5.681, 5.756, 5.842, 5.927, 6.023,
    6.119, 6.234, 6.360, 6.495, 6.651, 6.837, 7.072, 7.378, 7.864)
assert len(RATES) == 131 and len(LIMITS) == 131


def reference_ebno(rate):
    """`ebno(rate)` of simulation.c++:56-70, indexing included.

    rate <= 0.8 reads LIMITS[size_t(rate * 100)]: RATES[0] is 0.01, so this is the entry ONE rate step above
    the truncated rate (R = 16/31 = 0.516 reads the limit of R = 0.52).  rate >= 0.999 reads the last entry.
    In between, the first entry from index 80 (0.807) whose rate is >= `rate`, searched up to (not including)
    the last entry -- which is what the search returns when nothing matches.
    """
    rate = float(rate)
    if rate <= 0.800:
        return LIMITS[int(rate * 100)]
    if rate >= 0.999:
        return LIMITS[-1]
    index = 80
    while index < len(RATES) - 1 and not RATES[index] >= rate:
        index += 1
    return LIMITS[index]


def ladder(rate, step=0.5):
    """(start, max) of the Eb/N0 loop, simulation.c++:105-107: tmp = size_t(ebno(rate) / step) truncates toward
    zero (a negative limit gives tmp = 0: the conversion of a negative double is undefined in C++; every compiler
    the reference builds with yields 0 on x86-64 for values in (-1, 0], and the registry has no rate below 0.19)."""
    tmp = max(0, int(reference_ebno(rate) / step))
    start = (tmp + 1.0 / step) * step
    return start, max(8.0, start) + step / 2


def bpsk_capacity(snr_linear):
    """Capacity (bits/use) of the binary-input AWGN channel at Es/N0 = snr_linear, by Gauss-Hermite quadrature."""
    sigma2 = 1.0 / (2.0 * snr_linear)
    x, w = np.polynomial.hermite_e.hermegauss(96)
    y = 1.0 + math.sqrt(sigma2) * x
    llr = 2.0 * y / sigma2
    return 1.0 - float(np.sum(w * np.log2(1.0 + np.exp(-llr))) / math.sqrt(2.0 * math.pi))


def shannon_limit_ebno_db(rate):
    """Smallest Eb/N0 (dB) at which a rate-`rate` code can work on the BPSK-AWGN channel, solved numerically.
    Not used for the ladder (the reference's table is, `reference_ebno`); kept as the cross-check of that table
    (tests/test_host_logic.py: every entry within 0.12 dB of the solve)."""
    lo, hi = -3.0, 12.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if bpsk_capacity(rate * 10.0 ** (mid / 10.0)) >= rate:
            hi = mid
        else:
            lo = mid
    return hi


def samples(wer):
    """simulation.c++:91-93: min(1e6, 5e3 / wer); wer == 0 gives the cap (5e3 / 0.0 is +inf in the reference)."""
    return int(min(1e6, 5e3 / wer)) if wer > 0 else 1000000


def shard(total, rank, world):
    """Contiguous range of the global frame index owned by `rank`."""
    lo = total * rank // world
    hi = total * (rank + 1) // world
    return lo, hi - lo


def shard_blocks(total, rank, world, interleave):
    """`shard` cut at multiples of `interleave`: the contiguous range of whole blocks owned by `rank`."""
    lo, count = shard(total // interleave, rank, world)
    return lo * interleave, count * interleave


class DeviceBackend:
    """Counts one shard of one Eb/N0 point on this rank's GPU through cc_mc_run_dev."""

    symbol, leading = "cc_mc_run_dev", ()  # the entry point and the arguments between the handle and Eb/N0
    desc = None  # the cc_product of a product backend: the call takes it by reference in place of the handle

    def __init__(self, code, random_codewords=False):
        import torch
        self.torch = torch
        self.code = code
        self.random_codewords = bool(random_codewords)
        self.device = torch.device("cuda", torch.cuda.current_device())

    def target(self):
        """The first argument of the call."""
        return self.code._h if self.desc is None else C.byref(self.desc)

    def run(self, ebno_db, seed, first_frame, frames):
        torch = self.torch
        counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = getattr(capi.lib(), self.symbol)(self.target(), *self.leading, float(ebno_db), int(seed), int(first_frame),
                                              int(frames), int(self.random_codewords), C.c_void_p(counters.data_ptr()), stream)
        capi.check(rc, self.symbol)
        return counters  # stays on the device: reduced with RCCL


class ChaseBackend(DeviceBackend):
    """The same shard through cc_mc_run_chase_dev: Chase-II over the p least reliable positions of every frame
    (binary BCH with a hard tag, q <= 8, 2t <= 32)."""

    symbol = "cc_mc_run_chase_dev"

    def __init__(self, code, p, random_codewords=False):
        super().__init__(code, random_codewords)
        self.p = int(p)
        if not 0 <= self.p <= capi.CHASE_MAX_P:
            raise ValueError("chase= takes p in 0 .. %d" % capi.CHASE_MAX_P)
        self.leading = (self.p,)


class OsdBackend(DeviceBackend):
    """The same shard through cc_mc_run_osd_dev: ordered-statistics decoding of the given order on every frame (binary
    BCH with a hard tag, q <= 8); every frame decodes, so the failure counter stays 0."""

    symbol = "cc_mc_run_osd_dev"

    def __init__(self, code, order, random_codewords=False):
        super().__init__(code, random_codewords)
        self.order = int(order)
        if not 0 <= self.order <= capi.OSD_MAX_ORDER:
            raise ValueError("osd= takes an order in 0 .. %d" % capi.OSD_MAX_ORDER)
        self.leading = (self.order,)


class GmdBackend(DeviceBackend):
    """The same shard through cc_mc_run_gmd_dev: BPSK/AWGN per symbol bit, then GMD with m trials on every frame (RS with
    a hard tag, q <= 8, 2t <= 32, step = 1; m = True: all t + 1)."""

    symbol = "cc_mc_run_gmd_dev"

    def __init__(self, code, m, random_codewords=False):
        super().__init__(code, random_codewords)
        self.m = capi.gmd_trials(m)
        self.leading = (self.m,)


class ProductBackend(DeviceBackend):
    """Counts one shard of blocks of one Eb/N0 point through cc_mc_run_product_dev: a product_code decoded with len(alpha)
    half-iterations of the Chase-Pyndiah decoder at p."""

    symbol = "cc_mc_run_product_dev"

    def __init__(self, pc, p, alpha, beta, random_codewords=False):
        super().__init__(pc, random_codewords)
        self.p = int(p)
        if not 0 <= self.p <= capi.CHASE_MAX_P:
            raise ValueError("p in 0 .. %d" % capi.CHASE_MAX_P)
        if not len(alpha) or len(alpha) != len(beta):
            raise ValueError("one alpha and one beta per half-iteration, at least one")
        self.desc = pc._pc(self.p, alpha, beta)


class ProductHardBackend(DeviceBackend):
    """Counts one shard of blocks of one Eb/N0 point through cc_mc_run_product_hard_dev: a product_code decoded with
    `halves` half-iterations of bounded-distance row / column decoding on the hard decisions of the channel."""

    symbol = "cc_mc_run_product_hard_dev"

    def __init__(self, pc, halves, random_codewords=False):
        super().__init__(pc, random_codewords)
        self.desc = pc._pc_hard(halves)


class ProductAnchorBackend(DeviceBackend):
    """Counts one shard of blocks of one Eb/N0 point through cc_mc_run_product_anchor_dev: a product_code decoded with
    `halves` half-iterations of anchor decoding at `delta` (codes.product_code.correct_anchor_batch) on the hard decisions
    of the channel."""

    symbol = "cc_mc_run_product_anchor_dev"

    def __init__(self, pc, delta, halves, random_codewords=False):
        from .codes import _anchor_delta
        super().__init__(pc, random_codewords)
        self.delta = _anchor_delta(delta)
        self.desc = pc._pc_hard(halves)
        self.leading = (self.delta,)


class ProductSrBackend(DeviceBackend):
    """Counts one shard of blocks of one Eb/N0 point through cc_mc_run_product_sr_dev: a product_code decoded with
    len(weights) half-iterations of iBDD with scaled reliability (codes.product_code.correct_sr_batch)."""

    symbol = "cc_mc_run_product_sr_dev"

    def __init__(self, pc, weights, random_codewords=False):
        from .codes import _sr_weights
        super().__init__(pc, random_codewords)
        self.weights = _sr_weights(weights)
        self.desc = pc._pc_hard(len(self.weights))
        self.leading = (self.weights,)


class StaircaseBackend(DeviceBackend):
    """Counts one shard of streams of one Eb/N0 point through cc_mc_run_staircase_dev: a staircase_code under its
    sliding-window decoder on the hard decisions of the channel; bit errors are those of the counted blocks."""

    symbol = "cc_mc_run_staircase_dev"

    def __init__(self, sc, random_codewords=False):
        super().__init__(sc, random_codewords)
        self.desc = sc._sc()


class StaircaseSrBackend(DeviceBackend):
    """Counts one shard of streams of one Eb/N0 point through cc_mc_run_staircase_sr_dev: a staircase_code under its
    sliding-window decoder with scaled reliability (codes.staircase_code.correct_sr_batch), 2 * iters weights."""

    symbol = "cc_mc_run_staircase_sr_dev"

    def __init__(self, sc, weights, random_codewords=False):
        super().__init__(sc, random_codewords)
        self.weights = sc._weights(weights)
        self.desc = sc._sc()
        self.leading = (self.weights,)


class _ShardedSimulation:
    """What the AWGN, the discrete-channel and the burst-channel ladders share: the shard of this rank, the one all-reduce per point,
    rank 0's log file (its success agreed with every rank before the first collective) and the adaptive ladder."""

    counter_names = COUNTER_NAMES
    interleave = 1  # frames are counted and sharded in whole blocks of this many (burst_simulation)

    def _dist(self):
        try:
            import torch.distributed as dist
            if dist.is_available() and dist.is_initialized():
                return dist
        except ImportError:
            pass
        return None

    def _counters(self, point, frames, point_index):
        """The reduced counters of `frames` frames of one point, sharded over the ranks."""
        dist = self._dist()
        rank, world = (dist.get_rank(), dist.get_world_size()) if dist else (0, 1)
        I = self.interleave
        first, count = shard_blocks(-(-frames // I) * I, rank, world, I)
        # every point draws from its own stretch of the global frame sequence, from a block boundary on
        base = (point_index << 40) // I * I
        counters = self.backend.run(point, self.seed, base + first, count)
        if dist:
            dist.all_reduce(counters, op=dist.ReduceOp.SUM)  # the path's only exchange step
        c = counters.cpu().numpy() if hasattr(counters, "cpu") else np.asarray(counters)
        res = {k: int(c[i]) for k, i in self.counter_names.items()}
        res["iter_hist"] = [int(v) for v in c[capi.MC_ITER_HIST:]]
        return res

    def _agree(self, ok, seed):
        """Rank 0's decision (log file opened or not) and its seed, made known to every rank BEFORE the first
        collective of the ladder: a rank that raised alone would leave the others blocked in the all-reduce."""
        dist = self._dist()
        if dist is None:
            return ok, seed
        import torch
        device = getattr(self.backend, "device", None)
        if device is None or dist.get_backend() != "nccl":
            device = "cpu"
        # the seed travels as two 31-bit halves + sign-free high part: int64 holds any 64-bit seed bit pattern
        t = torch.tensor([int(ok), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=torch.int64, device=device)
        dist.broadcast(t, src=0)
        v = t.cpu().tolist()
        return bool(v[0]), int(v[1]) | (int(v[2]) << 32)

    def _ladder(self, log_name, column, row_value, header_note="", row_note=None):
        """Every point of self.points() with the adaptive sample count; rank 0 writes the reference-format log
        `log_name` whose first column, headed `column`, shows row_value(point); header_note is appended to the header
        line and row_note(res), where given, to the line of a point."""
        dist = self._dist()
        rank = dist.get_rank() if dist else 0
        log, error = None, None
        if self.log_dir is not None and rank == 0:
            path = os.path.join(self.log_dir, log_name)
            try:
                if os.path.exists(path):
                    raise RuntimeError("File %s already exists." % path)  # simulation.c++:72-81
                log = open(path, "w")
                log.write("%7s %21s%s\n" % (column, "wer", header_note))
            except (OSError, RuntimeError) as e:
                error = e
        ok, self.seed = self._agree(error is None, self.seed)
        if not ok:  # every rank leaves together
            raise error if error is not None else RuntimeError("rank 0 could not open the log file")
        wer, results = 0.5, []
        for idx, point in enumerate(self.points()):
            n = samples(wer) if self.samples_per_point is None else int(self.samples_per_point)
            if self.max_samples:
                n = min(n, self.max_samples)
            res = self.run_point(point, n, idx)
            results.append(res)
            wer = res["wer"]
            if log:
                log.write("%7s %s%s\n" % ("%.6g" % row_value(point), "%16.15e" % res["wer"], row_note(res) if row_note else ""))
                log.flush()
        if log:
            log.close()
        return results


class _EbnoLadder(_ShardedSimulation):
    """What the three Eb/N0 ladders share: step, seed, backend, log directory and the caps, the points from
    ladder(code.rate) (simulation.c++:105-107) unless start / stop say otherwise, and the counters of a point."""

    def __init__(self, code, backend, step, seed, log_dir, max_samples, start, stop, samples_per_point):
        self.code = code
        self.step = float(step)
        self.seed = int(seed)
        self.backend = backend
        self.log_dir = log_dir
        self.max_samples = max_samples
        self.samples_per_point = samples_per_point  # fixed frame count per point instead of the adaptive rule
        ref_start, _ = ladder(code.rate, self.step)
        self.start = ref_start if start is None else float(start)
        self.stop = (max(8.0, self.start) + self.step / 2) if stop is None else float(stop)

    def points(self):
        e, out = self.start, []
        while e < self.stop:
            out.append(e)
            e += self.step
        return out

    def run_point(self, ebno_db, frames, point_index=0):
        """Decode `frames` frames of one Eb/N0 point, sharded over the ranks; returns the reduced counters."""
        res = self._counters(ebno_db, frames, point_index)
        res["ebno"] = ebno_db
        res["wer"] = res["word_errors"] / max(1, res["frames"])
        res["ber"] = res["bit_errors"] / max(1, res["frames"] * self.code.n)
        return res


class awgn_simulation(_EbnoLadder):
    """awgn_simulation(decoder, step = 0.5, seed = 0) -- simulation.h:71-83."""

    def __init__(self, code, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None,
                 max_samples=None, start=None, stop=None, samples_per_point=None, chase=None, gmd=None, osd=None):
        # chase=p: every frame goes through Chase-II (ChaseBackend); the log name carries -chaseP
        self.chase = None if chase is None else int(chase)
        # gmd=m (RS): every frame goes through GMD with m trials (GmdBackend, True: all of them); the log name carries -gmdM
        if gmd is not None and chase is not None:
            raise TypeError("gmd= does not combine with chase=")
        # osd=order: every frame goes through ordered-statistics decoding (OsdBackend); the log name carries -osdO
        if osd is not None and (chase is not None or gmd is not None):
            raise TypeError("osd= does not combine with chase= or gmd=")
        self.osd = None if osd is None else int(osd)
        self.gmd = None if gmd is None else (int(code.t) + 1 if gmd is True else int(gmd))
        if backend is None:
            if gmd is not None:
                backend = GmdBackend(code, gmd, random_codewords)
            elif osd is not None:
                backend = OsdBackend(code, osd, random_codewords)
            else:
                backend = DeviceBackend(code, random_codewords) if chase is None else ChaseBackend(code, chase, random_codewords)
        super().__init__(code, backend, step, seed, log_dir, max_samples, start, stop, samples_per_point)

    def __call__(self):
        """awgn_simulation::operator()(): the whole ladder; rank 0 writes the reference-format log."""
        suffix = "" if self.chase is None else "-chase%d" % self.chase
        if self.gmd is not None:
            suffix = "-gmd%d" % self.gmd
        if self.osd is not None:
            suffix = "-osd%d" % self.osd
        return self._ladder(self.code.to_string() + suffix + ".log", "ebno", lambda ebno: ebno)


class product_simulation(_EbnoLadder):
    """The Eb/N0 ladder of a product code (codes.product_code) under the iterative decoder with the schedule alpha, beta
    (one entry each per half-iteration; there is no default) at p Chase positions.  Frames are blocks: sharded by block,
    wer is the block error rate, ber counts the n values of a block.  The ladder starts from ladder(pc.rate); the log
    is <pc.to_string()>-chaseP-hH.log with H = len(alpha)."""

    def __init__(self, pc, p, alpha, beta, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None,
                 max_samples=None, start=None, stop=None, samples_per_point=None):
        self.p, self.halves = int(p), len(alpha)
        if not self.halves or len(alpha) != len(beta):
            raise ValueError("one alpha and one beta per half-iteration, at least one")
        if backend is None:
            backend = ProductBackend(pc, p, alpha, beta, random_codewords)
        super().__init__(pc, backend, step, seed, log_dir, max_samples, start, stop, samples_per_point)

    def __call__(self):
        name = "%s-chase%d-h%d.log" % (self.code.to_string(), self.p, self.halves)
        return self._ladder(name, "ebno", lambda ebno: ebno)


class product_hard_simulation(_EbnoLadder):
    """The Eb/N0 ladder of a product code under `halves` half-iterations of hard-decision row / column decoding
    (cc_mc_run_product_hard_dev): the ladder and the sharding by block of product_simulation.  The log is
    <pc.to_string()>-hard-h<halves>.log; next to wer it shows the mean of `last`, the half-iterations a block took to
    its final state (CC_MC_ITER_SUM over the blocks)."""

    def __init__(self, pc, halves, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None,
                 max_samples=None, start=None, stop=None, samples_per_point=None):
        self.halves = int(halves)
        if self.halves < 1:
            raise ValueError("halves >= 1")
        if backend is None:
            backend = ProductHardBackend(pc, self.halves, random_codewords)
        super().__init__(pc, backend, step, seed, log_dir, max_samples, start, stop, samples_per_point)

    def run_point(self, ebno_db, frames, point_index=0):
        res = super().run_point(ebno_db, frames, point_index)
        res["mean_last"] = res["iter_sum"] / max(1, res["frames"])
        return res

    def __call__(self):
        name = "%s-hard-h%d.log" % (self.code.to_string(), self.halves)
        return self._ladder(name, "ebno", lambda ebno: ebno, " %12s" % "mean_last", lambda res: " %12.6f" % res["mean_last"])


class product_anchor_simulation(product_hard_simulation):
    """The Eb/N0 ladder of a product code under `halves` half-iterations of anchor decoding at `delta`
    (cc_mc_run_product_anchor_dev; there is no default for delta): ladder, sharding by block and the mean_last column of
    product_hard_simulation.  The log is <pc.to_string()>-anchor<delta>-h<halves>.log."""

    def __init__(self, pc, delta, halves, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None,
                 max_samples=None, start=None, stop=None, samples_per_point=None):
        from .codes import _anchor_delta
        self.delta = _anchor_delta(delta)
        if int(halves) < 1:
            raise ValueError("halves >= 1")
        if backend is None:
            backend = ProductAnchorBackend(pc, self.delta, halves, random_codewords)
        super().__init__(pc, halves, step, seed, random_codewords, backend, log_dir, max_samples, start, stop, samples_per_point)

    def __call__(self):
        name = "%s-anchor%d-h%d.log" % (self.code.to_string(), self.delta, self.halves)
        return self._ladder(name, "ebno", lambda ebno: ebno, " %12s" % "mean_last", lambda res: " %12.6f" % res["mean_last"])


class product_sr_simulation(product_hard_simulation):
    """The Eb/N0 ladder of a product code under iBDD with scaled reliability (cc_mc_run_product_sr_dev), one weight per
    half-iteration: ladder, sharding by block and the mean_last column of product_hard_simulation.  The log is
    <pc.to_string()>-sr<halves>.log."""

    def __init__(self, pc, weights, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None,
                 max_samples=None, start=None, stop=None, samples_per_point=None):
        self.weights = [float(w) for w in weights]
        if not self.weights:
            raise ValueError("one weight per half-iteration, at least one")
        if backend is None:
            backend = ProductSrBackend(pc, self.weights, random_codewords)
        super().__init__(pc, len(self.weights), step, seed, random_codewords, backend, log_dir, max_samples, start, stop,
                         samples_per_point)

    def __call__(self):
        name = "%s-sr%d.log" % (self.code.to_string(), self.halves)
        return self._ladder(name, "ebno", lambda ebno: ebno, " %12s" % "mean_last", lambda res: " %12.6f" % res["mean_last"])


class staircase_simulation(_EbnoLadder):
    """The Eb/N0 ladder of a staircase code (codes.staircase_code) under its sliding-window decoder
    (cc_mc_run_staircase_dev).  Frames are streams: sharded by stream, wer is the rate of streams that are wrong in a
    counted block or did not converge, and ber is taken over the counted blocks 1 .. L_c alone (L_c = blocks - window + 1,
    or blocks for a stream shorter than the window) -- the figure that does not depend on the stream length.  The log is
    <sc.to_string()>.log."""

    def __init__(self, sc, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None, max_samples=None,
                 start=None, stop=None, samples_per_point=None):
        self.counted_blocks = sc.blocks - sc.window + 1 if sc.blocks >= sc.window else sc.blocks
        if backend is None:
            backend = StaircaseBackend(sc, random_codewords)
        super().__init__(sc, backend, step, seed, log_dir, max_samples, start, stop, samples_per_point)

    def run_point(self, ebno_db, frames, point_index=0):
        res = super().run_point(ebno_db, frames, point_index)
        res["ber"] = res["bit_errors"] / max(1, res["frames"] * self.counted_blocks * self.code.m * self.code.m)
        return res

    def __call__(self):
        return self._ladder(self.code.to_string() + ".log", "ebno", lambda ebno: ebno)


class staircase_sr_simulation(staircase_simulation):
    """The Eb/N0 ladder of a staircase code under its sliding-window decoder with scaled reliability
    (cc_mc_run_staircase_sr_dev), one weight per half-pass of a window position: ladder, sharding by stream, wer and the
    ber over the counted blocks of staircase_simulation.  The log is <sc.to_string()>-sr.log."""

    def __init__(self, sc, weights, step=0.5, seed=0, random_codewords=False, backend=None, log_dir=None, max_samples=None,
                 start=None, stop=None, samples_per_point=None):
        self.weights = [float(w) for w in weights]
        if len(self.weights) != 2 * sc.iters:
            raise ValueError("one weight per half-pass of a window position: 2 * iters = %d" % (2 * sc.iters))
        if backend is None:
            backend = StaircaseSrBackend(sc, self.weights, random_codewords)
        super().__init__(sc, step, seed, random_codewords, backend, log_dir, max_samples, start, stop, samples_per_point)

    def __call__(self):
        return self._ladder(self.code.to_string() + "-sr.log", "ebno", lambda ebno: ebno)


# ---- discrete memoryless channels (cc_mc_run_discrete_dev): the BSC and BEC the reference's README leaves as a TODO --
CHANNELS = ("bsc", "bec", "bsec")
DISCRETE_COUNTER_NAMES = dict(COUNTER_NAMES, channel_erasures=capi.MC_CHANNEL_ERASURES)


def discrete_ladder():
    """The default points: 10^(-k/4) for k = 4 .. 16, from 0.1 down to 1e-4 (noisiest first)."""
    return [10.0 ** (-k / 4.0) for k in range(4, 17)]


def channel_probabilities(channel, point):
    """(p_error, p_erasure) of one point: p for bsc, the erasure probability for bec, a (p, erasure) pair for bsec;
    ValueError unless both are finite, >= 0 and sum to <= 1 (the device's own check, made before any collective)."""
    if channel == "bsc":
        p, e = float(point), 0.0
    elif channel == "bec":
        p, e = 0.0, float(point)
    elif channel == "bsec":
        p, e = (float(v) for v in point)
    else:
        raise ValueError("unknown channel %r (one of %s)" % (channel, ", ".join(CHANNELS)))
    if not (math.isfinite(p) and math.isfinite(e) and p >= 0.0 and e >= 0.0 and p + e <= 1.0):
        raise ValueError("bad channel point %r: probabilities must be finite, >= 0 and sum to <= 1" % (point,))
    return p, e


class DiscreteBackend:
    """Counts one shard of one channel point on this rank's GPU through cc_mc_run_discrete_dev."""

    def __init__(self, code, channel="bsc", random_codewords=False):
        import torch
        self.torch = torch
        self.code = code
        self.channel = channel
        self.random_codewords = bool(random_codewords)
        self.device = torch.device("cuda", torch.cuda.current_device())

    def run(self, point, seed, first_frame, frames):
        torch = self.torch
        p_error, p_erasure = channel_probabilities(self.channel, point)
        counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = capi.lib().cc_mc_run_discrete_dev(self.code._h, p_error, p_erasure, int(seed), int(first_frame),
                                               int(frames), int(self.random_codewords),
                                               C.c_void_p(counters.data_ptr()), stream)
        capi.check(rc, "cc_mc_run_discrete_dev")
        return counters  # stays on the device: reduced with RCCL


class PackedBscBackend:
    """Counts one shard of one BSC point on this rank's GPU through cc_mc_run_bsc_packed_dev: the packed word is the only
    container, so binary BCH codes of every q = 3 .. 15 run, the long ones (q > 8) included."""

    def __init__(self, code, random_codewords=False):
        import torch
        self.torch = torch
        self.code = code
        self.random_codewords = bool(random_codewords)
        self.device = torch.device("cuda", torch.cuda.current_device())

    def run(self, point, seed, first_frame, frames):
        torch = self.torch
        p_error, _ = channel_probabilities("bsc", point)
        counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = capi.lib().cc_mc_run_bsc_packed_dev(self.code._h, p_error, int(seed), int(first_frame), int(frames),
                                                 int(self.random_codewords), C.c_void_p(counters.data_ptr()), stream)
        capi.check(rc, "cc_mc_run_bsc_packed_dev")
        return counters  # stays on the device: reduced with RCCL


def hard_decision_p(code, ebno_db):
    """The crossover probability a hard-decision decoder sees behind BPSK over AWGN at this Eb/N0:
    p = 1/2 erfc(1 / (sigma sqrt 2)) = Q(1 / sigma) with sigma = code.sigma(ebno_db) (cc_sigma, the sigma of
    awgn_simulation) -- the point of discrete_simulation(channel="bsc") for a user who thinks in Eb/N0."""
    return 0.5 * math.erfc(1.0 / (code.sigma(ebno_db) * math.sqrt(2.0)))


class discrete_simulation(_ShardedSimulation):
    """Word-error rate over a ladder of discrete-channel points, sharded like awgn_simulation.

    channel "bsc": points are error probabilities p; "bec": erasure probabilities; "bsec": (p, erasure) pairs.  For RS
    codes the same points give the q-ary symmetric and the symbol erasure channel.  Default points: discrete_ladder()
    (for bsec the pairs (x, x)).  Rank 0 writes "<to_string()>.<channel>.log", its first column the point's p (the
    erasure probability for bec).

    Random codewords by default, unlike awgn_simulation: an erased position receives 0, which for the all-zero word is
    the symbol sent, so a decoder that reads erased positions as they are (RS BM / Euklid, BCH BM / Euklid, min-sum)
    would see a codeword in every frame without errors, whatever the number of erasures.

    packed=True (channel "bsc" only, binary BCH codes with a hard-decision tag): the same ladder through
    cc_mc_run_bsc_packed_dev (PackedBscBackend), whose only container is the packed word -- the route of the long codes,
    q = 9 .. 15, and for q <= 8 the same channel and counters at an eighth of the bytes.  Log name and sharding as ever."""

    counter_names = DISCRETE_COUNTER_NAMES

    def __init__(self, code, channel="bsc", points=None, seed=0, random_codewords=True, backend=None, log_dir=None,
                 max_samples=None, samples_per_point=None, packed=False):
        self.channel = str(channel).lower()
        if self.channel not in CHANNELS:
            raise ValueError("unknown channel %r (one of %s)" % (channel, ", ".join(CHANNELS)))
        self.packed = bool(packed)
        if self.packed and self.channel != "bsc":
            raise ValueError("packed=True runs the BSC only: channel %r has erasures, which packed words cannot carry"
                             % channel)
        if points is None:
            points = discrete_ladder()
            if self.channel == "bsec":
                points = [(x, x) for x in points]
        self._points = [tuple(pt) if self.channel == "bsec" else float(pt) for pt in points]
        for pt in self._points:
            channel_probabilities(self.channel, pt)
        self.code = code
        self.seed = int(seed)
        if backend is None:
            backend = PackedBscBackend(code, random_codewords) if self.packed else \
                DiscreteBackend(code, self.channel, random_codewords)
        self.backend = backend
        self.log_dir = log_dir
        self.max_samples = max_samples
        self.samples_per_point = samples_per_point

    def points(self):
        return list(self._points)

    def run_point(self, point, frames, point_index=0):
        """Decode `frames` frames of one channel point, sharded over the ranks; returns the reduced counters."""
        res = self._counters(point, frames, point_index)
        res["p_error"], res["p_erasure"] = channel_probabilities(self.channel, point)
        res["wer"] = res["word_errors"] / max(1, res["frames"])
        res["ber"] = res["bit_errors"] / max(1, res["frames"] * self.code.n)  # wrong symbols per symbol for RS
        return res

    def __call__(self):
        row = (lambda pt: pt[0]) if self.channel == "bsec" else (lambda pt: pt)
        return self._ladder("%s.%s.log" % (self.code.to_string(), self.channel), "p", row)


# ---- the Gilbert-Elliott burst channel along interleaved blocks (cc_mc_run_burst_dev) ----
class BurstBackend:
    """Counts one shard of one burst-channel point on this rank's GPU through cc_mc_run_burst_dev; a point is the symbol
    error probability of the bad state.  With a burst detector (p_detect or p_false_alarm not 0) through
    cc_mc_run_burst_erasure_dev: the flagged symbols are erasures to the decoder."""

    def __init__(self, code, interleave=1, p_gb=0.0, p_bg=1.0, p_error_good=0.0, random_codewords=False, *,
                 p_detect=0.0, p_false_alarm=0.0):
        import torch
        self.torch = torch
        self.code = code
        self.interleave, self.p_gb, self.p_bg, self.p_error_good = int(interleave), p_gb, p_bg, p_error_good
        self.p_detect, self.p_false_alarm = p_detect, p_false_alarm
        self.random_codewords = bool(random_codewords)
        self.device = torch.device("cuda", torch.cuda.current_device())

    def run(self, point, seed, first_frame, frames):
        torch = self.torch
        ch = capi.BurstChannel(self.interleave, self.p_gb, self.p_bg, self.p_error_good, point)
        counters = torch.zeros(capi.MC_NCOUNTERS, dtype=torch.int64, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        if self.p_detect == 0.0 and self.p_false_alarm == 0.0:
            rc = capi.lib().cc_mc_run_burst_dev(self.code._h, C.byref(ch), int(seed), int(first_frame), int(frames),
                                                int(self.random_codewords), C.c_void_p(counters.data_ptr()), stream)
            capi.check(rc, "cc_mc_run_burst_dev")
        else:
            det = capi.BurstDetector(self.p_detect, self.p_false_alarm)
            rc = capi.lib().cc_mc_run_burst_erasure_dev(self.code._h, C.byref(ch), C.byref(det), int(seed),
                                                        int(first_frame), int(frames), int(self.random_codewords),
                                                        C.c_void_p(counters.data_ptr()), stream)
            capi.check(rc, "cc_mc_run_burst_erasure_dev")
        return counters  # stays on the device: reduced with RCCL


def _probability(value, what):
    p = float(value)
    if not (math.isfinite(p) and 0.0 <= p <= 1.0):
        raise ValueError("bad %s %r: a probability must be finite and in [0, 1]" % (what, value))
    return p


class burst_simulation(_ShardedSimulation):
    """Word-error rate over the two-state Gilbert-Elliott channel run along symbol-interleaved blocks of depth
    `interleave` -- what an interleaver of that depth buys on a channel with memory.  p_gb / p_bg: the transition
    probabilities good -> bad / bad -> good per transmitted symbol; a point is p_error_bad, the symbol error probability
    in the bad state (default points: discrete_ladder()), p_error_good that of the good state.  The frames of a point are
    rounded up to whole blocks and the ranks' shards cut at blocks.  Rank 0 writes "<to_string()>.burst.log".
    p_detect / p_false_alarm: a burst detector that flags a symbol with these probabilities in the bad / good state; the
    flagged symbols are erasures to the decoder (cc_mc_run_burst_erasure_dev) and the log's header line names the
    detector.  Both 0 (the default): no detector, errors-only decoding, the log as it always was."""

    counter_names = DISCRETE_COUNTER_NAMES

    def __init__(self, code, interleave=1, p_gb=0.01, p_bg=0.1, p_error_good=0.0, p_error_bad=None, points=None, seed=0,
                 random_codewords=True, backend=None, log_dir=None, max_samples=None, samples_per_point=None, *,
                 p_detect=0.0, p_false_alarm=0.0):
        self.p_detect = _probability(p_detect, "p_detect")
        self.p_false_alarm = _probability(p_false_alarm, "p_false_alarm")
        self.interleave = int(interleave)
        if not 1 <= self.interleave <= 256:
            raise ValueError("the interleaving depth is 1 .. 256")
        self.p_gb, self.p_bg = _probability(p_gb, "p_gb"), _probability(p_bg, "p_bg")
        self.p_error_good = _probability(p_error_good, "p_error_good")
        if self.p_gb + self.p_bg == 0.0:
            raise ValueError("p_gb + p_bg must be > 0")
        if points is None:
            points = discrete_ladder() if p_error_bad is None else [p_error_bad]
        self._points = [_probability(pt, "point") for pt in points]
        self.code = code
        self.seed = int(seed)
        self.backend = backend if backend is not None else BurstBackend(
            code, self.interleave, self.p_gb, self.p_bg, self.p_error_good, random_codewords,
            p_detect=self.p_detect, p_false_alarm=self.p_false_alarm)
        self.log_dir = log_dir
        self.max_samples = max_samples
        self.samples_per_point = samples_per_point

    def points(self):
        return list(self._points)

    def run_point(self, point, frames, point_index=0):
        """Decode `frames` frames (rounded up to whole blocks) of one point, sharded over the ranks."""
        res = self._counters(point, frames, point_index)
        res["p_error_bad"], res["interleave"] = point, self.interleave
        if self.p_detect or self.p_false_alarm:
            res["p_detect"], res["p_false_alarm"] = self.p_detect, self.p_false_alarm
        res["wer"] = res["word_errors"] / max(1, res["frames"])
        res["ber"] = res["bit_errors"] / max(1, res["frames"] * self.code.n)  # wrong symbols per symbol for RS
        return res

    def __call__(self):
        note = ""
        if self.p_detect or self.p_false_alarm:
            note = "  detector p_detect=%.6g p_false_alarm=%.6g" % (self.p_detect, self.p_false_alarm)
        return self._ladder("%s.burst.log" % self.code.to_string(), "p", lambda pt: pt, note)


class bitflip_simulation:
    """bitflip_simulation(decoder, errors) -- simulation.h:85-92, simulation.c++:152-213.

    Exhaustive word-error rate by number of flipped bits: for every weight w <= errors and every one of the
    C(n, w) flip patterns the all-zero word is sent as +1 / -1 (x = -2*bit + 1, :190-191), decoded, and
    counted as a word error when the result is non-zero or the decoder fails (:193-199).  The reference
    walks the patterns with std::next_permutation one frame at a time; here all patterns of a weight are
    decoded as one batch on the GPU.
    """

    def __init__(self, code, errors=0, log_dir=None, batch=1 << 18):
        self.code, self.errors, self.log_dir, self.batch = code, int(errors), log_dir, int(batch)

    def patterns(self, w):
        """All C(n, w) flip patterns as rows of positions, in chunks of at most `batch` rows."""
        import itertools
        n = self.code.n
        if w == 0:
            yield np.zeros((1, 0), np.int64)
            return
        it = itertools.combinations(range(n), w)
        while True:
            chunk = np.fromiter(itertools.chain.from_iterable(itertools.islice(it, self.batch)), np.int64)
            if chunk.size == 0:
                return
            yield chunk.reshape(-1, w)

    def run_weight(self, w):
        import torch
        n = self.code.n
        patterns = word_errors = 0
        for pos in self.patterns(w):
            x = torch.ones((pos.shape[0], n), dtype=torch.float32, device="cuda")
            if w:
                x.scatter_(1, torch.from_numpy(pos).cuda(), -1.0)
            res = self.code.correct_batch(x)
            bad = (res["status"] != 0) | (res["out"] != 0).any(dim=1)
            patterns += pos.shape[0]
            word_errors += int(bad.sum())
        return patterns, word_errors

    def __call__(self):
        log = None
        if self.log_dir is not None:
            path = os.path.join(self.log_dir, self.code.to_string() + ".log")
            if os.path.exists(path):
                raise RuntimeError("File %s already exists." % path)
            log = open(path, "w")
            log.write("%7s %21s\n" % ("errors", "wer"))
        out = []
        for w in range(self.errors + 1):
            patterns, word_errors = self.run_weight(w)
            out.append(dict(errors=w, patterns=patterns, word_errors=word_errors, wer=word_errors / patterns))
            if log:
                log.write("%7s %s\n" % ("%.6g" % w, "%16.15e" % (word_errors / patterns)))
        if log:
            log.close()
        return out
