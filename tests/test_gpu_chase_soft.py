"""GPU tests of the Chase-Pyndiah soft output: cc_correct_chase_soft_batch(_dev) bit for bit against
tests/chase_soft_model.py on ext (compared as u32) and on out, nerr, status and metric; the four outputs against
cc_correct_chase_batch_dev; a wavefront's second group of frames; absent outputs, guard elements and odd offsets; the
host-pointer against the device entry point; and cc.product_decode on device tensors against the model's loop."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import channelcoding_amd as cc
from channelcoding_amd import capi
import chase_model as M
import chase_soft_model as S
from checkers import awgn_llr
from test_chase_soft_host import ALPHA, BETA, P, PRODUCTS, product_batch

pytestmark = pytest.mark.gpu

# (q, t, N, Eb/N0 found with the model on the CPU so that the batch below is not degenerate)
CASES = [(4, 2, None, 3.0),    # BCH(15,7): the register variant of the root search, t = 2
         (4, 3, None, 2.0),    # BCH(15,5): t = 3
         (5, 5, None, 2.0),    # BCH(31,11): the LDS variant, t = 5
         (6, 3, None, 4.0),    # BCH(63,45)
         (7, 3, None, 4.0),    # BCH(127,106)
         (8, 3, None, 5.0),    # BCH(255,231): four position chunks, F bounded by LDS at p <= 3
         (8, 8, None, 4.0),    # BCH(255,191): t = 8, two syndrome reductions
         (4, 1, None, 3.0),    # BCH(15,11), a Hamming code
         (7, 3, 64, 4.0), (8, 3, 65, 4.0), (8, 3, 129, 4.5), (8, 3, 193, 5.0),  # shortened, next to a multiple of 64
         (3, 1, 5, 3.0), (3, 1, 6, 3.0)]  # p = n
IDS = ["bch%d-t%d%s" % (q, t, "" if N is None else "-N%d" % N) for q, t, N, _ in CASES]
PS = (0, 1, 3, 6)
BETAS = (0.5, 0.0)


def perfect(case):
    """a full-length t = 1 code is a Hamming code: no frame is without a candidate"""
    return case[1] == 1 and case[2] is None


def make(q, t, N=None):
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **({} if N is None else {"n": N}))


def frames_per_wave(code, p):
    """F of launch_chase_soft, asked of the library: 64 >> p, fewer where LDS bounds it"""
    F = capi.lib().cc_chase_frames_per_wavefront(code._h, p, 1)
    assert 1 <= F <= 64 >> p
    return F


def quantised(rng, shape):
    """values in {+-0.5, +-1, +-1.5} with a few +-0.0: equal keys in every frame, equal metrics in many"""
    y = rng.choice(np.array([-1.5, -1.0, -0.5, 0.5, 0.5, 1.0, 1.0, 1.5, 1.5, 1.5], np.float32), shape)
    y[::3, 1] = np.float32(0.0)
    y[::4, shape[1] - 1] = np.float32(-0.0)
    y[1::5, 0] = np.float32(-0.0)
    return y.astype(np.float32)


def between_two_codewords(rng, dec, count):
    """BCH(255,191) only.  1 + x^15 + .. + x^240 = (x^255 - 1) / (x^15 - 1) vanishes at every alpha^i with 17 not
    dividing i, the roots alpha^1 .. alpha^16 and their conjugates among them: a codeword w of weight 17 = d_min, and so
    is every cyclic shift.  A frame lies between a codeword c and c + w: of the 17 positions of w eight carry c + w's
    sign, six carry c's sign with the smallest magnitudes of the frame (L_0 .. L_5) and three carry c's sign a little
    larger.  Pattern 0 is eight positions from c; every other pattern is 9 - f <= 8 from c + w (f flips): two different
    candidates from p = 1 on, which differ at all 17 positions.  Even frames make c + w the nearer one, odd frames c."""
    assert (dec.n, dec.t) == (255, 8)
    c = dec.encode(rng.integers(0, 2, (count, dec.l)).astype(np.uint8))
    y = ((1.0 - 2.0 * c.astype(np.float32)) * rng.uniform(0.6, 1.4, c.shape)).astype(np.float32)
    for f in range(count):
        D = rng.permutation((15 * np.arange(17) + int(rng.integers(0, 15))) % 255)
        sign = np.sign(y[f, D]).astype(np.float32)
        wrong, weak, rest = (0.35, 0.05, 0.2) if f % 2 == 0 else (0.12, 0.05, 0.5)
        y[f, D[:8]] = -sign[:8] * rng.uniform(wrong, wrong + 0.05, 8).astype(np.float32)
        y[f, D[8:14]] = sign[8:14] * rng.uniform(weak, weak + 0.04, 6).astype(np.float32)
        y[f, D[14:]] = sign[14:] * rng.uniform(rest, rest + 0.05, 3).astype(np.float32)
    return y


@functools.lru_cache(maxsize=None)
def batches(q, t, N, ebno):
    """300 frames of one code -- AWGN, quantised, -2 dB; for BCH(255,191) forty of the AWGN frames give way to frames
    between two codewords -- and the model's candidates for all 64 patterns, made once"""
    dec = M.decoder(q, t, N)
    rng = np.random.default_rng(2000 * q + 10 * t + (N or 0))
    sizes = (200, 50, 50)
    words = dec.encode(rng.integers(0, 2, (sizes[0] + sizes[2], dec.l)).astype(np.uint8))
    rate = dec.l / dec.n
    y = np.concatenate([awgn_llr(rng, words[: sizes[0]], rate, ebno), quantised(rng, (sizes[1], dec.n)),
                        awgn_llr(rng, words[sizes[0]:], rate, -2.0)])
    if (q, t, N) == (8, 8, None):
        y[3:163:4] = between_two_codewords(rng, dec, 40)  # spread over the groups of every F
    y = np.ascontiguousarray(y, np.float32)
    y.setflags(write=False)
    return dict(dec=dec, y=y, cand=M.candidates(dec, y))


def to_host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def same(got, want, rows, what, ext=True):
    got = to_host(got) if not isinstance(got["out"], np.ndarray) else got
    for k in ("out", "nerr", "status"):
        assert np.array_equal(got[k], want[k][:rows]), (what, k)
    assert np.array_equal(got["metric"].view(np.uint32), want["metric"][:rows].view(np.uint32)), (what, "metric")
    if ext:
        bad = np.argwhere(got["ext"].view(np.uint32) != want["ext"][:rows].view(np.uint32))
        assert bad.size == 0, (what, "ext", bad[:4].tolist())


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_model(case, p):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    n = bt["dec"].n
    p = min(p, n)  # a frame of five positions: p = 6 stands for p = n
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"].copy()).cuda()
    F, total = frames_per_wave(code, p), y.shape[0]
    for beta in BETAS:
        want = S.soft(bt["cand"], p, beta)
        for B in sorted({1, max(F - 1, 1), F + 1, total}):
            got = code.correct_batch(y[:B], chase=p, soft=beta)
            assert sorted(got) == ["ext", "metric", "nerr", "out", "status"] and got["ext"].dtype == torch.float32
            same(got, want, B, (case, p, beta, B))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_batches_are_not_degenerate(case):
    """what makes the comparison above worth something, asserted on the model alone, over the four values of p together:
    positions with a competitor and positions without one under decisions of either sign, frames without a candidate,
    frames whose winner is not pattern 0.  Per p they differ: p = 0 has one pattern and so no competitor anywhere, p = n
    has one at every position, and at p = 1 two different candidates are rare.
    Two codewords of BCH(255,191) are 17 or more positions apart and noise alone hardly ever puts a frame between two of
    them: its competitors come from the frames of between_two_codewords.  A Hamming code has no frame without a
    candidate."""
    bt = batches(*case)
    n = bt["dec"].n
    with_, without, lost, late = np.zeros(2, int), np.zeros(2, int), 0, 0
    for p in PS:
        r = S.soft(bt["cand"], min(p, n), 0.5)
        won = r["winner"] >= 0
        for bit in (0, 1):
            with_[bit] += (r["has"] & (r["out"] == bit)).sum()
            without[bit] += (~r["has"] & (r["out"] == bit) & won[:, None]).sum()
        lost += (~won).sum()
        late += (r["winner"] > 0).sum()
        assert not (r["has"] & ~won[:, None]).any() and (r["ext"][~won].view(np.uint32) == 0).all()
        if p == 0:
            assert not r["has"].any()
    assert (with_ >= 20).all(), with_
    assert (without >= 20).all() and late >= 5, (without, late)
    assert lost >= 5 or perfect(case), lost


# ---- the four outputs of cc_correct_chase_batch_dev ----
def scaled(y, kind):
    with np.errstate(over="ignore"):
        small = (y * np.float32(1e-42)).astype(np.float32)
        large = np.clip((y * np.float32(1e38)).astype(np.float32), np.float32(-3e38), np.float32(3e38)).astype(np.float32)
    if kind == "denormal":
        return small
    mixed = large.copy()  # the frames that share a wavefront lie eighty orders of magnitude apart
    mixed[::2] = small[::2]
    return mixed


@pytest.mark.parametrize("kind", ["plain", "denormal", "mixed"])
@pytest.mark.parametrize("case", [CASES[3], CASES[2], CASES[5]], ids=["bch6-t3", "bch5-t5", "bch8-t3"])
def test_same_four_outputs_as_the_hard_output_call(case, kind):
    """out, nerr, metric and status are those of cc_correct_chase_batch_dev; where every metric is finite (plain and
    denormal values) ext is the model's as well -- a kernel that flushed denormals could not pass"""
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    y_host = bt["y"] if kind == "plain" else scaled(bt["y"], kind)
    assert np.isfinite(y_host).all()
    if kind == "denormal":
        assert (np.abs(y_host) < np.finfo(np.float32).tiny).all() and (y_host != 0).mean() > 0.9
    code = make(q, t, N)
    y = torch.from_numpy(y_host.copy()).cuda()
    with np.errstate(over="ignore"):
        cand = bt["cand"] if kind == "plain" else M.candidates(bt["dec"], y_host)
    for p in (0, 2, 6):
        hard, soft = code.correct_batch(y, chase=p), code.correct_batch(y, chase=p, soft=0.5)
        for k in ("out", "nerr", "metric", "status"):
            assert torch.equal(hard[k].view(torch.uint8), soft[k].view(torch.uint8)), (kind, p, k)
        with np.errstate(over="ignore", invalid="ignore"):
            want = S.soft(cand, p, 0.5)
        same(soft, want, y.shape[0], (case, kind, p), ext=False)
        finite = np.isfinite(np.where(cand["ok"][:, : 1 << p], cand["M"][:, : 1 << p], 0)).all(axis=1)
        assert finite.all() if kind != "mixed" else (finite.any() and not finite.all())
        got = soft["ext"].cpu().numpy()
        assert np.array_equal(got[finite].view(np.uint32), want["ext"][finite].view(np.uint32)), (kind, p)
        if kind == "denormal" and p:
            assert (want["has"] & (want["ext"] != 0)).sum() > 100


# ---- a wavefront's second group of frames ----
SECOND = [(4, 2, 3.0, 6), (4, 2, 3.0, 3), (5, 5, 2.0, 2)]


def second_batch(q, t, ebno, p, W):
    """B frames for a grid of W wavefronts, the subset the model decodes, and the model's answer on it"""
    dec = M.decoder(q, t)
    n = dec.n
    F = 64 >> p
    B = 2 * W * F + 37 * F + 3
    rng = np.random.default_rng(7100 + 100 * q + p)
    words = dec.encode(rng.integers(0, 2, (1024, dec.l)).astype(np.uint8))
    y = awgn_llr(rng, words[rng.integers(0, 1024, B)], dec.l / n, ebno)
    y[W * F - 2 * F: W * F + 2 * F] = quantised(rng, (4 * F, n))
    low = np.arange(W * F + 5 * F, B, 11)  # frames at -2 dB among the later groups: some have no candidate
    y[low] = awgn_llr(rng, words[rng.integers(0, 1024, low.size)], dec.l / n, -2.0)
    y = np.ascontiguousarray(y, np.float32)
    pick = np.zeros(B, bool)
    pick[::397] = True
    pick[W * F - 2 * F: W * F + 4 * F] = True
    pick[2 * W * F - 2 * F: 2 * W * F + 4 * F] = True
    pick[B - 600:] = True
    idx = np.flatnonzero(pick)
    assert idx.size <= 3000
    want = S.chase_soft(dec, y[idx], p, 0.5)
    later = idx >= W * F  # without these the comparison beyond the first pass proves nothing
    assert (want["winner"][later] > 0).sum() >= 5 and want["has"][later].sum() >= 50
    assert (~want["has"][later][want["winner"][later] >= 0]).sum() >= 50
    return F, y, idx, want


@pytest.mark.parametrize("q,t,ebno,p", SECOND, ids=["bch%d-t%d-p%d" % (q, t, p) for q, t, _, p in SECOND])
def test_second_visit_of_a_wavefront(q, t, ebno, p):
    """more than twice the frames one pass of the grid takes, so that every wavefront meets a second and some a third
    group in the LDS region that the group before has left: its K and M_D among the rest"""
    import torch
    W = 32 * torch.cuda.get_device_properties(0).multi_processor_count  # the grid is capped at 8 workgroups of 4 per CU
    F, y, idx, want = second_batch(q, t, ebno, p, W)
    B = y.shape[0]
    code = make(q, t)
    assert frames_per_wave(code, p) == F  # LDS does not bound these codes: one pass takes exactly W F frames
    dev = torch.from_numpy(y).cuda()
    res = code.correct_batch(dev, chase=p, soft=0.5)
    got = to_host(res)
    same({k: v[idx] for k, v in got.items()}, want, idx.size, (q, t, p))

    # no state carries from group to group: the call on a prefix and the call on the rest give the same
    head = code.correct_batch(dev[: W * F], chase=p, soft=0.5)
    tail = code.correct_batch(dev[W * F:], chase=p, soft=0.5)
    for k in ("out", "ext", "nerr", "status", "metric"):
        assert torch.equal(torch.cat([head[k], tail[k]]).view(torch.uint8), res[k].view(torch.uint8)), k

    # every frame without a candidate: +0.0f throughout, whatever the group before it left in K
    lost = got["status"] == M.FRAME_LOCATOR
    assert set(np.unique(got["status"])) <= {M.FRAME_OK, M.FRAME_LOCATOR}
    # (BCH(15,7) at p = 6 has no frame without a candidate: see test_gpu_chase.py)
    assert lost[W * F:].sum() >= 1 or (q, t, p) == (4, 2, 6)
    assert (got["ext"][lost].view(np.uint32) == 0).all()
    assert np.isfinite(got["ext"]).all()
    hard = code.correct_batch(dev, chase=p)
    for k in ("out", "nerr", "status", "metric"):
        assert torch.equal(hard[k].view(torch.uint8), res[k].view(torch.uint8)), k


# ---- optional outputs, guard elements, buffers at odd addresses ----
GUARD, SENTINEL = 8, 0x5A


def guarded(torch, count, dtype):
    """count elements between two runs of GUARD elements, every byte SENTINEL"""
    size = torch.empty(0, dtype=dtype).element_size()
    whole = torch.full(((count + 2 * GUARD) * size,), SENTINEL, dtype=torch.uint8, device="cuda").view(dtype)
    return whole, whole[GUARD: GUARD + count]


def guards_intact(torch, whole):
    b = whole.view(torch.uint8)
    g = GUARD * whole.element_size()
    return bool((b[:g] == SENTINEL).all()) and bool((b[-g:] == SENTINEL).all())


def soft_dev(torch, code, llr, p, beta, out, ext, nerr, metric, status, B):
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    rc = capi.lib().cc_correct_chase_soft_batch_dev(code._h, ptr(llr), p, C.c_float(beta), ptr(out), ptr(ext), ptr(nerr),
                                                    ptr(metric), ptr(status), B, None)
    capi.check(rc, "cc_correct_chase_soft_batch_dev")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", [CASES[3], CASES[2]], ids=["bch6-t3", "bch5-t5"])
def test_optional_outputs_guards_and_offset_buffers(case):
    import torch
    q, t, N, _ = case
    bt = batches(*case)
    B, p, n = 200, 3, bt["dec"].n
    code = make(q, t, N)
    y = torch.from_numpy(bt["y"][:B].copy()).cuda()
    full = code.correct_batch(y, chase=p, soft=0.5)
    same(full, S.soft(bt["cand"], p, 0.5), B, (case, "full"))
    kinds = dict(nerr=torch.int32, metric=torch.float32, status=torch.int32)
    for mask in range(8):
        passed = [k for i, k in enumerate(kinds) if (mask >> i) & 1]
        bufs = {k: guarded(torch, B, kinds[k]) for k in passed}
        out_whole, out = guarded(torch, B * n, torch.uint8)
        ext_whole, ext = guarded(torch, B * n, torch.float32)
        args = {k: bufs[k][1] if k in bufs else None for k in kinds}  # an output not passed has no buffer at all
        soft_dev(torch, code, y, p, 0.5, out, ext, args["nerr"], args["metric"], args["status"], B)
        assert torch.equal(out.view(B, n), full["out"]) and guards_intact(torch, out_whole), (mask, "out")
        assert torch.equal(ext.view(B, n).view(torch.uint8), full["ext"].view(torch.uint8)), (mask, "ext")
        assert guards_intact(torch, ext_whole), (mask, "ext")
        for k in passed:
            assert torch.equal(bufs[k][1].view(torch.uint8), full[k].view(torch.uint8)), (mask, k)
            assert guards_intact(torch, bufs[k][0]), (mask, k)
    # llr and ext one float, out one byte into larger allocations (rows of an odd n are misaligned anyway)
    llr_big = torch.zeros(B * n + 1, dtype=torch.float32, device="cuda")
    llr_big[1:] = y.reshape(-1)
    ext_big = torch.full((B * n + 2,), 7.0, dtype=torch.float32, device="cuda")
    out_big = torch.full((B * n + 2,), SENTINEL, dtype=torch.uint8, device="cuda")
    llr, ext, out = llr_big[1:], ext_big[1: 1 + B * n], out_big[1: 1 + B * n]
    assert llr.data_ptr() % 8 == 4 and ext.data_ptr() % 8 == 4 and out.data_ptr() % 2 == 1
    nerr, status = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
    metric = torch.empty(B, dtype=torch.float32, device="cuda")
    soft_dev(torch, code, llr, p, 0.5, out, ext, nerr, metric, status, B)
    assert int(out_big[0]) == SENTINEL and int(out_big[-1]) == SENTINEL
    assert float(ext_big[0]) == 7.0 and float(ext_big[-1]) == 7.0
    got = dict(out=out.view(B, n), ext=ext.view(B, n), nerr=nerr, status=status, metric=metric)
    same(got, to_host(full), B, (case, "offset"))


def test_host_pointers_equal_device_pointers():
    """numpy (pageable and page-locked) against torch, with the staging chunk forced small in a process of its own (the
    value is read once): 200 frames of n = 255 in chunks of 39"""
    here = os.path.dirname(os.path.abspath(__file__))
    script = (
        "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import numpy as np, torch\n"
        "import channelcoding_amd as cc\n"
        "rng = np.random.default_rng(6)\n"
        "for q, t, N in ((8, 3, None), (6, 3, 50)):\n"
        "    code = cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), **({} if N is None else {'n': N}))\n"
        "    y = (1.0 + 0.6 * rng.standard_normal((200, code.n))).astype(np.float32)\n"
        "    pinned = torch.from_numpy(y).pin_memory().numpy()\n"
        "    for p, beta in ((0, 0.5), (4, 0.25), (6, 0.0)):\n"
        "        dev = {k: v.cpu().numpy() for k, v in code.correct_batch(torch.from_numpy(y.copy()).cuda(), chase=p, soft=beta).items()}\n"
        "        assert (dev['status'] == 0).any() and (dev['nerr'] > 0).any() and (dev['ext'] != 0).any()\n"
        "        for src in (y, pinned):\n"
        "            host = code.correct_batch(src, chase=p, soft=beta)\n"
        "            assert sorted(host) == ['ext', 'metric', 'nerr', 'out', 'status']\n"
        "            for k in host:\n"
        "                assert host[k].dtype == dev[k].dtype and host[k].shape == dev[k].shape, (p, k)\n"
        "                assert np.array_equal(host[k].view(np.uint8), dev[k].view(np.uint8)), (p, k)\n"
        "        dec = code.decode_batch(y, chase=p, soft=beta)\n"
        "        assert np.array_equal(dec['out'], dev['out']) and np.array_equal(dec['msg'], code.extract_batch(dev['out']))\n"
        "        assert np.array_equal(dec['ext'].view(np.uint32), dev['ext'].view(np.uint32))\n"
        "print('CHASE SOFT HOST OK')\n" % (here, os.path.dirname(here)))
    env = dict(os.environ, CC_AMD_HOST_CHUNK_BYTES="40000")
    out = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "CHASE SOFT HOST OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- product decoding ----
@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_product_decode_on_device_tensors_equals_the_model_loop(name):
    import torch
    rows, cols, sent, y = product_batch(name)
    blocks = 100
    y = np.ascontiguousarray(y[:blocks])
    (rq, rt), (cq, ct) = PRODUCTS[name][:2]
    r, c = make(rq, rt), make(cq, ct)
    steps = S.product_decode(rows, cols, y, P, ALPHA, BETA)
    dev = torch.from_numpy(y.copy()).cuda()
    for halves in (1, 2, 3, 4):
        got = cc.product_decode(r, c, dev, P, ALPHA[:halves], BETA[:halves])
        want = steps[halves - 1]
        assert sorted(got) == ["ext", "out", "status"] and got["out"].shape == (blocks, cols.n, rows.n)
        assert np.array_equal(got["out"].cpu().numpy(), want["out"]), (name, halves)
        assert np.array_equal(got["status"].cpu().numpy(), want["status"]), (name, halves)
        bad = np.argwhere(got["ext"].cpu().numpy().view(np.uint32) != want["ext"].view(np.uint32))
        assert bad.size == 0, (name, halves, bad[:4].tolist())
    # the numpy route through the host-pointer entry point is the same loop
    host = cc.product_decode(r, c, y, P, ALPHA, BETA)
    assert np.array_equal(host["out"], steps[-1]["out"])
    assert np.array_equal(host["ext"].view(np.uint32), steps[-1]["ext"].view(np.uint32))
    errors = [int((s["out"] != sent[:blocks]).any(axis=(1, 2)).sum()) for s in steps]
    assert errors[-1] < errors[0]  # and it does what it is for
