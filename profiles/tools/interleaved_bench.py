"""Symbol-interleaved hard decoding and encoding against the plain calls, 2^22 frames resident on the
device, random codewords with 0 .. t symbol errors per frame (uniform), Berlekamp-Massey tag, the same frames for every
leg; RS(255,239) mu = 0 at depth 16 (an OTU row) and RS(255,223) at depth 5 (CCSDS):

    (a) cc_correct_hard_batch_dev on frame-major words                      the ceiling
    (b) cc_correct_hard_interleaved_batch_dev, native route
    (c) the same call with CC_AMD_INTERLEAVED_NATIVE=0 (de-interleave, plain chain, interleave) -- in a process of its
        own, since the switch is read once
    (d) what a caller does without the feature: torch transpose(1, 2).contiguous() of the blocks, the plain call, the
        transpose back                                                       the baseline

Three timed runs per leg after a warm-up call of the same size, the legs alternating within one process, timed with
device events; slowest - fastest reported.  The native route is held against (d): the slowest (b) run must be faster
than the fastest (d) run.  Encode of RS(255,239) gets the same four legs.

    python profiles/tools/interleaved_bench.py                    everything (spawns the process of leg (c) itself)
    python profiles/tools/interleaved_bench.py --only rs239 --legs b   one leg of one code (for a rocprofv3 run of its own)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES = 1 << 22
CODES = {"rs239": (8, 0, 16), "rs223": (16, 1, 5)}  # t, mu, depth


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def workload(code, frames):
    """messages and received words (frames, n) uint8 on the device: random codewords, 0 .. t symbol errors each"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(8)
    msg = torch.randint(0, 256, (frames, code.l), dtype=torch.uint8, device="cuda", generator=g)
    rx = code.encode_batch(msg)
    ne = torch.randint(0, code.t + 1, (frames,), device="cuda", generator=g)
    rows = torch.arange(frames, device="cuda")
    for e in range(code.t):  # (two errors of one frame may meet: still a word within the capability)
        pos = torch.randint(0, code.n, (frames,), device="cuda", generator=g)
        val = torch.randint(1, 256, (frames,), dtype=torch.uint8, device="cuda", generator=g)
        hit = ne > e
        rx[rows[hit], pos[hit]] ^= val[hit]
    return msg, rx


def run_code(name, legs, frames):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    t, mu, I = CODES[name]
    frames -= frames % I
    code = cc.rs(8, cc.errors(t), cc.berlekamp_massey_tag(), mu=mu)
    lib = capi.lib()
    msg, rx = workload(code, frames)
    to_blocks = lambda x: x.view(frames // I, I, x.shape[1]).transpose(1, 2).contiguous()  # noqa: E731
    from_blocks = lambda y: y.transpose(1, 2).contiguous().view(frames, y.shape[1])  # noqa: E731
    rxi, msgi = to_blocks(rx), to_blocks(msg)
    out, outi = torch.empty_like(rx), torch.empty_like(rxi)
    cw, cwi = torch.empty_like(rx), torch.empty_like(rxi)
    nerr = torch.empty(frames, dtype=torch.int32, device="cuda")
    st = torch.empty(frames, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    keep = {}

    def plain(src=None):
        src = rx if src is None else src
        capi.check(lib.cc_correct_hard_batch_dev(code._h, p(src), None, None, p(out), p(nerr), p(st), frames, None), "plain")

    def interleaved():
        capi.check(lib.cc_correct_hard_interleaved_batch_dev(code._h, p(rxi), None, None, p(outi), p(nerr), p(st), frames, I,
                                                             None), "interleaved")

    def caller():
        plain(from_blocks(rxi))
        keep["d"] = to_blocks(out)

    def enc_plain(src=None):
        capi.check(lib.cc_encode_batch_dev(code._h, p(msg if src is None else src), p(cw), frames, None), "encode")

    def enc_interleaved():
        capi.check(lib.cc_encode_interleaved_batch_dev(code._h, p(msgi), p(cwi), frames, I, None), "encode interleaved")

    def enc_caller():
        enc_plain(from_blocks(msgi))
        keep["ed"] = to_blocks(cw)

    res = {"code": code.to_string(), "frames": frames, "depth": I}
    res["route"] = code.interleaved_route(frames, I)
    res["map_route"] = code.interleaved_map_route(0, I)
    table = {"a": plain, "b": interleaved, "d": caller}
    if name == "rs239":
        table.update({"enc_a": enc_plain, "enc_b": enc_interleaved, "enc_d": enc_caller})
    calls = [(k, fn) for k, fn in table.items() if k[-1] in legs]
    for _, fn in calls:  # warm-up of the same size
        fn()
    torch.cuda.synchronize()
    for k, _ in calls:
        res[k] = []
    for _ in range(3):  # alternating
        for k, fn in calls:
            res[k].append(timed(fn))
    if "a" in legs and "b" in legs:  # the calls agree (every frame)
        plain()
        a_st, a_ne = st.clone(), nerr.clone()
        interleaved()
        assert torch.equal(a_st, st) and torch.equal(a_ne, nerr) and torch.equal(from_blocks(outi), out)
        if "enc_b" in table:
            enc_plain()
            enc_interleaved()
            assert torch.equal(from_blocks(cwi), cw)
    res["failed"] = int((st != 0).sum())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--legs", default=None, help="some of a, b, d (this process as it is); default: a, b, d here, c in a child")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    names = [a.only] if a.only else list(CODES)
    if a.legs:  # one process, as told
        for name in names:
            r = run_code(name, list(a.legs), a.frames)
            print(json.dumps(r) if a.json else r, flush=True)
        return
    ok = True
    for name in names:
        r = run_code(name, ["a", "b", "d"], a.frames)
        torch.cuda.empty_cache()
        env = dict(os.environ, CC_AMD_INTERLEAVED_NATIVE="0")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--legs", "b", "--json", "--frames",
                                str(a.frames)], env=env, capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            print(child.stdout[-2000:], child.stderr[-2000:])
            raise SystemExit("leg (c) failed")
        c = json.loads(child.stdout.strip().splitlines()[-1])
        assert r["route"] == 1 and c["route"] == 0, (r["route"], c["route"])
        f = r["frames"]
        rate = lambda ms: f / ms / 1e3  # noqa: E731  M frames/s
        print("%s, depth %d, %d frames, %d failed" % (r["code"], r["depth"], f, r["failed"]))
        for pre, what in (("", "decode"), ("enc_", "encode")):
            if pre + "a" not in r:
                continue
            rows = (("a", "plain call", r[pre + "a"]), ("b", "interleaved native", r[pre + "b"]),
                    ("c", "interleaved generic", c[pre + "b"]), ("d", "transpose + plain + transpose", r[pre + "d"]))
            for leg, label, v in rows:
                print("  %s (%s) %-30s ms %s   M frames/s %s" % (what, leg, label, " ".join("%8.3f" % x for x in v),
                                                               " ".join("%6.0f" % rate(x) for x in v)))
            b, d, top = r[pre + "b"], r[pre + "d"], r[pre + "a"]
            win = max(b) < min(d)
            ok = ok and win
            print("  %s: slowest (b) %.3f ms %s fastest (d) %.3f ms: native route %s; best (d) / best (b) = %.2f; best (a) / best "
                  "(b) = %.2f; spread of (d) %.3f ms" % (what, max(b), "<" if win else ">=", min(d), "WINS" if win else "DOES NOT WIN",
                                                         min(d) / min(b), min(top) / min(b), max(d) - min(d)))
        sys.stdout.flush()
    print("(b) vs (d) condition: %s" % ("met for every workload" if ok else "NOT met"))


if __name__ == "__main__":
    main()
