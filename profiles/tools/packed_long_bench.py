"""Packed hard decoding of the long binary BCH codes (q = 9 .. 15) against the 16-bit call, 2^16 frames
resident on the device, random codewords with 0 .. t bit errors per frame (uniform), Berlekamp-Massey tag, the same
frames for every leg:

    (a) cc_correct_hard_batch_u16_dev      one 16-bit word per bit
    (b) cc_correct_hard_packed_batch_dev   native route (packed_long_correct_kernel)
    (c) the same call with CC_AMD_PACKED_NATIVE=0: unpack, wide_correct_kernel, pack -- in a process of its own, since
        the switch is read once.  This is the code path every such call took before the native route existed.

Three timed runs per leg after a warm-up call of the same size, (a) and (b) alternating within one process, timed with
device events.  The rule of DESIGN 4.8: the native route is on for a class of codes only if the slowest (b) run is
faster than the fastest (c) run.

    python profiles/tools/packed_long_bench.py                    every code (spawns the process of leg (c) itself)
    python profiles/tools/packed_long_bench.py --sweep            the crossover: B = 256 .. 2^16 for two codes, native
                                                                  (CC_AMD_PACKED_LONG_MIN_FRAMES=1) and generic, a child each
    python profiles/tools/packed_long_bench.py --only dvbs2_full --legs b    one leg of one code (for a rocprofv3 run of
                                                                  its own; with CC_AMD_PACKED_NATIVE=0 that is leg (c))
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FRAMES = 1 << 16
# name: (q, t, N, modular polynomial)
CODES = {"dvbs2_full": (14, 12, None, 0x402B), "dvbs2_3240": (14, 12, 3240, 0x402B), "nand_4200": (13, 8, 4200, 0x201B),
         "bch1023": (10, 2, None, 0x409), "bch511": (9, 3, None, 0x211)}
SWEEP = ("dvbs2_3240", "bch1023")
SWEEP_SIZES = [1 << k for k in range(8, 17)]


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def make(name):
    import channelcoding_amd as cc
    q, t, N, poly = CODES[name]
    return cc.primitive_bch(q, cc.errors(t), cc.berlekamp_massey_tag(), n=N, modular_polynomial=poly)


def workload(code, frames):
    """received words (frames, n) int16 on the device: 1024 random codewords repeated, 0 .. t flipped bits each"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(6)
    distinct = min(frames, 1024)
    msg = torch.randint(0, 2, (distinct, code.l), dtype=torch.int16, device="cuda", generator=g)
    cw = code.encode_batch(msg)
    rx = cw.repeat((frames + distinct - 1) // distinct, 1)[:frames].contiguous()
    ne = torch.randint(0, code.t + 1, (frames,), device="cuda", generator=g)
    rows = torch.arange(frames, device="cuda")
    for e in range(code.t):  # (two flips of one frame may meet: then they cancel, still a word within the capability)
        pos = torch.randint(0, code.n, (frames,), device="cuda", generator=g)
        hit = ne > e
        rx[rows[hit], pos[hit]] ^= 1
    return rx


def run_code(name, legs, frames):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    code = make(name)
    lib = capi.lib()
    rx = workload(code, frames)
    pk = cc.pack_bits(rx)
    out, pout = torch.empty_like(rx), torch.empty_like(pk)
    nerr = torch.empty(frames, dtype=torch.int32, device="cuda")
    st = torch.empty(frames, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def u16_call():
        capi.check(lib.cc_correct_hard_batch_u16_dev(code._h, p(rx), None, None, p(out), p(nerr), p(st), frames, None), "u16")

    def packed_call():
        capi.check(lib.cc_correct_hard_packed_batch_dev(code._h, p(pk), None, None, p(pout), p(nerr), p(st), frames, None),
                   "packed")

    res = {"code": code.to_string(), "n": code.n, "frames": frames, "route": code.packed_route(frames)}
    calls = [(leg, u16_call if leg == "a" else packed_call) for leg in legs]
    for _, fn in calls:  # warm-up of the same size
        fn()
    torch.cuda.synchronize()
    for leg, _ in calls:
        res[leg] = []
    for _ in range(3):  # alternating
        for leg, fn in calls:
            res[leg].append(timed(fn))
    if "a" in legs and len(legs) > 1:  # the two calls agree (every frame)
        u16_call()
        a_st, a_ne = st.clone(), nerr.clone()
        packed_call()
        assert torch.equal(a_st, st) and torch.equal(a_ne, nerr)
        assert torch.equal(cc.unpack_bits(pout, code.n, torch.int16), out)
    res["failed"] = int((st != 0).sum())
    return res


def run_sweep(name):
    """the packed call of this process (native or generic by its environment) at every size of the sweep"""
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    code = make(name)
    lib = capi.lib()
    rx = workload(code, SWEEP_SIZES[-1])
    pk = cc.pack_bits(rx)
    pout = torch.empty_like(pk)
    nerr = torch.empty(len(pk), dtype=torch.int32, device="cuda")
    st = torch.empty(len(pk), dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    res = {"code": code.to_string(), "sizes": SWEEP_SIZES, "route": [], "us": []}
    for B in SWEEP_SIZES:
        fn = lambda: capi.check(lib.cc_correct_hard_packed_batch_dev(code._h, p(pk), None, None, p(pout), p(nerr), p(st), B,  # noqa: E731
                                                                     None), "packed")
        fn()
        torch.cuda.synchronize()
        res["route"].append(code.packed_route(B))
        res["us"].append(sorted(1e3 * timed(fn) for _ in range(3)))
    return res


def child(args, **env):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=1100)
    if out.returncode != 0:
        print(out.stdout[-2000:], out.stderr[-2000:])
        raise SystemExit("child failed: %s" % " ".join(args))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--legs", default=None, help="a, b, ab (this process as it is); default: a + b here, c in a child")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-here", default=None, help="(internal) the sweep of one code in this process")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    if a.sweep_here:
        print(json.dumps(run_sweep(a.sweep_here)), flush=True)
        return
    if a.sweep:
        for name in ([a.only] if a.only else SWEEP):
            nat = child(["--sweep-here", name], CC_AMD_PACKED_LONG_MIN_FRAMES="1")
            gen = child(["--sweep-here", name], CC_AMD_PACKED_NATIVE="0")
            assert set(nat["route"]) == {1} and set(gen["route"]) == {0}
            print("%s: packed call, us per call (fastest .. slowest of three)" % nat["code"])
            for B, x, y in zip(nat["sizes"], nat["us"], gen["us"]):
                print("  B = %6d   native %9.1f .. %9.1f   generic %9.1f .. %9.1f   %s"
                      % (B, x[0], x[-1], y[0], y[-1], "native wins" if x[-1] < y[0] else "native does not win"))
            sys.stdout.flush()
        return
    names = [a.only] if a.only else list(CODES)
    if a.legs:  # one process, as told
        for name in names:
            r = run_code(name, list(a.legs), a.frames)
            print(json.dumps(r) if a.json else r, flush=True)
        return
    ok = True
    for name in names:
        r = run_code(name, ["a", "b"], a.frames)
        torch.cuda.empty_cache()
        c = child(["--only", name, "--legs", "b", "--json", "--frames", str(a.frames)], CC_AMD_PACKED_NATIVE="0")
        assert r["route"] == 1 and c["route"] == 0, (r["route"], c["route"])
        f = r["frames"]
        rate = lambda ms: f / ms / 1e3  # noqa: E731  M frames/s
        print("%s, n = %d, %d frames, %d failed" % (r["code"], r["n"], f, r["failed"]))
        for leg, what, v in (("a", "16-bit call", r["a"]), ("b", "packed native", r["b"]), ("c", "packed generic", c["b"])):
            print("  (%s) %-15s ms %s   M frames/s %s" % (leg, what, " ".join("%8.3f" % x for x in v),
                                                         " ".join("%8.2f" % rate(x) for x in v)))
        win = max(r["b"]) < min(c["b"])
        ok = ok and win
        print("  slowest (b) %.3f ms %s fastest (c) %.3f ms: native route %s; best (c) / best (b) = %.1f, best (a) / best (b) = %.1f"
              % (max(r["b"]), "<" if win else ">=", min(c["b"]), "WINS" if win else "DOES NOT WIN", min(c["b"]) / min(r["b"]),
                 min(r["a"]) / min(r["b"])))
        sys.stdout.flush()
    print("(b) vs (c) condition: %s" % ("met for every code" if ok else "NOT met"))


if __name__ == "__main__":
    main()
