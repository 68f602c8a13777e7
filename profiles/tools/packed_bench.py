"""Packed-bit hard decoding against the byte call, 2^22 frames resident on the device, random codewords
with 0 .. 3 bit errors per frame (uniform), the same frames for every leg:

    (a) cc_correct_hard_batch_dev          one byte per bit
    (b) cc_correct_hard_packed_batch_dev   native route (packed_syndrome_kernel / packed_fix_kernel)
    (c) the same call with CC_AMD_PACKED_NATIVE=0: unpack, byte chain, pack -- in a process of its own, since the
        switch is read once

for BCH(255,231), BCH(255,139) and shortened BCH(200,176), Berlekamp-Massey tag; three timed runs per leg after a warm-up
call of the same size, (a) and (b) alternating within one process, timed with device events.  The native route is held
against (c): the slowest (b) run must be faster than the fastest (c) run.  Encode and extract of BCH(255,231): the
byte calls against the packed ones, in this process (native) and in the child (generic route).

    python profiles/tools/packed_bench.py                 everything (spawns the process of leg (c) itself)
    python profiles/tools/packed_bench.py --only bch231 --legs b   one leg of one code (for a rocprofv3 run of its own;
                                                          with CC_AMD_PACKED_NATIVE=0 in the environment that is leg (c))
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
CODES = {"bch231": (3, None), "bch139": (15, None), "bch200": (3, 200)}


def timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)  # ms


def workload(code, frames):
    """received words (frames, n) uint8 on the device: random codewords, 0 .. 3 flipped bits each"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(6)
    msg = torch.randint(0, 2, (frames, code.l), dtype=torch.uint8, device="cuda", generator=g)
    rx = code.encode_batch(msg)
    ne = torch.randint(0, 4, (frames,), device="cuda", generator=g)
    rows = torch.arange(frames, device="cuda")
    for e in range(3):  # (two flips of one frame may meet: then they cancel, still a word within the capability)
        pos = torch.randint(0, code.n, (frames,), device="cuda", generator=g)
        hit = ne > e
        rx[rows[hit], pos[hit]] ^= 1
    return msg, rx


def run_code(name, legs, frames, enc_in_child=False):
    import torch
    import channelcoding_amd as cc
    from channelcoding_amd import capi
    t, n = CODES[name]
    code = cc.primitive_bch(8, cc.errors(t), cc.berlekamp_massey_tag(), n=n)
    lib = capi.lib()
    msg, rx = workload(code, frames)
    pk = cc.pack_bits(rx)
    out, pout = torch.empty_like(rx), torch.empty_like(pk)
    nerr = torch.empty(frames, dtype=torch.int32, device="cuda")
    st = torch.empty(frames, dtype=torch.int32, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731

    def byte_call():
        capi.check(lib.cc_correct_hard_batch_dev(code._h, p(rx), None, None, p(out), p(nerr), p(st), frames, None), "byte")

    def packed_call():
        capi.check(lib.cc_correct_hard_packed_batch_dev(code._h, p(pk), None, None, p(pout), p(nerr), p(st), frames, None),
                   "packed")

    res = {"code": code.to_string(), "frames": frames, "route": code.packed_route(frames)}
    calls = [(leg, byte_call if leg == "a" else packed_call) for leg in legs]
    for _, fn in calls:  # warm-up of the same size
        fn()
    torch.cuda.synchronize()
    for leg, _ in calls:
        res[leg] = []
    for _ in range(3):  # alternating
        for leg, fn in calls:
            res[leg].append(timed(fn))
    if "a" in legs and len(legs) > 1:  # the two calls agree (every frame)
        byte_call()
        a_st, a_ne = st.clone(), nerr.clone()
        packed_call()
        assert torch.equal(a_st, st) and torch.equal(a_ne, nerr) and torch.equal(cc.unpack_bits(pout, code.n), out)
    res["failed"] = int((st != 0).sum())
    if name == "bch231" and (len(legs) > 1 or enc_in_child):  # encode / extract: byte against packed
        pm = cc.pack_bits(msg)
        cw, pcw = torch.empty_like(rx), torch.empty_like(pk)
        m2, pm2 = torch.empty_like(msg), torch.empty_like(pm)
        enc = {"enc_byte": lambda: capi.check(lib.cc_encode_batch_dev(code._h, p(msg), p(cw), frames, None), "enc"),
               "enc_packed": lambda: capi.check(lib.cc_encode_packed_batch_dev(code._h, p(pm), p(pcw), frames, None), "encp"),
               "ext_byte": lambda: capi.check(lib.cc_extract_batch_dev(code._h, p(rx), p(m2), frames, None), "ext"),
               "ext_packed": lambda: capi.check(lib.cc_extract_packed_batch_dev(code._h, p(pk), p(pm2), frames, None), "extp")}
        for fn in enc.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(cc.unpack_bits(pcw, code.n), cw) and torch.equal(cc.unpack_bits(pm2, code.l), m2)
        res["map_route"] = [code.packed_map_route(0), code.packed_map_route(1)]
        for k in enc:
            res[k] = []
        for _ in range(3):
            for k, fn in enc.items():
                res[k].append(timed(fn))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--legs", default=None, help="a, b, ab (this process as it is); default: a + b here, c in a child")
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--maps", action="store_true", help="with --legs b: time encode / extract too (the child of leg (c))")
    a = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    names = [a.only] if a.only else list(CODES)
    if a.legs:  # one process, as told
        for name in names:
            r = run_code(name, list(a.legs), a.frames, a.maps)
            print(json.dumps(r) if a.json else r, flush=True)
        return
    ok = True
    for name in names:
        r = run_code(name, ["a", "b"], a.frames)
        torch.cuda.empty_cache()
        env = dict(os.environ, CC_AMD_PACKED_NATIVE="0")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--legs", "b", "--json", "--maps", "--frames",
                                str(a.frames)], env=env, capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            print(child.stdout[-2000:], child.stderr[-2000:])
            raise SystemExit("leg (c) failed")
        c = json.loads(child.stdout.strip().splitlines()[-1])
        assert r["route"] == 1 and c["route"] == 0, (r["route"], c["route"])
        f = r["frames"]
        rate = lambda ms: f / ms / 1e3  # noqa: E731  M frames/s
        print("%s, %d frames, %d failed" % (r["code"], f, r["failed"]))
        for leg, what, v in (("a", "byte call", r["a"]), ("b", "packed native", r["b"]), ("c", "packed generic", c["b"])):
            print("  (%s) %-15s ms %s   M frames/s %s" % (leg, what, " ".join("%7.3f" % x for x in v),
                                                         " ".join("%7.0f" % rate(x) for x in v)))
        win = max(r["b"]) < min(c["b"])
        ok = ok and win
        print("  slowest (b) %.3f ms %s fastest (c) %.3f ms: native route %s; best (b) / best (a) = %.2f"
              % (max(r["b"]), "<" if win else ">=", min(c["b"]), "WINS" if win else "DOES NOT WIN", min(r["a"]) / min(r["b"])))
        if "enc_byte" in r:
            assert r["map_route"] == [1, 1] and c["map_route"] == [0, 0]
            for key, what in (("enc", "encode"), ("ext", "extract")):
                for label, v in (("byte call", r[key + "_byte"]), ("packed native", r[key + "_packed"]),
                                 ("packed generic", c[key + "_packed"])):
                    print("  %-7s %-15s ms %s   M frames/s %s" % (what, label, " ".join("%7.3f" % x for x in v),
                                                                 " ".join("%7.0f" % rate(x) for x in v)))
        sys.stdout.flush()
    print("(b) vs (c) condition: %s" % ("met for every code" if ok else "NOT met"))


if __name__ == "__main__":
    main()
