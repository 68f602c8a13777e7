#!/usr/bin/env python3
"""Instruction mix of a kernel's hottest loop from hipcc -S output.

    hipcc ... --cuda-device-only -S file.hip -o file.s
    python profiles/tools/isa_mix.py file.s <mangled-name-substring> [--all] [--lds]

Finds the function whose label contains the substring, takes its longest basic-block run that ends in a backward
branch (the min-sum iteration body is one straight-line block of 24 unrolled rows) -- or the whole function with
--all -- and prints the count per issue class measured in profiles/r02_ubench_valu_issue_classes.txt:
  valu_full  : v_add/sub/mul/fma/fmac_f32 (any encoding without DPP/SDWA), v_and/or/xor_b32, v_add/sub_u32, v_mov_b32
  valu_half  : every other VALU instruction (min/max/med3, shifts, bfi, DPP, SDWA, compares, conversions ...)
  lds, salu, vmem, waitcnt, nop
With --lds it also prints the block's LDS request-to-wait strip and its summary (lds_strip below).
"""
import json
import re
import sys

FULL = re.compile(r"^v_(add|sub|subrev|mul|fma|fmac|mul_legacy)_f32(_e32|_e64)?$|^v_(and|or|xor)_b32(_e32|_e64)?$|"
                  r"^v_(add|sub|subrev)_u32(_e32|_e64)?$|^v_mov_b32(_e32|_e64)?$")


def classify(op):
    if op.startswith("v_"):
        return "valu_full" if FULL.match(op) else "valu_half"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_nop"):
        return "nop"
    if op.startswith("s_"):
        return "salu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    return "other"


def blocks(lines):
    cur_label, cur = None, []
    for ln in lines:
        t = ln.strip()
        if not t or t.startswith((";", ".")) and not t.startswith(".LBB"):
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            yield cur_label, cur
            cur_label, cur = m.group(1), []
            continue
        if t.startswith(";;#"):
            continue
        op = t.split()[0]
        if re.match(r"^[a-z_0-9]+$", op):
            cur.append((op, t))
    yield cur_label, cur


def lgkmcnt_of(text):
    """The lgkmcnt of an s_waitcnt line, or None when it does not wait on that counter."""
    m = re.search(r"lgkmcnt\((\d+)\)", text)
    return int(m.group(1)) if m else None


def lds_strip(ins):
    """LDS request-to-wait distances of a straight-line block, ins = [(opcode, line), ...].

    Returns (strip, summary).  The strip is a list of tokens in program order: a run of LDS instructions as
    'ds_read_b64 x5' (runs of different opcodes joined by ' + '), an s_waitcnt by its operands ('lgkmcnt(0)'), 's_nop',
    and the NUMBER of other instructions between two of those as a decimal string.  LDS operations of a wavefront
    return in order, so s_waitcnt lgkmcnt(N) covers every LDS instruction except the N issued last before it; the
    distance of a read group (a run of LDS instructions with a ds_read in it) is the number of other instructions --
    neither LDS nor s_waitcnt nor s_nop -- between its last instruction and the first wait that covers it.  Groups that
    no wait of the block covers (their wait sits behind the backward branch) are left out of the summary."""
    strip, other = [], 0
    groups = []   # [index of the group's last LDS instruction, it holds a read, other instructions before it]
    waits = []    # (LDS instructions before it, other instructions before it, lgkmcnt)
    n_lds = n_other = 0
    run = []      # opcodes of the LDS run in hand

    def close_run():
        if run:
            parts, k = [], 0
            while k < len(run):
                j = k
                while j < len(run) and run[j] == run[k]:
                    j += 1
                parts.append("%s x%d" % (run[k], j - k))
                k = j
            strip.append(" + ".join(parts))
            groups.append((n_lds, any(op.startswith("ds_read") for op in run), n_other))
            del run[:]

    def close_other():
        nonlocal other
        if other:
            strip.append(str(other))
            other = 0

    for op, text in ins:
        if op.startswith("ds_"):
            close_other()
            run.append(op)
            n_lds += 1
            continue
        close_run()
        if op.startswith("s_waitcnt"):
            close_other()
            strip.append(" ".join(text.split()[1:]))
            c = lgkmcnt_of(text)
            if c is not None:
                waits.append((n_lds, n_other, c))
        elif op.startswith("s_nop"):
            close_other()
            strip.append("s_nop")
        else:
            other += 1
            n_other += 1
    close_run()
    close_other()
    dist = []
    for last, has_read, at in groups:
        if not has_read:
            continue
        cover = next((w for w in waits if w[0] >= last and w[0] - last >= w[2]), None)
        if cover is not None:
            dist.append(cover[1] - at)
    dist.sort()
    summary = {
        "waits_on_lgkmcnt": len(waits),
        "waits_lgkmcnt_0": sum(1 for w in waits if w[2] == 0),
        "read_groups_covered": len(dist),
        "distance_min": dist[0] if dist else None,
        "distance_median": (dist[(len(dist) - 1) // 2] + dist[len(dist) // 2]) / 2 if dist else None,
    }
    return strip, summary


def main():
    path, key = sys.argv[1], sys.argv[2]
    whole = "--all" in sys.argv
    text = open(path).read().splitlines()
    start = next(i for i, l in enumerate(text) if re.match(r"^_Z\S*:", l) and key in l)
    # (the function's end marker, not its first s_endpgm: the kernel has an early exit right behind its prologue)
    end = next(i for i in range(start + 1, len(text)) if text[i].strip().startswith(".Lfunc_end"))
    body = text[start + 1:end + 1]
    bl = list(blocks(body))
    if whole:
        ins = [x for _, b in bl for x in b]
    else:
        ins = max((b for _, b in bl), key=len)
    mix = {}
    for op, t in ins:
        c = classify(op)
        if c == "valu_full" and (" row_" in t or "quad_perm" in t or "_dpp" in op or "_sdwa" in op):
            c = "valu_half"
        mix[c] = mix.get(c, 0) + 1
    mix["total"] = len(ins)
    mix["dpp"] = sum(1 for op, t in ins if "_dpp" in op or "quad_perm" in t or " row_" in t)
    print(json.dumps(mix, indent=1, sort_keys=True))
    if "--lds" in sys.argv:
        strip, summary = lds_strip(ins)
        print(" | ".join(strip))
        print(json.dumps(summary, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
