#!/usr/bin/env python3
"""Counts for what follows the iteration block of a diagonal min-sum kernel in hipcc -S output: the frame switch.

    hipcc ... --cuda-device-only -S minsum_diag_geo.hip -o geo.s
    python profiles/tools/isa_switch_path.py geo.s <mangled-name-substring>

Takes the function whose label contains the substring, finds its longest basic block (the row block and stop scan of
one iteration, see isa_mix.py) and counts the instructions between that block's end and the function's end: all of
them, LDS instructions by opcode, s_waitcnt that wait on lgkmcnt, s_*saveexec, v_mov_b32 and VMEM.  The stop scan's
tail and the group reduction of the stop test sit in that range too when the compiler splits them off the loop block;
the counts are for comparing two builds of the same instantiation.
"""
import json
import re
import sys

from isa_mix import blocks, lgkmcnt_of


def main():
    path, key = sys.argv[1], sys.argv[2]
    text = open(path).read().splitlines()
    start = next(i for i, l in enumerate(text) if re.match(r"^_Z\S*:", l) and key in l)
    end = next(i for i in range(start + 1, len(text)) if text[i].strip().startswith(".Lfunc_end"))
    bl = list(blocks(text[start + 1:end + 1]))
    at = max(range(len(bl)), key=lambda k: len(bl[k][1]))
    tail = [x for _, b in bl[at + 1:] for x in b]
    out = {"loop_block": len(bl[at][1]), "after": len(tail), "blocks_after": len(bl) - at - 1}
    out["valu"] = sum(1 for op, _ in tail if op.startswith("v_"))
    out["salu"] = sum(1 for op, _ in tail if op.startswith("s_") and not op.startswith(("s_waitcnt", "s_nop")))
    out["v_mov_b32"] = sum(1 for op, _ in tail if op.startswith("v_mov_b32"))
    out["vmem"] = sum(1 for op, _ in tail if op.startswith(("global_", "buffer_", "flat_")))
    out["saveexec"] = sum(1 for op, _ in tail if "saveexec" in op)
    out["waits_on_lgkmcnt"] = sum(1 for op, t in tail if op.startswith("s_waitcnt") and lgkmcnt_of(t) is not None)
    lds = {}
    for op, _ in tail:
        if op.startswith("ds_"):
            lds[op] = lds.get(op, 0) + 1
    out["lds"] = sum(lds.values())
    out["lds_by_opcode"] = lds
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
