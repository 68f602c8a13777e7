"""Instruction streams of the kernels in two device assemblies of one unit, before and after a change that should leave
the code as it is (profiles/r27_ibdd_block_frame.txt), the way chase_object_diff.py compared chase.hip:

    hipcc <the Makefile's flags> --cuda-device-only -S csrc/product_hard.hip -o before.s     (and after.s)
    python profiles/tools/kernel_stream_diff.py before.s after.s [N]

Per kernel, matched by its demangled name (c++filt must be on the PATH): the lines between its label and its end label
without comments, section and kernel-descriptor directives, the function index inside local labels (.LBB<k>_) dropped;
the count of differing lines and the first N of them (default 10).  No GPU needed."""
import difflib
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for l in open(path).read().splitlines():
        m = re.match(r'^(_Z\S+):', l)
        if m:
            name, body = m.group(1), []
            continue
        if name and re.match(r'^\.Lfunc_end\d+:', l):
            out[name] = body
            name = None
            continue
        if name is not None:
            s = re.sub(r'\s*;.*$', '', l).strip()
            if s and not s.startswith('.amdhsa') and not re.match(r'^\.(p2align|section|type|size|globl|protected|text)', s):
                body.append(re.sub(r'\.LBB\d+_', '.LBB_', s))
    names = subprocess.run(['c++filt'], input='\n'.join(out), capture_output=True, text=True).stdout.split('\n')
    short = lambda d: re.sub(r'\(.*$', '', d.replace('void ', '').replace('ccamd::(anonymous namespace)::', ''))
    return {short(d): b for d, b in zip(names, out.values())}


if __name__ == '__main__':
    P, N = kernels(sys.argv[1]), kernels(sys.argv[2])
    sha = lambda b: hashlib.sha256('\n'.join(b).encode()).hexdigest()[:16]
    for k in sorted(set(P) | set(N)):
        if k not in P or k not in N:
            print('%s: only %s' % (k, 'before' if k in P else 'after'))
            continue
        d = [l for l in difflib.unified_diff(P[k], N[k], lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
        print('%s: %d / %d instruction lines, sha256 %s / %s, %d differing lines'
              % (k, len(P[k]), len(N[k]), sha(P[k]), sha(N[k]), len(d)))
        for l in d[:int(sys.argv[3]) if len(sys.argv) > 3 else 10]:
            print('   ', l)
