"""Instruction streams of chase_kernel in two device assemblies of csrc/chase.hip, one from before and one from after the
template gained its bool argument (profiles/r19_chase_extended_object.txt):

    hipcc <the Makefile's flags> --cuda-device-only -S chase.hip -o before.s     (and after.s)
    python profiles/tools/chase_object_diff.py before.s after.s

Per kernel: the lines between its label and its end label without comments, section and kernel-descriptor directives,
the function index inside local labels (.LBB<k>_) dropped, since the kernels come in another order.  No GPU needed."""
import re, subprocess, hashlib, sys, difflib
def kernels(path):
    out, name, body = {}, None, []
    for l in open(path).read().splitlines():
        m = re.match(r'^(_ZN\S+):', l)
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
    return out
def key(n):
    d = subprocess.run(['c++filt', n], capture_output=True, text=True).stdout.strip()
    a = re.search(r'chase_kernel<([^>]*)>', d).group(1).replace('ccamd::(anonymous namespace)::', '')
    return a
P = {key(n): b for n, b in kernels(sys.argv[1]).items()}
N = {key(n): b for n, b in kernels(sys.argv[2]).items()}
sha = lambda b: hashlib.sha256('\n'.join(b).encode()).hexdigest()[:16]
for k, b in P.items():
    k2 = k.replace('3', '3, false', 1) if k.startswith('3') else k.replace('0', '0, false', 1)
    d = [l for l in difflib.unified_diff(b, N[k2], lineterm='', n=0) if l[:1] in '+-' and l[:3] not in ('+++', '---')]
    print('chase_kernel<%s> -> <%s>: %d / %d instruction lines, sha256 %s / %s, %d differing lines' % (k, k2, len(b), len(N[k2]), sha(b), sha(N[k2]), len(d)))
    for l in d[:10]: print('   ', l)
for k, b in N.items():
    if 'true' in k: print('chase_kernel<%s>: %d instruction lines' % (k, len(b)))
