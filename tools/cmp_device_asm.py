#!/usr/bin/env python3
"""Are two builds of one translation unit the same device program?  `python tools/cmp_device_asm.py A.s B.s`, the two files from
`hipcc <flags of coper_amd/build.py> --cuda-device-only -S csrc/X.hip`.  Splits each at its kernels (the function's text and its
.amdhsa_kernel descriptor), drops what depends on the order of the kernels in the file (local label numbers, comments), pairs
kernels whose mangled name changed with a moved namespace by their k_* name, and prints one hash per file and what differs."""
import hashlib
import re
import sys


def pieces(path):
    s = open(path).read()
    syms = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', s, re.M)
    out = {}
    for sym in syms:
        a = s.index('\t.type\t%s,@function' % sym)
        b = s.index('.end_amdhsa_kernel', s.index('.amdhsa_kernel %s' % sym))
        t = s[a:b]
        t = re.sub(r'\.LBB\d+_', '.LBB_', t)
        t = re.sub(r'\.Lfunc_(begin|end)\d+', r'.Lfunc_\1', t)
        t = re.sub(r'\.L__unnamed_\d+|\.Ltmp\d+', '.Lx', t)
        t = re.sub(r'[ \t]*;.*$', '', t, flags=re.M)      # comments: block numbers, padding behind a label
        out[sym] = t
    return out
A, B = pieces(sys.argv[1]), pieces(sys.argv[2])
onlyA, onlyB = sorted(set(A) - set(B)), sorted(set(B) - set(A))
print("kernels:", len(A), len(B), "only parent:", onlyA, "only branch:", onlyB)
ren = {}
for a in onlyA:
    key = re.search(r'k_[a-z0-9_]+', a).group(0)
    for b in onlyB:
        if key in b: ren[a] = b
bad = 0
for a in sorted(A):
    b = ren.get(a, a)
    if b not in B: print("MISSING", a); bad += 1; continue
    ta = A[a].replace(a, 'SYM'); tb = B[b].replace(b, 'SYM')
    if ta != tb: print("DIFFERS", a); bad += 1
def H(P, ren={}):
    h = hashlib.sha256()
    inv = {v: k for k, v in ren.items()}
    for sym in sorted(P, key=lambda x: inv.get(x, x)):
        h.update(P[sym].replace(sym, 'SYM').encode())
    return h.hexdigest()
print("sha256 parent", H(A)); print("sha256 branch", H(B, ren)); print("differences:", bad)
