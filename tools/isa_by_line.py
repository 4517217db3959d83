#!/usr/bin/env python3
"""usage: tools/isa_by_line.py file.s function-substring source-file-substring [first-line last-line]  -- static instructions of one
kernel of a gfx950 listing made with `hipcc -S -gline-tables-only --cuda-device-only`, attributed to the source line of the innermost
inlined frame (the `.loc` in force), for the lines of one source file: vector / LDS / scalar per line, and their sums.  No GPU."""
import re
import sys
from collections import defaultdict

src, fn, want = sys.argv[1], sys.argv[2], sys.argv[3]
lo = int(sys.argv[4]) if len(sys.argv) > 4 else 0
hi = int(sys.argv[5]) if len(sys.argv) > 5 else 1 << 30
lines = open(src).read().split("\n")
files = {}
for l in lines:
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[int(m.group(1))] = m.group(3) or m.group(2)
start = next(i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_].*:", l) and fn in l and not l.startswith("."))
acc = defaultdict(lambda: [0, 0, 0])
cur = None
total = [0, 0, 0]
for l in lines[start + 1:]:
    if l.startswith("\t.end_amdhsa_kernel") or l.startswith(".Lfunc_end"):
        break
    t = l.strip().split()
    if not t or t[0].startswith(";"):
        continue
    if t[0] == ".loc":
        cur = (files.get(int(t[1]), "?"), int(t[2]))
        continue
    if t[0].startswith("."):
        continue
    cls = 0 if t[0].startswith("v_") else 1 if t[0].startswith("ds_") else 2 if t[0].startswith("s_") else None
    if cls is None:
        continue
    total[cls] += 1
    if cur and want in cur[0] and lo <= cur[1] <= hi:
        acc[cur[1]][cls] += 1
print("line     vector  lds  scalar")
for ln in sorted(acc):
    print("%5d   %6d %4d %6d" % (ln, *acc[ln]))
s = [sum(a[c] for a in acc.values()) for c in range(3)]
print("lines %d..%d of %s: vector %d, lds %d, scalar %d   (kernel: vector %d, lds %d, scalar %d)" % (lo, min(hi, 99999), want, *s, *total))
