#!/usr/bin/env python3
"""Timeline of the headline's steps from a rocprofv3 --kernel-trace run of bench.py (tracing only, csv output).
A step is one call of kde_sweep_pruned_d8_kernel; its first kernel is the last-but-(N-k)th prune_keys_kernel, its screen pack and its
finish are found the same way (the fit's own calls of those kernels come first in the trace and are left out).  Per step:
  front   first query-side kernel's start -> screen pack's start (on one stream: the query side's length; with the front lanes: how
          long before its screen pack the step's query side began)
  gap     kde_finish_kernel's end -> the NEXT step's first kernel's start; negative = the next step began that long before the finish ended
and the kernels' milliseconds per step, by name.
    tools/step_timeline.py <kernel_trace.csv> [label]"""
import csv
import re
import sys
from collections import defaultdict


def base(name):
    head = name.split("(")[0].split("<")[0].split("::")[-1].split()
    return head[-1] if head else name[:60]


rows = []
with open(sys.argv[1], newline="") as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()


def calls(sub):   # (some names arrive mangled: match on the substring)
    return [(s, e) for s, e, n in rows if sub in n]


steps = len(calls("kde_sweep_pruned_d8_kernel"))
if not steps:
    sys.exit("no call of kde_sweep_pruned_d8_kernel in " + sys.argv[1])
label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
first = calls("prune_keys_kernel")[-steps:]
spack = calls("kde_screen_pack_kernel")[-steps:]
fin = calls("kde_finish_kernel")[-steps:]
print(f"{label}: {steps} steps (calls of the sweep)")
print("  step   front ms   gap to next ms   first kernel -> finish end ms")
for k in range(steps):
    front = (spack[k][0] - first[k][0]) * 1e-6
    gap = (first[k + 1][0] - fin[k][1]) * 1e-6 if k + 1 < steps else float("nan")
    print(f"  {k:4d}   {front:8.4f}   {gap:14.4f}   {(fin[k][1] - first[k][0]) * 1e-6:10.4f}")
if steps > 2:   # the first step follows the fit (or the warm-up's synchronisation): the steady state is the rest
    span = (fin[-1][1] - fin[0][1]) * 1e-6 / (steps - 1)
    print(f"  finish to finish, steps 1 .. {steps - 1}: {span:.4f} ms a step")
t0 = first[0][0]
tot = defaultdict(lambda: [0, 0])
for s, e, n in rows:
    if s >= t0:
        b = base(n)
        m = re.match(r"_ZN3pbn\d+([a-z0-9_]+?_kernel)", n)
        if m:
            b = m.group(1)
        if b == "trampoline_kernel":
            b = "rocprim (sort)"
        tot[b][0] += e - s
        tot[b][1] += 1
print("  kernel ms per step (from the first step's first kernel on):")
for b, (ns, count) in sorted(tot.items(), key=lambda kv: -kv[1][0]):
    print(f"    {ns / steps * 1e-6:9.4f}  {count:5d} calls  {b}")
print(f"    {sum(v[0] for v in tot.values()) / steps * 1e-6:9.4f}  all kernels")
