#!/usr/bin/env python3
"""Milliseconds per step of the headline's kernels from a rocprofv3 --kernel-trace --stats run of bench.py (the first line of
tools/profile_bench.sh): the d = 8 screen, the pruned d = 8 sweep, the window pass and the sum of the rest.  A step is one call of the sweep.
    tools/kernel_ms.py <kernel_stats.csv> [label]"""
import csv
import sys

ROWS = (("screen", "kde_screen_d8_kernel"), ("screen (serial)", "kde_screen_d8_serial_kernel"), ("screen (dense)", "kde_screen_d8_dense_kernel"),
        ("screen far", "kde_screen_d8_far_kernel"), ("screen far (ser)", "kde_screen_d8_serial_far_kernel"), ("screen far (dns)", "kde_screen_d8_dense_far_kernel"),
        ("sweep", "kde_sweep_pruned_d8_kernel"), ("far pass", "kde_sweep_far32_d8_kernel"), ("window", "query_window_kernel"))
tot = {k: [0.0, 0] for k, _ in ROWS}
rest, names = 0.0, []
with open(sys.argv[1], newline="") as f:
    for row in csv.DictReader(f):
        name, calls, ns = row["Name"], int(row["Calls"]), float(row["TotalDurationNs"])
        base = name.split("(")[0].split("<")[0].split("::")[-1].strip()
        for k, kern in ROWS:
            if base == kern:
                tot[k][0] += ns
                tot[k][1] += calls
                break
        else:
            rest += ns
            names.append((ns, calls, name[:90]))
steps = tot["sweep"][1]
if not steps:
    sys.exit("no call of kde_sweep_pruned_d8_kernel in " + sys.argv[1])
label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
print(f"{label}: {steps} steps (calls of the sweep)")
for k, _ in ROWS:
    if tot[k][1]:
        print(f"  {k:16s} {tot[k][0] / steps * 1e-6:8.3f} ms/step  ({tot[k][1]} calls)")
print(f"  {'rest':16s} {rest / steps * 1e-6:8.3f} ms/step, the largest:")
for ns, calls, name in sorted(names, reverse=True)[:6]:
    print(f"    {ns / steps * 1e-6:8.3f} ms/step  {calls:5d} calls  {name}")
print(f"  {'all kernels':16s} {(rest + sum(v[0] for v in tot.values())) / steps * 1e-6:8.3f} ms/step")
