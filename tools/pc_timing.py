"""Measurements behind DESIGN.md 3.10 (recorded, not pass / fail): writes one JSON object to profiles/r10/pc_timing.json.

  batch   tests per second of LinearCorrelation's batch function per conditioning-set size k = 0 ... K_DEV and batch size: the device
          kernel (threshold 0, upload + launch + download + host redo included) against the host-only handle's batch, which is a C loop
          over the scalar routine - no Python frame in either number.  The smallest measured size from which the device wins for EVERY
          k is the crossover that csrc/lincor.hpp carries as LINCOR_BATCH_MIN_TESTS.
  pc      wall time of PC().estimate(LinearCorrelation(df)) at 256 / 512 / 1 024 variables x 5 000 rows, default options, batched
          against batch_fn = NULL, with both test counters; the v-structure phase's share is the difference to a use_sepsets = True run
          (which evaluates no test in that phase).

Timing: one warm-up, then `--reps` repetitions; the median with the min and max, clocks untouched.  The 1 024-variable searches take
minutes on one host thread and run once each.  An existing output file is updated section by section.
`--only pc1024` runs that one search twice (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402


def timed(fn, reps, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}


def batch_section(reps):
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib
    from test_lincor_batch_gpu import batch, random_tests
    from test_pc_cpu import linear_gaussian_table

    df = linear_gaussian_table(256, 5000, 2, 2.0)
    dev = pbn.LinearCorrelation(df)
    dev.set_batch_threshold(0)
    host = pbn.LinearCorrelation.from_covariance(dev.variable_names(), dev.covariance(), len(df))
    k_dev = _lib.load().pbn_lincor_batch_max_cond()
    rng = np.random.default_rng(0)
    sizes = [100, 200, 500, 1000, 2000, 5000, 10000, 20000, 50000, 100000, 1000000]
    rows, wins = [], {}
    for k in range(k_dev + 1):
        for size in sizes:
            tests = random_tests(rng, 256, np.full(size, k))
            r = 3 if size >= 1000000 else reps
            d = timed(lambda: batch(dev._handle, *tests), r)
            h = timed(lambda: batch(host._handle, *tests), r)
            rows.append({"k": k, "tests": size, "device": d, "host": h, "device_tests_per_s": size / d["median_s"],
                         "host_tests_per_s": size / h["median_s"], "speedup": h["median_s"] / d["median_s"]})
            wins.setdefault(size, []).append(d["median_s"] < h["median_s"])
            print(f"k {k} tests {size}: device {size / d['median_s']:.3g}/s host {size / h['median_s']:.3g}/s x{h['median_s'] / d['median_s']:.2f}", flush=True)
    crossover = next((s for i, s in enumerate(sizes) if all(all(wins[t]) for t in sizes[i:])), None)
    return {"rows": rows, "crossover_all_k": crossover, "device_stats": dev.batch_stats()}


def pc_once(n, batched, use_sepsets=False):
    import pybnesian_amd as pbn
    from pybnesian_amd.constraint import pc_estimate_indices
    from test_pc_cpu import linear_gaussian_table

    df = linear_gaussian_table(n, 5000, 2, 2.0)
    test = pbn.LinearCorrelation(df)
    names = test.variable_names()
    return test, lambda: pc_estimate_indices(test, names, batched=None if batched else False, use_sepsets=use_sepsets)


def pc_section(reps, sizes, save):
    out = []
    for n in sizes:
        big = n >= 1024   # minutes per serial run: one repetition each, the first batched run as warm-up, no serial use_sepsets run
        r = 1 if big else reps
        test, run = pc_once(n, True)
        res = run()
        b = timed(run, r, warm=False)
        stats = test.batch_stats()
        print(f"{n}: batched {b['median_s']:.2f} s", flush=True)
        _, run_s = pc_once(n, False)
        s = timed(run_s, max(1, r // 2), warm=not big)
        print(f"{n}: serial {s['median_s']:.2f} s", flush=True)
        _, run_bs = pc_once(n, True, use_sepsets=True)
        res_bs = run_bs()
        bs = timed(run_bs, r, warm=False)
        ss = None
        if not big:
            _, run_ss = pc_once(n, False, use_sepsets=True)
            ss = timed(run_ss, max(1, r // 2))
        row = {"variables": n, "rows": 5000, "batched": b, "serial": s, "speedup": s["median_s"] / b["median_s"], "serial_tests": res["serial_tests"],
               "evaluated": res["evaluated"], "band_redone": res["band_redone"], "v_structure_tests": res["serial_tests"] - res_bs["serial_tests"],
               "v_structure_share_batched": 1 - bs["median_s"] / b["median_s"],
               "v_structure_share_serial": None if ss is None else 1 - ss["median_s"] / s["median_s"],
               "batch_stats_cumulative": stats, "arcs": len(res["arcs"]), "edges": len(res["edges"]),
               "largest_sepset": max(len(v[0]) for v in res["sepsets"].values())}
        out.append(row)
        print(json.dumps(row), flush=True)
        save(out)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--sizes", default="256,512,1024")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "pc_timing.json"))
    a = ap.parse_args()
    if a.only == "pc1024":
        _, run = pc_once(1024, True)
        run()
        run()
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    result = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save(rows=None):
        if rows is not None:
            kept = [r for r in result.get("pc", []) if r["variables"] not in {q["variables"] for q in rows}]
            result["pc"] = sorted(kept + rows, key=lambda r: r["variables"])
        json.dump(result, open(a.out, "w"), indent=1)

    if a.only in ("", "batch"):
        result["batch"] = batch_section(a.reps)
        save()
    if a.only in ("", "pc"):
        pc_section(a.reps, [int(v) for v in a.sizes.split(",")], save)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
