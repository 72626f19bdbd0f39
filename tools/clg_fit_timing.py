"""Measurements behind DESIGN.md 3.17 (recorded, not pass / fail): CLGNetwork.fit and DynamicCLGNetwork.fit through the public
interface only, so the same file measures any checkout of the package - `--tree` names the one to import (default: the one this file
lies in).  The networks are tools/clg_model_timing.py's; what is timed is fit() on the WHOLE table (that tool fits on the first 20 000
rows only).

  n<nodes>_r<rows>     a CLGNetwork of 16 / 48 nodes over 1e5 / 1e6 rows: the first third of the nodes discrete (2 to 4 categories, up
                       to two earlier discrete parents), the others continuous (float64) with up to two discrete and up to three
                       earlier continuous parents; a new network per repetition, fit() on the whole table
  dbn<vars>_r<rows>    a DynamicCLGNetwork of 12 variables (4 discrete), order 1 (each variable given its own lag, the continuous
                       ones a discrete and up to two continuous present parents): fit() over 1e6 rows, the lagged tables included

One warm-up, then 3 repetitions, the median with min and max; clocks untouched.  One invocation = one run of one tree under `--label`:
its figures are appended to that label's runs in profiles/clg_fit/clg_fit_timing.json (`--out`), and the file's "summary" - per label
the median, minimum and maximum over its runs' medians, the ratio between the labels "parent" and "this" and whether their ranges
overlap - is rebuilt.  To compare two checkouts, alternate invocations between them (parent, this, parent, this, ...).

Not measured here: the kernels' own time, their traffic, and the share of the upload in a fit."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "clg_fit", "clg_fit_timing.json")
SHAPES = [(16, 100000), (48, 100000), (16, 1000000), (48, 1000000)]
DBN_SHAPE = (12, 1000000)


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}


def network(pbn, n, rows, seed):
    """(record batch, a function that makes the unfitted CLGNetwork, description): clg_model_timing.network without its fit"""
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    n_disc = n // 3
    names = [f"d{i}" for i in range(n_disc)] + [f"v{i}" for i in range(n - n_disc)]
    arrays, arcs, configs = [], [], 0
    for i in range(n_disc):
        card = int(rng.integers(2, 5))
        codes = rng.integers(0, card, size=rows).astype(np.int8)
        arrays.append(pa.DictionaryArray.from_arrays(pa.array(codes), pa.array([f"c{k}" for k in range(card)])))
        for p in (rng.choice(i, min(i, int(rng.integers(0, 3))), replace=False).tolist() if i else []):
            arcs.append((names[p], names[i]))
    for i in range(n - n_disc):
        arrays.append(pa.array(rng.standard_normal(rows)))
        dpar = rng.choice(n_disc, min(n_disc, int(rng.integers(0, 3))), replace=False).tolist()
        cpar = rng.choice(i, min(i, int(rng.integers(0, 4))), replace=False).tolist() if i else []
        arcs += [(names[p], names[n_disc + i]) for p in dpar] + [(names[n_disc + p], names[n_disc + i]) for p in cpar]
        cfg = 1
        for p in dpar:
            cfg *= len(arrays[p].dictionary)
        configs += cfg
    rb = pa.RecordBatch.from_arrays(arrays, names=names)
    make = lambda: pbn.CLGNetwork(names, arcs, [(names[i], pbn.DiscreteFactorType()) for i in range(n_disc)])
    return rb, make, {"nodes": n, "discrete_nodes": n_disc, "rows": rows, "arcs": len(arcs), "continuous_node_configurations": configs}


def dynamic_network(pbn, n, rows, seed):
    """(data frame, a function that makes the unfitted DynamicCLGNetwork): clg_model_timing.dynamic_network without its fit"""
    import numpy as np
    import pandas as pd

    rng = np.random.default_rng(seed)
    n_disc = n // 3
    names = [f"d{i}" for i in range(n_disc)] + [f"v{i}" for i in range(n - n_disc)]
    arcs = []
    for i, v in enumerate(names):
        arcs.append((f"{v}_t_1", f"{v}_t_0"))
        if i >= n_disc:
            arcs.append((f"{names[int(rng.integers(0, n_disc))]}_t_0", f"{v}_t_0"))
            for p in rng.choice(np.arange(n_disc, i), min(i - n_disc, 2), replace=False).tolist() if i > n_disc else []:
                arcs.append((f"{names[p]}_t_0", f"{v}_t_0"))

    def make():
        dbn = pbn.DynamicCLGNetwork(names, 1)
        for s, t in arcs:
            dbn.transition_bn().add_arc(s, t)
        return dbn

    cols = {}
    for i, v in enumerate(names):
        cols[v] = pd.Categorical.from_codes(rng.integers(0, 3, size=rows), ["a", "b", "c"]) if i < n_disc else rng.standard_normal(rows)
    return pd.DataFrame(cols), make


def measure(only=None):
    import pybnesian_amd as pbn
    from pybnesian_amd.dataset import as_record_batch

    print("measuring", os.path.dirname(pbn.__file__), flush=True)
    res = {}
    for nodes, rows in SHAPES:
        key = f"n{nodes}_r{rows}"
        if only and key not in only:
            continue
        rb, make, entry = network(pbn, nodes, rows, nodes)
        entry["fit"] = timed(lambda: make().fit(rb))
        model = make()
        model.fit(rb)
        entry["slogl_value"] = model.slogl(rb.slice(0, 20000))   # (of the fitted network on a slice: the same on both sides to ~1e-10)
        res[key] = entry
        print(key, json.dumps(entry), flush=True)
        del rb, model
    key = f"dbn{DBN_SHAPE[0]}_r{DBN_SHAPE[1]}"
    if not only or key in only:
        df, make = dynamic_network(pbn, DBN_SHAPE[0], DBN_SHAPE[1], 3)
        rb = as_record_batch(df)   # (the conversion from pandas is not what is measured)
        entry = {"variables": DBN_SHAPE[0], "rows": DBN_SHAPE[1], "order": 1}
        entry["fit"] = timed(lambda: make().fit(rb))
        res[key] = entry
        print(key, json.dumps(entry), flush=True)
    return res


def summarise(results):
    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    summary = {}
    for label, runs in results.get("runs", {}).items():
        for run in runs:
            for key, entry in run.items():
                if "fit" in entry:
                    summary.setdefault(key, {}).setdefault("fit", {}).setdefault(label, []).append(entry["fit"]["median_s"])
    out = {}
    for key, per in summary.items():
        out[key] = {}
        for what, by_label in per.items():
            row = {}
            for label, v in by_label.items():
                row.update({f"{label}_median_s": med(v), f"{label}_min_s": min(v), f"{label}_max_s": max(v), f"{label}_runs": len(v)})
            if "parent" in by_label and "this" in by_label:
                row["parent_over_this"] = med(by_label["parent"]) / med(by_label["this"])
                row["ranges_overlap"] = not (max(by_label["this"]) < min(by_label["parent"]) or max(by_label["parent"]) < min(by_label["this"]))
            out[key][what] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout whose pybnesian_amd is measured")
    ap.add_argument("--label", default="this", help="key of this run in the output file (parent / this)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--only", nargs="*", help="shapes to run, e.g. n16_r100000 (default: all)")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    run = measure(args.only)
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            results = json.load(fh)
    results.setdefault("runs", {}).setdefault(args.label, []).append(run)
    results["summary"] = summarise(results)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
