"""Measurements behind DESIGN.md 3.15 (recorded, not pass / fail): GaussianNetwork.logl / slogl and DynamicGaussianNetwork.logl through
the public interface only, so the same file measures any checkout of the package - `--tree` names the one to import (default: the one
this file lies in).

  n<nodes>_r<rows>     a GaussianNetwork of 16 / 64 nodes (random DAG, at most 4 parents per node, coefficients given with add_cpds)
                       over 1e5 / 2e6 rows of float64: logl and slogl on the same table
  dbn<vars>_r<rows>    a DynamicGaussianNetwork of 16 variables, order 2 (each variable given two lagged and up to two present
                       parents), fitted on 1e4 rows: logl over 1e6 rows

One warm-up, then 3 repetitions, the median with min and max; clocks untouched.  One invocation = one run of one tree under `--label`:
its figures are appended to that label's runs in profiles/gaussian/gaussian_model_timing.json (`--out`), and the file's "summary" - per
label the median, minimum and maximum over its runs' medians, and the ratio between the labels "parent" and "this" when both are there
- is rebuilt.  To compare two checkouts, alternate invocations between them (parent, this, parent, this, ...)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "gaussian", "gaussian_model_timing.json")
SHAPES = [(16, 100000), (64, 100000), (16, 2000000), (64, 2000000)]
DBN_SHAPE = (16, 1000000)


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
    """(record batch, model): n float64 columns and a GaussianNetwork over them, node v with up to four earlier parents."""
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    names = [f"v{i}" for i in range(n)]
    rb = pa.RecordBatch.from_arrays([pa.array(rng.standard_normal(rows)) for _ in names], names=names)
    arcs, cpds = [], []
    for v in range(n):
        k = min(v, int(rng.integers(0, 5)))
        par = sorted(rng.choice(v, k, replace=False).tolist()) if k else []
        arcs += [(names[p], names[v]) for p in par]
        cpds.append((names[v], [names[p] for p in par], rng.normal(size=k + 1), float(rng.uniform(0.5, 2.0))))
    model = pbn.GaussianNetwork(names, arcs)
    model.add_cpds([pbn.LinearGaussianCPD(v, model.parents(v), beta, var) for v, _, beta, var in cpds])
    return rb, model, len(arcs)


def dynamic_network(pbn, n, rows, seed):
    import numpy as np
    import pandas as pd

    rng = np.random.default_rng(seed)
    names = [f"v{i}" for i in range(n)]
    dbn = pbn.DynamicGaussianNetwork(names, 2)
    tr = dbn.transition_bn()
    for i, v in enumerate(names):
        tr.add_arc(f"{v}_t_1", f"{v}_t_0")
        tr.add_arc(f"{names[(i + 1) % n]}_t_2", f"{v}_t_0")
        for p in rng.choice(i, min(i, 2), replace=False).tolist() if i else []:
            tr.add_arc(f"{names[p]}_t_0", f"{v}_t_0")
    dbn.fit(pd.DataFrame(rng.standard_normal((10000, n)), columns=names))
    return pd.DataFrame(rng.standard_normal((rows, n)), columns=names), dbn


def measure(only=None):
    import pybnesian_amd as pbn
    from pybnesian_amd.dataset import as_record_batch

    print("measuring", os.path.dirname(pbn.__file__), flush=True)
    res = {}
    for nodes, rows in SHAPES:
        key = f"n{nodes}_r{rows}"
        if only and key not in only:
            continue
        rb, model, n_arcs = network(pbn, nodes, rows, nodes)
        entry = {"nodes": nodes, "rows": rows, "arcs": n_arcs}
        entry["logl"] = timed(lambda: model.logl(rb))
        entry["slogl"] = timed(lambda: model.slogl(rb))
        entry["slogl_value"] = model.slogl(rb)
        res[key] = entry
        print(key, json.dumps(entry), flush=True)
        del rb
    key = f"dbn{DBN_SHAPE[0]}_r{DBN_SHAPE[1]}"
    if not only or key in only:
        df, dbn = dynamic_network(pbn, DBN_SHAPE[0], DBN_SHAPE[1], 3)
        rb = as_record_batch(df)   # (the conversion from pandas is not what is measured)
        entry = {"variables": DBN_SHAPE[0], "rows": DBN_SHAPE[1], "order": 2}
        entry["logl"] = timed(lambda: dbn.logl(rb))
        entry["slogl_value"] = dbn.slogl(rb)
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
                for what in ("logl", "slogl"):
                    if what in entry:
                        summary.setdefault(key, {}).setdefault(what, {}).setdefault(label, []).append(entry[what]["median_s"])
    out = {}
    for key, per in summary.items():
        out[key] = {}
        for what, by_label in per.items():
            row = {}
            for label, v in by_label.items():
                row.update({f"{label}_median_s": med(v), f"{label}_min_s": min(v), f"{label}_max_s": max(v), f"{label}_runs": len(v)})
            if "parent" in by_label and "this" in by_label:
                row["parent_over_this"] = med(by_label["parent"]) / med(by_label["this"])
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
    results = json.load(open(args.out)) if os.path.exists(args.out) else {}
    results.setdefault("runs", {}).setdefault(args.label, []).append(run)
    results["summary"] = summarise(results)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(results, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
