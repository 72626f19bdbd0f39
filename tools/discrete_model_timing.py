"""Measurements behind DESIGN.md 3.13 (recorded, not pass / fail): DiscreteBN.fit / logl / slogl through the public interface only, so
the same file measures any checkout of the package - `--tree` names the one to import (default: the one this file lies in).

  n<nodes>_r<rows>   a DiscreteBN of 20 / 40 nodes, at most 3 parents per node, 2 - 5 categories, over 1e5 / 1e6 rows sampled from a
                     network of that structure: fit of a fresh model, then logl and slogl of the fitted one on the same table

One warm-up, then 3 repetitions, the median with min and max; clocks untouched.  One invocation = one run of one tree under `--label`:
its figures are appended to that label's runs in profiles/discrete/discrete_model_timing.json (`--out`), and the file's "summary" - the
median over each label's runs, and the ratio between the labels "parent" and "this" when both are there - is rebuilt.  To compare two
checkouts, alternate invocations between them (parent, this, parent, this, ...)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "discrete", "discrete_model_timing.json")
SHAPES = [(20, 100000), (40, 100000), (20, 1000000), (40, 1000000)]


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}


def network(n, rows, seed):
    """(frame, arcs): n categorical columns of 2 ... 5 categories, each with up to three earlier parents, sampled from random CPTs."""
    import numpy as np
    import pandas as pd

    rng = np.random.default_rng(seed)
    cards = rng.integers(2, 6, n)
    cols, arcs = [], []
    for v in range(n):
        k = min(v, int(rng.integers(0, 4)))
        pa = sorted(rng.choice(v, k, replace=False).tolist()) if k else []
        cfg, m = np.zeros(rows, dtype=np.int64), 1
        for p in pa:
            cfg += cols[p] * m
            m *= int(cards[p])
            arcs.append((f"v{p}", f"v{v}"))
        cpt = rng.dirichlet(np.full(cards[v], 0.35), size=m)
        u = rng.random(rows)
        cols.append((u[:, None] > np.cumsum(cpt[cfg], axis=1)).sum(1).clip(0, cards[v] - 1))
    df = pd.DataFrame({f"v{i}": pd.Categorical.from_codes(cols[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(n)})
    return df, arcs


def measure(only=None):
    import pybnesian_amd as pbn
    from pybnesian_amd.dataset import as_record_batch

    print("measuring", os.path.dirname(pbn.__file__), flush=True)
    res = {}
    for nodes, rows in SHAPES:
        key = f"n{nodes}_r{rows}"
        if only and key not in only:
            continue
        df, arcs = network(nodes, rows, nodes)
        rb = as_record_batch(df)   # (the conversion from pandas is not what is measured)
        names = list(df.columns)
        fitted = pbn.DiscreteBN(names, arcs)
        fitted.fit(rb)
        entry = {"nodes": nodes, "rows": rows, "arcs": len(arcs)}
        entry["fit"] = timed(lambda: pbn.DiscreteBN(names, arcs).fit(rb))
        entry["logl"] = timed(lambda: fitted.logl(rb))
        entry["slogl"] = timed(lambda: fitted.slogl(rb))
        entry["slogl_value"] = fitted.slogl(rb)
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
                for what in ("fit", "logl", "slogl"):
                    summary.setdefault(key, {}).setdefault(what, {}).setdefault(label, []).append(entry[what]["median_s"])
    out = {}
    for key, per in summary.items():
        out[key] = {}
        for what, by_label in per.items():
            row = {f"{label}_median_s": med(v) for label, v in by_label.items()}
            row.update({f"{label}_runs": len(v) for label, v in by_label.items()})
            if "parent" in by_label and "this" in by_label:
                row["parent_over_this"] = med(by_label["parent"]) / med(by_label["this"])
            out[key][what] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout whose pybnesian_amd is measured")
    ap.add_argument("--label", default="this", help="key of this run in the output file (parent / this)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--only", nargs="*", help="shapes to run, e.g. n20_r100000 (default: all)")
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
