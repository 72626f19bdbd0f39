"""Measurements behind DESIGN.md 3.20 (recorded, not pass / fail): fit / logl / slogl of a stand-alone HCKDE and CLinearGaussianCPD
and of a hybrid SemiparametricBN, through the public interface, with the device row grouping (pybnesian_amd/adaptator_group.py) on
and off.  The comparator is the switch-off side, PBN_ADAPTATOR_GROUP=0: _DiscreteAdaptator's per-configuration loop, which is the
parent commit's code path unchanged.  Both sides run in this process on the same record batch, taking turns.

  hckde_<dtype>_r<rows>, clg_<dtype>_r<rows>
        x given two discrete parents (3 x 4 configurations) and two continuous ones, as a stand-alone factor
  n<nodes>_<dtype>_r<rows>
        a SemiparametricBN of 16 / 48 nodes: the first third discrete (2 to 4 categories, up to two earlier discrete parents), the
        others continuous, alternately CKDE and LinearGaussianCPD typed, with up to two discrete and up to two earlier continuous parents -
        so HCKDE, CLinearGaussianCPD, CKDE, LinearGaussianCPD and DiscreteFactor nodes side by side

`fit` runs on the whole table.  `logl` / `slogl` of a CLinearGaussianCPD run on the whole table too; wherever a KDE is evaluated they run
on the first --eval-rows rows (default 20 000), against factors fitted on the first --kde-train-rows rows (default 20 000) - a KDE's
evaluation is (training rows x test rows) work a configuration, the same on both sides, and would bury what is compared here.

Per side and run one warm-up and 3 repetitions, the median; --runs runs a side (default 3), off and on alternating; reported: the
median over a side's run medians with their range, off / on, and whether the two ranges overlap.  Written to
profiles/adaptator_group/adaptator_group_timing.json (`--out`); entries of shapes not run again are kept.

Not measured here: the kernels' own time and the share of uploads and gathers in a call."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "adaptator_group", "adaptator_group_timing.json")
NODES, ROWS, DTYPES = (16, 48), (100000, 1000000), ("float32", "float64")


def timed(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def both_sides(fn, runs):
    """{off, on: {median_s, min_s, max_s over the runs' medians}, off_over_on, ranges_overlap}"""
    per = {"off": [], "on": []}
    for _ in range(runs):
        for side in ("off", "on"):
            os.environ["PBN_ADAPTATOR_GROUP"] = "0" if side == "off" else "1"
            per[side].append(timed(fn))
    os.environ.pop("PBN_ADAPTATOR_GROUP", None)
    out = {}
    for side, v in per.items():
        v = sorted(v)
        out[side] = {"median_s": v[len(v) // 2], "min_s": v[0], "max_s": v[-1], "runs": len(v)}
    out["off_over_on"] = out["off"]["median_s"] / out["on"]["median_s"]
    out["ranges_overlap"] = not (out["on"]["max_s"] < out["off"]["min_s"] or out["off"]["max_s"] < out["on"]["min_s"])
    return out


def factor_batch(rows, dtype, seed):
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    d1, d2 = rng.integers(0, 3, size=rows).astype(np.int8), rng.integers(0, 4, size=rows).astype(np.int8)
    y, z = rng.standard_normal(rows), rng.standard_normal(rows)
    x = (1.0 + d1) * y - 0.5 * z + (0.5 + 0.25 * d2) * rng.standard_normal(rows)
    arrays = [pa.DictionaryArray.from_arrays(pa.array(d1), pa.array(["a", "b", "c"])), pa.DictionaryArray.from_arrays(pa.array(d2), pa.array(["p", "q", "r", "s"]))]
    arrays += [pa.array(v.astype(dtype)) for v in (x, y, z)]
    return pa.RecordBatch.from_arrays(arrays, names=["D1", "D2", "x", "y", "z"])


def network(pbn, n, rows, dtype, seed):
    """(record batch, a function that makes the unfitted network, description)"""
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(seed)
    n_disc = n // 3
    names = [f"d{i}" for i in range(n_disc)] + [f"v{i}" for i in range(n - n_disc)]
    arrays, arcs, types, kinds = [], [], [], {"HCKDE": 0, "CLinearGaussianCPD": 0, "CKDE": 0, "LinearGaussianCPD": 0}
    for i in range(n_disc):
        card = int(rng.integers(2, 5))
        arrays.append(pa.DictionaryArray.from_arrays(pa.array(rng.integers(0, card, size=rows).astype(np.int8)), pa.array([f"c{k}" for k in range(card)])))
        types.append((names[i], pbn.DiscreteFactorType()))
        for p in (rng.choice(i, min(i, int(rng.integers(0, 3))), replace=False).tolist() if i else []):
            arcs.append((names[p], names[i]))
    for i in range(n - n_disc):
        arrays.append(pa.array(rng.standard_normal(rows).astype(dtype)))
        dpar = rng.choice(n_disc, min(n_disc, int(rng.integers(0, 3))), replace=False).tolist()
        cpar = rng.choice(i, min(i, int(rng.integers(0, 3))), replace=False).tolist() if i else []
        arcs += [(names[p], names[n_disc + i]) for p in dpar] + [(names[n_disc + p], names[n_disc + i]) for p in cpar]
        kde = i % 2 == 0
        types.append((names[n_disc + i], pbn.CKDEType() if kde else pbn.LinearGaussianCPDType()))
        kinds[("HCKDE" if dpar else "CKDE") if kde else ("CLinearGaussianCPD" if dpar else "LinearGaussianCPD")] += 1
    rb = pa.RecordBatch.from_arrays(arrays, names=names)
    return rb, (lambda: pbn.SemiparametricBN(names, arcs, types)), {"nodes": n, "discrete_nodes": n_disc, "rows": rows, "arcs": len(arcs), "node_kinds": kinds}


def measure(args):
    import pybnesian_amd as pbn
    from pybnesian_amd import adaptator_group as ag

    print("measuring", os.path.dirname(pbn.__file__), flush=True)
    res = {}

    def wanted(key):
        return not args.only or key in args.only

    for dtype in DTYPES:
        for rows in ROWS:
            rb = None
            for kind, cls in (("hckde", pbn.HCKDE), ("clg", pbn.CLinearGaussianCPD)):
                key = f"{kind}_{dtype}_r{rows}"
                if not wanted(key):
                    continue
                rb = factor_batch(rows, dtype, 1) if rb is None else rb
                entry = {"rows": rows, "dtype": dtype, "configurations": 12}
                entry["fit"] = both_sides(lambda: cls("x", ["D1", "y", "D2", "z"]).fit(rb), args.runs)
                f = cls("x", ["D1", "y", "D2", "z"])
                f.fit(rb.slice(0, args.kde_train_rows) if kind == "hckde" else rb)
                test = rb.slice(0, args.eval_rows) if kind == "hckde" else rb
                entry["eval_rows"] = test.num_rows
                entry["logl"] = both_sides(lambda: f.logl(test), args.runs)
                entry["slogl"] = both_sides(lambda: f.slogl(test), args.runs)
                res[key] = entry
                print(key, json.dumps(entry), flush=True)
            for nodes in NODES:
                key = f"n{nodes}_{dtype}_r{rows}"
                if not wanted(key):
                    continue
                rb, make, entry = network(pbn, nodes, rows, dtype, nodes)
                entry["dtype"] = dtype
                before = dict(ag.counters)
                entry["fit"] = both_sides(lambda: make().fit(rb), args.runs)
                model = make()
                model.fit(rb.slice(0, args.kde_train_rows))
                test = rb.slice(0, args.eval_rows)
                entry["eval_rows"] = test.num_rows
                entry["logl"] = both_sides(lambda: model.logl(test), args.runs)
                entry["slogl"] = both_sides(lambda: model.slogl(test), args.runs)
                entry["counters"] = {k: ag.counters[k] - before[k] for k in before}
                res[key] = entry
                print(key, json.dumps(entry), flush=True)
                del rb, model
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--only", nargs="*", help="shapes to run, e.g. hckde_float64_r100000 n16_float32_r1000000 (default: all)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--eval-rows", type=int, default=20000)
    ap.add_argument("--kde-train-rows", type=int, default=20000)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    results = {}
    if os.path.exists(args.out):
        with open(args.out) as fh:
            results = json.load(fh)
    results.setdefault("shapes", {}).update(measure(args))
    results["comparator"] = "PBN_ADAPTATOR_GROUP=0: the per-configuration loop, the parent commit's code path"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
