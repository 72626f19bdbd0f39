"""Measurements behind DESIGN.md 3.14 (recorded, not pass / fail): writes one JSON object to profiles/nulls/null_scores_timing.json.

  gauss<rows>  the start-cache batch of a hill-climb over 32 Gaussian nodes with 1 % nulls per column: 32 roots + 32 x 31 one-parent
               candidates in ONE pbn_score_batch, rows 1e5 / 1e6, BIC and BGe: the masked moment pass against PBN_NULL_MOMENTS=0 on the same
               build - the per-candidate path (host loop over the rows, upload of the gather list, gathered Gram), whose text this pass
               left as it was
  bde<rows>    the same batch shape over 16 discrete nodes (2-4 categories) with 1 % nulls per column under BDe: the engine (null codes in
               the family-count pass) against the class BDe was on such tables before (ParentBDe in tools/discrete_scores_timing.py: one
               `pbn_mi_counts` row grouping and a Python lgamma loop per candidate)
  kernel       the masked pass alone through pbn_debug_masked_moments at 1e6 rows x 32 columns: 496 two-column units and 128 eight-column
               units per call, wall time per (unit x row)
  small        batches of 1 / 4 / 16 / 64 one-parent candidates at 1e5 rows, both paths: where a crossover would show

One warm-up, then 5 repetitions (3 for the per-candidate path at 1e6 rows), the median with min and max; clocks untouched.  Every section
runs in a child process of its own under a time limit; the first one that fails ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "nulls", "null_scores_timing.json")
SECTIONS = {"gauss1e5": 300, "gauss1e6": 600, "bde1e5": 240, "bde1e6": 420, "kernel": 240, "small": 240}


def timed(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}


def gaussian(rows, n, seed=0):
    import pandas as pd

    rng = np.random.default_rng(seed)
    mix = np.triu(rng.uniform(-0.5, 0.5, size=(n, n)), 1) + np.eye(n)
    x = rng.normal(size=(rows, n)) @ mix
    for j in range(n):
        x[rng.integers(0, rows, size=rows // 100), j] = np.nan
    return pd.DataFrame(x, columns=[f"g{j}" for j in range(n)])


def start_batch(names):
    return [(v, []) for v in names] + [(v, [p]) for v in names for p in names if p != v]


def encode(score, cands, code):
    var, off, par = [], [0], []
    for v, ev in cands:
        var.append(score._col[v])
        par.extend(score._col[e] for e in ev)
        off.append(len(par))
    return var, [code] * len(var), off, par


def section_gauss(rows):
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    df = gaussian(rows, 32)
    names = list(df.columns)
    cands = start_batch(names)
    model = pbn.GaussianNetwork(names)
    res = {"rows": rows, "candidates": len(cands)}
    for name, make in (("bic", lambda: pbn.BIC(df)), ("bge", lambda: pbn.BGe(df))):
        s = make()
        enc = encode(s, cands, _lib.PBN_NODE_LG)
        values = {}
        for knob in ("1", "0"):
            os.environ["PBN_NULL_MOMENTS"] = knob
            key = f"{name}_{'masked' if knob == '1' else 'per_candidate'}"
            res[key] = timed(lambda: values.__setitem__(knob, s._batch_raw(model, *enc, s._kind)), reps=5 if knob == "1" or rows <= 100000 else 3)
        res[f"{name}_speedup"] = res[f"{name}_per_candidate"]["median_s"] / res[f"{name}_masked"]["median_s"]
        res[f"{name}_max_rel_diff"] = float(np.max(np.abs(values["1"] - values["0"]) / np.abs(values["0"])))
    os.environ["PBN_NULL_MOMENTS"] = "1"
    return res


def section_bde(rows):
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib
    from discrete_scores_timing import ParentBDe, table

    df = table(16, rows, 1)
    rng = np.random.default_rng(2)
    for c in df.columns:
        df.loc[rng.integers(0, rows, size=rows // 100), c] = np.nan
    names = list(df.columns)
    cands = start_batch(names)
    model = pbn.DiscreteBN(names)
    res = {"rows": rows, "candidates": len(cands)}
    s = pbn.BDe(df)
    enc = encode(s, cands, _lib.PBN_NODE_DISCRETE)
    got = []
    res["engine"] = timed(lambda: got.append(s._batch_raw(model, *enc, s._kind)))
    old = ParentBDe(df)
    want = []
    res["parent_class"] = timed(lambda: want.append([old.local_score(model, v, ev) for v, ev in cands]), reps=5 if rows <= 100000 else 3)
    res["speedup"] = res["parent_class"]["median_s"] / res["engine"]["median_s"]
    res["max_rel_diff"] = float(np.max(np.abs(got[-1] - np.asarray(want[-1])) / np.abs(want[-1])))
    return res


def masked_call(score, units):
    from pybnesian_amd import _lib

    L = _lib.load()
    ip, lp, dp = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.pbn_debug_masked_moments.restype = C.c_int
    L.pbn_debug_masked_moments.argtypes = [C.c_void_p, C.c_int, ip, ip, lp, C.POINTER(C.c_int32), ip, lp, C.c_int64, lp, dp, dp, dp]
    col_off = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(u) for u in units])]), dtype=np.int32)
    cols = np.ascontiguousarray([c for u in units for c in u], dtype=np.int32)
    k = len(units)
    N, S, G = np.zeros(k, dtype=np.int64), np.zeros((k, 8)), np.zeros((k, 36))

    def run():
        _lib.check(L.pbn_debug_masked_moments(score._handle, k, col_off.ctypes.data_as(ip), cols.ctypes.data_as(ip), None, None, None, None, k,
                                              N.ctypes.data_as(lp), S.ctypes.data_as(dp), G.ctypes.data_as(dp), None))
    return run


def section_kernel():
    import pybnesian_amd as pbn

    rows, n = 1000000, 32
    res = {"rows": rows, "columns": n}
    for dtype in ("float64", "float32"):
        s = pbn.BIC(gaussian(rows, n).astype(dtype))
        rng = np.random.default_rng(0)
        for d, units in ((2, [[i, j] for i in range(n) for j in range(i + 1, n)]), (8, [rng.choice(n, 8, replace=False).tolist() for _ in range(128)])):
            t = timed(masked_call(s, units))
            t["units"] = len(units)
            t["ns_per_unit_row"] = t["median_s"] * 1e9 / (len(units) * rows)
            # what the plain form reads through L2: d values and one validity word per (unit, row)
            t["read_GB_per_s"] = len(units) * rows * (d * (8 if dtype == "float64" else 4) + 8) / t["median_s"] / 1e9
            t["fma_G_per_s"] = len(units) * rows * (d * (d + 1) / 2) / t["median_s"] / 1e9
            res[f"{dtype}_d{d}"] = t
    return res


def section_small():
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    df = gaussian(100000, 32)
    names = list(df.columns)
    model = pbn.GaussianNetwork(names)
    s = pbn.BIC(df)
    res = {"rows": 100000}
    for size in (1, 4, 16, 64):
        enc = encode(s, [(names[i % 32], [names[(i + 1 + i // 32) % 32]]) for i in range(size)], _lib.PBN_NODE_LG)
        for knob in ("1", "0"):
            os.environ["PBN_NULL_MOMENTS"] = knob
            res[f"batch{size}_{'masked' if knob == '1' else 'per_candidate'}"] = timed(lambda: s._batch_raw(model, *enc, s._kind))
    os.environ["PBN_NULL_MOMENTS"] = "1"
    return res


def run_section(name):
    if name.startswith("gauss"):
        return section_gauss(int(float(name[5:])))
    if name.startswith("bde"):
        return section_bde(int(float(name[3:])))
    return {"kernel": section_kernel, "small": section_small}[name]()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", help="run one section in this process and print its JSON")
    ap.add_argument("--only", nargs="*", help="sections to run (default: all)")
    args = ap.parse_args()
    if args.section:
        print("RESULT " + json.dumps(run_section(args.section)))
        return 0
    results = json.load(open(OUT)) if os.path.exists(OUT) else {}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for name in (args.only or SECTIONS):
        proc = subprocess.run(["timeout", "-k", "10", str(SECTIONS[name]), sys.executable, os.path.abspath(__file__), "--section", name],
                              capture_output=True, text=True)
        line = [ln for ln in proc.stdout.splitlines() if ln.startswith("RESULT ")]
        if proc.returncode != 0 or not line:
            print(f"section {name} failed (rc {proc.returncode}); stopping\n{proc.stdout[-2000:]}\n{proc.stderr[-2000:]}")
            return 1
        results[name] = json.loads(line[-1][7:])
        json.dump(results, open(OUT, "w"), indent=1)
        print(name, json.dumps(results[name])[:900], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
