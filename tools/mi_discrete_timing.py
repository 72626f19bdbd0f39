"""Measurements behind DESIGN.md 3.19 (recorded, not pass / fail): writes one JSON object to profiles/mi_discrete/mi_discrete_timing.json.

Three variants of pbn_mi_pvalue_batch on count-only tests (x, y and Z all categorical), called through ctypes with no Python frame inside
the timed call:
  device   this build, the eligible tests counted by the joint-count kernel (threshold 0)
  off      this build with PBN_MI_DISCRETE_BATCH=0: every test builds the row grouping of its variable set
  parent   the library of the parent commit (--parent-lib; built from a checkout of it), which has nothing but that grouping path
Each variant lives in a worker process of its own that holds the table and its handles; the driver sends one timed call at a time to
the workers in turn, so that the variants are interleaved call by call: one warm-up, then 5 repetitions, the median with min and max,
clocks untouched.  Every call of `off` and `parent` gets variable sets its handle has not grouped yet - a repeated set is served by the
grouping cache and says nothing about a skeleton level - so these two are measured up to 100 tests per call (40 columns hold 780 pairs)
and their rate at 100 stands for the larger calls; `device` keeps no cache and is measured up to 1e5 tests per call.

  batch<rows>  tests per second at 5e3 / 1e5 / 1e6 rows, k = 0 ... 4, 1, 2, 5, 10 ... 1e5 tests per call over 40 columns of 2 ... 4 categories (LDS form)
  global       the global-atomics form: tables of 4 097 ... 2^22 cells at 1e5 and 1e6 rows, 1 and 16 tests per call
               (4 097 = 17 * 241 only 1: the table holds eight such pairs).  `device` needs a
               build whose cell cap admits them: `make EXPERIMENTS=1 OUT=../libpbn_hip_exp.so` and --device-lib .../libpbn_hip_exp.so
               (the section sets PBN_MI_DISCRETE_MAX_CELLS for it)
  pc           wall time of PC over MutualInformation, discrete_table(64, 100 000, 1), batched, switch on and off, a fresh handle per
               repetition, with the three counters of pbn_mi_discrete_batch_stats; both runs must give the same arcs and edges

MI_DISCRETE_BATCH_MIN_TESTS in csrc/mi.hip is the smallest call size at which the range of `device` lies wholly above that of `parent`
for every row count and k; mi::DISCRETE_MAX_CELLS the largest table for which it does at both 1e5 and 1e6 rows (the `decision` entries).
An existing output file is updated section by section; a worker that fails or runs into its time limit ends the run."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "mi_discrete", "mi_discrete_timing.json")
SECTIONS = {"batch5e3": 300, "batch1e5": 300, "batch1e6": 600, "global": 600, "pc": 900}
REPS = 5
GLOBAL_CAP = 1 << 22


def discrete_table(n, rows, seed):
    """The generator of tests/test_chisq_batch_gpu.py: n categorical columns of 2 ... 4 categories, each with up to two earlier parents."""
    rng = np.random.default_rng(seed)
    cards = rng.integers(2, 5, n)
    cols = []
    for v in range(n):
        k = min(v, int(rng.integers(0, 3)))
        pa = sorted(rng.choice(v, k, replace=False)) if k else []
        cfg = np.zeros(rows, dtype=np.int64); m = 1
        for p in pa:
            cfg += cols[p] * m; m *= cards[p]
        cpt = rng.dirichlet(np.full(cards[v], 0.35), size=m)
        u = rng.random(rows)
        cols.append((u[:, None] > np.cumsum(cpt[cfg], axis=1)).sum(1).clip(0, cards[v] - 1))
    return np.stack(cols), cards


def frame(cols, cards):
    import pandas as pd

    return pd.DataFrame({f"v{i}": pd.Categorical.from_codes(cols[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(len(cards))})


GLOBAL_CARDS = [16] * 8 + [4] * 4 + [2] * 4 + [17] * 4 + [241] * 2
# cells of a table -> how many of its columns have 16, 4, 2 and 17 categories (4 097 = 17 * 241 apart)
GLOBAL_SHAPES = {4352: (2, 0, 0, 1), 8192: (3, 0, 1, 0), 16384: (3, 1, 0, 0), 65536: (3, 2, 0, 0), 1 << 18: (4, 1, 0, 0), 1 << 20: (4, 2, 0, 0),
                 1 << 22: (5, 1, 0, 0)}
GLOBAL_SIZES = (1, 16)


def global_frame(rows):
    rng = np.random.default_rng(7)
    return frame(np.stack([rng.integers(0, c, rows) for c in GLOBAL_CARDS]), GLOBAL_CARDS)


def global_sets(cells):
    """Distinct variable sets of GLOBAL_CARDS whose table has `cells` cells, in a fixed order."""
    from itertools import combinations, product

    if cells == 4097:
        return [[a, b] for a in (16, 17, 18, 19) for b in (20, 21)]
    n16, n4, n2, n17 = GLOBAL_SHAPES[cells]
    groups = (combinations(range(8), n16), combinations(range(8, 12), n4), combinations(range(12, 16), n2), combinations(range(16, 20), n17))
    return [[v for part in parts for v in part] for parts in product(*groups)]


def pack(tests):
    n = len(tests)
    v1 = np.array([t[0] for t in tests], dtype=np.int32)
    v2 = np.array([t[1] for t in tests], dtype=np.int32)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) - 2 for t in tests])
    cond = np.array([v for t in tests for v in t[2:]] or [0], dtype=np.int32)
    return n, v1, v2, off, cond, np.zeros(n)


def summary(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


# ---- worker: one variant, one table; commands on stdin, one JSON line per answer --------------------------------------------------------
def worker(variant, table, rows):
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    if variant == "parent":                               # the parent's library has none of this commit's entry points
        for name in [n for n in _lib.SIGNATURES if n.startswith("pbn_mi_discrete_")]:
            del _lib.SIGNATURES[name]
    lib = _lib.load()
    df = global_frame(rows) if table == "global" else frame(*discrete_table(40, rows, 1))
    n_vars = df.shape[1]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    state = {"key": None, "mi": None, "used": set(), "rng": np.random.default_rng(0), "drawn": {}}
    print(json.dumps({"ready": variant}), flush=True)
    for line in sys.stdin:
        cmd = json.loads(line)
        if cmd["op"] == "quit":
            break
        key = cmd["handle"]                               # a fresh handle (an empty grouping cache) per key
        if key != state["key"]:
            state.update(key=key, mi=pbn.MutualInformation(df), used=set(), drawn={})
            if variant == "device":
                state["mi"].set_batch_threshold(0)
            # one small call outside the clock: the handle's buffers (byte mirror and count scratch; sort keys and temporaries) exist
            first = [12, 13] if table == "global" else [0, 1]
            state["used"].add(frozenset(first))
            n, v1, v2, off, cond, out = pack([first])
            lib.pbn_mi_pvalue_batch(state["mi"]._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
        if "sets" in cmd:
            tests = cmd["sets"]
        elif variant == "device" and cmd["size"] > 100:   # the kernel keeps no cache: a repeated set costs what a fresh one costs
            tests = np.argsort(state["rng"].random((cmd["size"], n_vars)), axis=1)[:, :2 + cmd["k"]].tolist()
        else:                                             # sets this handle has not met
            tests = []
            while len(tests) < cmd["size"]:
                vs = state["rng"].choice(n_vars, 2 + cmd["k"], replace=False).tolist()
                if frozenset(vs) not in state["used"]:
                    state["used"].add(frozenset(vs)); tests.append(vs)
        n, v1, v2, off, cond, out = pack(tests)
        t0 = time.perf_counter()
        lib.pbn_mi_pvalue_batch(state["mi"]._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
        dt = time.perf_counter() - t0
        ans = {"s": dt, "finite": int(np.isfinite(out).sum()), "sum": float(np.nansum(out))}
        if variant != "parent":
            ans["stats"] = state["mi"].batch_stats()
        print(json.dumps(ans), flush=True)


class Workers:
    def __init__(self, table, rows, libs, limit):
        self.deadline = time.monotonic() + limit
        self.procs = {}
        for variant in ("device", "off", "parent"):
            env = dict(os.environ)
            env.pop("PBN_MI_DISCRETE_BATCH", None)
            if variant == "off":
                env["PBN_MI_DISCRETE_BATCH"] = "0"
            if libs.get(variant):
                env["PBN_LIB"] = libs[variant]
            if variant == "device" and table == "global":
                env["PBN_MI_DISCRETE_MAX_CELLS"] = str(GLOBAL_CAP)
            self.procs[variant] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", variant, "--table", table, "--rows", str(rows)],
                                                   env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        for variant in self.procs:
            self.read(variant)

    def read(self, variant):
        line = self.procs[variant].stdout.readline()
        if not line or time.monotonic() > self.deadline:
            self.close(kill=True)
            raise SystemExit(f"worker {variant} ended or the section ran past its time limit: stopping")
        return json.loads(line)

    def ask(self, variant, **cmd):
        p = self.procs[variant]
        p.stdin.write(json.dumps(cmd) + "\n"); p.stdin.flush()
        return self.read(variant)

    def close(self, kill=False):
        for p in self.procs.values():
            try:
                if kill:
                    p.kill()
                else:
                    p.stdin.write(json.dumps({"op": "quit"}) + "\n"); p.stdin.flush()
                p.wait(timeout=60)
            except Exception:
                p.kill()


def interleaved(w, variants, **cmd):
    """One warm-up and REPS timed calls per variant, the variants taking turns."""
    ts, last = {v: [] for v in variants}, {}
    for rep in range(REPS + 1):
        for v in variants:
            sets = cmd.get("sets")
            one = {**cmd, **({"sets": sets[rep]} if sets else {})}
            if cmd.get("fresh_handles") and v != "device":    # tables of millions of cells: the groupings of one call are all a cache should hold
                one["handle"] = f"{cmd['handle']}r{rep}s{len(sets[rep])}"
            one.pop("fresh_handles", None)
            a = w.ask(v, op="run", **one)
            last[v] = a
            if rep:
                ts[v].append(a["s"])
    return {v: dict(summary(ts[v]), **{k: last[v][k] for k in ("finite", "sum", "stats") if k in last[v]}) for v in variants}


def batch_section(rows, libs, limit):
    w = Workers("batch", rows, libs, limit)
    out = []
    for k in range(5):
        base = {}
        for size in (1, 2, 5, 10, 100, 1000, 10000, 100000):
            variants = ("device", "off", "parent") if size <= 100 else ("device",)
            r = interleaved(w, variants, handle=f"k{k}", k=k, size=size)
            if size <= 100:
                base = r
            row = {"rows": rows, "k": k, "tests": size, "measured": list(variants)}
            for v in ("device", "off", "parent"):
                src = r.get(v) or base[v]
                n = size if v in r else 100
                row[v] = src
                row[v + "_tests_per_s"] = n / src["median_s"]
                row[v + "_range_tests_per_s"] = [n / src["max_s"], n / src["min_s"]]
            row["speedup_vs_parent"] = row["device_tests_per_s"] / row["parent_tests_per_s"]
            row["device_wholly_above_parent"] = row["device_range_tests_per_s"][0] > row["parent_range_tests_per_s"][1]
            if size <= 100:
                assert r["device"]["sum"] == r["device"]["sum"]
            out.append(row)
            print(f"rows {rows} k {k} tests {size}: device {row['device_tests_per_s']:.4g}/s off {row['off_tests_per_s']:.4g}/s "
                  f"parent {row['parent_tests_per_s']:.4g}/s x{row['speedup_vs_parent']:.1f} above={row['device_wholly_above_parent']}", flush=True)
    w.close()
    return out


def global_section(libs, limit):
    out = []
    for rows in (100_000, 1_000_000):
        w = Workers("global", rows, libs, limit / 2)
        for cells in (4097,) + tuple(GLOBAL_SHAPES):
            sets = global_sets(cells)
            pos = 0
            for size in ((1,) if cells == 4097 else GLOBAL_SIZES):
                need = size * (REPS + 1)
                assert pos + need <= len(sets), (cells, size)
                per_rep = [sets[pos + i * size:pos + (i + 1) * size] for i in range(REPS + 1)]
                pos += need
                r = interleaved(w, ("device", "off", "parent"), handle=f"g{cells}", sets=per_rep, fresh_handles=cells >= 1 << 18)
                row = {"rows": rows, "cells": cells, "tests": size}
                for v, s in r.items():
                    row[v] = s
                    row[v + "_tests_per_s"] = size / s["median_s"]
                    row[v + "_range_tests_per_s"] = [size / s["max_s"], size / s["min_s"]]
                row["on_device"] = r["device"]["stats"][0] > 0
                row["speedup_vs_parent"] = row["device_tests_per_s"] / row["parent_tests_per_s"]
                row["device_wholly_above_parent"] = row["device_range_tests_per_s"][0] > row["parent_range_tests_per_s"][1]
                out.append(row)
                print(f"rows {rows} cells {cells} tests {size}: device {row['device_tests_per_s']:.4g}/s off {row['off_tests_per_s']:.4g}/s parent "
                      f"{row['parent_tests_per_s']:.4g}/s x{row['speedup_vs_parent']:.2f} above={row['device_wholly_above_parent']} "
                      f"on_device={row['on_device']}", flush=True)
        w.close()
    return out


def pc_child():
    import pybnesian_amd as pbn
    from pybnesian_amd.constraint import pc_estimate_indices

    df = frame(*discrete_table(64, 100_000, 1))
    res, graphs = {}, {}
    runs = {"on": [], "off": []}
    for rep in range(REPS + 1):
        for name in ("on", "off"):                        # interleaved; the switch is read per call
            if name == "off":
                os.environ["PBN_MI_DISCRETE_BATCH"] = "0"
            try:
                test = pbn.MutualInformation(df)
                t0 = time.perf_counter()
                r = pc_estimate_indices(test, test.variable_names())
                runs[name].append(time.perf_counter() - t0)
            finally:
                os.environ.pop("PBN_MI_DISCRETE_BATCH", None)
            graphs[name] = (r["arcs"], r["edges"])
            res[name] = {"serial_tests": r["serial_tests"], "evaluated": r["evaluated"], "band_redone": r["band_redone"], "arcs": len(r["arcs"]),
                         "edges": len(r["edges"]), "batch_stats": test.batch_stats(), "passes": test.passes(),
                         "largest_sepset": max((len(s) for s, _ in r["sepsets"].values()), default=0)}
            print(name, rep, runs[name][-1], flush=True)
    for name in runs:
        res[name].update(summary(runs[name][1:]), first_s=runs[name][0])
    res["same_graph"] = graphs["on"] == graphs["off"]
    assert res["same_graph"]
    res["speedup"] = res["off"]["median_s"] / res["on"]["median_s"]
    return res


def decisions(doc):
    d = {}
    rows = [r for name in ("batch5e3", "batch1e5", "batch1e6") for r in doc.get(name, [])]
    if rows:
        sizes = sorted({r["tests"] for r in rows})
        ok = [s for s in sizes if all(r["device_wholly_above_parent"] for r in rows if r["tests"] >= s)]
        d["batch_threshold"] = ok[0] if ok else None
    g = doc.get("global", [])
    if g:   # calls of at least the threshold: smaller ones never reach the kernel
        t = d.get("batch_threshold") or 1
        good = [c for c in sorted({r["cells"] for r in g})
                if any(r["cells"] == c and r["tests"] >= t for r in g) and all(r["device_wholly_above_parent"] for r in g if r["cells"] == c and r["tests"] >= t)]
        d["max_cells"] = good[-1] if good else 4096
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--parent-lib", default=None, help="libpbn_hip.so built from the parent commit")
    ap.add_argument("--device-lib", default=None, help="an experiments build of this commit for the global section")
    ap.add_argument("--worker", default=None)
    ap.add_argument("--table", default="batch")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.table, args.rows)
    if args.child == "pc":
        print("RESULT " + json.dumps(pc_child()), flush=True)
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for name in args.sections.split(","):
        if name != "pc" and not args.parent_lib:
            raise SystemExit("--parent-lib is needed for every section but pc")
        libs = {"parent": args.parent_lib}
        if name.startswith("batch"):
            doc[name] = batch_section(int(float(name[5:])), libs, SECTIONS[name])
        elif name == "global":
            libs.update(device=args.device_lib)
            doc[name] = global_section(libs, SECTIONS[name])
        elif name == "pc":
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "pc"], capture_output=True, text=True, timeout=SECTIONS[name])
            except subprocess.TimeoutExpired:
                raise SystemExit("section pc ran into its time limit: stopping")
            sys.stdout.write(p.stdout)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"section pc failed with status {p.returncode}: stopping")
            doc[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        else:
            raise SystemExit(f"unknown section {name}")
        doc["decision"] = decisions(doc)
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
    print("decision", doc.get("decision"))
    print("wrote", OUT)


if __name__ == "__main__":
    main()
