"""Measurements behind DESIGN.md 3.12 (recorded, not pass / fail): writes one JSON object to profiles/discrete/discrete_scores_timing.json.

  start<rows>  the start-cache batch of a hill-climb over 40 discrete nodes (2-4 categories): 40 roots + 40 x 39 one-parent families in ONE
               pbn_score_batch, rows 5e3 / 1e5 / 1e6, for BIC, CVLikelihood (k = 10) and BDe: the device count pass against
               PBN_DISCRETE_COUNTS=0 on the same build (the host loop, the code from before the pass), a fresh score object per repetition
               for the likelihood scores (they remember local scores).  BDe also against its class from before the engine path: one
               `pbn_mi_counts` row grouping and a Python lgamma loop per candidate (ParentBDe below; what a table with null codes took as well
               until the engine accepted them: tools/null_scores_timing.py).
  hc           GreedyHillClimbing to convergence over a 20-node DiscreteBN with BDe at 1e5 rows: the engine path (whole batches) against
               the same score behind a plain Score subclass (one trampoline call per candidate)
  large        the global form: a batch of 24 five-parent families of five-category columns (15 625 cells each) at 1e5 and 1e6 rows,
               against the host loop

One warm-up, then 5 repetitions, the median with min and max; clocks untouched.  Every section runs in a child process of its own under
a time limit; the first one that fails ends the run.  An existing output file is updated section by section."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "discrete", "discrete_scores_timing.json")
SECTIONS = {"start5e3": 240, "start1e5": 300, "start1e6": 600, "hc": 420, "large": 420}


def timed(fn, reps=5, warm=True):
    if warm:
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": reps}


def table(n, rows, seed, cards=None):
    """n categorical columns of 2 ... 4 categories (or `cards`), each with up to two earlier parents (the generator of tools/chisq_timing.py)."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    cards = rng.integers(2, 5, n) if cards is None else np.asarray(cards)
    cols = []
    for v in range(n):
        k = min(v, int(rng.integers(0, 3)))
        pa = sorted(rng.choice(v, k, replace=False)) if k else []
        cfg, m = np.zeros(rows, dtype=np.int64), 1
        for p in pa:
            cfg += cols[p] * m
            m *= cards[p]
        cpt = rng.dirichlet(np.full(cards[v], 0.35), size=m)
        u = rng.random(rows)
        cols.append((u[:, None] > np.cumsum(cpt[cfg], axis=1)).sum(1).clip(0, cards[v] - 1))
    return pd.DataFrame({f"v{i}": pd.Categorical.from_codes(cols[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(n)})


def encode(score, cands):
    from pybnesian_amd import _lib

    var, off, par = [], [0], []
    for v, ev in cands:
        var.append(score._col[v])
        par.extend(score._col[e] for e in ev)
        off.append(len(par))
    return var, [_lib.PBN_NODE_DISCRETE] * len(var), off, par


class ParentBDe:
    """BDe as it was before the engine path (and, until null codes reached the engine, the path of tables with nulls): one
    `pbn_mi_counts` row grouping per family through a MutualInformation handle, Python lgamma arithmetic (bde.cpp:5-47)."""

    def __init__(self, df, iss=1.0):
        from pybnesian_amd.dataset import as_record_batch
        from pybnesian_amd.independences import MutualInformation

        rb = as_record_batch(df)
        self._iss = float(iss)
        self._card = {f.name: len(rb.column(i).dictionary) for i, f in enumerate(rb.schema)}
        self._counts = MutualInformation(rb, True)

    def _joint_counts(self, variables):
        from pybnesian_amd import _lib

        lib, h = _lib.load(), self._counts._handle
        _lib.check(lib.pbn_mi_set_order(h, 0, None))
        out = np.zeros(int(np.prod([self._card[v] for v in variables])))
        _lib.check(lib.pbn_mi_counts(h, len(variables), _lib.int_array([self._counts._var(v) for v in variables]), _lib.dptr(out)))
        return out

    def local_score(self, model, variable, parents):
        from math import lgamma

        counts = self._joint_counts([variable] + list(parents))
        card0, total = self._card[variable], counts.size
        alpha = self._iss / total
        res = -total * lgamma(alpha) + float(sum(lgamma(m + alpha) for m in counts))
        if not parents:
            return res + lgamma(self._iss) - lgamma(self._iss + float(counts.sum()))
        sums = counts.reshape(-1, card0).sum(axis=1)
        sum_alpha = alpha * card0
        return res + float(sum(lgamma(sum_alpha) - lgamma(sum_alpha + s) for s in sums))


def parent_bde(pbn, df):
    return ParentBDe(df)


def section_start(rows):
    import pybnesian_amd as pbn

    df = table(40, rows, 1)
    names = list(df.columns)
    cands = [(v, []) for v in names] + [(v, [p]) for v in names for p in names if p != v]
    model = pbn.DiscreteBN(names)
    res = {"rows": rows, "candidates": len(cands)}
    makers = {"bic": lambda: pbn.BIC(df), "cv10": lambda: pbn.CVLikelihood(df, k=10, seed=0), "bde": lambda: pbn.BDe(df)}
    for name, make in makers.items():
        for knob in ("1", "0"):
            os.environ["PBN_DISCRETE_COUNTS"] = knob
            if name == "cv10":   # (remembers its local scores: a fresh handle per repetition, built outside the clock)
                def run():
                    s = make()
                    enc = encode(s, cands)
                    t0 = time.perf_counter()
                    s._batch_raw(model, *enc, s._kind)
                    return time.perf_counter() - t0
                run()
                ts = sorted(run() for _ in range(5))
                t = {"median_s": ts[2], "min_s": ts[0], "max_s": ts[-1], "reps": 5}
            else:
                s = make()
                enc = encode(s, cands)
                t = timed(lambda: s._batch_raw(model, *enc, s._kind))
            res[f"{name}_{'device' if knob == '1' else 'host_loop'}"] = t
        res[f"{name}_speedup"] = res[f"{name}_host_loop"]["median_s"] / res[f"{name}_device"]["median_s"]
    os.environ["PBN_DISCRETE_COUNTS"] = "1"
    old = parent_bde(pbn, df)
    res["bde_parent_class"] = timed(lambda: [old.local_score(model, v, ev) for v, ev in cands], reps=5 if rows <= 100000 else 3)
    res["bde_speedup_over_parent_class"] = res["bde_parent_class"]["median_s"] / res["bde_device"]["median_s"]
    return res


def section_hc():
    import pybnesian_amd as pbn

    df = table(20, 100000, 2)
    names = list(df.columns)

    class Hidden(pbn.Score):
        def __init__(self, inner):
            self.inner = inner

        def local_score(self, model, variable, evidence=None):
            return self.inner.local_score(model, variable, evidence)

        def has_variables(self, variables):
            return self.inner.has_variables(variables)

        def compatible_bn(self, model):
            return self.inner.compatible_bn(model)

    score = pbn.BDe(df)
    arcs = {}

    def climb(s, key):
        arcs[key] = pbn.GreedyHillClimbing().estimate(pbn.ArcOperatorSet(), s, pbn.DiscreteBN(names)).num_arcs()

    res = {"rows": 100000, "nodes": 20}
    res["engine"] = timed(lambda: climb(score, "engine"))
    res["trampoline"] = timed(lambda: climb(Hidden(score), "trampoline"))
    res["arcs"] = arcs
    res["speedup"] = res["trampoline"]["median_s"] / res["engine"]["median_s"]
    return res


def section_large():
    import pybnesian_amd as pbn

    res = {}
    for rows in (100000, 1000000):
        df = table(12, rows, 3, cards=[5] * 12)
        names = list(df.columns)
        rng = np.random.default_rng(0)
        cands = []
        for _ in range(24):
            cols = rng.choice(12, 6, replace=False)
            cands.append((names[cols[0]], [names[c] for c in cols[1:]]))
        model = pbn.DiscreteBN(names)
        entry = {"rows": rows, "families": len(cands), "cells": 5 ** 6}
        for knob in ("1", "0"):
            os.environ["PBN_DISCRETE_COUNTS"] = knob
            s = pbn.BDe(df)
            enc = encode(s, cands)
            entry["device" if knob == "1" else "host_loop"] = timed(lambda: s._batch_raw(model, *enc, s._kind), reps=5 if knob == "1" else 3)
        entry["speedup"] = entry["host_loop"]["median_s"] / entry["device"]["median_s"]
        res[f"rows{rows}"] = entry
    return res


def run_section(name):
    if name.startswith("start"):
        return section_start(int(float(name[5:])))
    return {"hc": section_hc, "large": section_large}[name]()


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
        print(name, json.dumps(results[name])[:600], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
