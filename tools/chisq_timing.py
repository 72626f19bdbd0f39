"""Measurements behind DESIGN.md 3.11 (recorded, not pass / fail): writes one JSON object to profiles/chisq/chisq_timing.json.

  batch       tests per second of pbn_chisq_pvalue_batch on the device (threshold 0: upload of the request, memset, launch, download
              and host finish included) against the C loop over pbn_chisq_pvalue (the same function with the threshold out of reach:
              no Python frame in either number).  Rows 5e3 / 1e5 / 1e6, k = 0 ... 4, batches of 1 ... 1e5 random tests over 40 columns (the
              batch keeps no cache, so a repeated variable set costs it what a fresh one costs).  The loop is
              timed on tests whose variable sets the handle has not grouped yet - a repeated set is served by the grouping cache and
              says nothing about a skeleton level - so it gets at most 200 tests per repetition and its rate is used for every size.
              CHISQ_BATCH_MIN_TESTS in csrc/chisq.hip is the smallest size from which the device wins for every row count and k.
  widths      the same batch on the byte mirror and on int32 codes (a 300-category column added), 1e6 rows
  contention  x, y constant columns of cardinality 2 - every row in one cell - against uniform columns, 1e6 rows, with the LDS copies as
              built (32) and capped at 1, 8 and 16 (needs the experiments build: PBN_LIB=.../libpbn_hip_exp.so; the contention_r<N>
              sections set PBN_CHISQ_COPIES)
  pc          wall time of PC over ChiSquare, 64 variables x 1e5 rows, batched against batched=False, a fresh handle per repetition.
              Timed is pc_estimate_indices, the search behind PC().estimate without the graph object built from its result: it takes the
              batched switch and returns the counts of serial and evaluated tests, which the public call does neither
  phases      request / memset / kernel / download / host finish of one batch call (pbn_debug_chisq's phase clock)

One warm-up, then 5 repetitions, the median with min and max; clocks untouched.  Every section runs in a child process of its own under
a time limit; the first one that fails ends the run.  An existing output file is updated section by section."""
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

OUT = os.path.join(ROOT, "profiles", "chisq", "chisq_timing.json")
SECTIONS = {"batch5e3": 240, "batch1e5": 300, "batch1e6": 600, "widths": 240, "contention": 240, "contention_r1": 240, "contention_r8": 240, "contention_r16": 240, "pc": 420, "phases": 240}
HOST_LOOP = 1 << 40


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


def table(n, rows, seed, wide=False):
    import pandas as pd

    cols, cards = discrete_table(n, rows, seed)
    data = {f"v{i}": pd.Categorical.from_codes(cols[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(n)}
    if wide:
        rng = np.random.default_rng(seed)
        data["wide"] = pd.Categorical.from_codes(rng.integers(0, 300, rows), [f"w{j}" for j in range(300)])
    return pd.DataFrame(data)


def draw_tests(rng, n_vars, k, count, used=None):
    """count tests (x, y, Z) of k conditioning variables; distinct variable SETS (and none of `used`) while the columns allow it."""
    used = set() if used is None else used
    limit = 1
    for i in range(2 + k):
        limit = limit * (n_vars - i) // (i + 1)
    tests = []
    while len(tests) < count:
        vs = rng.choice(n_vars, 2 + k, replace=False).tolist()
        key = frozenset(vs)
        if key in used and len(used) < limit:
            continue
        used.add(key)
        tests.append(vs)
    return tests


def draw_fast(rng, n_vars, k, count):
    """count random tests of k conditioning variables (the batch keeps no cache: repeats cost what fresh sets cost)."""
    return np.argsort(rng.random((count, n_vars)), axis=1)[:, :2 + k].tolist()


def pack(tests):
    n = len(tests)
    v1 = np.array([t[0] for t in tests], dtype=np.int32)
    v2 = np.array([t[1] for t in tests], dtype=np.int32)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) - 2 for t in tests])
    cond = np.array([v for t in tests for v in t[2:]] or [0], dtype=np.int32)
    return n, v1, v2, off, cond, np.zeros(n)


def call(chi, packed):
    from pybnesian_amd import _lib

    n, v1, v2, off, cond, out = packed
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _lib.load().pbn_chisq_pvalue_batch(chi._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
    return out


def batch_section(rows, sizes=(1, 10, 100, 1000, 10000, 100000), ks=range(5), wide=False):
    import pybnesian_amd as pbn

    chi = pbn.ChiSquare(table(40, rows, 1, wide))
    rng = np.random.default_rng(0)
    out = []
    for k in ks:
        # the loop: 6 x n_loop tests, all over variable sets the handle meets for the first time
        n_loop = 100 if k == 0 else 200
        used = set()
        chunks = [pack(draw_tests(rng, 40, k, n_loop, used)) for _ in range(6)]
        chi.set_batch_threshold(HOST_LOOP)
        it = iter(chunks)
        loop = timed(lambda: call(chi, next(it)))
        loop_rate = n_loop / loop["median_s"]
        chi.set_batch_threshold(0)
        for size in sizes:
            packed = pack(draw_fast(rng, 40, k, size))
            d = timed(lambda: call(chi, packed), 3 if size * rows >= 10 ** 10 else 5)
            rate = size / d["median_s"]
            out.append({"rows": rows, "k": k, "tests": size, "device": d, "device_tests_per_s": rate, "loop": loop, "loop_tests": n_loop,
                        "loop_tests_per_s": loop_rate, "speedup": rate / loop_rate})
            print(f"rows {rows} k {k} tests {size}: device {rate:.4g}/s loop {loop_rate:.4g}/s x{rate / loop_rate:.1f}", flush=True)
    return {"rows": out, "stats": chi.batch_stats(), "code_bytes": 4 if wide else 1}


def phase_clock():
    from pybnesian_amd import _lib

    fn = _lib.load().pbn_debug_chisq
    fn.restype = C.c_int64
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int64]
    return fn


def phases_of(chi, packed, reps=5):
    fn = phase_clock()
    call(chi, packed)
    fn(3, None, 0)
    t0 = time.perf_counter()
    for _ in range(reps):
        call(chi, packed)
    wall = (time.perf_counter() - t0) / reps
    buf = np.zeros(5, dtype=np.int64)
    fn(4, buf.ctypes.data, 5)
    fn(0, None, 0)
    names = ("request_s", "memset_s", "kernel_s", "download_s", "host_finish_s")
    res = {n: float(v) * 1e-9 / reps for n, v in zip(names, buf)}
    res["call_s"] = wall
    return res


def contention_section():
    """1 000 tests over the same pair: two constant columns (every add of a wave on one cell) against two uniform ones."""
    import pandas as pd

    import pybnesian_amd as pbn

    rows = 1_000_000
    rng = np.random.default_rng(5)
    cat = lambda v: pd.Categorical.from_codes(v, ["a", "b"])
    df = pd.DataFrame({"c0": cat(np.zeros(rows, dtype=np.int64)), "c1": cat(np.zeros(rows, dtype=np.int64)),
                       "u0": cat(rng.integers(0, 2, rows)), "u1": cat(rng.integers(0, 2, rows))})
    chi = pbn.ChiSquare(df)
    chi.set_batch_threshold(0)
    res = {"copies_env": os.environ.get("PBN_CHISQ_COPIES"), "lib": os.path.basename(os.environ.get("PBN_LIB") or "libpbn_hip.so"), "rows": rows, "tests": 1000}
    for name, pair in (("constant", [0, 1]), ("uniform", [2, 3])):
        res[name] = phases_of(chi, pack([pair] * 1000))
        print(name, res[name], flush=True)
    return res


def pc_section():
    import pybnesian_amd as pbn
    from pybnesian_amd.constraint import pc_estimate_indices

    df = table(64, 100_000, 1)
    res = {}
    for name, batched in (("batched", None), ("serial", False)):
        runs = []
        for rep in range(6):
            chi = pbn.ChiSquare(df)
            names = chi.variable_names()
            t0 = time.perf_counter()
            r = pc_estimate_indices(chi, names, batched=batched)
            runs.append(time.perf_counter() - t0)
            last = (r, chi.batch_stats())
        ts = sorted(runs[1:])
        r, stats = last
        res[name] = {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts), "first_s": runs[0], "serial_tests": r["serial_tests"],
                     "evaluated": r["evaluated"], "band_redone": r["band_redone"], "arcs": len(r["arcs"]), "edges": len(r["edges"]),
                     "device_tests": stats[0], "host_tests": stats[1], "largest_sepset": max((len(s) for s, _ in r["sepsets"].values()), default=0)}
        print(name, res[name], flush=True)
    res["speedup"] = res["serial"]["median_s"] / res["batched"]["median_s"]
    return res


def phases_section():
    import pybnesian_amd as pbn

    res = []
    rng = np.random.default_rng(2)
    for rows in (100_000, 1_000_000):
        chi = pbn.ChiSquare(table(40, rows, 1))
        chi.set_batch_threshold(0)
        for k in (0, 2, 4):
            p = phases_of(chi, pack(draw_fast(rng, 40, k, 10000)))
            p.update({"rows": rows, "k": k, "tests": 10000})
            res.append(p)
            print(p, flush=True)
    return res


def run_section(name):
    if name.startswith("batch"):
        return batch_section(int(float(name[5:])))
    if name == "widths":
        return {"bytes": batch_section(1_000_000, (1000, 10000), (0, 2)), "int32": batch_section(1_000_000, (1000, 10000), (0, 2), wide=True)}
    if name.startswith("contention"):
        return contention_section()
    if name == "pc":
        return pc_section()
    if name == "phases":
        return phases_section()
    raise SystemExit(f"unknown section {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default=",".join(SECTIONS))
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(run_section(args.child)), flush=True)
        return
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    doc = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for name in args.sections.split(","):
        env = dict(os.environ)
        if name.startswith("contention_r"):
            env["PBN_CHISQ_COPIES"] = name[len("contention_r"):]
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True,
                               timeout=SECTIONS[name])
        except subprocess.TimeoutExpired:
            raise SystemExit(f"section {name} ran into its time limit: stopping")
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"section {name} failed with status {p.returncode}: stopping")
        doc[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        with open(OUT, "w") as f:
            json.dump(doc, f, indent=1)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
