"""RCoT timing on one MI355X (csrc/rcot.hip): single tests with |Z| in {0, 1, 3} at N = 1e6, the 1 128 marginal tests of a
48-column table through the batch entry, K1's executed-MFMA rate (flop from shapes over K1's event-timed launches), and - as a CPU column, labelled as such - the
numpy restatement (tests/rcot_restatement.py) of the same tests on 16 threads.  It is not the reference.

    python tools/rcot_timing.py OUT.json            full record
    python tools/rcot_timing.py --quick OUT.json    one test per |Z| and a 128-test batch (for a rocprofv3 --kernel-trace run)
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("OMP_NUM_THREADS", "16")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "16")

import numpy as np  # noqa: E402

import pybnesian_amd as pbn  # noqa: E402
from pybnesian_amd import _lib  # noqa: E402

FP64_MFMA_PEAK_TF = 78.6


def k1_mfma_flop(n_rows, F):
    """MFMA flop K1 executes for one test: every 16-row chunk of every block runs 4 k-steps x the tile pairs of [f, 1]."""
    rpb = max(1024, (-(-n_rows // 512) + 15) // 16 * 16)
    chunks = 0
    for r0 in range(0, n_rows, rpb):
        chunks += -(-(min(n_rows, r0 + rpb) - r0) // 16)
    nt = -(-(F + 1) // 16)
    return chunks * 4 * (nt * (nt + 1) // 2) * 16 * 16 * 4 * 2


def main():
    quick = "--quick" in sys.argv
    out_path = [a for a in sys.argv[1:] if not a.startswith("--")][0]
    N, V = 1_000_000, 48
    rng = np.random.default_rng(0)
    data = rng.normal(size=(N, V))
    data[:, 1] += np.sin(2 * data[:, 0])
    import pandas as pd

    df = pd.DataFrame(data, columns=[f"v{i}" for i in range(V)])
    t0 = time.perf_counter()
    ctx = pbn.Context(0)
    test = pbn.RCoT(df, seed=1, ctx=ctx)
    rec = {"N": N, "columns": V, "nxy": 5, "nz": 100, "create_s": time.perf_counter() - t0, "single": {}}
    reps = 1 if quick else 10
    for k in (0, 1, 3):
        z = [f"v{2 + i}" for i in range(k)] or None
        test.pvalue("v0", "v1", z)   # warm-up
        ctx.sync()
        ctx.set_profiling(True)
        t0 = time.perf_counter()
        for _ in range(reps):
            p = test.pvalue("v0", "v1", z)
        wall = (time.perf_counter() - t0) / reps
        k1_ms, k1_n = ctx.kernel_time(_lib.PBN_K_GRAM)        # K1 (rcot_gram_kernel), HIP events around each launch
        k2_ms, k2_n = ctx.kernel_time(_lib.PBN_K_RCOT_PROD)   # K2 (rcot_prod_kernel)
        ctx.set_profiling(False)
        F = 10 + (100 if k else 0)
        flop = k1_mfma_flop(N, F)
        k1_each = k1_ms / max(k1_n, 1)
        k2_each = k2_ms / max(k2_n, 1)
        tf = flop / (k1_each * 1e-3) / 1e12
        rec["single"][str(k)] = {"wall_ms": wall * 1e3, "pvalue": p, "k1_ms": k1_each, "k2_ms": k2_each, "k1_launches": k1_n,
                                 "k1_mfma_gflop": flop / 1e9, "k1_mfma_tflops": tf, "k1_share_of_fp64_peak": tf / FP64_MFMA_PEAK_TF}
        print(f"|Z|={k}: {wall * 1e3:.3f} ms per test (p = {p:.4g}); K1 {k1_each:.3f} ms ({tf:.1f} TF/s executed MFMA, "
              f"{100 * tf / FP64_MFMA_PEAK_TF:.1f} % of {FP64_MFMA_PEAK_TF} TF), K2 {k2_each:.3f} ms", flush=True)
    # the 1 128 marginal tests through the batch entry
    pairs = [(i, j) for i in range(V) for j in range(i + 1, V)]
    if quick:
        pairs = pairs[:128]
    lib = _lib.load()
    _lib.check(lib.pbn_rcot_set_order(test._handle, 0, None))
    v1 = _lib.int_array([a for a, _ in pairs])
    v2 = _lib.int_array([b for _, b in pairs])
    off = _lib.int_array([0] * (len(pairs) + 1))
    outp = np.zeros(len(pairs))
    lib.pbn_rcot_pvalue_batch(test._handle, min(len(pairs), 16), v1, v2, off, _lib.int_array([0]), _lib.dptr(outp))   # warm-up
    ctx.sync()
    t0 = time.perf_counter()
    lib.pbn_rcot_pvalue_batch(test._handle, len(pairs), v1, v2, off, _lib.int_array([0]), _lib.dptr(outp))
    wall = time.perf_counter() - t0
    assert np.all(np.isfinite(outp))
    rec["marginal_batch"] = {"tests": len(pairs), "wall_s": wall, "min_p": float(outp.min()), "p_v0_v1": float(outp[0])}
    print(f"{len(pairs)} marginal tests: {wall:.3f} s", flush=True)
    if not quick:
        # numpy restatement as the CPU column (16 threads), not the reference
        from rcot_restatement import rcot_from_detail

        table = {c: df[c].to_numpy() for c in ["v0", "v1", "v2", "v3", "v4"]}
        cpu = {}
        for k in (0, 1, 3):
            det = test.detail("v0", "v1", [f"v{2 + i}" for i in range(k)] or None)
            t0 = time.perf_counter()
            rcot_from_detail(table, det, 5, 100)
            cpu[str(k)] = time.perf_counter() - t0
        rec["cpu_numpy_restatement_16_threads_s"] = cpu
        det = test.detail("v0", "v1")
        t0 = time.perf_counter()
        for _ in range(8):
            rcot_from_detail(table, det, 5, 100)
        rec["cpu_numpy_restatement_marginal_batch_s_extrapolated"] = (time.perf_counter() - t0) / 8 * 1128
        print("CPU numpy restatement (16 threads, not the reference):", cpu, flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
