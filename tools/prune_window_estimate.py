"""Which bound should the pruned d = 8 sum-only sweep prune with?  The window-sum bound (kde_prepass.hip query_window_kernel) against the
prepass bound and the exact one, on bench.py's C2 table, CPU only.  python tools/prune_window_estimate.py [--groups G] [--seed S]

The mirror of tools/prune_d8_estimate.py (same table, whitening, rotation and block rule), with the Morton order of the first four principal
axes as the proxy of the shipped Hilbert order.  For each sampled 16-query group:
  prepass        query_prepass_kernel (prune_d8_estimate.prepass_bound)
  window W       the prepass bound raised to the smallest log2 sum, over the group's queries, of the exact terms of the training tiles
                 [t - W, t + W) around the group's position t (query_window_kernel; its 2^-8 slack included)
  exact          the smallest log2 sum over ALL training rows
Printed: the fraction of (tile, group) blocks visited, and of those the share of far blocks (every term 26+ below the bound: the blocks an
fp32 tail would take), and how far each bound sits below the exact one.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_d8_estimate as E  # noqa: E402

SLACK = 2.0 ** -8   # PBN_WINDOW_SLACK
FAR = 26.0          # margin - far span (43 - 17)


def window_bound(zq_g, tile0, zt_sorted, window):
    """query_window_kernel for one group: min over its queries of log2 of the exact terms over the training tiles [tile0 - W, tile0 + W)."""
    n = zt_sorted.shape[0]
    T = (n + 15) // 16
    t0, t1 = max(tile0 - window, 0), min(tile0 + window, T)
    rows = zt_sorted[16 * t0:min(16 * t1, n)]
    return float(E.log2_sums(zq_g, rows).min()) - SLACK


def block_fractions(lo_t, hi_t, glo, ghi, thr, margin=E.MARGIN, far=FAR):
    """(visited fraction, far share of the visited blocks) for the groups' bounds thr."""
    g = np.maximum(np.maximum(lo_t[None] - ghi[:, None], glo[:, None] - hi_t[None]), 0.0)
    ex = -0.5 * (g * g).sum(2)
    visit = ex >= (thr - margin)[:, None]
    farb = visit & (ex < (thr - far)[:, None])
    return float(visit.mean()), float(farb.sum() / max(visit.sum(), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=96, help="query groups sampled (16 rows each)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", type=int, nargs="*", default=[64, 256, 1024])
    args = ap.parse_args()

    tr, te = E.bench_table(args.n_train, args.seed), E.bench_table(args.n_test, args.seed + 1)
    h = E.normal_reference_diag(tr)
    mu = tr.mean(0)
    ztr, zte = (tr - mu) * np.sqrt(E.LOG2E / h), (te - mu) * np.sqrt(E.LOG2E / h)
    R, _ = E.principal_rotation(ztr)
    zt, zq = ztr @ R.T, zte @ R.T
    tk, qk = E.morton_keys(zt), E.morton_keys(zq)
    tperm, qperm = np.argsort(tk, kind="stable"), np.argsort(qk, kind="stable")
    zts, zqs = zt[tperm], zq[qperm]
    lo_t, hi_t = E.tile_boxes(zts, E.D)
    rng = np.random.default_rng(args.seed + 7)
    nqg = args.n_test // 16
    gsel = np.sort(rng.choice(nqg, size=min(args.groups, nqg), replace=False))
    qrows = np.concatenate([np.arange(16 * g, 16 * g + 16) for g in gsel])
    zg = zqs[qrows].reshape(-1, 16, E.D)
    glo, ghi = zg.min(1), zg.max(1)
    tpos = np.searchsorted(tk[tperm], qk[qperm][qrows]).reshape(-1, 16)

    pre = np.array([E.prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t) for i in range(zg.shape[0])])
    exact = E.log2_sums(zqs[qrows], zts).reshape(-1, 16).min(1)
    rows = [("prepass", pre)]
    for w in args.windows:
        wb = np.array([window_bound(zg[i], int(tpos[i][0]) // 16, zts, w) for i in range(zg.shape[0])])
        assert np.all(wb <= exact + 1e-9)
        rows.append((f"window +-{w} tiles", np.maximum(pre, wb)))
    rows.append(("exact", exact))
    print(f"N={args.n_train} M={args.n_test} d={E.D} margin={E.MARGIN}: {len(gsel)} groups x {lo_t.shape[0]} tiles, rotated Morton-4 order")
    print(f"  {'bound':<22s} {'visited':>8s} {'far/visited':>12s} {'below exact (median)':>22s}")
    for name, thr in rows:
        v, f = block_fractions(lo_t, hi_t, glo, ghi, thr)
        print(f"  {name:<22s} {v:8.3f} {f:12.2f} {np.median(exact - thr):22.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
