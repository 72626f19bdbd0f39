"""Which threshold should a column of the d = 8 screen be compared against - its group's or its own query's?  CPU only.
    python tools/screen_rowthr_estimate.py [--groups G] [--seed S] [--window W]

The mirror of tools/prune_window_estimate.py (bench.py's C2 table, the same whitening, rotation, Morton-4 proxy of the shipped Hilbert order,
window W and margin), one level down: every (tile, group) block that passes the group's box test is recomputed pair by pair in fp64 - the exact
exponents, WITHOUT the f16 screen's error term E - and kept or dropped under three rules:
  group       a block is kept when any of its 256 exponents reaches the GROUP's bound less the margin (csrc/kde_screen_d8.inc through round 13);
              the group's bound = the prepass bound raised to the smallest window sum of its queries (query_window_kernel)
  per query   ... when any column reaches ITS query's bound less the margin: the query's own window sum where that lies above the group's bound
              (SweepArgs::qrow_thr)
  exact       ... the same with log2 of each query's whole sum as its bound: what no bound can beat
Printed: the fractions of all (tile, group) blocks box-visited and kept under each rule, how far the queries' thresholds lie above their
group's, and how many of a kept block's 16 columns are live under the per-query rule.  The levels are the proxy order's, a little above the
device's (tools/screen_d8_counts.py prints those): read the ratios.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_d8_estimate as E  # noqa: E402
import prune_window_estimate as W  # noqa: E402


def window_sums(zq_g, tile0, zt_sorted, window):
    """query_window_kernel for one group: per query log2 of the exact terms over the training tiles [tile0 - W, tile0 + W), less the slack."""
    n = zt_sorted.shape[0]
    T = (n + 15) // 16
    t0, t1 = max(tile0 - window, 0), min(tile0 + window, T)
    return E.log2_sums(zq_g, zt_sorted[16 * t0:min(16 * t1, n)]) - W.SLACK


def column_maxima(zq_g, zt_tiles, nt_tiles, chunk=4096):
    """[tiles][16]: per training tile and query column the largest exponent of the tile's 16 rows (padding rows carry -inf norms)."""
    nq = -0.5 * (zq_g * zq_g).sum(1)
    out = np.empty((zt_tiles.shape[0], 16))
    for s in range(0, zt_tiles.shape[0], chunk):
        t = zt_tiles[s:s + chunk]
        ex = np.einsum("tik,jk->tij", t, zq_g) + nt_tiles[s:s + chunk][:, :, None] + nq[None, None, :]
        out[s:s + chunk] = ex.max(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=48, help="query groups sampled (16 rows each)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=256, help="PBN_SUM_WINDOW")
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
    T = lo_t.shape[0]
    pad = T * 16 - zts.shape[0]
    zt_tiles = np.concatenate([zts, np.zeros((pad, E.D))]).reshape(T, 16, E.D)
    nt_tiles = np.concatenate([-0.5 * (zts * zts).sum(1), np.full(pad, -np.inf)]).reshape(T, 16)
    rng = np.random.default_rng(args.seed + 7)
    nqg = args.n_test // 16
    gsel = np.sort(rng.choice(nqg, size=min(args.groups, nqg), replace=False))
    qrows = np.concatenate([np.arange(16 * g, 16 * g + 16) for g in gsel])
    zg = zqs[qrows].reshape(-1, 16, E.D)
    G = zg.shape[0]
    glo, ghi = zg.min(1), zg.max(1)
    tpos = np.searchsorted(tk[tperm], qk[qperm][qrows]).reshape(-1, 16)
    exact = E.log2_sums(zqs[qrows], zts).reshape(-1, 16)

    box = kept_g = kept_q = kept_x = 0
    live_cols = []
    spread = []
    for i in range(G):
        pre = E.prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t)
        lb = window_sums(zg[i], int(tpos[i][0]) // 16, zts, args.window)
        assert np.all(lb <= exact[i] + 1e-9)
        thr_g = max(pre, float(lb.min()))                 # qthr as query_window_kernel leaves it
        thr_q = np.where(lb > thr_g, lb, thr_g)           # qrow_thr
        spread.append(thr_q - thr_g)
        gap = np.maximum(np.maximum(lo_t - ghi[i], glo[i] - hi_t), 0.0)
        visit = np.nonzero(-0.5 * (gap * gap).sum(1) >= thr_g - E.MARGIN)[0]
        cm = column_maxima(zg[i], zt_tiles[visit], nt_tiles[visit])
        kg = (cm >= thr_g - E.MARGIN).any(1)
        cq = cm >= (thr_q - E.MARGIN)[None, :]
        kq = cq.any(1)
        kx = (cm >= (exact[i] - E.MARGIN)[None, :]).any(1)
        assert not np.any(kq & ~kg) and not np.any(kx & ~kq)
        box += len(visit); kept_g += int(kg.sum()); kept_q += int(kq.sum()); kept_x += int(kx.sum())
        live_cols.append(cq[kq].sum(1))
    total = G * T
    spread, live_cols = np.concatenate(spread), np.concatenate(live_cols)
    print(f"N={args.n_train} M={args.n_test} d={E.D} margin={E.MARGIN} window={args.window}: {G} groups x {T} tiles, rotated Morton-4 order, exact fp64 exponents")
    print(f"  box-visited                      {box / total:.3f} of the blocks")
    print(f"  kept, group rule                 {kept_g / total:.3f}")
    print(f"  kept, per-query rule             {kept_q / total:.3f}  (ratio to the group rule {kept_q / max(kept_g, 1):.3f})")
    print(f"  kept, each query's exact sum     {kept_x / total:.3f}  (ratio {kept_x / max(kept_g, 1):.3f})")
    print(f"  thr_q - thr_group, log2 units    mean {spread.mean():.1f}, median {np.median(spread):.1f}, 90th percentile {np.percentile(spread, 90):.1f}, max {spread.max():.1f}")
    print(f"  live query columns per kept block (per-query rule)   mean {live_cols.mean():.1f} of 16")
    return 0


if __name__ == "__main__":
    sys.exit(main())
