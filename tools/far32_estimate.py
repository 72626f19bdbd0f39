"""How many kept blocks of the d = 8 sweep are FAR, and what an fp32 evaluation of them costs in accuracy?  CPU only.
    python tools/far32_estimate.py [--n-train N] [--n-test M] [--groups G] [--seed S] [--ncap C ...] [--theta T ...]

The mirror of tools/screen_rowthr_estimate.py (bench.py's C2 table, the same whitening, rotation, Morton-4 proxy of the shipped Hilbert order,
window and margin, exact fp64 exponents - WITHOUT the f16 screen's error term E, so the shares are a little above the device's, which
tools/screen_d8_counts.py prints) with the far rule of csrc/kde_screen_d8.inc on top: a kept block is far when every column lies below its own
query's bound less theta, no row of the tile and no query of the group has 1/2|z|^2 above the cap, and the bound is within 4 caps in magnitude.
The far blocks are then evaluated as csrc/kde_far32_d8.inc evaluates them - operands, norm and constant rounded to fp32, eight products into
the constant in fp32, 2^x and the sums in fp32 - and compared with fp64.

Printed per (cap, theta): the far share of the kept blocks, the worst |x32 - x| against the proven bound delta(cap), and how far the queries'
sums move.  theta defaults to the rule's own value for the cap (the smallest integer with 10^6 2^-theta eps(cap) <= 8e-8, + log2(N / 10^6)),
which is what the library uses; the mirror's margin is 43 at every N, so give --theta to compare at a fixed distance.
"""
import argparse
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_d8_estimate as E  # noqa: E402
import screen_rowthr_estimate as S  # noqa: E402

U, V, BIAS, BUDGET = 2.0 ** -24, 2.0 ** -23, 64.0, 8e-8


def delta(C):
    K = 5.0 * C + BIAS + 1.0
    return (2 * U + U * U) * 2 * C + U * C + U * K + U * (1 + U) * (C + K) + ((1 + V) ** 10 - 1) * (1 + U) ** 2 * (3 * C + K)


def eps(C):
    return 2.0 ** delta(C) * (1 + V) * (1 + U) ** 255 - 1.0


def theta_rule(C, n):
    return math.ceil(math.log2(1e6 * eps(C) / BUDGET)) + math.log2(n / 1e6)


def x32(zt, zq, off):
    """[tiles][16 rows][16 queries] exponents as the far kernel forms them, and the exact ones."""
    f = np.float32
    a, b = zt.astype(f), zq.astype(f)
    nt = (-0.5 * (zt * zt).sum(-1)).astype(f)
    cq = (-0.5 * (zq * zq).sum(-1) - off + BIAS).astype(f)
    acc = (cq[None, None, :] + nt[:, :, None]).astype(f)
    for k in range(8):
        acc = (acc + (a[:, :, k, None] * b[None, None, :, k]).astype(f)).astype(f)
    x = np.einsum("tik,jk->tij", zt, zq) - 0.5 * (zt * zt).sum(-1)[:, :, None] - 0.5 * (zq * zq).sum(-1)[None, None, :] - off[None, None, :] + BIAS
    return acc, x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=24, help="query groups sampled (16 rows each)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=256, help="PBN_SUM_WINDOW")
    ap.add_argument("--ncap", type=float, nargs="+", default=[128.0, 256.0, 512.0])
    ap.add_argument("--theta", type=float, nargs="*", default=[], help="bits below the query's bound (default: the rule's value for each cap)")
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
    n_half = -nt_tiles.min(1)                      # per tile the largest 1/2|z|^2 (+inf with a padding row)
    print(f"N={args.n_train} M={args.n_test}: 1/2|z|^2 of the training rows median {np.median(-nt_tiles[np.isfinite(nt_tiles)]):.0f}, "
          f"99th percentile {np.percentile(-nt_tiles[np.isfinite(nt_tiles)], 99):.0f}, max {-nt_tiles[np.isfinite(nt_tiles)].min():.0f}")
    rng = np.random.default_rng(args.seed + 7)
    nqg = args.n_test // 16
    gsel = np.sort(rng.choice(nqg, size=min(args.groups, nqg), replace=False))
    qrows = np.concatenate([np.arange(16 * g, 16 * g + 16) for g in gsel])
    zg = zqs[qrows].reshape(-1, 16, E.D)
    tpos = np.searchsorted(tk[tperm], qk[qperm][qrows]).reshape(-1, 16)
    exact = E.log2_sums(zqs[qrows], zts).reshape(-1, 16)
    cases = [(C, th) for C in args.ncap for th in (args.theta or [theta_rule(C, args.n_train)])]
    stats = {c: dict(far=0, plain_tiles=0, worst=0.0, rel=[]) for c in cases}
    kept = 0
    for i in range(zg.shape[0]):
        pre = E.prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t)
        lb = S.window_sums(zg[i], int(tpos[i][0]) // 16, zts, args.window)
        thr_g = max(pre, float(lb.min()))
        thr_q = np.where(lb > thr_g, lb, thr_g)
        gap = np.maximum(np.maximum(lo_t - zg[i].max(0), zg[i].min(0) - hi_t), 0.0)
        visit = np.nonzero(-0.5 * (gap * gap).sum(1) >= thr_g - E.MARGIN)[0]
        cm = S.column_maxima(zg[i], zt_tiles[visit], nt_tiles[visit])
        live = (cm >= (thr_q - E.MARGIN)[None, :]).any(1)
        kept += int(live.sum())
        nq_half = 0.5 * (zg[i] * zg[i]).sum(1)
        for C, th in cases:
            st = stats[(C, th)]
            ok_q = bool(np.all(nq_half <= C) and np.all(np.abs(thr_q) <= 4 * C))
            far = live & (cm < (thr_q - th)[None, :]).all(1) & (n_half[visit] <= C) & ok_q
            st["far"] += int(far.sum())
            if not far.any():
                continue
            off = np.ceil(thr_q)
            a32, x = x32(zt_tiles[visit][far], zg[i], off)
            st["worst"] = max(st["worst"], float(np.abs(a32.astype(np.float64) - x).max()))
            t32 = np.exp2(a32).astype(np.float32).sum(axis=(0, 1), dtype=np.float32).astype(np.float64)
            t64 = np.exp2(x).sum(axis=(0, 1))
            st["rel"].append(np.abs(t32 - t64) * np.exp2(off - BIAS) / np.exp2(exact[i]))
    print(f"  {zg.shape[0]} groups x {T} tiles; kept blocks (per-query rule, exact exponents) {kept}")
    for (C, th), st in stats.items():
        rel = np.concatenate(st["rel"]) if st["rel"] else np.zeros(1)
        print(f"  cap {C:6.0f}  theta {th:6.2f} (rule {theta_rule(C, args.n_train):.2f}): far share {st['far'] / max(kept, 1):.3f};  worst |x32 - x| {st['worst']:.2e} "
              f"(bound {delta(C):.2e}, eps {eps(C):.2e});  a query's sum moves by median {np.median(rel):.1e}, max {rel.max():.1e} (budget {BUDGET:.0e})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
