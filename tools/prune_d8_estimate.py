"""How many (tile, group) blocks must a pruned d = 8 sum-only sweep visit on bench.py's C2 table?  A numpy mirror of the partition
and the bound, CPU only.  python tools/prune_d8_estimate.py [--groups G] [--seed S]

Table: bench.py's generator (mixing matrix tril(0.3, -1) + I, 1e6 training and 1e5 test rows, numpy's normal numbers instead of
torch's), ProductKDE's normal-reference diagonal bandwidth, coordinates whitened to base-2 units (a pair's term is 2^(-|z_t - z_q|^2 / 2),
as in the sweep).  Blocks: 16-row training tiles x 16-query groups.  A block is visited when the smallest distance between the tile's
box and the group's box leaves some term within 2^-margin of the group's bound of its sum (margin = the sum-only margin at 1e6 rows).

  current   raw (diagonal-whitened) axes, Morton order of 4 key axes, boxes over those 4 axes, exact row sums (the shipped d <= 6 form,
            with Morton in place of Hilbert and without its subsample bound)
  kd        raw axes, 8-D kd-tree order, 8-D boxes, exact row sums
  rot+kd    principal axes, 8-D kd-tree order, 8-D boxes, exact row sums
  rot+kd+pre  the same with the prepass bound in place of the exact sums (kde_prepass.hip query_prepass_kernel: the 64 training rows
            around the group's position and the far corners of the 512 tiles around it)
  rot+kd4   principal axes, kd-tree splits on the widest of the first 4 principal axes only, 8-D boxes (+pre: prepass bound)
  rot+morton4+pre  principal axes, Morton order of the first 4, 8-D boxes, prepass bound - the shipped form sorts by the Hilbert
            order of those 4 axes (kde_prune_rotates)

kd order: a kd-tree of median splits on the widest axis of each node's box, at multiples of 16 rows (kd_order); each query descends
that tree to a leaf tile, stable sort by leaf.  The library (kde_prune_rotates) ships the rotation with the Hilbert order of the widest
four principal axes - the rot+kd4 / rot+morton4 rows are its proxies; profiles/r7/ has this output beside the GPU's visit count.
"""
import argparse
import math
import sys

import numpy as np

D = 8
LOG2E = 1.4426950408889634
MARGIN = 43.0               # PBN_PRUNE_MARGIN_SUM at 1e6 training rows
WINDOW = 32                 # PBN_PRUNE_WINDOW
TILE_WINDOW = 256           # PBN_GROUP_TILE_WINDOW


def bench_table(n, seed):
    mix = np.tril(np.full((D, D), 0.3), -1) + np.eye(D)
    rng = np.random.default_rng(seed)
    return (mix @ rng.standard_normal((D, n))).T.copy()   # (n, d)


def normal_reference_diag(x):
    """kde_model.hip bandwidth_from_cov, diagonal kind (Chacon & Duong 2018 eq. 3.4)."""
    n, d = x.shape
    cov = np.cov(x, rowvar=False)
    delta = cov / np.diag(cov)[:, None]
    dinv = np.linalg.inv(delta)
    tr, tr2 = np.trace(dinv), np.trace(dinv @ dinv)
    k = 4.0 * d * math.sqrt(np.linalg.det(delta)) / (2.0 * tr2 + tr * tr)
    return (k / n) ** (2.0 / (d + 4.0)) * np.diag(cov)


def principal_rotation(z):
    """Orthonormal R (rows = principal axes, widest first) of the whitened rows' covariance: z' = z R^T."""
    w, v = np.linalg.eigh(np.cov(z, rowvar=False))
    order = np.argsort(w)[::-1]
    return v[:, order].T, np.sqrt(w[order])


def kd_order(z, axes=None):
    """Median splits on the widest axis of each node's box at multiples of 16 rows.  Nodes are ranges of tiles [a, b) in heap
    numbering (root 1); returns the row order, the per-node split axis and value (a query goes left when z[axis] < value)."""
    n = z.shape[0]
    T = (n + 15) // 16
    size = 2
    while size < 2 * T:
        size *= 2
    axis = np.full(size, -1, np.int32)
    split = np.zeros(size)
    perm = np.arange(n)
    stack = [(1, 0, T)]
    while stack:
        node, a, b = stack.pop()
        if b - a <= 1:
            continue
        r0, r1 = 16 * a, min(16 * b, n)
        seg = perm[r0:r1]
        zz = z[seg]
        ext = zz.max(0) - zz.min(0)
        if axes is not None:
            ext[axes:] = -1.0
        ax = int(np.argmax(ext))
        mid = a + (b - a) // 2
        k = 16 * mid - r0
        part = np.argpartition(zz[:, ax], k)
        perm[r0:r1] = seg[part]
        axis[node], split[node] = ax, z[perm[16 * mid], ax]
        stack.append((2 * node, a, mid))
        stack.append((2 * node + 1, mid, b))
    return perm, axis, split, T


def kd_leaf(zq, axis, split, T):
    """Leaf tile of every query row (the same descent as the library's query-key kernel)."""
    nq = zq.shape[0]
    node = np.ones(nq, np.int64)
    a = np.zeros(nq, np.int64)
    b = np.full(nq, T, np.int64)
    active = b - a > 1
    while active.any():
        i = np.nonzero(active)[0]
        mid = a[i] + (b[i] - a[i]) // 2
        left = zq[i, axis[node[i]]] < split[node[i]]
        b[i] = np.where(left, mid, b[i])
        a[i] = np.where(left, a[i], mid)
        node[i] = 2 * node[i] + np.where(left, 0, 1)
        active = b - a > 1
    return a


def morton_keys(z, kd=4, bits=8, cell=0.5):
    half, top = 1 << (bits - 1), (1 << bits) - 1
    c = np.clip(np.floor(z[:, :kd] / cell) + half, 0, top).astype(np.uint64)
    key = np.zeros(z.shape[0], np.uint64)
    for bit in range(bits):
        for i in range(kd):
            key |= ((c[:, i] >> np.uint64(bit)) & np.uint64(1)) << np.uint64(bit * kd + i)
    return key


def tile_boxes(zs, pd):
    n = zs.shape[0]
    T = (n + 15) // 16
    pad = np.full((T * 16 - n, zs.shape[1]), np.nan)
    zt = np.concatenate([zs[:, :pd], pad[:, :pd]]).reshape(T, 16, pd)
    return np.nanmin(zt, 1), np.nanmax(zt, 1)


def log2_sums(zq, zt, chunk=20000):
    """log2 of sum_t 2^(-|z_q - z_t|^2 / 2) for every query row, exactly (blocked over the training rows)."""
    best = np.full(zq.shape[0], -np.inf)
    acc = np.zeros(zq.shape[0])
    qn = (zq * zq).sum(1)
    for s in range(0, zt.shape[0], chunk):
        t = zt[s:s + chunk]
        e = -0.5 * np.maximum(qn[:, None] + (t * t).sum(1)[None, :] - 2.0 * zq @ t.T, 0.0)
        m = e.max(1)
        nb = np.maximum(best, m)
        acc = acc * np.exp2(best - nb) + np.exp2(e - nb[:, None]).sum(1)
        best = nb
    return best + np.log2(acc)


def prepass_bound(zq_g, tpos, zt_sorted, lo_t, hi_t):
    """query_prepass_kernel for one group of 16 query rows with 8-D boxes: min over the queries of the log2 sum over the 2 WINDOW
    training rows around the group's position, raised to the tiles' far-corner bound of the 2 TILE_WINDOW tiles around it (+ 4)."""
    n = zt_sorted.shape[0]
    thr = np.inf
    for q, p in zip(zq_g, tpos):
        b, e = max(p - WINDOW, 0), min(p + WINDOW, n)
        ex = -0.5 * ((zt_sorted[b:e] - q) ** 2).sum(1)
        m = ex.max()
        thr = min(thr, m + np.log2(np.exp2(ex - m).sum()))
    glo, ghi = zq_g.min(0), zq_g.max(0)
    T = lo_t.shape[0]
    tt = tpos[0] // 16
    t0, t1 = max(tt - TILE_WINDOW, 0), min(tt + TILE_WINDOW, n // 16)
    far = np.maximum(hi_t[t0:t1] - glo, ghi - lo_t[t0:t1])
    ex = -0.5 * (far * far).sum(1)
    m = ex.max()
    tb = m + np.log2(np.exp2(ex - m).sum()) + 4.0
    return max(thr, tb)


def visited_fraction(lo_t, hi_t, glo, ghi, thr, margin):
    g = np.maximum(np.maximum(lo_t[None] - ghi[:, None], glo[:, None] - hi_t[None]), 0.0)
    ex = -0.5 * (g * g).sum(2)
    return float((ex >= (thr - margin)[:, None]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=1_000_000)
    ap.add_argument("--n-test", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=96, help="query groups sampled (16 rows each)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    tr, te = bench_table(args.n_train, args.seed), bench_table(args.n_test, args.seed + 1)
    h = normal_reference_diag(tr)
    mu = tr.mean(0)   # (the library centres on the training mean: a translation, no distance moves)
    ztr, zte = (tr - mu) * np.sqrt(LOG2E / h), (te - mu) * np.sqrt(LOG2E / h)
    R, spread = principal_rotation(ztr)
    print(f"N={args.n_train} M={args.n_test} d={D} margin={MARGIN}")
    print("principal spreads (base-2 bandwidth units):", " ".join(f"{s:.2f}" for s in spread))
    print("raw-axis spreads:", " ".join(f"{s:.2f}" for s in ztr.std(0)))
    rng = np.random.default_rng(args.seed + 7)
    nqg = args.n_test // 16
    gsel = np.sort(rng.choice(nqg, size=min(args.groups, nqg), replace=False))
    results = {}

    # current: Morton order of 4 raw key axes on both sides, boxes over those 4 axes
    tperm = np.argsort(morton_keys(ztr), kind="stable")
    qperm = np.argsort(morton_keys(zte), kind="stable")
    zq_sorted = zte[qperm]
    qrows = np.concatenate([np.arange(16 * g, 16 * g + 16) for g in gsel])
    sums_raw = log2_sums(zq_sorted[qrows], ztr).reshape(-1, 16)
    lo_t, hi_t = tile_boxes(ztr[tperm], 4)
    zg = zq_sorted[qrows].reshape(-1, 16, D)
    results["current"] = visited_fraction(lo_t, hi_t, zg[:, :, :4].min(1), zg[:, :, :4].max(1), sums_raw.min(1), MARGIN)

    for name, rot, axes in (("kd", False, None), ("rot+kd", True, None), ("rot+kd4", True, 4)):
        zt = ztr @ R.T if rot else ztr
        zq = zte @ R.T if rot else zte
        tperm, axis, split, T = kd_order(zt, axes)
        zts = zt[tperm]
        leaf = kd_leaf(zq, axis, split, T)
        qperm = np.argsort(leaf, kind="stable")
        zqs = zq[qperm]
        lo_t, hi_t = tile_boxes(zts, D)
        zg = zqs[qrows].reshape(-1, 16, D)
        glo, ghi = zg.min(1), zg.max(1)
        sums = log2_sums(zqs[qrows], zts).reshape(-1, 16)
        results[name] = visited_fraction(lo_t, hi_t, glo, ghi, sums.min(1), MARGIN)
        results[name + " (margin 26)"] = visited_fraction(lo_t, hi_t, glo, ghi, sums.min(1), MARGIN - 17.0)
        if rot:
            tpos = 16 * leaf[qperm][qrows].reshape(-1, 16)
            pre = np.array([prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t) for i in range(zg.shape[0])])
            results[name + "+pre"] = visited_fraction(lo_t, hi_t, glo, ghi, pre, MARGIN)
            print(f"{name}: prepass bound below the exact group bound: median {np.median(sums.min(1) - pre):.2f}, "
                  f"max {np.max(sums.min(1) - pre):.2f} (log2 units)")
            rng_w = ghi - glo
            print(f"{name}: query-group box widths per principal axis (median):", " ".join(f"{w:.2f}" for w in np.median(rng_w, 0)))
            rng_t = hi_t - lo_t
            print(f"{name}: training-tile box widths per principal axis (median):", " ".join(f"{w:.2f}" for w in np.median(rng_t, 0)))
    # the rotated 4-axis Morton order with 8-D boxes (the Hilbert order the library sorts by is close to it)
    zt, zq = ztr @ R.T, zte @ R.T
    tk, qk = morton_keys(zt), morton_keys(zq)
    tperm, qperm = np.argsort(tk, kind="stable"), np.argsort(qk, kind="stable")
    zts, zqs = zt[tperm], zq[qperm]
    lo_t, hi_t = tile_boxes(zts, D)
    zg = zqs[qrows].reshape(-1, 16, D)
    glo, ghi = zg.min(1), zg.max(1)
    tpos = np.searchsorted(tk[tperm], qk[qperm][qrows]).reshape(-1, 16)
    pre = np.array([prepass_bound(zg[i], tpos[i], zts, lo_t, hi_t) for i in range(zg.shape[0])])
    results["rot+morton4+pre"] = visited_fraction(lo_t, hi_t, glo, ghi, pre, MARGIN)
    print(f"visited (tile, group) fraction over {len(gsel)} groups x {lo_t.shape[0]} tiles:")
    for k, v in results.items():
        print(f"  {k:<22s} {v:.3f}")
    for name in ("rot+kd+pre", "rot+kd4+pre"):
        real = results[name]
        print(f"{name}: " + ("go" if real <= 0.8 else "no-go"), f"(realistic variant {real:.3f}, limit 0.8)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
