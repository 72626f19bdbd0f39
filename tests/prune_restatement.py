"""Plain numpy restatement of the pruning prepass of the fitted KDE handles (csrc/kde_prepass.hip, driven by kde_pack_train and
kde_eval_enqueue in csrc/kde_model.hip), stage by stage and by the definitions in those files' comments: fp64 throughout, np.longdouble
where a sum is the truth something is held against.  No device, no library: tests/test_prune_restatement_cpu.py holds the restatement
against itself and against brute force, tests/test_prune_stages_gpu.py holds the kernels against the restatement.

What the grouped chain shares - tile and batch boxes, the scan and tile-window bounds, brute-force truths, the rounding slack - is imported
from group_restatement; this file adds what the stand-alone chain has on top: key cells, Morton and Hilbert keys, the subsample, the host's
split rule and the two-level visit rule of the sweep.  Every exponent and bound is a base-2 logarithm (the kernel of a pair is
2^(-|z_q - z_t|^2 / 2))."""
import math

import numpy as np

from group_restatement import TILE, batch_boxes, bound_slack, bounds, tile_boxes, true_exponents, true_log2_sums, true_max_exponent  # noqa: F401

WINDOW = 32            # PBN_PRUNE_WINDOW: training rows scanned on either side of a query's position
TILE_WINDOW = 256      # PBN_GROUP_TILE_WINDOW: full training tiles on either side whose box corners bound a tile's sums
BATCH = 64             # tiles per batch of the sweep's walk
SUPER = 4096           # tiles per super-batch
LD = np.longdouble


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
def key_bits(kd):
    """prune_key_bits: bits per key axis."""
    return 16 if kd <= 2 else (10 if kd == 3 else 32 // kd)


def key_cell(kd):
    """prune_key_cell: width of a key cell in whitened units."""
    return 0.03125 if kd <= 2 else (0.5 if kd <= 4 else (1.0 if kd == 5 else 2.0))


def key_cells(z, kd):
    """[n][kd] uint32: floor(z / cell) + half, clamped to [0, 2^bits - 1], of the first kd coordinates."""
    bits = key_bits(kd)
    half, top = float(1 << (bits - 1)), float((1 << bits) - 1)
    c = np.floor(np.asarray(z, dtype=np.float64)[:, :kd] * (1.0 / key_cell(kd))) + half
    return np.clip(c, 0.0, top).astype(np.uint32)


def clamped(z, kd):
    """Rows whose cell was clamped on some key axis (the unclamped cell lies outside the key range)."""
    bits = key_bits(kd)
    c = np.floor(np.asarray(z, dtype=np.float64)[:, :kd] * (1.0 / key_cell(kd))) + float(1 << (bits - 1))
    return ((c < 0.0) | (c > float((1 << bits) - 1))).any(1)


def morton(cells, kd, bits):
    """Bit b of axis i -> bit b kd + i."""
    cells = np.asarray(cells, dtype=np.uint64)
    key = np.zeros(len(cells), dtype=np.uint64)
    for i in range(kd):
        for b in range(bits):
            key |= ((cells[:, i] >> np.uint64(b)) & np.uint64(1)) << np.uint64(b * kd + i)
    return key.astype(np.uint32)


def hilbert2(cells, bits):
    """Position along the 2-D Hilbert curve (the classic xy -> d walk from the top bit down), uint32 arithmetic as the kernel's."""
    x = np.asarray(cells, dtype=np.uint64)[:, 0].copy()
    y = np.asarray(cells, dtype=np.uint64)[:, 1].copy()
    n1 = np.uint64((1 << bits) - 1)
    key = np.zeros(len(x), dtype=np.uint64)
    sq = 1 << (bits - 1)
    while sq > 0:
        s = np.uint64(sq)
        rx = ((x & s) != 0).astype(np.uint64)
        ry = ((y & s) != 0).astype(np.uint64)
        key = (key + s * s * ((np.uint64(3) * rx) ^ ry)) & np.uint64(0xFFFFFFFF)
        flip = (ry == 0) & (rx == 1)
        x = np.where(flip, n1 - x, x)
        y = np.where(flip, n1 - y, y)
        swap = ry == 0
        x, y = np.where(swap, y, x), np.where(swap, x, y)
        sq >>= 1
    return key.astype(np.uint32)


def hilbert_nd(cells, n, bits):
    """Position along the n-dimensional Hilbert curve, Skilling's transpose form: undo the excess rotations from the top bit down,
    Gray-encode, interleave with axis 0 most significant (hilbert_key in kde_kernels.hpp)."""
    X = [np.asarray(cells, dtype=np.uint64)[:, i].copy() for i in range(n)]
    M = 1 << (bits - 1)
    Q = M
    while Q > 1:
        P = np.uint64(Q - 1)
        for i in range(n):
            hit = (X[i] & np.uint64(Q)) != 0
            t = (X[0] ^ X[i]) & P
            x0 = np.where(hit, X[0] ^ P, X[0] ^ t)
            xi = np.where(hit, X[i], X[i] ^ t)
            if i == 0:          # (i = 0: t = 0, the exchange is the identity; only the inversion acts)
                X[0] = x0
            else:
                X[0], X[i] = x0, xi
        Q >>= 1
    for i in range(1, n):
        X[i] = X[i] ^ X[i - 1]
    t = np.zeros(len(X[0]), dtype=np.uint64)
    Q = M
    while Q > 1:
        t = np.where((X[n - 1] & np.uint64(Q)) != 0, t ^ np.uint64(Q - 1), t)
        Q >>= 1
    key = np.zeros(len(X[0]), dtype=np.uint64)
    for i in range(n):
        X[i] = X[i] ^ t
        for q in range(bits):
            key |= ((X[i] >> np.uint64(q)) & np.uint64(1)) << np.uint64(q * n + (n - 1 - i))
    return key.astype(np.uint32)


def curve_kind(kd, hilbert_3_4=True):
    return "morton" if kd == 1 or (kd > 2 and not hilbert_3_4) else "hilbert"


def keys(z, kd, hilbert_3_4=True):
    """prune_keys_kernel: the sort key of every row from its whitened coordinates."""
    bits = key_bits(kd)
    c = key_cells(z, kd)
    if kd == 2:
        return hilbert2(c, bits)
    if hilbert_3_4 and kd in (3, 4):
        return hilbert_nd(c, kd, bits)
    return morton(c, kd, bits)


def stable_order(k):
    """sort_keys: the permutation of a stable sort (equal keys in ascending row order)."""
    return np.argsort(np.asarray(k, dtype=np.uint32), kind="stable").astype(np.int64)


def lower_bound(sorted_keys, k):
    """First position whose key is not below k (the binary search of query_prepass_kernel)."""
    return np.searchsorted(np.asarray(sorted_keys, dtype=np.uint32), np.asarray(k, dtype=np.uint32), side="left").astype(np.int64)


# ---- subsample ----------------------------------------------------------------------------------------------------------------------------
def nsub_of(N, d, pdims):
    """kde_pack_train: more dimensions than the boxes cover -> min(4096, N / 64) rounded down to whole tiles."""
    return min(4096, N // 64) // 16 * 16 if d > pdims else 0


def subsample_rows(N, nsub):
    """Sorted positions k (N / nsub), k < nsub."""
    return np.arange(nsub, dtype=np.int64) * (N // nsub) if nsub else np.zeros(0, dtype=np.int64)


def log2_sum_over(zs_rows, zq):
    """log2 sum_t 2^(-|z_q - z_t|^2 / 2) over the given rows, in longdouble -> float64."""
    a, b = np.asarray(zs_rows, dtype=LD), np.asarray(zq, dtype=LD)
    out = np.empty(len(b))
    for i in range(0, len(b), 128):
        e = -((b[i:i + 128, None, :] - a[None, :, :]) ** 2).sum(2) / LD(2)
        m = e.max(1)
        out[i:i + 128] = (m + np.log2(np.exp2(e - m[:, None]).sum(1))).astype(np.float64)
    return out


def subsample_slack(f16x2):
    """prune_subsample_slack: (absolute log2 units, relative to |log2 sum|) taken off the subsample's log2 sum - the error budget of the sweep
    that computed it.  fp64 fragments 2^-24; f16x2 fragments 2^-10 + 2^-13 |log2 sum| (atol 5e-4 / rtol 1e-4 in natural units, rounded up)."""
    return (2.0 ** -10, 2.0 ** -13) if f16x2 else (2.0 ** -24, 0.0)


def subsample_bounds(ls, nsub, f16x2=False):
    """(bound of the largest exponent, bound of the log2 sum) from the subsample's log2 sum AS THE SWEEP COMPUTED IT: the slack comes off, then
    its mean term and the sum itself."""
    a, r = subsample_slack(f16x2)
    ls = ls - (a + r * np.abs(ls))
    return ls - math.log2(nsub), ls


def scan_bounds(zs, zq, qpos, window=WINDOW):
    """Per query (largest exponent, log2 sum) over the training rows [qpos - window, qpos + window): group_restatement.bounds on one-query
    tiles, where the tile's minimum is the query's own sum."""
    best, sumb = np.empty(len(zq)), np.empty(len(zq))
    for q in range(len(zq)):
        lb, thr = bounds(zs, zq[q:q + 1], qpos[q:q + 1], -1, window, 0, True, zs[:0])
        best[q], sumb[q] = lb[0], thr[0]
    return best, sumb


def prepass_bounds(zs, zq, qpos, pd, box, ls=None, nsub=0, tile_box_bound=True, f16x2=False, window=WINDOW, tile_window=TILE_WINDOW):
    """(qlb [nqtiles 16], qthr [nqtiles]) of query_prepass_kernel, queries in their sorted order.  Without a subsample this is
    group_restatement.bounds: the scan of `window` rows around the position and, where the boxes cover every dimension of an unconditional
    model (tile_box_bound and pd == d), the tile-window bound.  With one (ls = its log2 sum per query as the subsample sweep left it, f16x2 =
    on half-precision fragments): less its slack, ls - log2(nsub) raises a query's largest-exponent bound and ls its sum bound BEFORE the
    tile's minimum is taken; such a model has more dimensions than boxes and no tile-window bound."""
    nq, d = zq.shape
    if ls is None:
        return bounds(zs, zq, qpos, pd if (tile_box_bound and pd == d) else -1, window, tile_window, True, box)
    assert pd != d, "a model with a subsample has more dimensions than boxes"
    best, sumb = scan_bounds(zs, zq, qpos, window)
    lb, sb = subsample_bounds(np.asarray(ls, dtype=np.float64)[:nq], nsub, f16x2)
    best, sumb = np.maximum(best, lb), np.maximum(sumb, sb)
    thr_q = np.where(sumb > best, sumb, best)
    nqt = (nq + TILE - 1) // TILE
    qlb = np.full(nqt * TILE, -np.inf)
    qlb[:nq] = best
    return qlb, np.array([thr_q[t * TILE:(t + 1) * TILE].min() for t in range(nqt)])


# ---- the host's split rule ----------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def split_rule(ntiles, nqtiles, num_cus, qg, tile_bytes, prune=True, blocks_per_cu=24, split_kb=2048, max_tiles=1024, min_tiles=64):
    """(nsplit, tps, batches_per_split) as kde_eval_enqueue computes them."""
    qblocks = ceil_div(nqtiles, 4 * qg)
    nsplit = max(1, ceil_div(num_cus * blocks_per_cu, qblocks))
    nsplit = max(nsplit, ceil_div(ntiles * tile_bytes, split_kb * 1024))
    if prune:
        nsplit = max(nsplit, ceil_div(ntiles, max_tiles))
    if nsplit > 1:
        nsplit = ceil_div(nsplit, 8) * 8
    nsplit = min(nsplit, max(1, ntiles // min_tiles))
    nsplit = min(nsplit, 4096)
    tps = ceil_div(ntiles, nsplit)
    nsplit = ceil_div(ntiles, tps)
    return nsplit, tps, ceil_div(tps, BATCH)


# ---- the visit rule -----------------------------------------------------------------------------------------------------------------------
def box_gap2(lo_a, hi_a, lo_b, hi_b):
    """Squared distance between two boxes, per pair of rows of a (one box each) and the single box b: per axis the positive part of the
    larger of the two gaps, squared and added up in the order of the axes."""
    g = np.maximum(np.maximum(lo_a - hi_b, lo_b - hi_a), 0.0)
    d2 = np.zeros(len(g))
    for k in range(g.shape[1]):
        d2 = d2 + g[:, k] * g[:, k]
    return d2


def visit_counts(tile_box, bbox, qbox, thr, pd, tps, qg, rel=8 * 2.0 ** -53):
    """The two-level walk of the pruned fp64 sweep (batch_in_reach, then prune_group_mask per (tile, 16-query group)) over every wave:
    -> (certain, borderline, offered).  A wave owns qg consecutive query tiles - the last tile repeated where they run past nqtiles, and
    counted again, as the kernel does - and walks the tiles of every split.  A pair is visited when neither test drops it: the test is
    !(-d2 / 2 < thr).  `certain` counts the pairs both tests keep by more than the slack rel max(|d2 / 2|, |thr|) (numpy's unfused sum of
    squares against the kernel's fma), `borderline` those where either test lies within it (and neither drops the pair by more)."""
    ntiles, nqtiles = len(tile_box), len(qbox)
    tlo, thi = tile_box[:, :pd], tile_box[:, pd:]
    blo, bhi = bbox[:, :pd], bbox[:, pd:]
    batch_of = _batch_of(ntiles, tps)
    certain = borderline = offered = 0
    nwaves = ceil_div(nqtiles, qg)
    for w in range(nwaves):
        offered += ntiles * qg
        for g in range(qg):
            qt = min(w * qg + g, nqtiles - 1)
            c, b = _classify(tlo, thi, blo, bhi, batch_of, qbox[qt, :pd], qbox[qt, pd:], thr[qt], rel)
            certain += c
            borderline += b
    return certain, borderline, offered


def _margin_state(e, thr, rel):
    """+1 kept for certain, -1 dropped for certain, 0 within the slack (e = -d2 / 2; the kernel keeps a pair unless e < thr)."""
    if thr == -np.inf:
        return np.ones(len(e), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        slack = rel * np.maximum(np.abs(e), abs(thr))
        return np.where(e < thr - slack, -1, np.where(e >= thr + slack, 1, 0))


def _classify(tlo, thi, blo, bhi, batch_of, qlo, qhi, thr, rel):
    sb = _margin_state(-0.5 * box_gap2(blo, bhi, qlo, qhi), thr, rel)[batch_of]
    st = _margin_state(-0.5 * box_gap2(tlo, thi, qlo, qhi), thr, rel)
    both = np.minimum(sb, st)
    return int((both == 1).sum()), int((both == 0).sum())


def _batch_of(ntiles, tps):
    nsplit, nbps = ceil_div(ntiles, tps), ceil_div(tps, BATCH)
    out = np.empty(ntiles, dtype=np.int64)
    for s in range(nsplit):
        t0, t1 = s * tps, min(s * tps + tps, ntiles)
        out[t0:t1] = s * nbps + (np.arange(t0, t1) - t0) // BATCH
    return out


def skipped_pairs(tile_box, bbox, qbox, thr, pd, tps, rel=8 * 2.0 ** -53):
    """[nqtiles][ntiles] bool: the (query tile, training tile) pairs the restated rule skips for certain (dropped by either test by more
    than the slack)."""
    batch_of = _batch_of(len(tile_box), tps)
    out = np.zeros((len(qbox), len(tile_box)), dtype=bool)
    for qt in range(len(qbox)):
        c = _margin_state(-0.5 * box_gap2(bbox[:, :pd], bbox[:, pd:], qbox[qt, :pd], qbox[qt, pd:]), thr[qt], rel)[batch_of]
        t = _margin_state(-0.5 * box_gap2(tile_box[:, :pd], tile_box[:, pd:], qbox[qt, :pd], qbox[qt, pd:]), thr[qt], rel)
        out[qt] = np.minimum(c, t) == -1
    return out


# ---- finish -------------------------------------------------------------------------------------------------------------------------------
LN2 = math.log(2.0)


def merge_partials(part, slot=0):
    """kde_finish_kernel: part [rows][queries][P], a pair (o, s) at (slot, slot + 1) stands for s 2^o -> log2 of the sum per query."""
    o, s = part[:, :, slot], part[:, :, slot + 1]
    m = o.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return m + np.log2((s * np.exp2(o - m[None, :])).sum(0))


# ---- the tables of the stage tests (shared by the CPU and the GPU tier) --------------------------------------------------------------------
LOG2E = 1.4426950408889634
IDENTICAL = 40         # a block of identical training rows: tiles of zero extent


def training_rows(N, d, seed, far_sd):
    """Four clusters, correlated columns, IDENTICAL equal rows in a block and one row at +far_sd, one at -far_sd standard deviations
    (far_sd = 0: none)."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(4, d)) * 4.0
    x = centres[rng.integers(0, 4, N)] + rng.normal(size=(N, d)) * np.linspace(0.3, 0.6, d)
    for j in range(1, d):
        x[:, j] += 0.3 * np.tanh(x[:, j - 1])
    a = N // 2
    x[a:a + IDENTICAL] = x[a]
    if far_sd:
        sd, mean = x.std(0), x.mean(0)
        x[N // 3], x[2 * N // 3] = mean + far_sd * sd, mean - far_sd * sd
    return x


def far_units(kd):
    """Whitened distance from the centre, per key axis, that lies beyond the key range (half the range is 2^(bits - 1) cells): 1.5 times it."""
    return 1.5 * (1 << (key_bits(kd) - 1)) * key_cell(kd)


def query_rows(train, n, seed, W, mu, kd, order, full_w=False):
    """n query rows in the columns' order of W: draws from the training clusters, a tenth of them copies of training rows and - from 15
    queries on - four edge queries built from the model's own whitening z = W (x - mu): one beyond the low end of every key axis (cell 0 on
    every axis: key 0, position 0), one at the far corner whose key is the largest of all corners (the end of the curve: position N unless a
    training row shares the cell), and copies of the training rows at the sorted positions 5 and N - 6 (`order`: the training rows' sorted
    order)."""
    rng = np.random.default_rng(seed)
    N, d = train.shape
    q = train[rng.integers(0, N, n)] + rng.normal(size=(n, d)) * 0.2
    copies = rng.choice(n, max(1, n // 10), replace=False) if n >= 10 else np.zeros(0, dtype=np.int64)
    q[copies] = train[rng.integers(0, N, len(copies))]
    if n >= 15:
        Wm = np.asarray(W, dtype=np.float64).reshape(d, d)
        if not full_w:
            Wm = np.tril(Wm)
        far = far_units(kd)
        corners = np.array([[far if (c >> i) & 1 else -far for i in range(kd)] + [0.0] * (d - kd) for c in range(1 << kd)])
        ck = keys(corners, kd)
        assert ck[0] == 0
        edge = np.stack([corners[0], corners[int(ck.argmax())]])
        slots = [s for s in range(n) if s not in set(copies.tolist())][:4]
        q[slots[0]], q[slots[1]] = (np.linalg.solve(Wm, edge.T).T + np.asarray(mu)[:d])
        q[slots[2]], q[slots[3]] = train[order[5]], train[order[N - 6]]
    return q


def cpu_whitening(train):
    """(W row-major lower, mu) of a full normal-reference bandwidth H = (4 / (N (d + 2)))^(2 / (d + 4)) cov: W = sqrt(log2 e) chol(H)^-1,
    centred on the column means.  The CPU tier's stand-in for the handle's own matrix: the same rule, not the same bits."""
    N, d = train.shape
    H = (4.0 / (N * (d + 2.0))) ** (2.0 / (d + 4.0)) * np.atleast_2d(np.cov(train.T))
    W = math.sqrt(LOG2E) * np.linalg.inv(np.linalg.cholesky(H))
    return np.tril(W), train.mean(0)


def restate_chain(train, W, mu, n, qseed, pdims, kdims, num_cus, qg, tile_bytes):
    """The whole chain on the CPU for an unconditional fp64 model: -> dict of every stage's restated output."""
    N, d = train.shape
    Wm = np.tril(np.asarray(W).reshape(d, d))
    z = (train - mu) @ Wm.T
    k = keys(z, kdims)
    order = stable_order(k)
    zs, ks = z[order], k[order]
    xq = query_rows(train, n, qseed, Wm, mu, kdims, order)
    zq_row = (xq - mu) @ Wm.T
    qk = keys(zq_row, kdims)
    qorder = stable_order(qk)
    zq, qks = zq_row[qorder], qk[qorder]
    qpos = lower_bound(ks, qks)
    box = tile_boxes(zs, pdims)
    nsub = nsub_of(N, d, pdims)
    ls = log2_sum_over(zs[subsample_rows(N, nsub)], zq) if nsub else None
    qlb, qthr = prepass_bounds(zs, zq, qpos, pdims, box, ls, nsub)
    ntiles, nqtiles = ceil_div(N, TILE), ceil_div(n, TILE)
    nsplit, tps, nbps = split_rule(ntiles, nqtiles, num_cus, qg, tile_bytes)
    return dict(z=z, keys=k, order=order, zs=zs, ks=ks, xq=xq, zq_row=zq_row, qkeys=qk, qorder=qorder, zq=zq, qpos=qpos, box=box, nsub=nsub,
                ls=ls, qlb=qlb, qthr=qthr, nsplit=nsplit, tps=tps, nbps=nbps, bbox=batch_boxes(box, pdims, tps), qbox=tile_boxes(zq, pdims))


def prune_margin(N, base=52.0):
    """prune_margin: the base at 10^6 training rows + log2(N / 10^6), at least 8."""
    return max(8.0, base + math.log2(N / 1e6))


# name: (class, d, dtype, training rows, queries).  The fp64 plain models are the ones the visit rule is checked on.
CASES = {
    "kde-d1": ("KDE", 1, "float64", 257, 17),
    "kde-d2": ("KDE", 2, "float64", 4133, 600),
    "kde-d3": ("KDE", 3, "float64", 1100, 255),
    "kde-d4": ("KDE", 4, "float64", 4133, 257),
    "kde-d5-nosub": ("KDE", 5, "float64", 1023, 33),
    "kde-d5": ("KDE", 5, "float64", 1100, 16),
    "kde-d6": ("KDE", 6, "float64", 4133, 15),
    "pkde-d3": ("ProductKDE", 3, "float64", 257, 1),
    "ckde-d2": ("CKDE", 2, "float64", 1100, 33),
    "ckde-d3": ("CKDE", 3, "float64", 4133, 17),
    "ckde-d5": ("CKDE", 5, "float64", 4133, 600),
    "f32-d2": ("KDE", 2, "float32", 4133, 257),
    "f32-d5": ("KDE", 5, "float32", 1100, 255),
    "f32-widen-d2": ("ProductKDE", 2, "float32", 1023, 16),
    "rot-d7": ("KDE", 7, "float64", 4133, 255),
    "rot-d8": ("KDE", 8, "float64", 4133, 600),
}
TRAIN_SEED, QUERY_SEED = 7, 11
VISIT_CASES = [c for c, v in CASES.items() if v[0] == "KDE" and v[2] == "float64" and v[1] <= 6]


def case_training(name):
    cls, d, dtype, N, n = CASES[name]
    far = 0.0 if name == "f32-widen-d2" else (40.0 if dtype == "float64" else 10.0)
    return training_rows(N, d, TRAIN_SEED + N + d, far).astype(dtype).astype(np.float64)
