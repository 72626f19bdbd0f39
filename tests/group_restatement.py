"""Plain numpy restatement of the grouped KDE evaluation's prepass (csrc/kde_group.hip), stage by stage and by the definitions in that
file's comments: fp64 throughout, np.longdouble for the tile-moment coefficients.  No device, no library: tests/test_group_restatement_cpu.py
holds the restated bounds against brute force, tests/test_group_stages_gpu.py holds the kernels against the restatement.

Conventions of kde_group.hip: a pool is a row list cut into R regions by the borders rb (region r = pool positions [rb[r], rb[r + 1]));
`vals` lists the pool positions in the pool's sorted order; a unit trains on the regions of `train_mask` and is tested on `test_region`,
both in the pool's order (a stable compaction).  W is the unit's whitening (row-major lower triangle, base-2 units: the kernel of a pair
is 2^(-|z_q - z_t|^2 / 2)), so every exponent and bound here is a base-2 logarithm."""
import math

import numpy as np

TILE = 16
MOM_ORDER = 8          # PBN_MOM_ORDER
LN2 = math.log(2.0)


def region_of(rb, R, pos):
    """Largest r < R with rb[r] <= pos (region_of in kde_group.hip)."""
    return np.searchsorted(np.asarray(rb)[1:R], pos, side="right").astype(np.int64)


def orders(vals, rb, R, train_mask, test_region):
    """(training order, query order, qpos, reg): pool positions of the unit's training / test rows in the pool's order, per query the number
    of the unit's training rows before it in that order, and the region of every sorted element."""
    vals = np.asarray(vals, dtype=np.int64)
    reg = region_of(rb, R, vals)
    in_train = np.array([(int(train_mask) >> r) & 1 for r in range(R)], dtype=bool)[reg]
    is_q = reg == test_region
    before = np.cumsum(in_train) - in_train          # training rows strictly before each element
    return vals[in_train], vals[is_q], before[is_q].astype(np.int64), reg


def whiten(x, W, mu, d):
    """z = W (x - mu), W the d x d lower triangle stored row-major."""
    Wm = np.tril(np.asarray(W, dtype=np.float64)[:d * d].reshape(d, d))
    return (np.asarray(x, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[:d]) @ Wm.T


def whiten_scale(x, W, mu, d):
    """sum_j |W_ij| |x_j - mu_j| per coordinate: the magnitude the rounding of z is measured against."""
    Wm = np.abs(np.tril(np.asarray(W, dtype=np.float64)[:d * d].reshape(d, d)))
    return np.abs(np.asarray(x, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[:d]) @ Wm.T


def tile_boxes(z, kd):
    """[tiles][2 kd]: per 16-row tile the minima, then the maxima, of the first kd coordinates over the tile's REAL rows."""
    n = len(z)
    nt = (n + TILE - 1) // TILE
    out = np.empty((nt, 2 * kd))
    for t in range(nt):
        rows = z[t * TILE:min(n, (t + 1) * TILE), :kd]
        out[t, :kd] = rows.min(0)
        out[t, kd:] = rows.max(0)
    return out


def batch_boxes(box, kd, tps):
    """[nsplit * nbps][2 kd]: batch k of split s covers the tiles [s tps + 64 k, min(s tps + 64 (k + 1), (s + 1) tps, ntiles)); an empty
    batch keeps (+inf, -inf)."""
    nt = len(box)
    nsplit = (nt + tps - 1) // tps
    nbps = (tps + 63) // 64
    out = np.empty((nsplit * nbps, 2 * kd))
    out[:, :kd] = np.inf
    out[:, kd:] = -np.inf
    for s in range(nsplit):
        t1 = min(s * tps + tps, nt)
        for k in range(nbps):
            a = s * tps + 64 * k
            b = min(a + 64, t1)
            if a < b:
                out[s * nbps + k, :kd] = box[a:b, :kd].min(0)
                out[s * nbps + k, kd:] = box[a:b, kd:].max(0)
    return out


def _logsumexp2(e):
    m = e.max()
    return m, m + math.log2(float(np.exp2(e - m).sum()))


def bounds(zs, zq, qpos, kd, window, tile_window, use_sum_bound=True, box=None):
    """(qlb [nqtiles 16], qthr [nqtiles]) of group_prepass_kernel.  Per query: the exact exponents of the training rows
    [qpos - window, qpos + window) give its largest one (qlb) and, with use_sum_bound, their log2 sum (else the largest); a tile's threshold
    is the smallest over its valid queries.  With tile_window > 0, use_sum_bound and boxes over every dimension: the FULL training tiles
    (all 16 rows real: t < N >> 4) within tile_window tiles of the tile of the first query's position each add 16 terms of at least
    2^(-maxdist(query box, tile box)^2 / 2); their log2 sum replaces the threshold where it is larger, the largest single exponent raises qlb."""
    N, d = zs.shape
    nq = len(zq)
    nqt = (nq + TILE - 1) // TILE
    qlb = np.full(nqt * TILE, -np.inf)
    rowsum = np.full(nq, -np.inf)
    for q in range(nq):
        b, e = max(int(qpos[q]) - window, 0), min(int(qpos[q]) + window, N)
        if e > b:
            ex = -0.5 * ((zs[b:e] - zq[q]) ** 2).sum(1)
            qlb[q], s = _logsumexp2(ex)
            rowsum[q] = s if use_sum_bound else qlb[q]
    qthr = np.empty(nqt)
    if box is None:
        box = tile_boxes(zs, kd)
    full = N >> 4
    for t in range(nqt):
        a, b = t * TILE, min(nq, (t + 1) * TILE)
        qthr[t] = rowsum[a:b].min()
        if tile_window > 0 and use_sum_bound and kd == d:
            lob, hib = zq[a:b, :kd].min(0), zq[a:b, :kd].max(0)
            tt = int(qpos[a]) >> 4
            t_lo, t_hi = max(tt - tile_window, 0), min(tt + tile_window, full)
            if t_hi > t_lo:
                far = np.maximum(box[t_lo:t_hi, kd:] - lob, hib - box[t_lo:t_hi, :kd])
                bmax, s = _logsumexp2(-0.5 * (far ** 2).sum(1))
                qthr[t] = max(qthr[t], s + 4.0)
                qlb[a:b] = np.maximum(qlb[a:b], bmax)
    return qlb, qthr


def query_boxes(zq, kd):
    return tile_boxes(zq, kd)


def true_exponents(zs, zq):
    """[nq][N] exponents -|z_q - z_t|^2 / 2, by brute force."""
    return -0.5 * ((zq[:, None, :] - zs[None, :, :]) ** 2).sum(2)


def true_max_exponent(zs, zq):
    out = np.empty(len(zq))
    for i in range(0, len(zq), 128):
        out[i:i + 128] = true_exponents(zs, zq[i:i + 128]).max(1)
    return out


def true_log2_sums(zs, zq):
    """log2 sum_t 2^(-|z_q - z_t|^2 / 2) over ALL training rows."""
    out = np.empty(len(zq))
    for i in range(0, len(zq), 128):
        e = true_exponents(zs, zq[i:i + 128])
        m = e.max(1)
        out[i:i + 128] = m + np.log2(np.exp2(e - m[:, None]).sum(1))
    return out


def bound_slack(N, d, exponent):
    """Rounding slack of `bound <= truth` for an exponent (or log2 sum) of the given magnitude: both sides round their squared distances
    (d + 1 operations, relative 2^-53 each) and their sum of up to N terms: (d + 3) ulps of the exponent's magnitude on either side plus
    log2(1 + N eps) for the sum, doubled for the two sides; 2^-52 absolute for log2 near 0."""
    eps = 2.0 ** -53
    return 2.0 * ((d + 3) * eps * np.abs(exponent) + math.log2(1.0 + N * eps)) + 2.0 ** -52


def tile_moments(zs, centroids=None):
    """(centroids [tiles][d], rho2 [tiles], coefficients [tiles][coefs] in np.longdouble, scales [tiles][coefs]) for d = 1, 2.
    c = mean of the tile's real rows; rho^2 = max_t |z_t - c|^2; C_alpha = a^|alpha| / alpha! sum_t 2^(-|delta_t|^2 / 2) delta_t^alpha with
    a = ln 2, delta_t = z_t - c, in the order group_tile_moments_kernel stores them (d = 1: i = 8 .. 0; d = 2: j = 8 .. 0 outer, i = 8 - j .. 0
    inner, alpha = (i, j)).  `centroids`, where given, replaces the means in delta (the coefficients about the kernel's own centroid);
    scales is the same sum over absolute values (what the rounding of a coefficient is measured against)."""
    LD = np.longdouble
    N, d = zs.shape
    assert d in (1, 2)
    nt = (N + TILE - 1) // TILE
    alphas = [(i, 0) for i in range(MOM_ORDER, -1, -1)] if d == 1 else \
             [(i, j) for j in range(MOM_ORDER, -1, -1) for i in range(MOM_ORDER - j, -1, -1)]
    a = np.log(LD(2))
    cen = np.empty((nt, d))
    rho2 = np.empty(nt)
    coef = np.empty((nt, len(alphas)), dtype=LD)
    scale = np.empty((nt, len(alphas)), dtype=LD)
    for t in range(nt):
        rows = zs[t * TILE:min(N, (t + 1) * TILE)].astype(LD)
        c = rows.mean(0)
        cen[t] = c.astype(np.float64)
        rho2[t] = float((((rows - c) ** 2).sum(1)).max())
        dl = rows - (c if centroids is None else np.asarray(centroids[t], dtype=LD))
        w = np.exp2(-(dl ** 2).sum(1) / LD(2))
        for k, (i, j) in enumerate(alphas):
            term = w * dl[:, 0] ** i * (dl[:, d - 1] ** j if d == 2 else LD(1))
            f = a ** (i + j) / LD(math.factorial(i) * math.factorial(j))
            coef[t, k] = term.sum() * f
            scale[t, k] = np.abs(term).sum() * f
    return cen, rho2, coef, scale


def merge_partials(part, lognorm):
    """group_finish_kernel: part [rows][queries][2] pairs (o, s) standing for s 2^o -> per query lognorm + ln 2 (m + log2 sum s 2^(o - m))."""
    o, s = part[:, :, 0], part[:, :, 1]
    m = o.max(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        tot = (s * np.exp2(o - m[None, :])).sum(0)
        return lognorm + LN2 * (m + np.log2(tot))


def restate(rows, rb, R, vals, train_mask, test_region, W, mu, d, kd, window, tile_window, tps, use_sum_bound=True):
    """Everything the prepass leaves for one unit, from the pool's rows (pool-position order) and its sorted order."""
    tr, qu, qpos, reg = orders(vals, rb, R, train_mask, test_region)
    zs, zq = whiten(rows[tr], W, mu, d), whiten(rows[qu], W, mu, d)
    box = tile_boxes(zs, kd)
    qlb, qthr = bounds(zs, zq, qpos, kd, window, tile_window, use_sum_bound, box)
    out = dict(train=tr, query=qu, qpos=qpos, reg=reg, zs=zs, zq=zq, box=box, bbox=batch_boxes(box, kd, tps), qbox=query_boxes(zq, kd),
               qlb=qlb, qthr=qthr)
    if d <= 2:
        out["centroid"], out["rho2"], out["coef"], out["coef_scale"] = tile_moments(zs)
    return out
