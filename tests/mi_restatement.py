"""Plain numpy restatement of what hybrid MutualInformation's moment kernels compute (tests/test_mi_shapes_gpu.py): per configuration of
a plan's discrete variables the count, the sums and the upper-triangle products of the shifted continuous columns.  Shares nothing with
the library or oracle/: integers are added in int64, real values in np.longdouble.  The launch arithmetic of csrc/mi.hip that the test
predicts (piece counts, the aligned / plain launch order, the LDS windows of the legacy kernel) is restated here as host formulas."""
import numpy as np

MI_SORTED_ROWS = 4096        # csrc/mi.hip: rows of one piece of a configuration


def keys(codes, cards):
    """Configuration id per row, the first variable the fastest index; -1 where any code is -1 (a null category).  codes: [m][n]."""
    n = codes[0].shape[0] if len(codes) else 0
    key = np.zeros(n, dtype=np.int64)
    ok = np.ones(n, dtype=bool)
    stride = 1
    for c, k in zip(codes, cards):
        ok &= c >= 0
        key += c.astype(np.int64) * stride
        stride *= int(k)
    key[~ok] = -1
    return key, stride


def layout(count, S, P):
    """[G][1 + c + c (c + 1) / 2]: count, sums, products for i <= j (row-major upper triangle)."""
    c = S.shape[1]
    iu = np.triu_indices(c)
    return np.concatenate([count[:, None].astype(S.dtype), S, P[:, iu[0], iu[1]]], axis=1)


def segments(key, G):
    """Stable order of the rows with key >= 0 by key, and the [G + 1] bounds of the configurations in it."""
    rows = np.flatnonzero(key >= 0)
    order = rows[np.argsort(key[rows], kind="stable")]
    count = np.bincount(key[rows], minlength=G)
    return order, np.concatenate([[0], np.cumsum(count)]), count


def int_moments(X, key, G):
    """X: [n][c] int64 (already shifted); rows with key < 0 or, for a masked array's mask, dropped by the caller.  Returns count [G],
    S [G][c], P [G][c][c] in int64."""
    assert X.dtype == np.int64
    order, b, count = segments(key, G)
    c = X.shape[1]
    S = np.zeros((G, c), dtype=np.int64)
    P = np.zeros((G, c, c), dtype=np.int64)
    Xs = X[order]
    np.add.at(S, np.repeat(np.arange(G), count), Xs)
    for g in np.flatnonzero(count):
        seg = Xs[b[g]:b[g + 1]]
        P[g] = seg.T @ seg
    return count.astype(np.int64), S, P


def pool(count, S, P, index, G):
    """Moments of a coarser grouping: fine configuration f belongs to index[f] (additivity; int64 adds are exact)."""
    c2, S2, P2 = np.zeros(G, dtype=count.dtype), np.zeros((G,) + S.shape[1:], dtype=S.dtype), np.zeros((G,) + P.shape[1:], dtype=P.dtype)
    np.add.at(c2, index, count)
    np.add.at(S2, index, S)
    np.add.at(P2, index, P)
    return c2, S2, P2


def real_moments(X, key, G):
    """X: [n][c] float64, the rounded x - shift.  Products and sums in np.longdouble; also the bound's magnitudes in float64:
    returns count, S, P (longdouble) and aS = sum |x_i|, aP = sum |x_i x_j| per configuration."""
    order, b, count = segments(key, G)
    c = X.shape[1]
    S = np.zeros((G, c), dtype=np.longdouble)
    P = np.zeros((G, c, c), dtype=np.longdouble)
    aS = np.zeros((G, c))
    aP = np.zeros((G, c, c))
    Xs = X[order]
    for g in np.flatnonzero(count):
        seg = Xs[b[g]:b[g + 1]]
        segl = seg.astype(np.longdouble)
        S[g] = segl.sum(axis=0)
        P[g] = segl.T @ segl
        a = np.abs(seg)
        aS[g] = a.sum(axis=0)
        aP[g] = a.T @ a
    return count.astype(np.int64), S, P, aS, aP


# ---- launch arithmetic of csrc/mi.hip -----------------------------------------------------------------------------------------------
def pieces(count):
    """Pieces of at most MI_SORTED_ROWS rows per configuration (Engine::group_for's block table)."""
    return [(int(n) + MI_SORTED_ROWS - 1) // MI_SORTED_ROWS for n in count]


def gram_launch(count):
    """Engine::ensure_full's launch order for a grouping with these configuration sizes: (order, launched blocks, nblk) with order 2 =
    the partial slots' own (one configuration), 1 = stripe-major aligned in groups of 8 stripes with padding, 0 = plain stripe-major."""
    P = pieces(count)
    nblk = sum(P)
    if len(P) <= 1:
        return 2, nblk, nblk
    T = max(1, max(P))
    cell = [0] * T
    for p in P:
        for pc in range(p):
            cell[((2 * pc + 1) * T) // (2 * p)] += 1
    cells = sum(8 * max(cell[s0:s0 + 8]) for s0 in range(0, T, 8))
    if cells <= 2 * nblk + 64:
        return 1, cells, nblk
    return 0, nblk, nblk


def legacy_window(c):
    """Plan::max_window: configurations whose LDS accumulators fit 60 KB beside the 64-row staging area."""
    stats = 1 + c + c * (c + 1) // 2
    fixed = 64 * (c + 1) * 8 + 64 * 4 + 2 * stats + 16
    return (60 * 1024 - fixed) // (stats * 8)


def legacy_launch(n, rows):
    """group_stats_device: (nblocks, chunks_per_block) of a launch of `rows` grid rows over n table rows."""
    chunks = (n + 63) // 64
    nblocks = min(chunks, 512 if rows >= 8 else (2048 if rows >= 2 else 4096))
    return nblocks, (chunks + nblocks - 1) // nblocks
