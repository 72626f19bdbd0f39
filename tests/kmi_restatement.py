"""numpy restatement of the k-nearest-neighbour conditional mutual information (learning/independences/continuous/
mutual_information.{hpp,cpp}: KMutualInformation) by brute force, for the tests.

It works on the integer ordinal ranks R (N x dims, columns [x, y, z...]) that the library took - tie order among equal values is the
sorting routine's, so the ranks are an input here and have tests of their own - and states what the estimator needs of every row i:

    eps_i  the (k+1)-th smallest Chebyshev distance from row i to all rows, the row itself (distance 0) included;
    n_xz, n_yz, n_z  the rows j with |z_j - z_i| < eps_i in every conditioning column (and |x_j - x_i| < eps_i, resp. y), i included;

and the estimate from them with digamma(n) = H(n-1) - gamma on a harmonic table.  neighbor_distances is the reference of the conditional
shuffle's neighbour lists on the original double values.  Nothing under pybnesian_amd/ imports this file and it imports nothing of the
product or of its CPU checker: numpy only.
"""
import numpy as np

EULER = 0.57721566490153286060651209008240243


def _chunks(rows, n, dims, budget=1 << 25):
    """rows in blocks whose (block x n) distance matrices stay around `budget` entries."""
    step = max(1, budget // max(n, 1))
    for a in range(0, len(rows), step):
        yield rows[a:a + step]


def eps_counts(R, ks, rows=None):
    """R: integer ranks (N x dims), ks: iterable of k, rows: row indices (default: all).
    Returns {k: (eps[len(rows)], cnt[3, len(rows)] or None with two columns)}; cnt rows are n_xz, n_yz, n_z."""
    R = np.asarray(R)
    n, dims = R.shape
    assert np.array_equal(R, R.astype(np.int64)) and R.min() >= 0 and R.max() < n
    # the smallest signed type that holds every difference of two ranks
    R = R.astype(np.int16 if n <= 1 << 15 else np.int32)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    ks = sorted(set(int(k) for k in ks))
    assert ks and 1 <= ks[0] and ks[-1] < n
    out = {k: (np.empty(len(rows), np.int64), np.empty((3, len(rows)), np.int64) if dims > 2 else None) for k in ks}
    at = 0
    for blk in _chunks(rows, n, dims):
        dx = np.abs(R[blk, None, 0] - R[None, :, 0])
        dy = np.abs(R[blk, None, 1] - R[None, :, 1])
        dz = np.zeros_like(dx)
        for d in range(2, dims):
            np.maximum(dz, np.abs(R[blk, None, d] - R[None, :, d]), out=dz)
        dist = np.maximum(np.maximum(dx, dy), dz)
        kth = np.partition(dist, ks, axis=1)[:, ks]          # the row itself is the 0-th smallest
        for c, k in enumerate(ks):
            eps, cnt = out[k]
            e = kth[:, c:c + 1]
            eps[at:at + len(blk)] = e[:, 0]
            if cnt is not None:
                inz = dz < e
                cnt[0, at:at + len(blk)] = (inz & (dx < e)).sum(axis=1)
                cnt[1, at:at + len(blk)] = (inz & (dy < e)).sum(axis=1)
                cnt[2, at:at + len(blk)] = inz.sum(axis=1)
        at += len(blk)
    return out


def digamma_table(n):
    """psi[m] = digamma(m) for the integers 1 <= m <= n (psi[0] = -inf): H(m-1) - gamma, the harmonic numbers summed upwards."""
    h = np.concatenate(([0.0], np.cumsum(1.0 / np.arange(1, n + 1))))       # h[m] = H(m)
    psi = np.empty(n + 1)
    psi[0] = -np.inf
    psi[1:] = h[:-1] - EULER
    return psi


def _row_order_mean(terms):
    """The mean as mutual_information.cpp takes it: `res += term` row after row, then `res /= N`.  The estimate is psi(k) plus a mean of
    nearly the same size and opposite sign, so the order of summation shows in it: at 40 001 rows and k = 64 on columns that are monotone
    in each other (estimate 0.0158) numpy's pairwise sum and the row-order sum differ by 3.8e-12, 2.4e-10 of the value."""
    return np.cumsum(terms)[-1] / len(terms)


def mi_from_integers(R, k, eps, cnt):
    """The estimate from every row's integers.  Two columns: the marginal counts have a closed form on ranks (the ranks within eps of
    r on either side, clipped at the ends); otherwise the Frenzel-Pompe mean of digammas of the three counts."""
    R = np.asarray(R).astype(np.int64)
    n, dims = R.shape
    psi = digamma_table(n)
    eps = np.asarray(eps, dtype=np.int64)
    if dims == 2:
        nx = np.minimum(1 + R[:, 0], eps) + np.minimum(n - R[:, 0], eps) - 1
        ny = np.minimum(1 + R[:, 1], eps) + np.minimum(n - R[:, 1], eps) - 1
        return -_row_order_mean(psi[nx] + psi[ny]) + (psi[k] + psi[n])
    cnt = np.asarray(cnt, dtype=np.int64)
    return _row_order_mean(psi[cnt[2]] - psi[cnt[0]] - psi[cnt[1]]) + psi[k]


def mi(R, k):
    eps, cnt = eps_counts(R, [k])[k]
    return mi_from_integers(R, k, eps, cnt)


def chebyshev(Z, i, j):
    """Chebyshev distances (doubles: max of |differences|, no rounding beyond the subtraction's) from rows i to rows j of Z (N x nz);
    i and j broadcast against each other."""
    Z = np.asarray(Z, dtype=np.float64)
    return np.abs(Z[i] - Z[j]).max(axis=-1)


def neighbor_distances(Z, m, rows=None):
    """Per row, the sorted m smallest Chebyshev distances to all rows (the row itself, at 0, included): what the conditional shuffle's
    neighbour lists must realise, whichever rows realise it where distances tie."""
    Z = np.asarray(Z, dtype=np.float64)
    n = len(Z)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    out = np.empty((len(rows), m))
    at = 0
    for blk in _chunks(rows, n, Z.shape[1], budget=1 << 22):
        dist = np.zeros((len(blk), n))
        for d in range(Z.shape[1]):
            np.maximum(dist, np.abs(Z[blk, None, d] - Z[None, :, d]), out=dist)
        part = np.partition(dist, m - 1, axis=1)[:, :m]
        out[at:at + len(blk)] = np.sort(part, axis=1)
        at += len(blk)
    return out


def row_sample(R, axis, seed, edge=64, ends=4, random=128):
    """The rows a large table is held to brute force at: the first and last `edge` rows in row order, the rows at the `ends` lowest and
    highest ranks of column `axis` (the window form's one-sided walks) and `random` others."""
    R = np.asarray(R)
    n = len(R)
    rank = R[:, axis].astype(np.int64)
    at_rank = np.empty(n, np.int64)
    at_rank[rank] = np.arange(n)
    pick = np.concatenate((np.arange(edge), np.arange(n - edge, n), at_rank[:ends], at_rank[n - ends:],
                           np.random.default_rng(seed).choice(n, random, replace=False)))
    return np.unique(pick)
