"""Exact least squares for the tests of the double-double LinearGaussianCPD refit (csrc/lg_accurate.hip, csrc/lg_dd_solve.hpp).

The tables here hold only values xi * 2^-shift with xi an integer small enough for the table's dtype, so the data ARE integers up to a
power of two: the raw moments are computed in Python integers, the centred normal equations are solved in fractions.Fraction, and the
coefficients and the variance are rounded ONCE, to double, at the very end.  Whatever the conditioning, the result is the least-squares
solution of the data as the device reads them, to the last bit - a reference with no error of its own, unlike a QR (kappa * eps).

    exact_fit(xi, shift, keep=None)    beta (intercept first) and RSS / (n - p - 1) of column 0 on columns 1..p
    make_table(...)                    a table with the conditioning asked for, its integers, and the figures the bounds need
    beta_bound(kappa, m)               the bound of the issue that introduced these tests (derived there, not tuned)
    check_full_rank / check_dependent  the assertions that the CPU and the GPU tier share; `worst` collects error / bound per family

Nothing under pybnesian_amd/ imports this file and it imports nothing of the product or of its CPU checker: numpy and the standard
library only.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
DD = 2.0 ** -104


def _shifts(shift, d):
    s = np.broadcast_to(np.asarray(shift, dtype=np.int64), (d,))
    return [int(v) for v in s]


def _solve(A, b):
    """Gauss-Jordan on Fractions (A symmetric positive definite: no pivoting needed, a zero pivot is an error of the caller)."""
    k = len(b)
    M = [[Fraction(A[i][j]) for j in range(k)] + [Fraction(b[i])] for i in range(k)]
    for c in range(k):
        piv = M[c][c]
        if piv == 0:
            raise ZeroDivisionError("exact_fit: the kept parents are exactly dependent")
        for r in range(c + 1, k):
            if M[r][c] != 0:
                f = M[r][c] / piv
                M[r] = [a - f * t for a, t in zip(M[r], M[c])]
    x = [Fraction(0)] * k
    for c in range(k - 1, -1, -1):
        x[c] = (M[c][k] - sum(M[c][j] * x[j] for j in range(c + 1, k))) / M[c][c]
    return x


def exact_fit(xi, shift, keep=None):
    """xi: int64 (n, d), the data are xi[:, j] * 2^-shift[j] (shift a scalar or one per column).  Column 0 is the response, columns
    1..p the parents; keep: the parents (1-based column indices) that enter the fit, the others get coefficient 0 (default: all).
    Returns (beta[d], variance) with variance = RSS / (n - p - 1), p = d - 1 (inf when n <= p + 1), each rounded once to double."""
    xi = np.asarray(xi)
    assert xi.dtype == np.int64 and xi.ndim == 2
    n, d = xi.shape
    p = d - 1
    sh = _shifts(shift, d)
    keep = list(range(1, d)) if keep is None else [int(k) for k in keep]
    assert all(1 <= k <= p for k in keep) and len(set(keep)) == len(keep)
    X = xi.astype(object)
    G = X.T @ X                     # Python integers
    S = X.sum(axis=0)
    A = [[n * int(G[i, j]) - int(S[i]) * int(S[j]) for j in range(d)] for i in range(d)]   # n * centred SSE
    b = _solve([[A[i][j] for j in keep] for i in keep], [A[i][0] for i in keep]) if keep else []
    # back to the data's units: column j is xi_j 2^-s_j
    two = lambda e: Fraction(2) ** e
    beta = [Fraction(0)] * d
    for k, v in zip(keep, b):
        beta[k] = v * two(sh[k] - sh[0])
    beta[0] = (int(S[0]) - sum(v * int(S[k]) for k, v in zip(keep, b))) / Fraction(n) * two(-sh[0])
    rss = (A[0][0] - sum(v * A[k][0] for k, v in zip(keep, b))) / Fraction(n) * two(-2 * sh[0])
    assert rss >= 0
    variance = float(rss / (n - p - 1)) if n > p + 1 else float("inf")
    return np.array([float(v) for v in beta]), variance


class Table:
    """xi (n, d) int64, shift, data = xi * 2^-shift in `dtype` (exactly), kappa (the generator's 1 / noise ratio), m (largest
    |column mean| / sigma), dependent (the 1-based parent columns of the exact dependency, or ())."""

    def __init__(self, xi, shift, dtype, kappa, dependent, exact_moments=True):
        self.xi, self.shift, self.kappa, self.dependent = xi, int(shift), float(kappa), tuple(dependent)
        bits = 24 if np.dtype(dtype) == np.float32 else 53
        assert int(np.abs(xi).max()) < 2 ** bits, "the grid needs more bits than the dtype has"
        # and every raw moment, an integer below 2^104 in units of 2^-2shift, is exact in double-double in whatever order it is summed:
        # the tests measure the solve and the addressing, not the roundoff of the accumulation order (with more bits a sequential
        # double-double sum of n products rounds n times, ~sqrt(n) 2^-106 of the RAW moment, which no solve can undo)
        # (make_table(full_width=True) asks for the opposite, for the rank decision under that roundoff)
        assert (int(np.abs(xi).max()) ** 2 * len(xi) < 2 ** 104) == exact_moments, "raw moments: exact in double-double or not, as asked"
        self.data = np.ldexp(xi.astype(np.float64), -self.shift).astype(dtype)
        # every value survives the round trip through the table's dtype
        back = np.ldexp(self.data.astype(np.float64), self.shift)
        assert np.array_equal(back, xi.astype(np.float64)) and np.array_equal(back.astype(np.int64), xi)
        self.m = self.offset_ratio(np.arange(len(xi)))

    def offset_ratio(self, rows):
        x = np.ldexp(self.xi[rows].astype(np.float64), -self.shift)
        sd = x.std(axis=0)
        return float(np.max(np.abs(x.mean(axis=0)) / np.where(sd > 0, sd, 1.0)))

    def exact(self, rows=None, keep=None):
        return exact_fit(self.xi if rows is None else self.xi[np.asarray(rows)], self.shift, keep)


def make_table(seed, n, d, kappa=None, offset=0.0, resp_noise=0.5, dependency=None, dtype=np.float64, shift=None, full_width=False):
    """n rows of [y, x1..xp], p = d - 1: the parents are standard normals through a unit lower-triangular mixing matrix (off-diagonal
    0.3 N(0, 1)) plus `offset`; with kappa the LAST parent is a near copy of the first, x_p = x_1 + N(0, 1) / kappa; dependency = "sum":
    x_p = x_1 + x_2, "double": x_p = 2 x_1, on the integers, hence exact; y = X b + resp_noise N(0, 1), b uniform in [0.5, 1.5].
    Every value is rounded to the grid 2^-shift (default: the finest, 40 at the most, that leaves the integers inside the dtype and
    the raw moments of n rows inside double-double).  full_width: the parents fill the dtype's bits instead (y is scaled down to no
    more), so that the raw moments do NOT fit and their accumulation rounds."""
    rng = np.random.default_rng(seed)
    p = d - 1
    X = rng.normal(size=(n, p)) @ (np.eye(p) + 0.3 * np.tril(rng.normal(size=(p, p)), -1)).T + offset
    if kappa is not None:
        X[:, p - 1] = X[:, 0] + rng.normal(size=n) / kappa
    coef = rng.uniform(0.5, 1.5, size=p)
    if dependency is not None:
        coef[p - 1] = 0.0    # (the dependent column is rebuilt below; y must not need more bits than the parents)
    y = X @ coef + resp_noise * rng.normal(size=n)
    if np.dtype(dtype) == np.float32:
        # 24 bits: bring the response down to the parents' magnitude by a power of two (an exact scaling, the conditioning is untouched)
        y = np.ldexp(y, -max(0, int(np.ceil(np.log2(np.abs(y).max() / np.abs(X).max())))))
    if full_width:
        y /= 2 * p
    full = np.column_stack([y, X])
    bits = 24 if np.dtype(dtype) == np.float32 else 53
    if full_width:
        shift = bits - 2 - int(np.ceil(np.log2(np.abs(full).max())))
    elif shift is None:
        # x_p = x_1 + x_2 / 2 x_1 doubles the magnitude: one more bit of room; n xi^2 < 2^104 (see Table)
        room = min(bits - 2, (104 - int(np.ceil(np.log2(n)))) // 2 - 1)
        shift = min(40, room - int(np.ceil(np.log2(np.abs(full).max()))))
    xi = np.rint(np.ldexp(full, shift)).astype(np.int64)
    dependent = ()
    if dependency == "sum":
        assert p >= 3
        xi[:, p] = xi[:, 1] + xi[:, 2]
        dependent = (1, 2, p)
    elif dependency == "double":
        assert p >= 2
        xi[:, p] = 2 * xi[:, 1]
        dependent = (1, p)
    else:
        assert dependency is None
    return Table(xi, shift, dtype, 1.0 if kappa is None else kappa, dependent, exact_moments=not full_width)


def beta_bound(kappa, m):
    """Largest admissible max|beta - exact| / max|exact| (and relative error of the variance): 64 eps for the final roundings and the
    intercept's sum, 16 kappa^2 (1 + m^2) 2^-104 for the double-double roundoff after centring and the collinear solve."""
    return 64 * EPS + 16 * kappa ** 2 * (1 + m ** 2) * DD


def beta_bound_rounded_moments(kappa, m, n):
    """The same where the raw moments do not fit double-double: each is then the result of up to n roundings of 2^-106 of itself,
    n 2^-106 in place of the 2^-104 of the centring."""
    return 64 * EPS + 16 * kappa ** 2 * (1 + m ** 2) * max(DD, n * 2.0 ** -106)


def _variance_error(got, want):
    if want == np.inf:   # n <= p + 1
        assert got == np.inf
        return 0.0
    return abs(got - want) / want


def beta_error(got, want):
    return float(np.max(np.abs(np.asarray(got) - want)) / np.max(np.abs(want)))


def note(worst, family, ratio):
    worst[family] = max(worst.get(family, 0.0), ratio)


def check_full_rank(t, rank, variance, beta, worst, family):
    want_beta, want_var = t.exact()
    bound = beta_bound(t.kappa, t.m)
    e_beta, e_var = beta_error(beta, want_beta), _variance_error(variance, want_var)
    print(f"{family}: beta error {e_beta:.3g}, variance error {e_var:.3g}, bound {bound:.3g}, m {t.m:.4g}")
    note(worst, family, max(e_beta, e_var) / bound)
    assert rank == len(beta) - 1
    assert e_beta <= bound and e_var <= bound, (e_beta, e_var, bound)


def check_dependent(t, rank, variance, beta, worst, family, rounded_moments=False):
    """rank p - 1; exactly one member of the dependent set has coefficient exactly 0; the rest is the exact fit without it.  The bound is
    the full-rank one with kappa = the 2-norm condition number of the kept parents, centred and scaled to unit length (numpy, float64)."""
    p = len(beta) - 1
    assert rank == p - 1, (rank, beta)
    zero = [j for j in t.dependent if beta[j] == 0.0]
    assert len(zero) == 1, (t.dependent, beta)
    assert all(beta[j] != 0.0 for j in range(1, p + 1) if j != zero[0])
    keep = [j for j in range(1, p + 1) if j != zero[0]]
    want_beta, want_var = t.exact(keep=keep)
    x = t.data[:, keep].astype(np.float64)
    x = x - x.mean(axis=0)
    kappa = np.linalg.cond(x / np.linalg.norm(x, axis=0))
    bound = beta_bound_rounded_moments(kappa, t.m, len(x)) if rounded_moments else beta_bound(kappa, t.m)
    e_beta, e_var = beta_error(beta, want_beta), _variance_error(variance, want_var)
    print(f"{family}: beta error {e_beta:.3g}, variance error {e_var:.3g}, bound {bound:.3g}, m {t.m:.4g}")
    note(worst, family, max(e_beta, e_var) / bound)
    assert e_beta <= bound and e_var <= bound, (e_beta, e_var, bound)
