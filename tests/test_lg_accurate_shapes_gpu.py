"""GPU tier: the double-double LinearGaussianCPD refit (csrc/lg_accurate.hip) at every launch shape, addressing form and trigger, against
exact rational least squares (tests/lg_exact.py).

gram_dd_kernel tiles the d columns into groups of four - grid (blocks, group pairs I <= J), 256 rows per block and trip, at most 128
blocks - and addresses its rows as one or two ranges, directly or through a device row list.  The test aid pbn_debug_lg_fit_accurate
(not in pbn_hip.h, bound here) calls lg_fit_accurate with any of these forms; the triggers go through pbn_lg_fit_table and the callers
through the Python scores.  The reference is always the exact fit of exactly the rows addressed, so a wrong tile-to-column map, a row
too many or too few at a range boundary, or a fit that was not refitted at all misses the bound
    beta, variance: 64 eps + 16 kappa^2 (1 + m^2) 2^-104        scores: 1e-10 relative
by orders of magnitude (the fp64 normal equations are off by 1e-6 ... 1 on these tables).  The tables keep their raw moments inside
double-double (lg_exact.Table): the sums are exact in any order, the grid-stride loop's as well as a sequential one's."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest

import lg_exact

pytestmark = pytest.mark.gpu

GRAM = 3          # pbn_kernel_class PBN_K_GRAM
SPLIT_CV = 1
WIDTH = 20        # columns of the device tables


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib(pbn):
    from pybnesian_amd import _lib

    L = _lib.load()
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    L.pbn_debug_lg_fit_accurate.restype = C.c_int
    L.pbn_debug_lg_fit_accurate.argtypes = [C.c_void_p, ip, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int64,
                                            dp, dp, ip]
    return L


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for family, ratio in sorted(w.items()):
        print(f"\nlg_accurate gpu {family}: worst error / bound = {ratio:.3g}")


class Dev:
    """A lg_exact.Table inside a WIDTH-column device table: data column j sits in table column pos[j], the other columns hold noise."""

    def __init__(self, lib, table, seed=0):
        from pybnesian_amd import _lib
        from pybnesian_amd.dataset import default_context

        self._lib, self.lib, self.table = _lib, lib, table
        n, d = table.data.shape
        rng = np.random.default_rng(1000 + seed)
        self.pos = [int(c) for c in 1 + rng.permutation(WIDTH - 1)[:d]]   # never column 0, in no particular order
        self.columns = [np.ascontiguousarray(rng.normal(size=n).astype(table.data.dtype)) for _ in range(WIDTH)]
        for j, c in enumerate(self.pos):
            self.columns[c] = np.ascontiguousarray(table.data[:, j])
        self.ctx = default_context()
        ptrs = (C.c_void_p * WIDTH)(*[a.ctypes.data for a in self.columns])
        h = C.c_void_p()
        dtype = _lib.PBN_F32 if table.data.dtype == np.float32 else _lib.PBN_F64
        _lib.check(lib.pbn_table_create(self.ctx.handle, ptrs, WIDTH, n, dtype, None, 0, C.byref(h)))
        self.h = h

    def close(self):
        self.lib.pbn_table_destroy(self.h)

    def cols(self, order=None):
        """table columns of data columns `order` (default: all, in order)"""
        return [self.pos[j] for j in (range(len(self.pos)) if order is None else order)]

    def refit(self, cols, row0, n0, row1, n, rows=None):
        d = len(cols)
        beta, var, rank = np.full(d, np.nan), C.c_double(np.nan), C.c_int(-1)
        rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        self._lib.check(self.lib.pbn_debug_lg_fit_accurate(self.h, self._lib.int_array(cols), d, row0, n0, row1, n,
                                                          None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          0 if rows is None else len(rows), beta.ctypes.data_as(C.POINTER(C.c_double)),
                                                          C.byref(var), C.byref(rank)))
        return rank.value, var.value, beta

    def fit_table(self, cols, row0, n):
        d = len(cols)
        beta, var = np.full(d, np.nan), C.c_double(np.nan)
        self._lib.check(self.lib.pbn_lg_fit_table(self.h, self._lib.int_array(cols), d, row0, n, beta.ctypes.data_as(C.POINTER(C.c_double)), C.byref(var)))
        return var.value, beta


class Rows:
    """a lg_exact.Table restricted to (and ordered by) some of its rows - what the checks of lg_exact need of a table"""

    def __init__(self, table, rows, order=None):
        self.xi = table.xi[np.asarray(rows)]
        if order is not None:
            self.xi = self.xi[:, order]
        self.shift, self.kappa, self.dependent = table.shift, table.kappa, table.dependent
        self.data = np.ldexp(self.xi.astype(np.float64), -self.shift)
        sd = self.data.std(axis=0)
        self.m = float(np.max(np.abs(self.data.mean(axis=0)) / np.where(sd > 0, sd, 1.0)))

    def exact(self, rows=None, keep=None):
        assert rows is None
        return lg_exact.exact_fit(self.xi, self.shift, keep)


# ---- tile map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", [4, 5, 8, 9, 13, 16])
def test_tile_map(lib, worst, d, dtype):
    """1, 2, 2, 3, 4, 4 column groups (1, 3, 3, 6, 10, 10 tiles); d = 5, 9, 13 leave one live column in the last group.  The variable is
    not table column 0 and the parents are passed in a shuffled order.  fp32: kappa = 3e5 on the grid 2^-19 (24 bits)."""
    n = 3000
    if dtype == "float64":
        t = lg_exact.make_table(40 + d, n, d, kappa=1e7, offset=5)
    else:
        t = lg_exact.make_table(40 + d, n, d, kappa=3e5, offset=0, dtype=np.float32, shift=19)
    dev = Dev(lib, t, seed=d)
    try:
        order = [0] + [int(j) for j in 1 + np.random.default_rng(d).permutation(d - 1)]
        rank, var, beta = dev.refit(dev.cols(order), 0, n, 0, n)
    finally:
        dev.close()
    lg_exact.check_full_rank(Rows(t, np.arange(n), order), rank, var, beta, worst, f"tile map {dtype}")


# ---- row counts ----------------------------------------------------------------------------------------------------------------------
ROW_COUNTS = [5, 6, 7, 255, 256, 257, 32768, 32769, 40001]
ROW0 = [0, 1, 4097]


@pytest.fixture(scope="module")
def long_table(lib):
    t = lg_exact.make_table(11, ROW0[-1] + ROW_COUNTS[-1], 5, offset=50, dependency="sum")
    dev = Dev(lib, t, seed=1)
    yield t, dev
    dev.close()


@pytest.mark.parametrize("row0", ROW0)
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts(long_table, worst, n, row0):
    """d = 5 with the exactly dependent column last (x4 = x1 + x2, means at 50 sigma), one range [row0, row0 + n): n = d the variance =
    +inf branch (n <= p + 1), d + 1 and d + 2 the smallest fits, 255 / 256 / 257 one block and its boundary, 32768 exactly 128 full
    blocks, 32769 and 40001 the grid-stride second trip."""
    t, dev = long_table
    rank, var, beta = dev.refit(dev.cols(), row0, n, 0, n)
    sub = Rows(t, np.arange(row0, row0 + n))
    assert (var == np.inf) == (n == 5)
    lg_exact.check_dependent(sub, rank, var, beta, worst, "row counts")


# ---- addressing forms ----------------------------------------------------------------------------------------------------------------
N_ADDR, N_USED = 1500, 700


@pytest.fixture(scope="module", params=[5, 9])
def addr_table(lib, request):
    d = request.param
    t = lg_exact.make_table(70 + d, N_ADDR, d, kappa=1e7, offset=5)
    dev = Dev(lib, t, seed=20 + d)
    yield t, dev
    dev.close()


def _shuffled(seed, count):
    return np.random.default_rng(seed).permutation(N_ADDR)[:count].astype(np.int32)


ADDRESSING = {
    # name: (row0, n0, row1, row list or None)   logical row r < N_USED is r < n0 ? row0 + r : row1 + r - n0
    "two ranges, first empty": (3, 0, 411, None),
    "two ranges": (100, 300, 600, None),
    "two ranges, second empty at the table's end": (100, N_USED, N_ADDR, None),
    "row list at base 0": (0, N_USED, 0, _shuffled(1, N_USED)),
    "row list at base 200": (200, N_USED, 0, _shuffled(2, 900)),
    "row list and two ranges": (50, 250, 450, _shuffled(3, 1000)),
    "row list and two ranges, second empty at the list's end": (300, N_USED, 1000, _shuffled(4, 1000)),
}


@pytest.mark.parametrize("form", list(ADDRESSING))
def test_addressing_forms(addr_table, worst, form):
    """The forms the seven call sites use: two ranges around a fold (first fold: n0 = 0, last fold: the second range is empty and begins
    where the region ends), a row list from its start and from a base (a configuration's block of the grouped list), and a list with two
    ranges (a configuration's rows around its own fold).  The reference is the exact fit of exactly the rows addressed."""
    t, dev = addr_table
    row0, n0, row1, rows = ADDRESSING[form]
    logical = np.concatenate([np.arange(row0, row0 + n0), np.arange(row1, row1 + N_USED - n0)])
    assert len(logical) == N_USED
    source = logical if rows is None else rows[logical]
    rank, var, beta = dev.refit(dev.cols(), row0, n0, row1, N_USED, rows)
    lg_exact.check_full_rank(Rows(t, source), rank, var, beta, worst, "addressing")


# ---- triggers ------------------------------------------------------------------------------------------------------------------------
def _gram_launches(dev, call):
    dev.ctx.set_profiling(2)
    try:
        out = call()
        return out, dev.ctx.kernel_time(GRAM)[1]
    finally:
        dev.ctx.set_profiling(0)


@pytest.mark.parametrize("case", ["kappa 1e4", "near-exact fit", "control"])
def test_triggers_through_lg_fit_table(lib, worst, case):
    """pbn_lg_fit_table: one Gram launch for the fp64 moments, and a second one - gram_dd_kernel - exactly where lg_fit marks the fit
    suspect: nearly collinear parents (smallest pivot ratio 1e-8 < 1e-6) and a nearly exact fit (RSS < 1e-8 SSE_y), not the
    well-conditioned control."""
    n, d = 3000, 6
    t = {"kappa 1e4": lambda: lg_exact.make_table(5, n, d, kappa=1e4, offset=5),
         "near-exact fit": lambda: lg_exact.make_table(6, n, d, offset=5, resp_noise=1e-5),
         "control": lambda: lg_exact.make_table(7, n, d, offset=5)}[case]()
    dev = Dev(lib, t, seed=3)
    try:
        (var, beta), launches = _gram_launches(dev, lambda: dev.fit_table(dev.cols(), 0, n))
    finally:
        dev.close()
    assert launches == (1 if case == "control" else 2), launches
    if case == "control":
        want_beta, want_var = t.exact()
        assert np.allclose(beta, want_beta, rtol=1e-9, atol=1e-9 * np.abs(want_beta).max()) and np.isclose(var, want_var, rtol=1e-9)
    else:
        lg_exact.check_full_rank(t, d - 1, var, beta, worst, "triggers")


def test_sixteen_parents_are_not_refitted(lib):
    """d = 17 with the nearly collinear parents of the trigger cases above (kappa = 1e4): the refit holds at most 15 parents (DD_MAX_D =
    16 columns), so the fp64 normal equations' answer stands - one Gram launch, a finite beta, and a variance within 1e-6 relative of
    the exact one.  This is the documented limit of the refit, not an accuracy claim: the error of that variance grows with kappa, and
    the same table at kappa = 1e7 - printed, not asserted - was 2.5e-6 off when this test was written, above the 1e-6 parity bar that
    the refit keeps for up to 15 parents."""
    n, d = 3000, 17
    errors = {}
    for kappa in (1e4, 1e7):
        t = lg_exact.make_table(8, n, d, kappa=kappa, offset=5)
        dev = Dev(lib, t, seed=4)
        try:
            (var, beta), launches = _gram_launches(dev, lambda: dev.fit_table(dev.cols(), 0, n))
        finally:
            dev.close()
        want_var = t.exact()[1]
        errors[kappa] = abs(var - want_var) / want_var
        print(f"d = 17, kappa = {kappa:g}: variance error {errors[kappa]:.3g}")
        assert launches == 1 and np.all(np.isfinite(beta)) and np.isfinite(var)
    assert errors[1e4] <= 1e-6


# ---- exact dependencies on the device -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("offset", [0, 1000])
@pytest.mark.parametrize("kind", ["sum", "double"])
def test_exact_dependency_on_the_device(lib, worst, kind, offset, seed):
    """The cases of the CPU tier at p = 4 with the moments from gram_dd_kernel: rank p - 1, one coefficient of the dependent set exactly 0."""
    p, n = 4, 2000
    t = lg_exact.make_table(1000 * seed + 10 * p + offset, n, p + 1, offset=offset, dependency=kind)
    dev = Dev(lib, t, seed=seed)
    try:
        rank, var, beta = dev.refit(dev.cols(), 0, n, 0, n)
    finally:
        dev.close()
    lg_exact.check_dependent(t, rank, var, beta, worst, "dependent")


# ---- callers -------------------------------------------------------------------------------------------------------------------------
def _logl(xi, shift, rows, beta, var):
    """sum of log N(y | beta0 + beta . x, var) over `rows`, residuals in long double"""
    x = np.ldexp(xi[rows].astype(np.longdouble), -shift)
    r = x[:, 0] - np.longdouble(beta[0]) - x[:, 1:] @ beta[1:].astype(np.longdouble)
    return float(-0.5 * len(rows) * np.log(2 * np.pi * np.longdouble(var)) - 0.5 * (r * r).sum() / np.longdouble(var))


def _bic_term(n, p, var):
    return 0.5 * (1 + p - n) - 0.5 * n * math.log(2 * math.pi) - 0.5 * n * math.log(var)


def _frame(t, extra=None):
    names = ["y"] + [f"x{j}" for j in range(1, t.data.shape[1])]
    df = pd.DataFrame({c: t.data[:, j].astype(np.float64) for j, c in enumerate(names)})
    for k, v in (extra or {}).items():
        df[k] = v
    return df, names


def _folds(lib, n, k, seed):
    from pybnesian_amd import _lib

    perm, limits = np.zeros(n, dtype=np.int32), np.zeros(k + 1, dtype=np.int32)
    n_cv, n_hold = C.c_int64(0), C.c_int64(0)
    _lib.check(lib.pbn_split_layout(n, SPLIT_CV, k, C.c_uint32(seed), 0.0, perm.ctypes.data, limits.ctypes.data, C.byref(n_cv), C.byref(n_hold)))
    assert n_cv.value == n and limits[0] == 0 and limits[-1] == n
    return [(np.concatenate([perm[:limits[f]], perm[limits[f + 1]:]]), perm[limits[f]: limits[f + 1]]) for f in range(k)]


def _score_ratio(worst, family, got, want):
    err = abs(got - want) / abs(want)
    print(f"{family}: got {got!r}, want {want!r}, relative error {err:.3g}")
    worst[family] = max(worst.get(family, 0.0), err / 1e-10)
    return err


def test_cv_likelihood_passes_the_train_rows_of_each_fold(pbn, lib, worst):
    """CVLikelihood at n = 403, k = 3 (folds of 135, 134, 134 rows, layout from pbn_split_layout) with kappa = 1e7 parents: per fold the
    exact fit of its train rows - two ranges around the fold - and the log-likelihood of its test rows."""
    n, k, seed = 403, 3, 5
    t = lg_exact.make_table(90, n, 5, kappa=1e7, offset=0)
    df, names = _frame(t)
    folds = _folds(lib, n, k, seed)
    assert sorted(len(te) for _, te in folds) == [134, 134, 135]
    want = 0.0
    for tr, te in folds:
        beta, var = t.exact(rows=tr)
        want += _logl(t.xi, t.shift, te, beta, var)
    got = pbn.CVLikelihood(df, k, seed).local_score(pbn.GaussianNetwork(names), "y", names[1:])
    assert _score_ratio(worst, "callers", got, want) <= 1e-10


def test_cpd_fit_and_bic_over_all_rows(pbn, worst):
    """LinearGaussianCPD.fit and BIC without nulls: one range, all rows."""
    n, p = 600, 4
    t = lg_exact.make_table(93, n, 5, kappa=1e7, offset=0)
    df, names = _frame(t)
    cpd = pbn.LinearGaussianCPD("y", names[1:])
    cpd.fit(df)
    lg_exact.check_full_rank(t, p, float(cpd.variance), np.asarray(cpd.beta, dtype=np.float64), worst, "callers, fit")
    want = _bic_term(n, p, t.exact()[1]) - math.log(n) * 0.5 * (p + 2)
    got = pbn.BIC(df).local_score(pbn.GaussianNetwork(names), "y", names[1:])
    assert _score_ratio(worst, "callers", got, want) <= 1e-10


def test_bic_with_nulls_passes_the_gathered_valid_rows(pbn, worst):
    """BIC on a table with nulls in the variable and in a parent: the refit reads the rows valid in all of the candidate's columns through
    the gather list."""
    n = 600
    t = lg_exact.make_table(91, n, 5, kappa=1e7, offset=0)
    df, names = _frame(t)
    rng = np.random.default_rng(2)
    null_y, null_x = rng.random(n) < 0.1, rng.random(n) < 0.1
    df.loc[null_y, "y"] = np.nan
    df.loc[null_x, "x2"] = np.nan
    valid = np.nonzero(~(null_y | null_x))[0]
    assert 400 < len(valid) < n - 60
    beta, var = t.exact(rows=valid)
    nv, p = len(valid), 4
    want = _bic_term(nv, p, var) - math.log(nv) * 0.5 * (p + 2)
    got = pbn.BIC(df).local_score(pbn.GaussianNetwork(names), "y", names[1:])
    assert _score_ratio(worst, "callers", got, want) <= 1e-10


def test_clg_candidate_passes_the_rows_of_each_configuration(pbn, lib, worst):
    """A CLG candidate with one discrete parent of two uneven configurations (about 30 / 70 %): BIC reads each configuration's block of the
    grouped row list (a list at a base), CVLikelihood each configuration's train rows around its own fold (a list and two ranges)."""
    n, k, seed, p = 601, 3, 7, 4
    t = lg_exact.make_table(92, n, 5, kappa=1e7, offset=0)
    a = (np.random.default_rng(3).random(n) < 0.7).astype(np.int32)
    df, names = _frame(t, {"A": pd.Categorical.from_codes(a, ["a0", "a1"])})
    assert 150 < (a == 0).sum() < 210
    want = 0.0
    for c in (0, 1):
        rows = np.nonzero(a == c)[0]
        want += _bic_term(len(rows), p, t.exact(rows=rows)[1])
    want -= math.log(n) * 0.5 * 2 * (p + 2)
    net = pbn.CLGNetwork(list(df.columns), [], [("A", pbn.DiscreteFactorType())])
    got = pbn.BIC(df).local_score(net, "y", ["A"] + names[1:])
    assert _score_ratio(worst, "callers", got, want) <= 1e-10
    want = 0.0
    for tr, te in _folds(lib, n, k, seed):
        for c in (0, 1):
            beta, var = t.exact(rows=tr[a[tr] == c])
            want += _logl(t.xi, t.shift, te[a[te] == c], beta, var)
    spbn = pbn.SemiparametricBN(list(df.columns), [], [("A", pbn.DiscreteFactorType())])
    got = pbn.CVLikelihood(df, k, seed).local_score_node_type(spbn, pbn.LinearGaussianCPDType(), "y", ["A"] + names[1:])
    assert _score_ratio(worst, "callers", got, want) <= 1e-10
