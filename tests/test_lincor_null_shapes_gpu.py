"""GPU tier: the moments of LinearCorrelation's batch over tables with nulls (csrc/lincor_null_batch.hip) at every launch shape,
tolerance ZERO.

Tables of small integers (float64 and float32) with integer shifts set through pbn_mi_set_continuous_nulls: every count, sum and
product of x - shift is then an integer far below 2^53, so the clean part (one matrix-unit Gram of all columns over the rows without
a null), the dirty part (lincor_null_moments_kernel: TILE rows of all columns staged in LDS, one test per lane, slices added in order)
and their sum, read through the test aid pbn_debug_mi_lincor_moments, must EQUAL int64 numpy on the same row sets - dropna of the
test's columns, split by the clean mask.  Shapes: M = 2 ... 8; dirty rows 0, 1, TILE - 1, TILE, TILE + 1, one slice, one slice + 1; clean
rows 0, 1, many; 1, 63, 64, 65 and a workgroup chunk +- 1 tests per call; 2, 31, 32, 33 and the cap of columns, and at cap + 1 every
test a host test; a column that is null in every row; tests over columns that hold no null beside columns that do; rows whose one valid
cell holds +-1e300 (3e38 in float32) next to NaN cells, which the select has to keep out of every sum.

Determinism: a test's records and its p-value are functions of the table, the shifts and the test alone - bit-identical alone, and
first, last and in the middle of three different batches."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib

pytestmark = pytest.mark.gpu

_ip = C.POINTER(C.c_int)
TILE, CHUNK, NC_MAX, SLICE = 16, 256, 256, 256      # asserted against the library's own in shape()


def acc(m):
    return 1 + m + m * (m + 1) // 2


def _args(tests):
    v1, v2, off, cond = tests
    v1, v2, off = (np.ascontiguousarray(a, dtype=np.int32) for a in (v1, v2, off))
    cond = np.ascontiguousarray(cond if len(cond) else [0], dtype=np.int32)
    return len(v1), v1.ctypes.data_as(_ip), v2.ctypes.data_as(_ip), off.ctypes.data_as(_ip), cond.ctypes.data_as(_ip), (v1, v2, off, cond)


def null_batch(lc, tests):
    n, a, b, c, d, keep = _args(tests)
    out = np.full(n, -7.0)
    _lib.load().pbn_mi_lincor_pvalue_batch(lc._per_test._handle, n, a, b, c, d, _lib.dptr(out))
    return out


def null_scalar(lc, tests):
    lib = _lib.load()
    v1, v2, off, cond = tests
    cond = np.ascontiguousarray(cond if len(cond) else [0], dtype=np.int32)
    base = cond.ctypes.data
    return np.array([lib.pbn_mi_lincor_pvalue(lc._per_test._handle, int(v1[i]), int(v2[i]), int(off[i + 1] - off[i]), C.cast(base + 4 * int(off[i]), _ip))
                     for i in range(len(v1))])


def moments(lc, tests):
    """pbn_debug_mi_lincor_moments: per test (clean, dirty, sum) records, and the kernel's shape."""
    n, a, b, c, d, keep = _args(tests)
    off = keep[2]
    ms = (off[1:] - off[:-1]) + 2
    total = int(sum(3 * acc(int(m)) for m in ms))
    out = np.full(total + 1, -7.0)
    shape = (C.c_int64 * 5)()
    got = _lib.load().pbn_debug_mi_lincor_moments(lc._per_test._handle, n, a, b, c, d, _lib.dptr(out), total, shape)
    assert got == total, (got, total, _lib.load().pbn_last_error())
    assert out[total] == -7.0
    recs, pos = [], 0
    for m in ms:
        recs.append(out[pos:pos + 3 * acc(int(m))].reshape(3, acc(int(m))))
        pos += 3 * acc(int(m))
    return recs, list(shape)


def random_tests(rng, n_vars, ks):
    ks = np.asarray(ks, dtype=np.int64)
    sel = rng.permuted(np.tile(np.arange(n_vars, dtype=np.int32), (len(ks), 1)), axis=1)[:, :int(ks.max()) + 2]
    used = np.arange(sel.shape[1] - 2)[None, :] < ks[:, None]
    return sel[:, 0].copy(), sel[:, 1].copy(), np.concatenate([[0], np.cumsum(ks)]), sel[:, 2:][used]


def columns_of(tests, i):
    v1, v2, off, cond = tests
    return [int(v1[i]), int(v2[i])] + [int(c) for c in cond[off[i]:off[i + 1]]]


class IntTable:
    """n_dirty rows with a null somewhere and n_clean without, shuffled; values integers in [-20, 20], shifts integers in [-3, 3].
    keep_clean: columns 0 and 1 never hold a null.  all_null: column n_cont - 1 is null in every row (so no row is clean).  poison: in
    two dirty rows every cell is null but the one of column 2, which holds + / - the largest magnitude."""

    def __init__(self, dtype, n_cont, n_dirty, n_clean, seed, keep_clean=True, all_null=False, poison=False):
        rng = np.random.default_rng(seed)
        n = n_dirty + n_clean
        X = rng.integers(-20, 21, size=(n, n_cont)).astype(np.float64)
        dirty = np.zeros(n, dtype=bool)
        dirty[rng.permutation(n)[:n_dirty]] = True
        first = 2 if (keep_clean and n_cont > 2) else 0
        for r in np.nonzero(dirty)[0]:
            cols = np.nonzero(rng.random(n_cont - first) < 0.3)[0] + first
            if len(cols) == 0:
                cols = [first + int(rng.integers(0, n_cont - first))]
            X[r, cols] = np.nan
        if all_null:
            X[:, n_cont - 1] = np.nan
        if poison:
            big = 1e300 if dtype is np.float64 else 3e38
            rows = np.nonzero(dirty)[0][:2]
            assert len(rows) == 2 and n_cont > 3
            X[rows, :] = np.nan
            X[rows, 2] = [big, -big]
        self.X = X
        self.shift = rng.integers(-3, 4, size=n_cont).astype(np.float64)
        self.clean = ~np.isnan(X).any(axis=1)
        self.n_cont = n_cont
        df = pd.DataFrame(X.astype(dtype), columns=[f"c{i}" for i in range(n_cont)])
        if np.isnan(X).any():
            self.lc = pbn.LinearCorrelation(df)
        else:
            # no null at all: LinearCorrelation(df) would take the cached covariance - the per-test handle is made by hand, as
            # LinearCorrelation makes it for a table with nulls (n_dirty = 0 is a shape of the C entry points only)
            from pybnesian_amd.independences import MutualInformation

            self.lc = pbn.LinearCorrelation.__new__(pbn.LinearCorrelation)
            self.lc._all_names = self.lc._names = list(df.columns)
            self.lc._index = {c: i for i, c in enumerate(df.columns)}
            self.lc._handle = None
            self.lc._per_test = MutualInformation(df, True)
        assert self.lc._per_test is not None
        h = self.lc._per_test._handle
        flags = np.ones(n_cont, dtype=np.uint8)
        _lib.check(_lib.load().pbn_mi_set_continuous_nulls(h, flags.ctypes.data_as(C.POINTER(C.c_ubyte)), _lib.dptr(self.shift)))
        _lib.check(_lib.load().pbn_mi_set_order(h, 0, None))
        self.lc.set_batch_threshold(0)

    def want(self, cols):
        """(clean, dirty, sum) records in int64 numpy."""
        Xc = self.X[:, cols]
        valid = ~np.isnan(Xc).any(axis=1)
        out = []
        for rows in (valid & self.clean, valid & ~self.clean, valid):
            D = (Xc[rows] - self.shift[cols]).astype(np.int64)
            P = D.T @ D
            iu = np.triu_indices(len(cols))
            out.append(np.concatenate([[rows.sum()], D.sum(axis=0), P[iu]]).astype(np.int64))
        return np.array(out)

    def check(self, tests, label):
        recs, shape = moments(self.lc, tests)
        assert shape[:3] == [TILE, CHUNK, NC_MAX], shape
        n_dirty = int((~self.clean).sum())
        assert shape[3] == SLICE and shape[4] == (n_dirty + SLICE - 1) // SLICE, (shape, n_dirty)
        assert self.lc.null_rows() == (int(self.clean.sum()), n_dirty)
        for i, got in enumerate(recs):
            want = self.want(columns_of(tests, i))
            assert np.all(np.isfinite(got)), (label, i, got)
            assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float64)), (label, i, columns_of(tests, i), got, want)


def ks_for(n_cont, count, rng):
    return rng.integers(0, min(6, n_cont - 2) + 1, count)


DIRTY = [0, 1, TILE - 1, TILE, TILE + 1, SLICE, SLICE + 1]
CLEAN = [0, 1, 300]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_row_shapes(dtype):
    """Every count of dirty rows against every count of clean rows; a mixed batch of all M per table."""
    rng = np.random.default_rng(3)
    for n_dirty in DIRTY:
        for n_clean in CLEAN:
            if n_dirty + n_clean == 0:
                continue
            t = IntTable(dtype, 9, n_dirty, n_clean, 100 * n_dirty + n_clean)
            ks = np.concatenate([np.arange(7), ks_for(9, 58, rng)])
            t.check(random_tests(rng, 9, ks), f"dirty {n_dirty} clean {n_clean}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_sizes_for_every_m(dtype):
    """1, 63, 64, 65 tests and a workgroup chunk - 1, chunk, chunk + 1, for every M = 2 ... 8, over three slices of dirty rows; columns 0 and 1
    hold no null, so the tests over them alone take all their rows although other columns are dirty."""
    rng = np.random.default_rng(4)
    t = IntTable(dtype, 11, 2 * SLICE + TILE + 3, 301, 7)
    assert not np.isnan(t.X[:, :2]).any() and np.isnan(t.X[:, 2:]).any(axis=0).all()
    for k in range(7):
        for size in (1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1):
            tests = random_tests(rng, 11, np.full(size, k))
            tests[0][0], tests[1][0] = 0, 1       # the first test leads with the two columns that hold no null
            t.check(tests, f"k {k} x {size}")
    recs, _ = moments(t.lc, (np.array([0]), np.array([1]), np.array([0, 0]), np.array([], dtype=int)))
    assert recs[0][2][0] == len(t.X) and recs[0][1][0] == int((~t.clean).sum())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_column_counts(dtype):
    rng = np.random.default_rng(5)
    for n_cont in (2, 31, 32, 33, NC_MAX):
        t = IntTable(dtype, n_cont, SLICE + 1, 40, n_cont, keep_clean=n_cont > 2)
        ks = ks_for(n_cont, 70, rng)
        ks[:min(7, n_cont - 1)] = np.arange(min(7, n_cont - 1))
        tests = random_tests(rng, n_cont, ks)
        if n_cont > 34:      # columns 32 doubles apart, and the last column
            tests[0][0], tests[1][0] = 1, 33
            tests[0][1], tests[1][1] = n_cont - 1, 0
        t.check(tests, f"n_cont {n_cont}")


def test_beyond_the_column_cap_every_test_is_a_host_test():
    rng = np.random.default_rng(6)
    t = IntTable(np.float64, NC_MAX + 1, 20, 60, 1)
    tests = random_tests(rng, NC_MAX + 1, ks_for(NC_MAX + 1, 12, rng))
    before = t.lc.batch_stats()
    got = null_batch(t.lc, tests)
    dev, host, redone = (a - b for a, b in zip(t.lc.batch_stats(), before))
    assert (dev, host, redone) == (0, 12, 0)
    assert np.array_equal(got, null_scalar(t.lc, tests), equal_nan=True)
    assert t.lc.null_rows() is None      # the rows were never split


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_all_null_column_and_poisoned_rows(dtype):
    rng = np.random.default_rng(8)
    # a column that is null in every row: no clean row at all, and no valid row for a test over that column
    t = IntTable(dtype, 9, 40, 200, 2, all_null=True)
    assert t.clean.sum() == 0
    tests = random_tests(rng, 9, np.concatenate([np.arange(7), ks_for(9, 60, rng)]))
    tests[0][0], tests[1][0] = 8, 0
    t.check(tests, "all-null column")
    recs, _ = moments(t.lc, (np.array([8]), np.array([0]), np.array([0, 0]), np.array([], dtype=int)))
    assert np.all(recs[0] == 0.0)
    p = null_batch(t.lc, (np.array([8, 0]), np.array([0, 1]), np.array([0, 0, 0]), np.array([], dtype=int)))
    assert np.isnan(p[0]) and not np.isnan(p[1])      # "not enough valid rows", as the scalar routine says
    # rows whose only valid cell is +-huge: invalid for every test, and nothing of them may reach a sum
    t = IntTable(dtype, 9, SLICE + TILE + 1, 100, 3, poison=True)
    assert np.nanmax(np.abs(t.X)) > 1e38
    tests = random_tests(rng, 9, np.concatenate([np.arange(7), ks_for(9, 120, rng)]))
    tests[0][:7] = 2      # column 2, the poisoned one, leads the first tests of every M
    tests[1][:7] = 3
    v1, v2, off, cond = tests
    for i in range(7):    # (keep the variables of a test distinct)
        cond[off[i]:off[i + 1]] = np.array([0, 1, 4, 5, 6, 7])[:off[i + 1] - off[i]]
    t.check(tests, "poisoned rows")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_test_does_not_depend_on_its_batch(dtype):
    """Real-valued data (rounding matters), three slices of dirty rows.  The same tests - one per M - alone, and first, in the middle and
    last of three batches of different sizes and mixes: bit-identical records and p-values."""
    rng = np.random.default_rng(9)
    n, n_cont = 1100, 12
    X = rng.normal(size=(n, n_cont)) @ (np.eye(n_cont) + 0.3 * rng.normal(size=(n_cont, n_cont)))
    X[rng.random((n, n_cont)) < 0.09] = np.nan
    lc = pbn.LinearCorrelation(pd.DataFrame(X.astype(dtype), columns=[f"c{i}" for i in range(n_cont)]))
    lc.set_batch_threshold(0)
    _lib.check(_lib.load().pbn_mi_set_order(lc._per_test._handle, 0, None))
    probes = random_tests(rng, n_cont, np.arange(7))

    def embed(filler_ks, at):
        f = random_tests(rng, n_cont, filler_ks)
        v1 = np.concatenate([f[0][:at], probes[0], f[0][at:]])
        v2 = np.concatenate([f[1][:at], probes[1], f[1][at:]])
        ks = np.concatenate([filler_ks[:at], np.arange(7), filler_ks[at:]])
        cond = []
        for part in (0, 1, 2):
            src, lo, hi = ((f, 0, at), (probes, 0, 7), (f, at, len(filler_ks)))[part]
            cond.extend(src[3][src[2][lo]:src[2][hi]])
        return (v1, v2, np.concatenate([[0], np.cumsum(ks)]), np.array(cond, dtype=np.int32)), slice(at, at + 7)

    alone_rec, shape = moments(lc, probes)
    assert shape[4] >= 3, shape      # more than one slice: the second step of the order of additions runs
    alone_p = null_batch(lc, probes)
    assert not np.isnan(alone_p).any()
    for filler, at in ((rng.integers(0, 7, 300), 0), (rng.integers(0, 7, 513), 257), (np.full(70, 3), 70), (rng.integers(0, 7, 1000), 999)):
        tests, where = embed(filler, at)
        recs, _ = moments(lc, tests)
        for a, b in zip(alone_rec, recs[where]):
            assert a.tobytes() == b.tobytes()
        assert null_batch(lc, tests)[where].tobytes() == alone_p.tobytes()
    # and a single test per call
    for i in range(7):
        one = (probes[0][i:i + 1], probes[1][i:i + 1], np.array([0, i]), probes[3][probes[2][i]:probes[2][i + 1]])
        assert null_batch(lc, one).tobytes() == alone_p[i:i + 1].tobytes()
