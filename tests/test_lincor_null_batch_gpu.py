"""GPU tier: LinearCorrelation's batch over a table with nulls (csrc/lincor_null_batch.hip) - p-values against an independent
reference and against the scalar routine pbn_mi_lincor_pvalue test by test, and PC on top of it against the serial search.

The table: linear_gaussian_table(40, 5000, 21, 2.0), nulls drawn with default_rng(5) into 12 columns at 1 - 8 % each: 1 602 dirty and
3 398 clean rows (asserted below), every test keeps at least 3 834 rows and every block is far from singular - so NO test may be
flagged or handed to the host there.

The batch and the scalar routine add a test's rows in different orders (clean Gram + slices of dirty rows against one masked pass), so
they agree to rounding.  How closely was MEASURED on an MI355X with this file (the figures are printed before they are asserted) and
fixes two constants:

  REL_TOL = 8 x the largest |p_batch - p_scalar| / p_scalar over all tests with scalar p in [1e-300, 1]
            measured 4.72e-11 on the float64 table, 2.77e-11 on the float32 one (both in the mixed batch; at most
            2.32e-11 in the batches of one k, 3.39e-11 on the table with singular columns)                -> REL_TOL = 3.8e-10
  BAND    = 64 x the largest relative difference over tests with scalar p in [alpha / 4, 4 alpha], alpha in {0.01, 0.05, 0.1}
            (pbn_mi_lincor_band(), csrc/lincor_null_batch.hip); measured 2.96e-12 (float64), 5.21e-12 (float32)
                                                                                                         -> BAND = 3.4e-10

The test asserts measured <= constant / 8.  Exact values - NaN for too few rows, 0 for an infinite statistic or an underflowing tail, 1
for a zero statistic - must be equal; a test whose block is singular comes back through the scalar routine, bit for bit, and so does a
test with few degrees of freedom."""
import os

import numpy as np
import pytest

import pybnesian_amd as pbn
from oracle import mmpc_oracle
from pybnesian_amd import _lib
from test_lincor_null_shapes_gpu import columns_of, null_batch, null_scalar, random_tests
from test_pc_cpu import linear_gaussian_table

pytestmark = pytest.mark.gpu

REL_TOL = 3.8e-10
ALPHAS = (0.01, 0.05, 0.1)
K_DEV = 6


def with_nulls(df):
    """Nulls into 12 of the 40 columns at 1 - 8 % each (the draw is part of the fixture: the counts are asserted)."""
    rng = np.random.default_rng(5)
    X = df.to_numpy().copy()
    cols = rng.choice(40, 12, replace=False)
    for c in cols:
        X[rng.random(len(X)) < rng.uniform(0.01, 0.08), c] = np.nan
    import pandas as pd

    return pd.DataFrame(X, columns=df.columns)      # (X keeps the table's dtype)


def design(dtype):
    return with_nulls(linear_gaussian_table(40, 5000, 21, 2.0, dtype))


def singular_design(dtype):
    """The same with a constant column, a copy of v0 and -2 v1, each with nulls of its own."""
    df = design(dtype)
    rng = np.random.default_rng(6)
    n = len(df)
    extra = {"const": np.full(n, 3.0), "dup0": df["v0"].to_numpy().astype(np.float64), "neg1": -2.0 * df["v1"].to_numpy().astype(np.float64)}
    for name, col in extra.items():
        col = col.copy()
        col[rng.random(n) < 0.03] = np.nan
        df[name] = col.astype(dtype)
    return df


def handle(df):
    lc = pbn.LinearCorrelation(df)
    assert lc._per_test is not None
    lc.set_batch_threshold(0)
    _lib.check(_lib.load().pbn_mi_set_order(lc._per_test._handle, 0, None))
    return lc


def stats_delta(lc, before):
    return tuple(a - b for a, b in zip(lc.batch_stats(), before))


def compare(got, want, label):
    """Exact where the scalar routine is exact; the measured relative differences otherwise."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), (label, got[zero][got[zero] != 0][:5])
    one = want == 1.0
    assert np.all(got[one] == 1.0), label
    body = (~nan) & (want >= 1e-300)
    rel = np.abs(got[body] - want[body]) / want[body]
    worst = float(rel.max()) if rel.size else 0.0
    window = np.zeros(len(want), dtype=bool)
    for a in ALPHAS:
        window |= (want >= a / 4) & (want <= 4 * a)
    relw = np.abs(got[window] - want[window]) / want[window]
    worst_w = float(relw.max()) if relw.size else 0.0
    print(f"{label}: {len(want)} tests, {int(nan.sum())} NaN, {int(zero.sum())} zero; max rel diff {worst:.3g} over {int(body.sum())}, "
          f"{worst_w:.3g} over {int(window.sum())} in the alpha windows")
    return worst, worst_w


@pytest.fixture(scope="module")
def df64():
    return design(np.float64)


@pytest.fixture(scope="module")
def lc64(df64):
    return handle(df64)


def test_the_fixture_is_the_table_the_bounds_were_derived_for(df64):
    X = df64.to_numpy()
    dirty = np.isnan(X).any(axis=1)
    assert (int(dirty.sum()), int((~dirty).sum())) == (1602, 3398)
    assert int(np.isnan(X).any(axis=0).sum()) == 12
    X32 = design(np.float32).to_numpy()
    assert np.array_equal(np.isnan(X32), np.isnan(X))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_against_the_scalar_routine(lc64, df64, dtype):
    lc = lc64 if dtype is np.float64 else handle(design(np.float32))
    band = _lib.load().pbn_mi_lincor_band()
    rng = np.random.default_rng(7)
    worst = worst_w = 0.0
    for k in range(K_DEV + 1):
        for size in (1, 65, 700):
            tests = random_tests(rng, 40, np.full(size, k))
            before = lc.batch_stats()
            got = null_batch(lc, tests)
            assert stats_delta(lc, before) == (size, 0, 0), (k, size)      # really the kernel, nothing flagged
            want = null_scalar(lc, tests)
            a, b = compare(got, want, f"k {k} x {size}")
            worst, worst_w = max(worst, a), max(worst_w, b)
            ok = ~np.isnan(want)
            assert np.all(np.abs(got - want)[ok] <= REL_TOL * want[ok]), (k, size)
    # a mixed batch, with conditioning sets beyond the device's among it: those loop over the scalar routine inside the same call
    ks = rng.integers(0, K_DEV + 3, 6000)
    tests = random_tests(rng, 40, ks)
    before = lc.batch_stats()
    got = null_batch(lc, tests)
    assert stats_delta(lc, before) == (int((ks <= K_DEV).sum()), int((ks > K_DEV).sum()), 0)
    want = null_scalar(lc, tests)
    a, b = compare(got, want, "mixed k")
    worst, worst_w = max(worst, a), max(worst_w, b)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= REL_TOL * want[ok])
    assert np.array_equal(got[ks > K_DEV], want[ks > K_DEV])
    assert lc.null_rows() == (3398, 1602)
    print(f"{np.dtype(dtype).name}: MEASURED max rel diff {worst:.3g} (REL_TOL / 8 = {REL_TOL / 8:.3g}); in the alpha windows {worst_w:.3g} "
          f"(band / 8 = {band / 8:.3g})")
    assert worst <= REL_TOL / 8
    assert worst_w <= band / 8


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_batch_against_numpy_covariances(lc64, df64, dtype):
    """np.cov of the dropna rows through the oracle's restatement of the reference's test; rel 1e-8, the tolerance of this path in
    tests/test_mmhc_gpu.py."""
    df = df64 if dtype is np.float64 else design(np.float32)
    lc = lc64 if dtype is np.float64 else handle(df)
    X = df.to_numpy().astype(np.float64)
    rng = np.random.default_rng(11)
    ks = np.concatenate([np.arange(K_DEV + 1), rng.integers(0, K_DEV + 1, 400)])
    tests = random_tests(rng, 40, ks)
    before = lc.batch_stats()
    got = null_batch(lc, tests)
    assert stats_delta(lc, before) == (len(ks), 0, 0)
    for i in range(len(ks)):
        cols = columns_of(tests, i)
        rows = X[:, cols]
        rows = rows[~np.isnan(rows).any(axis=1)]
        assert len(rows) >= 3834
        cov = np.cov(rows, rowvar=False)
        # the scalar routine as it stands takes n - 2 - (k + 2) degrees of freedom for k >= 2: the oracle's general branch with m = k + 2
        want = mmpc_oracle.lincor_pvalue(cov, len(rows), 0, 1, list(range(2, len(cols))))
        assert got[i] == pytest.approx(want, rel=1e-8, abs=1e-300), (i, cols, got[i], want)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_singular_blocks_come_back_through_the_scalar_routine(dtype):
    df = singular_design(dtype)
    lc = handle(df)
    names = lc.variable_names()
    ix = names.index
    rng = np.random.default_rng(13)
    ks = rng.integers(1, K_DEV + 1, 4000)
    tests = random_tests(rng, len(names), ks)
    v1, v2, off, cond = tests
    singular = np.zeros(len(ks), dtype=bool)
    for i in range(len(ks)):
        block = set(columns_of(tests, i))
        singular[i] = ({ix("v0"), ix("dup0")} <= block) or ({ix("v1"), ix("neg1")} <= block) or ix("const") in block
    assert singular.sum() > 100
    before = lc.batch_stats()
    got = null_batch(lc, tests)
    dev, host, redone = stats_delta(lc, before)
    want = null_scalar(lc, tests)
    assert (dev, host) == (len(ks), 0) and redone >= singular.sum()
    assert np.array_equal(got[singular], want[singular], equal_nan=True)
    compare(got, want, f"{np.dtype(dtype).name} singular design")
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= REL_TOL * want[ok])
    # exact values without a conditioning set: a constant column gives p = 1, copies an infinite statistic and p = 0
    t0 = (np.array([ix("const"), ix("v0"), ix("v1"), ix("v5")]), np.array([ix("v3"), ix("dup0"), ix("neg1"), ix("const")]),
          np.zeros(5, dtype=int), np.array([], dtype=int))
    got, want = null_batch(lc, t0), null_scalar(lc, t0)
    assert list(want) == [1.0, 0.0, 0.0, 1.0] and list(got) == list(want)
    # an index outside the table: NaN for that test alone, as the scalar routine answers it
    out = null_batch(lc, (np.array([0, 999, 1]), np.array([1, 2, -1]), np.array([0, 0, 0, 0]), np.array([], dtype=int)))
    assert not np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2])


def test_few_degrees_of_freedom_are_host_tests(df64):
    df = df64.copy()
    col = df["v7"].to_numpy().copy()
    col[30:] = np.nan                      # 30 valid rows
    df["v7"] = col
    lc = handle(df)
    rng = np.random.default_rng(17)
    ks = np.concatenate([np.arange(K_DEV + 1), rng.integers(0, K_DEV + 1, 300)])
    tests = random_tests(rng, 40, ks)
    few = np.array([7 in columns_of(tests, i) for i in range(len(ks))])
    tests[0][:7] = 7                       # (v7 leads one test of every k; keep its variables distinct)
    for i in range(7):
        tests[1][i] = 8
        tests[3][tests[2][i]:tests[2][i + 1]] = np.arange(9, 9 + i)
    few[:7] = True
    before = lc.batch_stats()
    got = null_batch(lc, tests)
    dev, host, redone = stats_delta(lc, before)
    want = null_scalar(lc, tests)
    assert host == int(few.sum()) and dev == len(ks) - host
    assert np.array_equal(got[few], want[few], equal_nan=True)
    assert not np.isnan(want[few]).all()   # 30 rows are enough for the small conditioning sets
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= REL_TOL * want[ok])
    # too few rows for the test at all: NaN on both sides
    col[8:] = np.nan
    df["v7"] = col
    lc = handle(df)
    t = (np.array([7]), np.array([8]), np.array([0, 6]), np.arange(9, 15))
    assert np.isnan(null_batch(lc, t)[0]) and np.isnan(null_scalar(lc, t)[0])


def search(lc, batched, use_sepsets):
    from pybnesian_amd.constraint import pc_estimate_indices

    return pc_estimate_indices(lc, lc.variable_names(), alpha=0.05, use_sepsets=use_sepsets, batched=batched)


@pytest.mark.parametrize("use_sepsets", [False, True])
def test_pc_is_the_serial_search(df64, use_sepsets):
    """Fails without the batch: the callback is None and batch_stats raises."""
    lc = pbn.LinearCorrelation(df64)
    lc.set_batch_threshold(0)
    serial = search(lc, False, use_sepsets)
    assert lc.batch_stats() == (0, 0, 0)
    assert lc._pc_batch_callback() is not None and lc._pc_band() == _lib.load().pbn_mi_lincor_band()
    # the switch that restores the loop: the same search, every test a host test
    os.environ["PBN_LINCOR_NULL_BATCH"] = "0"
    try:
        off = search(lc, None, use_sepsets)
    finally:
        del os.environ["PBN_LINCOR_NULL_BATCH"]
    dev, host, redone = lc.batch_stats()
    assert dev == 0 and host >= serial["serial_tests"] and redone == 0
    for key in ("arcs", "edges", "serial_tests", "sepsets"):
        assert off[key] == serial[key], key
    batched = search(lc, None, use_sepsets)
    dev, _, redone = lc.batch_stats()
    assert dev > 1000 and redone == 0
    for key in ("arcs", "edges", "serial_tests"):
        assert batched[key] == serial[key], key
    assert batched["sepsets"].keys() == serial["sepsets"].keys()
    for pair, (sep, p) in serial["sepsets"].items():
        assert batched["sepsets"][pair][0] == sep and batched["sepsets"][pair][1] == p, pair
    assert batched["evaluated"] >= serial["serial_tests"]
    # the public entry point
    pc = pbn.PC()
    g = pc.estimate(lc, alpha=0.05, use_sepsets=use_sepsets)
    names = lc.variable_names()
    assert sorted(g.arcs()) == sorted((names[a], names[b]) for a, b in serial["arcs"])
    assert pc.last_search["serial_tests"] == serial["serial_tests"] and pc.last_search["sepsets"] == serial["sepsets"]
    assert lc.batch_stats()[0] == 2 * dev
