"""GPU tier: the device batch of LinearCorrelation (csrc/lincor_batch.hip, one test per lane) against the scalar host routine
pbn_lincor_pvalue, test by test.

The two sides run the same rules on different arithmetic (FMA contraction, one triangle instead of the full block, pseudo-inverse summed
in index order), so they agree to rounding.  How closely was MEASURED on an MI355X with this file (the figures are printed before they
are asserted) and fixes two constants:

  REL_TOL  = 8 x the largest |p_dev - p_host| / p_host over all tests with host p in [1e-300, 1]
             measured 3.68e-11 on the float64 table, 2.12e-11 on the float32 one (both in the mixed batch; at most
             1.83e-11 in the batches of one k)                                                       -> REL_TOL = 3e-10
  PC_BAND  = 64 x the largest relative difference over tests with host p in [alpha / 4, 4 alpha], alpha in {0.01, 0.05, 0.1}
             (csrc/pc.hip, read here through pbn_pc_band()); measured 4.28e-12 (float64), 2.69e-12 (float32)
                                                                                                     -> PC_BAND = 3e-10

(the first figure comes from small p-values: the tail is exp() of a log of size |log p|, whose rounding grows with it).  The test
asserts measured <= constant / 8.  Exact values - NaN for too few rows, 0 for an infinite statistic or an underflowing tail, 1 for a zero
statistic - must be equal, and every test whose block is singular (duplicated or constant columns) must come back through the host redo and
equal the host bit for bit."""
import ctypes as C

import numpy as np
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib
from test_pc_cpu import linear_gaussian_table

pytestmark = pytest.mark.gpu

REL_TOL = 3e-10
ALPHAS = (0.01, 0.05, 0.1)
_ip = C.POINTER(C.c_int)


def batch(handle, v1, v2, off, cond):
    v1, v2, off = (np.ascontiguousarray(a, dtype=np.int32) for a in (v1, v2, off))
    cond = np.ascontiguousarray(cond if len(cond) else [0], dtype=np.int32)
    out = np.full(len(v1), -7.0)
    _lib.load().pbn_lincor_pvalue_batch(handle, len(v1), v1.ctypes.data_as(_ip), v2.ctypes.data_as(_ip), off.ctypes.data_as(_ip),
                                        cond.ctypes.data_as(_ip), _lib.dptr(out))
    return out


def scalar(handle, v1, v2, off, cond):
    lib = _lib.load()
    cond = np.ascontiguousarray(cond if len(cond) else [0], dtype=np.int32)
    base = cond.ctypes.data
    return np.array([lib.pbn_lincor_pvalue(handle, int(v1[i]), int(v2[i]), int(off[i + 1] - off[i]), C.cast(base + 4 * int(off[i]), _ip))
                     for i in range(len(v1))])


def random_tests(rng, n_vars, ks):
    """One test per entry of ks: distinct variables (v1, v2, conditioning set of that size), as (v1, v2, cond_off, cond)."""
    ks = np.asarray(ks, dtype=np.int64)
    sel = rng.permuted(np.tile(np.arange(n_vars, dtype=np.int16), (len(ks), 1)), axis=1)[:, :int(ks.max()) + 2].astype(np.int32)
    used = np.arange(sel.shape[1] - 2)[None, :] < ks[:, None]
    return sel[:, 0].copy(), sel[:, 1].copy(), np.concatenate([[0], np.cumsum(ks)]), sel[:, 2:][used]


def design(dtype):
    """40 variables of a sparse linear-Gaussian DAG x 5 000 rows, then: a constant column (variance below MACHINE_TOL), a copy of v0
    (singular blocks, correlation +1), -2 v1 (correlation -1)."""
    df = linear_gaussian_table(40, 5000, 21, 2.0, dtype)
    df["const"] = np.full(len(df), 3.0, dtype=dtype)
    df["dup0"] = df["v0"].to_numpy().copy()
    df["neg1"] = (-2.0 * df["v1"].to_numpy()).astype(dtype)
    return df


class Pair:
    """The device handle with its threshold at 0 (every batch really runs the kernel) and a host-only twin over the same covariance."""

    def __init__(self, df):
        self.dev = pbn.LinearCorrelation(df)
        self.dev.set_batch_threshold(0)
        self.host = pbn.LinearCorrelation.from_covariance(self.dev.variable_names(), self.dev.covariance(), len(df))
        self.n = len(self.dev.variable_names())
        self.k_dev = _lib.load().pbn_lincor_batch_max_cond()

    def both(self, tests):
        before = self.dev.batch_stats()
        got = batch(self.dev._handle, *tests)
        stats = tuple(a - b for a, b in zip(self.dev.batch_stats(), before))
        want = batch(self.host._handle, *tests)     # the host-only handle's batch IS the loop over the scalar routine
        return got, want, stats


def compare(got, want, label):
    """Exact where the host is exact; the measured relative differences otherwise."""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), label
    zero = want == 0.0
    assert np.all(got[zero] == 0.0), (label, got[zero][got[zero] != 0][:5])
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
def pair64():
    return Pair(design(np.float64))


def test_the_host_twin_is_the_scalar_routine(pair64):
    rng = np.random.default_rng(1)
    tests = random_tests(rng, pair64.n, rng.integers(0, pair64.k_dev + 3, 3000))
    assert np.array_equal(batch(pair64.host._handle, *tests), scalar(pair64.dev._handle, *tests), equal_nan=True)
    assert np.array_equal(batch(pair64.host._handle, *tests), scalar(pair64.host._handle, *tests), equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_device_batch_against_the_host_routine(pair64, dtype):
    pair = pair64 if dtype is np.float64 else Pair(design(np.float32))
    band = _lib.load().pbn_pc_band()
    rng = np.random.default_rng(7)
    worst = worst_w = 0.0
    k_max = pair.k_dev + 2
    # every k from 0 to K_DEV + 2 (the last two cross to the host loop inside the same call) at every batch size
    for k in range(k_max + 1):
        for size in (1, 63, 64, 65, 4097):
            tests = random_tests(rng, pair.n, np.full(size, k))
            got, want, (dev, host, redone) = pair.both(tests)
            if k <= pair.k_dev:
                assert (dev, host) == (size, 0), (k, size, dev, host)      # really the kernel
            else:
                assert (dev, host) == (0, size), (k, size, dev, host)
            a, b = compare(got, want, f"k {k} x {size}")
            worst, worst_w = max(worst, a), max(worst_w, b)
            assert np.all(np.abs(got - want)[~np.isnan(want)] <= REL_TOL * want[~np.isnan(want)]), (k, size)
    # a mixed batch of more than a million tests
    ks = rng.integers(0, k_max + 1, 1_200_000 if dtype is np.float64 else 200_000)
    tests = random_tests(rng, pair.n, ks)
    got, want, (dev, host, redone) = pair.both(tests)
    assert dev == int((ks <= pair.k_dev).sum()) and host == int((ks > pair.k_dev).sum())
    a, b = compare(got, want, "mixed k")
    worst, worst_w = max(worst, a), max(worst_w, b)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got - want)[ok] <= REL_TOL * want[ok])
    # singular blocks - both v0 and its copy, v1 and -2 v1, or the constant column with a conditioning set - are the host's work
    names = pair.dev.variable_names()
    special = {names.index(c) for c in ("const", "dup0", "neg1", "v0", "v1")}
    v1, v2, off, cond = tests
    singular = np.zeros(len(v1), dtype=bool)
    for i in np.nonzero(ks <= pair.k_dev)[0][:200_000]:
        block = {int(v1[i]), int(v2[i]), *map(int, cond[off[i]:off[i + 1]])}
        if ks[i] >= 1 and len(block & special) >= 2:
            pairs = ({names.index("v0"), names.index("dup0")} <= block) or ({names.index("v1"), names.index("neg1")} <= block) \
                or names.index("const") in block
            singular[i] = pairs
    assert singular.sum() > 100 and redone >= singular.sum()
    assert np.array_equal(got[singular], want[singular], equal_nan=True)
    print(f"{np.dtype(dtype).name}: redone on the host {redone} of {dev} device tests ({int(singular.sum())} known singular among the first 200 000)")
    print(f"{np.dtype(dtype).name}: MEASURED max rel diff {worst:.3g} (REL_TOL / 8 = {REL_TOL / 8:.3g}); in the alpha windows {worst_w:.3g} "
          f"(PC_BAND / 8 = {band / 8:.3g})")
    assert worst <= REL_TOL / 8
    assert worst_w <= band / 8


def test_exact_cases(pair64):
    names = pair64.dev.variable_names()
    ix = names.index
    # constant column: correlation 0 -> p = 1; copies: correlation +-1 -> an infinite statistic -> p = 0
    v1 = [ix("const"), ix("v0"), ix("v1"), ix("v5")]
    v2 = [ix("v3"), ix("dup0"), ix("neg1"), ix("const")]
    got, want, _ = pair64.both((np.array(v1), np.array(v2), np.zeros(5, dtype=int), np.array([], dtype=int)))
    assert list(want) == [1.0, 0.0, 0.0, 1.0] and list(got) == list(want)
    # bad indices: NaN for that test alone
    out = batch(pair64.dev._handle, np.array([0, 999, 1]), np.array([1, 2, -1]), np.array([0, 0, 0, 0]), np.array([], dtype=int))
    assert not np.isnan(out[0]) and np.isnan(out[1]) and np.isnan(out[2])


def test_too_few_rows_is_nan_on_both_sides():
    rng = np.random.default_rng(3)
    import pandas as pd

    df = pd.DataFrame(rng.normal(size=(8, 10)), columns=[f"c{i}" for i in range(10)])
    pair = Pair(df)
    for k in range(0, 9):
        tests = random_tests(rng, 10, np.full(65, k))
        got, want, _ = pair.both(tests)
        df_test = 8 - 2 if k == 0 else (8 - 3 if k == 1 else 8 - 2 - (k + 2))
        assert np.array_equal(got, want, equal_nan=True), k      # few degrees of freedom: the batch keeps these on the host
        assert np.all(np.isnan(want)) == (df_test <= 0), (k, df_test)


def test_ten_million_rows_underflow_to_zero():
    import pandas as pd

    rng = np.random.default_rng(5)
    n = 10_000_000
    x = rng.normal(size=n)
    y = x + 0.5 * rng.normal(size=n)
    z = y + 0.5 * rng.normal(size=n)
    w = rng.normal(size=n)
    pair = Pair(pd.DataFrame({"x": x, "y": y, "z": z, "w": w}))
    v1, v2 = np.array([0, 1, 0, 0, 0]), np.array([1, 2, 2, 3, 1])
    off, cond = np.array([0, 0, 0, 0, 0, 1]), np.array([3])
    got, want, (dev, host, _) = pair.both((v1, v2, off, cond))
    assert dev == 5 and host == 0
    assert want[0] == want[1] == want[2] == want[4] == 0.0 and 0 < want[3] <= 1
    assert np.all(got[[0, 1, 2, 4]] == 0.0) and abs(got[3] - want[3]) <= REL_TOL * want[3]
