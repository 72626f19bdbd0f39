"""Window-sum bound of the pruned sum-only sweeps at d = 7 and 8 (query_window_kernel): the exact terms over the training tiles around a
query tile's position raise the pruning threshold and the offsets.  The bound of every query is checked against its true log2 sum
(numpy, all training rows) on correlated, independent and heavy-tailed tables with duplicated rows, far outliers on both sides, null
test rows (left out by slogl) and a padded last training tile; slogl against the unpruned sweep and against the prepass bounds alone (PBN_SUM_WINDOW=0)."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

N, M = 40_003, 2_001   # a padded last training tile and a padded last query tile


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def window_lb():
    from pybnesian_amd import _lib

    fn = _lib.load().pbn_debug_sum_window
    fn.restype = C.c_int64
    fn.argtypes = [C.POINTER(C.c_double), C.c_int64, C.c_int]
    return fn


def table(kind, n, d, rng):
    if kind == "correlated":
        mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
        return rng.normal(size=(n, d)) @ mix.T
    if kind == "independent":
        return rng.normal(size=(n, d))
    return rng.standard_t(3, size=(n, d))


def frames(kind, d, seed):
    rng = np.random.default_rng(seed)
    names = [f"v{i}" for i in range(d)]
    tr = table(kind, N, d, rng)
    tr[100:400] = tr[7]                 # duplicated rows
    tr[500] = 40.0                      # far outliers on both sides
    tr[501] = -40.0
    te = table(kind, M, d, rng)
    te[:50] = tr[:50]                   # queries on training rows
    te[60] = 60.0
    te[61] = -60.0
    te[70, 3] = np.nan                  # null test rows
    te[M - 1, 0] = np.nan
    return names, pd.DataFrame(tr, columns=names), pd.DataFrame(te, columns=names)


def true_log2_sums(train, test, H):
    """log2 of sum_t exp(-1/2 (x_q - x_t)' H^-1 (x_q - x_t)) per query: the sum the sweep's base-2 exponents add up."""
    L = np.linalg.cholesky(H)
    zt = np.linalg.solve(L, train.T).T
    zq = np.linalg.solve(L, test.T).T
    out = np.empty(len(zq))
    for i in range(0, len(zq), 256):
        q = zq[i:i + 256]
        e = -0.5 * ((q ** 2).sum(1)[:, None] + (zt ** 2).sum(1)[None, :] - 2.0 * q @ zt.T)
        mx = e.max(1)
        out[i:i + 256] = (mx + np.log(np.exp(e - mx[:, None]).sum(1))) / np.log(2.0)
    return out


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
@pytest.mark.parametrize("d", [7, 8])
@pytest.mark.parametrize("cls", ["KDE", "ProductKDE"])
def test_window_bound_below_true_sum(pbn, window_lb, kind, d, cls):
    names, train, test = frames(kind, d, 300 + d)
    k = getattr(pbn, cls)(names)
    k.fit(train)
    window_lb(None, 0, 1)
    s = k.slogl(test)
    null = test.isna().any(axis=1).to_numpy()
    ok = ~null   # slogl leaves the null rows out: the bounds are those of the other rows, in their order
    lb = np.full(M, np.nan)
    n = window_lb(lb.ctypes.data_as(C.POINTER(C.c_double)), M, 0)
    assert n == ok.sum() and np.isfinite(s)
    H = np.asarray(k.bandwidth, dtype=np.float64)
    if H.ndim == 1:
        H = np.diag(H)
    truth = true_log2_sums(train.to_numpy(), test.to_numpy()[ok], H)
    got = lb[:n]
    # the bound is proven below the sum: only numpy's own rounding of the exponents (~1e-12 units) may show
    assert np.all(got <= truth + 1e-9), np.max(got - truth)
    assert np.all(np.isfinite(got))
    # and it is a useful one: the window holds most of a typical query's sum
    assert np.median(truth - got) < 2.0, np.median(truth - got)


def slogl(pbn, cls, names, train, test):
    k = getattr(pbn, cls)(names)
    k.fit(train)
    return k.slogl(test)


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
@pytest.mark.parametrize("d", [7, 8])
def test_window_slogl_matches_plain_and_window_off(pbn, monkeypatch, kind, d):
    names, train, test = frames(kind, d, 400 + d)
    test = test.dropna()
    s = slogl(pbn, "ProductKDE", names, train, test)
    monkeypatch.setenv("PBN_SUM_WINDOW", "0")
    off = slogl(pbn, "ProductKDE", names, train, test)
    monkeypatch.delenv("PBN_SUM_WINDOW")
    monkeypatch.setenv("PBN_SWEEP_PRUNE", "0")
    ref = slogl(pbn, "ProductKDE", names, train, test)
    monkeypatch.delenv("PBN_SWEEP_PRUNE")
    # sum-only budget: the dropped terms (margin 43 + log2(N / 1e6)) and 2^f on the fp32 unit
    assert np.isfinite(s) and abs(s - ref) <= 3e-7 * abs(ref), (s, ref)
    assert abs(s - off) <= 3e-7 * abs(off), (s, off)


def test_window_visits_fewer_blocks(pbn, monkeypatch):
    """The window bound prunes more (tile, group) blocks than the prepass bounds alone (PBN_SWEEP_COUNT_REDO counters)."""
    from pybnesian_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    d = 8
    names = [f"v{i}" for i in range(d)]
    mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
    train = pd.DataFrame(rng.normal(size=(200_000, d)) @ mix.T, columns=names)
    test = pd.DataFrame(rng.normal(size=(3_000, d)) @ mix.T, columns=names)
    k = pbn.ProductKDE(names)
    k.fit(train)
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")
    frac = {}
    for w in ("0", "256"):
        monkeypatch.setenv("PBN_SUM_WINDOW", w)
        lib.pbn_debug_sweep_visits(None, None, 1)
        k.slogl(test)
        v, t = C.c_ulonglong(0), C.c_ulonglong(0)
        lib.pbn_debug_sweep_visits(C.byref(v), C.byref(t), 1)
        assert t.value > 0
        frac[w] = v.value / t.value
    assert frac["256"] < frac["0"], frac
