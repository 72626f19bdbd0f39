"""Pruned sum-only sweeps at d = 7 and 8 (kde_prune_rotates): rows rotated to the principal axes of the whitened training rows, boxes
over all dimensions, keys on the widest four.  slogl against the unpruned sweep (PBN_SWEEP_PRUNE=0) on correlated, independent and
heavy-tailed tables, a near-collinear column pair, duplicated rows, far outliers on both sides, null test rows and training sizes around
PBN_PRUNE_MIN_ROWS; per-row logl of such a model stays on the plain sweep."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

N, M = 40_000, 3_000


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


def table(kind, n, d, rng):
    if kind == "correlated":
        mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
        return rng.normal(size=(n, d)) @ mix.T
    if kind == "independent":
        return rng.normal(size=(n, d))
    return rng.standard_t(3, size=(n, d))


def pruned_and_plain(pbn, monkeypatch, cls, names, train, test):
    k = getattr(pbn, cls)(names)
    k.fit(train)
    s = k.slogl(test)
    monkeypatch.setenv("PBN_SWEEP_PRUNE", "0")
    plain = getattr(pbn, cls)(names)
    plain.fit(train)
    ref = plain.slogl(test)
    monkeypatch.delenv("PBN_SWEEP_PRUNE")
    return k, s, plain, ref


def close(s, ref, rel=3e-7):
    # sum-only budget: the dropped terms (margin 43 + log2(N / 1e6)) and 2^f on the fp32 unit, in both sweeps
    return np.isfinite(s) and abs(s - ref) <= rel * abs(ref)


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
@pytest.mark.parametrize("d", [7, 8])
@pytest.mark.parametrize("cls", ["KDE", "ProductKDE"])
def test_rotated_pruned_slogl_matches_plain(pbn, monkeypatch, kind, d, cls):
    rng = np.random.default_rng(100 + d)
    names = [f"v{i}" for i in range(d)]
    train = pd.DataFrame(table(kind, N, d, rng), columns=names)
    test = pd.DataFrame(table(kind, M, d, rng), columns=names)
    k, s, plain, ref = pruned_and_plain(pbn, monkeypatch, cls, names, train, test)
    assert close(s, ref), (s, ref)
    # per-row outputs of the rotated model: the plain sweep over the sorted pack, the same values
    got = k.logl(test.iloc[:500])
    assert np.allclose(got, plain.logl(test.iloc[:500]), rtol=1e-9, atol=1e-9)


def test_rotated_pruned_visits_fewer_blocks(pbn, monkeypatch):
    """The d = 8 sum-only sweep is the pruned one, and it skips blocks of a wide table (the counters of PBN_SWEEP_COUNT_REDO)."""
    from pybnesian_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    d = 8
    names = [f"v{i}" for i in range(d)]
    mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
    train = pd.DataFrame(rng.normal(size=(200_000, d)) @ mix.T, columns=names)
    test = pd.DataFrame(rng.normal(size=(M, d)) @ mix.T, columns=names)
    k = pbn.ProductKDE(names)
    k.fit(train)
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")
    lib.pbn_debug_sweep_visits(None, None, 1)
    k.slogl(test)
    v, t = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.pbn_debug_sweep_visits(C.byref(v), C.byref(t), 1)
    assert t.value > 0 and v.value < t.value


@pytest.mark.parametrize("case", ["near_collinear", "duplicated", "outliers", "null_rows"])
@pytest.mark.parametrize("cls", ["KDE", "ProductKDE"])
def test_rotated_pruned_edge_tables(pbn, monkeypatch, case, cls):
    rng = np.random.default_rng(7)
    d = 8
    names = [f"v{i}" for i in range(d)]
    x = table("correlated", N, d, rng)
    q = table("correlated", M, d, rng)
    if case == "near_collinear":   # one near-degenerate eigenvalue of the whitened rows' covariance (a column ~ another one)
        x[:, 3] = x[:, 2] + 1e-5 * rng.normal(size=N)
        q[:, 3] = q[:, 2] + 1e-5 * rng.normal(size=M)
    elif case == "duplicated":
        x[N // 2:] = x[: N - N // 2]
        q[: M // 2] = x[: M // 2]
    elif case == "outliers":       # far rows on both sides: the clamp of exp2_magic and the checked redo
        x[:20] *= 300.0
        q[:20] *= 300.0
        q[20:25] = x[:5]
    train = pd.DataFrame(x, columns=names)
    test = pd.DataFrame(q, columns=names)
    if case == "null_rows":
        test.iloc[[3, 50, 777], [0, 5, 7]] = np.nan
    k, s, plain, ref = pruned_and_plain(pbn, monkeypatch, cls, names, train, test)
    assert close(s, ref), (s, ref)
    if case == "null_rows":
        got = k.logl(test)
        assert np.isnan(got[[3, 50, 777]]).all()
        assert abs(s - np.nansum(plain.logl(test))) <= 3e-7 * abs(s)


@pytest.mark.parametrize("n", [32_768 - 16, 32_768, 32_768 + 17])
def test_rotated_pruned_around_min_rows(pbn, monkeypatch, n):
    rng = np.random.default_rng(n)
    d = 8
    names = [f"v{i}" for i in range(d)]
    train = pd.DataFrame(table("correlated", n, d, rng), columns=names)
    test = pd.DataFrame(table("correlated", 1_001, d, rng), columns=names)
    _, s, _, ref = pruned_and_plain(pbn, monkeypatch, "ProductKDE", names, train, test)
    assert close(s, ref), (s, ref)
