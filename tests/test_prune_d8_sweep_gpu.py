"""The pruned sum-only sweeps at d = 7 and 8 after round 9 (kde_sweep_body: blind batches for the weighted-norm shape, exp2_magic without its
clamp on batches proven by batch_bare_wmul, box tests with the number of dimensions at compile time, the groups' boxes in LDS, one joint test
for a wave's groups).  d = 8 takes all of it; d = 7 (norm in a K slot) shares the walk and the group-mask path, not the weighted loop.

None of this may change WHAT is computed: the pruned slogl stays within the sum-only budget of the unpruned sweep, PBN_MAGIC_GUARD=0 (every batch
with the clamp) gives the same bits, the rare paths - a 2^x that overflows because a far-out query sits on a far-out training row, a NaN weight of
a row beyond -1/2|z|^2 = -1000 - are redone by the checked loop, and the sweep visits exactly the (tile, group) blocks it visited before."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

N, M = 40_003, 2_001   # a padded last training tile and a padded last query tile
BUDGET = 3e-7          # sum-only budget (tests/test_prune_window_gpu.py): dropped terms (margin 43 + log2(N / 1e6)) and 2^f on the fp32 unit


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib():
    from pybnesian_amd import _lib

    return _lib.load()


def table(kind, n, d, rng):
    if kind == "correlated":
        mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
        return rng.normal(size=(n, d)) @ mix.T
    if kind == "independent":
        return rng.normal(size=(n, d))
    return rng.standard_t(3, size=(n, d))


def frames(kind, d, seed, n=N, m=M):
    rng = np.random.default_rng(seed)
    names = [f"v{i}" for i in range(d)]
    tr = table(kind, n, d, rng)
    tr[100:400] = tr[7]                 # duplicated rows
    tr[500] = 40.0                      # far outliers on both sides: rows 1e4+ exponent units away inside visited tiles
    tr[501] = -40.0
    te = table(kind, m, d, rng)
    k = min(50, m)
    te[:k] = tr[:k]                     # queries on training rows
    if m > 61:
        te[60] = 60.0
        te[61] = -60.0
    return names, pd.DataFrame(tr, columns=names), pd.DataFrame(te, columns=names)


def slogl(pbn, names, train, test):
    k = pbn.ProductKDE(names)
    k.fit(train)
    return k.slogl(test)


def pruned_and_plain(pbn, monkeypatch, names, train, test):
    s = slogl(pbn, names, train, test)
    monkeypatch.setenv("PBN_SWEEP_PRUNE", "0")
    ref = slogl(pbn, names, train, test)
    monkeypatch.delenv("PBN_SWEEP_PRUNE")
    return s, ref


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
@pytest.mark.parametrize("d", [7, 8])
def test_pruned_slogl_matches_unpruned(pbn, monkeypatch, kind, d):
    names, train, test = frames(kind, d, 900 + d)
    s, ref = pruned_and_plain(pbn, monkeypatch, names, train, test)
    print(f"{kind} d={d}: pruned {s!r} unpruned {ref!r} relative {abs(s - ref) / abs(ref):.3e}")
    assert np.isfinite(s) and abs(s - ref) <= BUDGET * abs(ref), (s, ref)


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
@pytest.mark.parametrize("d", [7, 8])
def test_magic_guard_off_gives_the_same_bits(pbn, monkeypatch, kind, d):
    """A batch's sum does not depend on whether it was proven: the clamped and the bare exp2_magic are the same function inside the proof's range."""
    names, train, test = frames(kind, d, 910 + d)
    s = slogl(pbn, names, train, test)
    monkeypatch.setenv("PBN_MAGIC_GUARD", "0")
    off = slogl(pbn, names, train, test)
    monkeypatch.delenv("PBN_MAGIC_GUARD")
    assert np.isfinite(s) and s == off, (s, off)


def redo_counts(lib):
    r, u = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.pbn_debug_sweep_redo(C.byref(r), C.byref(u), 1)
    return r.value, u.value


def rare_path_frames(d, half_norm2_log2, seed):
    """An independent table whose rows 600.. sit at graded distances from the centre - base-2 exponent of the row's own norm, 1/2|z|^2 log2(e), as
    listed - in every coordinate alike, with a query on each of them and one a little off it."""
    rng = np.random.default_rng(seed)
    names = [f"v{i}" for i in range(d)]
    tr = rng.normal(size=(N, d))
    te = rng.normal(size=(M, d))
    h = np.sqrt(np.asarray(_bandwidth_diag(tr, d)))          # normal-reference bandwidths of the bulk (the few rows placed below hardly move them)
    for i, e in enumerate(half_norm2_log2):
        z = np.sqrt(2.0 * e * np.log(2.0) / d)               # per whitened coordinate
        sign = 1.0 if i % 2 == 0 else -1.0
        tr[600 + i] = tr.mean(axis=0) + sign * z * h
        te[100 + 2 * i] = tr[600 + i]
        te[101 + 2 * i] = tr[600 + i] + 0.3 * h
    return names, pd.DataFrame(tr, columns=names), pd.DataFrame(te, columns=names)


def _bandwidth_diag(x, d):
    n = len(x)
    return np.var(x, axis=0, ddof=1) * (4.0 / (d + 2.0)) ** (2.0 / (d + 4.0)) * n ** (-2.0 / (d + 4.0))


@pytest.mark.parametrize("case,norms", [
    # z_t.z_q - 1/2|z_q|^2 for a query ON a row whose own norm is 900+ units: the weighted form's exponent x' = 1/2|z_t|^2 - m + bias leaves the
    # exponent range although every weight is an ordinary number - 2^x' = inf or NaN must surface in the batch's sum
    ("overflow", [700.0, 850.0, 900.0, 930.0, 960.0, 990.0]),
    # rows beyond -1/2|z|^2 = -1000 carry a NaN weight on purpose
    ("nan_weight", [1010.0, 1100.0, 2000.0, 30000.0]),
])
def test_rare_paths_are_redone_checked(pbn, lib, monkeypatch, case, norms):
    names, train, test = rare_path_frames(8, norms, 920)
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")
    redo_counts(lib)
    s = slogl(pbn, names, train, test)
    redo, units = redo_counts(lib)
    monkeypatch.delenv("PBN_SWEEP_COUNT_REDO")
    monkeypatch.setenv("PBN_SWEEP_PRUNE", "0")
    ref = slogl(pbn, names, train, test)
    monkeypatch.delenv("PBN_SWEEP_PRUNE")
    print(f"{case}: batches redone {redo} of {units}; pruned {s!r} unpruned {ref!r} relative {abs(s - ref) / abs(ref):.3e}")
    assert units > 0 and redo > 0, (redo, units)
    assert np.isfinite(s) and abs(s - ref) <= BUDGET * abs(ref), (s, ref)


# tile = 16 rows, batch = 64 tiles = 1 024 rows, split <= 1 024 tiles = 16 384 rows (and a multiple of 8 splits), super-batch = 4 096 tiles = 65 536 rows
@pytest.mark.parametrize("d,n_train,n_test", [
    (8, 32_768, 16), (8, 32_769, 17), (8, 33_808, 1_024), (8, 34_815, 1_025), (8, 65_536, 31), (8, 65_537, 33), (8, 66_559, 48), (8, 131_072 + 15, 2_047),
    (7, 32_768, 17), (7, 65_537, 1_025),
])
def test_edges_of_tiles_batches_and_splits(pbn, monkeypatch, d, n_train, n_test):
    names, train, test = frames("correlated", d, 930 + d, n_train, n_test)
    s, ref = pruned_and_plain(pbn, monkeypatch, names, train, test)
    assert np.isfinite(s) and abs(s - ref) <= BUDGET * abs(ref), (d, n_train, n_test, s, ref)


# (tile, group) blocks visited / offered on the fixed tables below, measured on commit 6a12675 (the parent of round 9) with this very test
VISITS_BEFORE = {7: (625_544, 787_500), 8: (647_447, 787_500)}


@pytest.mark.parametrize("d", [7, 8])
def test_visits_are_the_parents(pbn, lib, monkeypatch, d):
    """Round 9 changes what a visited block costs, not which blocks are visited: the same masks, bit for bit."""
    rng = np.random.default_rng(940 + d)
    names = [f"v{i}" for i in range(d)]
    mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
    train = pd.DataFrame(rng.normal(size=(100_000, d)) @ mix.T, columns=names)
    test = pd.DataFrame(rng.normal(size=(2_000, d)) @ mix.T, columns=names)
    k = pbn.ProductKDE(names)
    k.fit(train)
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")
    lib.pbn_debug_sweep_visits(None, None, 1)
    k.slogl(test)
    v, t = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.pbn_debug_sweep_visits(C.byref(v), C.byref(t), 1)
    print(f"d={d}: visited {v.value} of {t.value}")
    assert (v.value, t.value) == VISITS_BEFORE[d], (d, v.value, t.value)
