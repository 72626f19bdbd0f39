"""The window pass as it runs since round 15 (query_window_kernel: one wave for four neighbouring query tiles against one stream of training
fragments, every tile adding up its own window; walks cut into parts and combined by query_window_finish_kernel), csrc/kde_prepass.hip, on
the smallest shapes at which those forms can go wrong: 40 003 training rows (a
padded last tile; 32 768 is the smallest table that prunes), d = 7 (the norm folded into a K slot) and 8, KDE and ProductKDE, and query sets of
 * 1, 15, 16, 17, 33, 65 and 1 000 rows - waves whose partner tiles do not exist, a padded last query tile; the sets below 1 000 are one
   neighbourhood, as the tiles of one wave are in a real launch (one walk over the hull of the windows, each tile clipped to its own);
 * 40 rows all over the table - tiles far apart, each of which walks its own window (beyond the issue's list; not held to (ii): query_sets);
 * 3 000 rows at the two ends of the sorted training order - windows clipped at tile 0 and at the last tile.  Every (class, d) sorts its own
   way: the order is taken from a launch whose queries are the training rows themselves (pbn_debug_window_pos: the training position each
   query tile's window stands around), and the launch of the set is asserted to have held windows clipped at either end;
 * 1 000 rows two of which lie 60 units out on either side - queries far outside their tile's window.
Every set holds queries equal to training rows and, from 15 rows on, a NaN query; the training table holds duplicated rows and far outliers.
(i) every window bound is at or below the fp64 truth + 1e-9 and finite, (ii) the median of truth - bound is below 2 log2 units, (iii) at
d = 8 every column's threshold plus the margin is at or below its query's truth and a padding column carries its tile's value, (iv) slogl is
within 3e-7 of the unpruned sweep and of the prepass bounds alone, (v) two calls give the same bits, (vi) a d = 5 fp64 model and an fp32
model - paths the round did not touch - do not see PBN_SUM_WINDOW at all."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from test_prune_d8_screen_gpu import margin_of
from test_prune_d8_screen_rowthr_gpu import Dump, env
from test_prune_d8_screen_stream_gpu import lib, pbn  # noqa: F401  (fixtures)
from test_prune_window_gpu import true_log2_sums, window_lb  # noqa: F401  (window_lb: fixture)

pytestmark = pytest.mark.gpu

N = 40_003
SIZES = (1, 15, 16, 17, 33, 65, 1000)
SETS = [f"m{m}" for m in SIZES] + ["ends", "far", "spread"]
W = 256                                 # PBN_SUM_WINDOW's default: training tiles on either side of a query tile's position
MIX = np.tril(np.full((8, 8), 0.3), -1) + np.eye(8)


def training():
    rng = np.random.default_rng(1500)
    tr = rng.normal(size=(N, 8)) @ MIX.T
    tr[100:400] = tr[7]                 # duplicated rows
    tr[500] = 40.0                      # far outliers on both sides
    tr[501] = -40.0
    return tr


def base_queries(tr):
    rng = np.random.default_rng(1501)
    te = rng.normal(size=(1000, 8)) @ MIX.T
    te[0] = tr[0]                       # queries on training rows (the first of them a duplicated one further down: row 7)
    te[1:10] = tr[1:10]
    te[10, 3] = np.nan                  # a NaN query
    te[20:50] = tr[20:50]
    return te


def bandwidth(k):
    H = np.asarray(k.bandwidth, dtype=np.float64)
    return np.diag(H) if H.ndim == 1 else H


@pytest.fixture(scope="module")
def models(pbn, lib):
    """Per (class, d): the fitted model and the frames' column names, fitted once; and the training table."""
    tr = training()
    fitted = {}

    def get(cls, d):
        if (cls, d) not in fitted:
            names = [f"v{i}" for i in range(d)]
            k = getattr(pbn, cls)(names)
            k.fit(pd.DataFrame(tr[:, :d], columns=names))
            fitted[(cls, d)] = (k, names)
        return fitted[(cls, d)]

    get.train = tr
    return get


def window_positions(lib, window_lb, k, frame):
    """Per (non-null) row of frame the position in the model's sorted training order around which its query tile's window stood."""
    fn = lib.pbn_debug_window_pos
    fn.restype = C.c_int64
    fn.argtypes = [C.POINTER(C.c_int64), C.c_int64]
    window_lb(None, 0, 1)
    try:
        k.slogl(frame)
        pos = np.full(len(frame), -1, dtype=np.int64)
        n = fn(pos.ctypes.data_as(C.POINTER(C.c_int64)), len(pos))
    finally:
        window_lb(None, 0, 0)
    assert 0 < n <= len(frame) and np.all(pos[:n] >= 0) and np.all(pos[:n] <= N)
    return pos[:n]


@pytest.fixture(scope="module")
def orders(models, lib, window_lb):
    """Per (class, d) the training rows in the model's sorted order, good to a query tile: the training table as the queries of one launch -
    the queries are sorted as the training rows are, so a query tile's position is (to within equal keys) that of its own sixteen rows."""
    done = {}

    def get(cls, d):
        if (cls, d) not in done:
            k, names = models(cls, d)
            pos = window_positions(lib, window_lb, k, pd.DataFrame(models.train[:, :d], columns=names))
            assert len(pos) == N and pos.min() < 16 * W and pos.max() > N - 16 * W
            done[(cls, d)] = np.argsort(pos, kind="stable")
        return done[(cls, d)]

    return get


@pytest.fixture(scope="module")
def query_sets(models, orders):
    """name, class, d -> the set's queries [m][8] (the caller takes the first d columns); only "ends" depends on the class and d."""
    tr = models.train
    te = base_queries(tr)
    rng = np.random.default_rng(1502)
    # the small sets: one neighbourhood - copies of training row 7, which the table holds 301 times, the first two exact, the others moved by a
    # hundredth of a standard deviation (a fiftieth of a key cell) - so that their few tiles are neighbours in the sorted order as the tiles
    # of a real launch are; a NaN query from 15 rows on
    near = tr[7] + 0.01 * rng.normal(size=(65, 8))
    near[:2] = tr[7]
    near[10, 3] = np.nan
    sets = {f"m{m}": (near[:m].copy() if m < 1000 else te.copy()) for m in SIZES}
    # 40 queries all over the table in three tiles: every tile's window lies somewhere else and the wave walks them one after the other.  A
    # tile's window stands around its FIRST query's position, so most of these queries' own neighbourhoods are outside it and the bound is
    # loose by construction (before round 15 as well): the set is held to every check but (ii)
    sets["spread"] = te[:40].copy()
    far = te.copy()
    far[60] = 60.0
    far[61] = -60.0
    sets["far"] = far
    jitter = 0.02 * rng.normal(size=(3000, 8))

    def get(name, cls, d):
        if name != "ends":
            return sets[name]
        if (cls, d) not in sets:
            order = orders(cls, d)
            ends = tr[np.concatenate([order[:1500], order[-1500:]])] + jitter
            ends[0] = tr[order[0]]          # the first and the last row of the order themselves
            ends[1] = tr[order[-1]]
            ends[5, 2] = np.nan
            sets[(cls, d)] = ends
        return sets[(cls, d)]

    return get


@pytest.fixture(scope="module")
def truths(models, query_sets):
    """fp64 log2 sums of the non-null queries per (class, d, set): computed once, shared, never changed."""
    done = {}

    def get(cls, d, name):
        if (cls, d, name) not in done:
            k, _ = models(cls, d)
            q = query_sets(name, cls, d)[:, :d]
            q = q[~np.isnan(q).any(axis=1)]
            t = true_log2_sums(models.train[:, :d], q, bandwidth(k))
            t.setflags(write=False)
            done[(cls, d, name)] = t
        return done[(cls, d, name)]

    return get


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("d", [7, 8])
@pytest.mark.parametrize("cls", ["KDE", "ProductKDE"])
def test_bounds_and_slogl(models, query_sets, truths, lib, window_lb, cls, d, name):
    k, names = models(cls, d)
    test = pd.DataFrame(query_sets(name, cls, d)[:, :d], columns=names)
    ok = ~test.isna().any(axis=1).to_numpy()
    truth = truths(cls, d, name)
    window_lb(None, 0, 1)
    try:
        s = k.slogl(test)
        lb = np.full(len(test), np.nan)
        n = window_lb(lb.ctypes.data_as(C.POINTER(C.c_double)), len(test), 1)
        s2 = k.slogl(test)
        lb2 = np.full(len(test), np.nan)
        n2 = window_lb(lb2.ctypes.data_as(C.POINTER(C.c_double)), len(test), 0)
    finally:
        window_lb(None, 0, 0)
    assert n == n2 == ok.sum()
    got = lb[:n]
    gap = truth - got
    print(f"{cls} d={d} {name}: truth - bound min {gap.min():.3e} median {np.median(gap):.3f} max {gap.max():.3f}; slogl {s!r}")
    # (i) proven below the sum: only numpy's own rounding of the exponents (~1e-12 units) may show; finite for every non-null row
    assert np.all(np.isfinite(got)), int(np.sum(~np.isfinite(got)))
    assert np.all(got <= truth + 1e-9), float(np.max(got - truth))
    # (ii) and a useful one
    assert name == "spread" or np.median(gap) < 2.0, float(np.median(gap))
    # (v) the parts of a walk are combined in a fixed order: the same bits from two calls
    assert np.array_equal(got, lb2[:n]) and s == s2 and np.isfinite(s), (s, s2)
    # (iv) sum-only budget: the dropped terms (margin 43 + log2(N / 1e6)) and 2^f on the fp32 unit
    with env(PBN_SWEEP_PRUNE="0"):
        ref = k.slogl(test)
    with env(PBN_SUM_WINDOW="0"):
        off = k.slogl(test)
    print(f"   relative to the unpruned sweep {abs(s - ref) / abs(ref):.3e}, to the prepass bounds alone {abs(s - off) / abs(off):.3e}")
    assert abs(s - ref) <= 3e-7 * abs(ref), (s, ref)
    assert abs(s - off) <= 3e-7 * abs(off), (s, off)
    if name == "ends":   # the set is what it is meant to be: windows cut off at tile 0 and at the table's last tile, in this model's own order
        tiles = window_positions(lib, window_lb, k, test) >> 4
        print(f"   window centres from training tile {tiles.min()} to {tiles.max()} of {(N + 15) // 16}")
        assert tiles.min() < W and tiles.max() + W > (N + 15) // 16, (int(tiles.min()), int(tiles.max()))


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("cls", ["KDE", "ProductKDE"])
def test_column_thresholds_d8(models, query_sets, lib, cls, name):
    """(iii) from the screened launch's dump: thresholds per column (what = 6) and per tile (what = 3), sorted order, the null rows left out
    beforehand (the dump is of the launch's own rows)."""
    k, names = models(cls, 8)
    q = query_sets(name, cls, 8)
    test = pd.DataFrame(q[~np.isnan(q).any(axis=1)], columns=names)
    on = Dump(lib, k, test)
    off = Dump(lib, k, test, PBN_D8_SCREEN_ROWTHR="0")
    m = margin_of(N)
    sums = on.log2_sums()   # brute force on the launch's own whitened rows, good to 1e-9 units
    thr_q = on.thr.reshape(on.nqt, 16)
    valid = (np.arange(on.nqt * 16) < on.nq).reshape(on.nqt, 16)
    print(f"{cls} {name}: truth - (threshold + margin) min {np.min(sums - on.thr[:on.nq] - m):.3e} median {np.median(sums - on.thr[:on.nq] - m):.3f}")
    assert np.all(on.thr[:on.nq] + m <= sums + 1e-9), float(np.max(on.thr[:on.nq] + m - sums))
    tile = np.repeat(off.thr_tile[:, None], 16, axis=1)   # the switch at 0 reports the tile's threshold, sixteen times over
    assert np.array_equal(off.thr.reshape(on.nqt, 16), tile)
    assert np.all(thr_q >= tile) and np.array_equal(thr_q.min(axis=1), off.thr_tile)
    assert np.array_equal(thr_q[~valid], tile[~valid]), "padding columns carry the tile's value"
    assert np.array_equal(on.thr_tile, thr_q.max(axis=1))
    assert abs(on.slogl - off.slogl) <= N * 2.0 ** -m * abs(off.slogl), (on.slogl, off.slogl)


@pytest.mark.parametrize("case", ["d5-f64", "d8-f32"])
def test_untouched_paths_do_not_see_the_window(pbn, models, query_sets, case):
    """(vi) d <= 6 and fp32 models have no window pass: the switch at 0 and at 256 gives the same bits."""
    d, dtype = (5, np.float64) if case == "d5-f64" else (8, np.float32)
    names = [f"v{i}" for i in range(d)]
    k = pbn.ProductKDE(names)
    k.fit(pd.DataFrame(models.train[:, :d].astype(dtype), columns=names))
    q = query_sets("m1000", "ProductKDE", d)[:, :d]
    test = pd.DataFrame(q[~np.isnan(q).any(axis=1)].astype(dtype), columns=names)
    with env(PBN_SUM_WINDOW="0"):
        a = k.slogl(test)
    with env(PBN_SUM_WINDOW="256"):
        b = k.slogl(test)
    assert np.isfinite(a) and a == b, (a, b)
