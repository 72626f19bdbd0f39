"""GPU tier: the d = 8 screen compares every query column against its OWN query's drop threshold (SweepArgs::qrow_thr, written by
query_window_kernel; csrc/kde_screen_d8.inc), not against the smallest of its group's sixteen.

A (tile, group) block is dropped when each of its 16 columns lies below that column's threshold - the query's window bound less the margin where
it is above the tile's, else the tile's.  What must hold: the rule itself, pair by pair in fp64 from the masks, the thresholds (pbn_debug_d8_masks,
what = 6) and the sorted whitened rows of real launches; every threshold a true lower bound of its query's sum less the margin, and never below
its tile's; the live words a subset of those of the same launch with PBN_D8_SCREEN_ROWTHR=0; the sums inside the budgets; padding columns, a NaN
query and a launch without the window pass exactly what the switch at 0 gives; and the three screen kernels the same words.
tests/test_prune_d8_screen_gpu.py::test_no_dropped_block_holds_a_live_pair reads what = 3, one number per tile: that is the LARGEST of the tile's
sixteen thresholds here - a necessary condition; test_exact_rule_pair_by_pair below is the sharp statement."""
import os

import numpy as np
import pandas as pd
import pytest

from test_prune_d8_screen_gpu import margin_of
from test_prune_d8_screen_stream_gpu import capture, fetch
from test_prune_d8_screen_stream_gpu import lib, pbn  # noqa: F401  (fixtures)
from test_prune_d8_sweep_gpu import BUDGET, frames

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


class env:
    """Environment variables for the launches inside (every switch used here is read per evaluation)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.before = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Dump:
    """slogl, masks, thresholds and sorted whitened rows of one screened launch (dense kernel unless `stream` says otherwise)."""

    def __init__(self, lib, k, test, stream="2", **kv):
        with env(**kv):
            self.slogl, self.box, self.live = capture(lib, k, test, stream)
            self.nw, self.nsplit, self.bps, self.tps, self.ntiles, self.nq = (int(v) for v in fetch(lib, 0, np.int64))
            self.thr_tile = fetch(lib, 3, np.float64)
            self.zq = fetch(lib, 4, np.float64).reshape(-1, 8)
            self.zt = fetch(lib, 5, np.float64).reshape(-1, 8)
            self.thr = fetch(lib, 6, np.float64)
        lib.pbn_debug_d8_masks(0, None, 0, 0)
        self.nqt = (self.nq + 15) // 16
        assert len(self.zq) == self.nq == len(test) and len(self.thr) == self.nqt * 16 and len(self.thr_tile) == self.nqt

    def bits(self, m):
        return np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(self.nw, self.nsplit, self.bps, 2, 8), axis=-1, bitorder="little").astype(bool)

    def tile_bits(self, m):
        """[query tile][training tile]: the words as one bit per block (the second group of an odd last wave repeats the last tile: left out)."""
        b = self.bits(m).transpose(0, 3, 1, 2, 4).reshape(self.nw * 2, self.nsplit, self.bps * 64)[:, :, :self.tps]
        return b.reshape(self.nw * 2, -1)[:self.nqt, :self.ntiles]

    def column_maxima(self, qt, tiles):
        """[len(tiles)][16] fp64: per training tile the largest exponent against each query column of tile qt (-inf: padding on either side)."""
        zt = np.zeros((self.ntiles * 16, 8))
        zt[:len(self.zt)] = self.zt
        nt = -0.5 * np.sum(zt * zt, axis=1)
        nt[len(self.zt):] = -np.inf
        zq = np.zeros((16, 8))
        rows = self.zq[qt * 16:qt * 16 + 16]
        zq[:len(rows)] = rows
        nq = -0.5 * np.sum(zq * zq, axis=1)
        nq[len(rows):] = -np.inf
        out = np.empty((len(tiles), 16))
        for i in range(0, len(tiles), 8192):
            t = tiles[i:i + 8192]
            s = np.einsum("bik,jk->bij", zt.reshape(-1, 16, 8)[t], zq) + nt.reshape(-1, 16)[t][:, :, None] + nq[None, None, :]
            out[i:i + 8192] = s.max(axis=1)
        return out

    def log2_sums(self):
        """Brute force, fp64: log2 of every (sorted) query's whole sum."""
        out = np.empty(self.nq)
        nt = -0.5 * np.sum(self.zt * self.zt, axis=1)
        for i in range(0, self.nq, 64):
            q = self.zq[i:i + 64]
            s = q @ self.zt.T + nt[None, :] - 0.5 * np.sum(q * q, axis=1)[:, None]
            m = s.max(axis=1)
            out[i:i + 64] = m + np.log2(np.exp2(s - m[:, None]).sum(axis=1))
        return out


def check_exact_rule(d):
    """No box-visited block with a column at or above that column's threshold is dropped.  Returns (box-visited, dropped) block counts."""
    box, live = d.tile_bits(d.box), d.tile_bits(d.live)
    assert not np.any(live & ~box), "live is a subset of box"
    n_box = n_drop = 0
    for qt in range(d.nqt):
        tiles = np.nonzero(box[qt])[0]
        if not len(tiles):
            continue
        cm = d.column_maxima(qt, tiles)
        thr = d.thr[qt * 16:qt * 16 + 16]
        alive = (cm >= thr[None, :]).any(axis=1) | np.isnan(thr).any()   # (a NaN threshold keeps the block)
        kept = live[qt, tiles]
        assert not np.any(alive & ~kept), f"query tile {qt}: a dropped block holds a column at or above its own threshold"
        n_box += len(tiles)
        n_drop += int((~kept).sum())
    return n_box, n_drop


@pytest.fixture(scope="module")
def launch33(pbn, lib):
    """32 768 x 528 correlated rows - 33 query tiles: an odd last sweep wave, a last screen wave that serves one - fitted once; per (switch, kernel)
    the dump of one launch, computed once."""
    names, train, test = frames("correlated", 8, 1600, 32_768, 528)
    k = pbn.ProductKDE(names)
    k.fit(train)
    done = {}

    def get(rowthr="1", stream="2"):
        if (rowthr, stream) not in done:
            done[(rowthr, stream)] = Dump(lib, k, test, stream, PBN_D8_SCREEN_ROWTHR=rowthr)
        return done[(rowthr, stream)]

    return get


def test_exact_rule_pair_by_pair(launch33):
    on, off = launch33("1"), launch33("0")
    assert on.nq == 528 and on.ntiles == 2_048 and on.nqt == 33
    m = margin_of(32_768)
    n_box, n_drop = check_exact_rule(on)
    # the thresholds are real bounds: qrow_thr + margin is at or below log2 of the query's whole sum (the window bound is at least 2^-8 below
    # the sum of a subset of its terms; the brute-force sum is good to 1e-9 units)
    sums = on.log2_sums()
    thr_q = on.thr.reshape(on.nqt, 16)
    valid = (np.arange(on.nqt * 16) < on.nq).reshape(on.nqt, 16)
    assert np.all(on.thr[:on.nq] + m <= sums + 1e-9), float(np.max(on.thr[:on.nq] + m - sums))
    # ... and never below the tile's, which is what the switch at 0 compares against and reports sixteen times over
    assert np.array_equal(off.thr.reshape(on.nqt, 16), np.repeat(off.thr_tile[:, None], 16, axis=1))
    assert np.all(thr_q >= off.thr_tile[:, None])
    assert np.all(thr_q[~valid] == np.repeat(off.thr_tile[:, None], 16, axis=1)[~valid]), "padding columns carry the tile's value"
    assert np.array_equal(thr_q.min(axis=1), off.thr_tile), "the smallest of a tile's sixteen is the tile's"
    assert np.array_equal(on.thr_tile, thr_q.max(axis=1)), "what = 3: the largest of the tile's sixteen"
    # the same launch with the switch at 0: the same boxes, and its live words hold every live word of this one, and more
    assert np.array_equal(on.box, off.box)
    assert not np.any(on.live & ~off.live)
    n_on, n_off = int(on.bits(on.live).sum()), int(off.bits(off.live).sum())
    spread = (thr_q - off.thr_tile[:, None])[valid]
    print(f"box-visited blocks {n_box}, dropped {n_drop}; live bits per-query {n_on}, group {n_off} (ratio {n_on / n_off:.3f}); "
          f"thr_q - thr_group mean {spread.mean():.2f} max {spread.max():.2f}")
    assert n_on < n_off
    n = 32_768
    assert abs(on.slogl - off.slogl) <= n * 2.0 ** -m * abs(off.slogl), (on.slogl, off.slogl)


def test_three_kernels_agree(launch33):
    dense, serial, ring = launch33("1", "2"), launch33("1", "0"), launch33("1", "1")
    for other in (serial, ring):
        assert np.array_equal(dense.thr, other.thr)
        assert np.array_equal(dense.box, other.box), "box words"
        assert np.array_equal(dense.live, other.live), f"live words: {int((dense.live != other.live).sum())} of {dense.live.size} differ"
        assert dense.slogl == other.slogl, (dense.slogl, other.slogl)
    assert np.any(dense.live != launch33("0").live), "the per-query rule was on"


# ---- a group with one sparse query.  Bandwidth I; raw coordinates, exponent of a pair = -1/2 log2(e) |x_t - x_q|^2.
N_CLUMP, N_FAR = 2_048, 16
RING = (3_200, 3_680, 4_160, 4_640)                 # rows at c - r e_i and as many at c + r e_i, i = 0 .. 3
N_SPARSE = N_CLUMP + N_FAR + 2 * sum(RING)          # 33 424
FAR, LEAD = 12.0, 256


def sparse_group_tables(seed=33):
    """One query tile: fifteen queries on a clump of 2 048 training rows at c and one query FAR away along axis 7, on a single training tile of
    16 rows.  The rest of the table is the ring: eight spots at c +- r e_i on axes 0 .. 3, r such that a ring row's exponent against a clump
    query lies 0.75 units below that query's own drop threshold (log2 of its sum, 11, less the margin) - seven units above the group's, which
    the far query's sum of 16 terms sets.  Against the far query the ring is 100 units further down.
    Every spot holds a multiple of 16 rows, and the rows of the ring sit on axes 0 .. 3 with four different spreads: the model sorts on the
    four widest principal axes - these, the rotation a signed permutation - in cells of 0.5 whitened units about the mean of the table's first
    1 024 rows.  Those are 256 rows of each spot c - r e_i: the centre lies r / 4 from c on each of the four axes, which puts the clump and the
    far tile - they differ in axis 7 alone - well inside ONE cell, and every other spot inside one of its own.  The stable sort on the cell
    keys then leaves every spot a run of whole tiles, the far rows one tile beside the clump's, inside the window of their query tile.  The
    test reads all of that back from the launch's sorted rows."""
    rng = np.random.default_rng(seed)
    d = 8
    n = N_SPARSE
    m = margin_of(n)
    e_ring = np.log2(N_CLUMP) - m - 0.75                       # (a clump query's sum is its 2 048 clump terms to 1e-5 units: jitter 0.0005)
    r = np.sqrt(-2.0 * e_ring / LOG2E)
    c = np.zeros(d)
    far = c.copy()
    far[7] = FAR

    def ring(i, sign):
        p = c.copy()
        p[i] += sign * r
        return p

    spots = [(ring(i, -1.0), LEAD) for i in range(4)] + [(far, N_FAR), (c, N_CLUMP)]
    for i, a in enumerate(RING):
        spots += [(ring(i, -1.0), a - LEAD), (ring(i, 1.0), a)]
    train = np.vstack([p + rng.normal(scale=0.0005, size=(count, d)) for p, count in spots])
    kind = np.concatenate([np.full(count, {4: 0, 5: 1}.get(j, 2)) for j, (_, count) in enumerate(spots)])   # 0 far, 1 clump, 2 ring
    test = np.vstack([c + rng.normal(scale=0.0005, size=(15, d)), far + rng.normal(scale=0.0005, size=(1, d))])
    assert len(train) == n
    return train, test, kind, e_ring


def test_group_with_one_sparse_query(pbn, lib):
    train, test, kind, e_ring = sparse_group_tables()
    n, d = train.shape
    m = margin_of(n)
    names = [f"v{i}" for i in range(d)]
    k = pbn.KDE(names)
    k.fit(pd.DataFrame(train, columns=names))
    k.bandwidth = np.eye(d)
    q = pd.DataFrame(test, columns=names)
    on = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="1")
    off = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="0")
    with env(PBN_SWEEP_PRUNE="0"):   # (read when a model is fitted: the unpruned sweep needs a fit of its own)
        k0 = pbn.KDE(names)
        k0.fit(pd.DataFrame(train, columns=names))
        k0.bandwidth = np.eye(d)
        plain = k0.slogl(q)
    assert on.nqt == 1 and on.ntiles == n // 16
    # the construction, read back from the sorted rows: against the 16 sorted queries every training tile is a far tile (an exponent near 0
    # against the far query), a clump tile (near 0 against the others) or a ring tile (e_ring against the others, -100 against the far query)
    cm = on.column_maxima(0, np.arange(on.ntiles))
    sums = on.log2_sums()
    fq = int(np.argmin(sums))                                  # the far query's column: a sum of 16 terms
    cq = np.delete(np.arange(16), fq)
    assert abs(sums[fq] - 4.0) < 0.01 and np.all(np.abs(sums[cq] - 11.0) < 0.01), sums
    far_t = np.nonzero(cm[:, fq] > -1.0)[0]
    clump_t = np.nonzero(cm[:, cq].max(axis=1) > -1.0)[0]
    ring_t = np.nonzero((np.abs(cm[:, cq] - e_ring) < 0.1).all(axis=1) & (cm[:, fq] < e_ring - 50.0))[0]
    assert len(far_t) == 1 and len(clump_t) == N_CLUMP // 16 and len(ring_t) == on.ntiles - 1 - N_CLUMP // 16, (len(far_t), len(clump_t), len(ring_t))
    # the thresholds: the far query's is the tile's; the clump queries' own lie log2(2 048 / 16) = 7 units above it
    thr, thr0 = on.thr, off.thr_tile[0]
    assert thr[fq] == thr0 and abs(thr0 + m - 4.0) < 0.01
    assert np.all(np.abs(thr[cq] + m - 11.0) < 0.01), thr + m
    assert np.all(cm[ring_t][:, cq] < thr[cq][None, :] - 0.70) and np.all(cm[ring_t][:, cq] >= thr0 + 1.0), "the ring: 0.75 below the columns' own thresholds, inside the group's"
    assert np.all(cm[far_t][:, cq] < thr0 - 50.0) and np.all(cm[far_t][:, fq] >= thr[fq]), "the far tile: within the far query's margin only"
    box_on, live_on, live_off = on.tile_bits(on.box)[0], on.tile_bits(on.live)[0], off.tile_bits(off.live)[0]
    assert np.array_equal(on.box, off.box) and box_on[ring_t].all() and box_on[far_t].all() and box_on[clump_t].all()
    assert live_on[far_t].all() and live_off[far_t].all(), "the far query's only tile stays"
    assert live_on[clump_t].all()
    assert live_off[ring_t].all(), "against the group's threshold the ring is kept"
    assert not live_on[ring_t].any(), "against the columns' own it is dropped"
    check_exact_rule(on)
    check_exact_rule(off)
    print(f"sparse group: per-query {on.slogl!r} group {off.slogl!r} unpruned {plain!r}; vs unpruned {abs(on.slogl - plain) / abs(plain):.3e}, "
          f"vs group {abs(on.slogl - off.slogl) / abs(off.slogl):.3e} (bound {n * 2.0 ** -m:.3e})")
    assert np.isfinite(on.slogl) and abs(on.slogl - plain) <= BUDGET * abs(plain)
    assert abs(on.slogl - off.slogl) <= n * 2.0 ** -m * abs(off.slogl)


# ---- edges
@pytest.fixture(scope="module")
def edge_model(pbn):
    """32 769 training rows (a padded last training tile), fitted once - and once more with pruning off (the switch is read at the fit), for
    the unpruned sums; the queries of a case are the first n_test of 33."""
    names, train, test = frames("correlated", 8, 1700, 32_769, 33)
    k = pbn.ProductKDE(names)
    k.fit(train)
    with env(PBN_SWEEP_PRUNE="0"):
        k0 = pbn.ProductKDE(names)
        k0.fit(train)
    return k, test, k0


@pytest.mark.parametrize("n_test", [1, 16, 17, 33])
def test_edges(lib, edge_model, n_test):
    """Padding columns (1, 17, 33 queries), one group in the last sweep wave (1, 16, 17: one wave; 33: a second wave of one group), a screen wave
    that serves one sweep wave, a padded last training tile."""
    k, test, k0 = edge_model
    q = test.iloc[:n_test]
    on = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="1")
    off = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="0")
    plain = k0.slogl(q)
    n = 32_769
    m = margin_of(n)
    assert on.nq == n_test and on.ntiles == 2_049
    check_exact_rule(on)
    thr_q = on.thr.reshape(on.nqt, 16)
    valid = (np.arange(on.nqt * 16) < on.nq).reshape(on.nqt, 16)
    assert np.all(thr_q >= off.thr_tile[:, None])
    assert np.all(thr_q[~valid] == np.repeat(off.thr_tile[:, None], 16, axis=1)[~valid]), "padding columns carry the tile's value"
    assert np.all(on.thr[:on.nq] + m <= on.log2_sums() + 1e-9)
    assert np.array_equal(on.box, off.box) and not np.any(on.live & ~off.live)
    print(f"n_test {n_test}: per-query {on.slogl!r} group {off.slogl!r} unpruned {plain!r}")
    assert np.isfinite(on.slogl) and abs(on.slogl - plain) <= BUDGET * abs(plain), (on.slogl, plain)
    assert abs(on.slogl - off.slogl) <= n * 2.0 ** -m * abs(off.slogl), (on.slogl, off.slogl)


def test_nan_query_is_what_the_group_rule_gives(lib, edge_model):
    """One NaN query among 33: its column carries the tile's value, its group keeps every block that passes the box test - the screen's
    operands flag the row, every exponent of it is +inf - and the sum is what the switch at 0 returns for it."""
    import pyarrow as pa

    k, test, _ = edge_model
    vals = test.to_numpy().copy()
    vals[20, 3] = np.nan
    # (an Arrow batch built from numpy keeps the NaN a value: a frame's NaN becomes a null, and rows with nulls never reach the device)
    q = pa.RecordBatch.from_arrays([pa.array(np.ascontiguousarray(vals[:, j])) for j in range(vals.shape[1])], names=list(test.columns))
    on = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="1")
    off = Dump(lib, k, q, PBN_D8_SCREEN_ROWTHR="0")
    pos = np.nonzero(np.isnan(on.zq).any(axis=1))[0]
    assert len(pos) == 1
    qt, col = int(pos[0]) // 16, int(pos[0]) % 16
    assert on.thr[qt * 16 + col] == off.thr_tile[qt]
    assert np.all(on.thr.reshape(-1, 16) >= off.thr_tile[:, None])
    box, live, live0 = on.tile_bits(on.box), on.tile_bits(on.live), off.tile_bits(off.live)
    assert np.array_equal(on.box, off.box) and box[qt].any()
    assert np.array_equal(live[qt], box[qt]) and np.array_equal(live0[qt], box[qt])
    assert not np.any(on.live & ~off.live)
    assert (np.isnan(on.slogl) and np.isnan(off.slogl)) or on.slogl == off.slogl, (on.slogl, off.slogl)


def test_without_the_window_pass_the_switch_changes_nothing(lib, edge_model):
    """PBN_SUM_WINDOW=0: no per-query bounds exist, every column is compared against its group's threshold whatever the switch says."""
    k, test, _ = edge_model
    on = Dump(lib, k, test, PBN_D8_SCREEN_ROWTHR="1", PBN_SUM_WINDOW="0")
    off = Dump(lib, k, test, PBN_D8_SCREEN_ROWTHR="0", PBN_SUM_WINDOW="0")
    assert np.array_equal(on.box, off.box) and np.array_equal(on.live, off.live)
    assert np.array_equal(on.thr, off.thr) and np.array_equal(on.thr_tile, off.thr_tile)
    assert np.array_equal(on.thr.reshape(-1, 16), np.repeat(on.thr_tile[:, None], 16, axis=1))
    assert on.slogl == off.slogl, (on.slogl, off.slogl)
