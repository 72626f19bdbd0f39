"""Hybrid MutualInformation's moment kernels (csrc/mi.hip, csrc/stats_kernels.hip) at every launch shape, against numpy.

Every value MutualInformation returns is host arithmetic on per-configuration moments: a count, the sums and the upper-triangle products
of the pilot-shifted continuous columns.  The test aids pbn_debug_mi_moments / pbn_debug_mi_full / pbn_debug_mi_shifts (layouts at their
definitions in csrc/mi.hip) hand back those raw moments for a batch of plans - run through Engine::group_stats_many in one call, as
pbn_mi_pvalue_batch runs them -, the path that served each plan and the handle's pilot shifts.

Exact leg.  Column j is s_j + e with an integer offset s_j and integers e in [-15, 15] whose pilot rows sum to zero, so the shift is exactly
s_j (asserted), x - shift is an integer and every product and partial sum is an integer far below 2^53: whatever the summation order, FMA
or f64 MFMA, float32 or float64 table, the moments must EQUAL the int64 result of tests/mi_restatement.py.  No tolerance.  The sizes of
the configurations are prescribed, not drawn (lengths() below): 0, 1, 2, k STEP + {-1, 0, 1} around the switch points of
gram_gring_kernel's ring for both of its (STEP, D) pairs, one block stride of moments_sorted_kernel and the piece length MI_SORTED_ROWS.
The list has 53 distinct lengths, so the main table has 7 x 8 = 56 configurations (first, last and two interior ones empty) and 46 052
rows; a third variable of 5 categories gives the 40-configuration plans (5 x 8) whose legacy launches take 2 and 3 windows.

Rounding leg.  Real-valued tables (offsets up to +-30), same configurations: |got - want| <= (n_g + 2) 2^-53 sum |x_i x_j| per cell (sums:
sum |x_i|), the bound of any summation order of n_g rounded products or FMAs, with want from np.longdouble products and sums of the
rounded x - shift (reported shifts).  No measured constant.

What is reached is asserted at the end (test_every_launch_form_was_seen).  NOT reached from here: the column-gather form
gram_gring_kernel<T, NCT, false>, which MutualInformation launches only when the row-major mirror cannot be allocated or exceeds its
16 GiB budget.  It is the production form of every hybrid local score (csrc/hybrid.hip cells_gram, csrc/scoring.hip gram_raw with a
row list) and is held there, cell by cell at the same prescribed sizes, by tests/test_hybrid_moments_shapes_gpu.py.

Measured on an MI355X (this file alone, one pytest process): 13 s for the 31 tests, the slowest (test_sorted_kernels, 112 plans) 1.8 s;
most of it is numpy.  Worst fraction of the rounding bound: 0.479 (float32 table, sorted and legacy kernels, (d1, d2)); float64 0.403
(legacy), 0.390 (full Gram); whole-table plans stay below 0.001 (the bound grows with n_g, the error of a blocked sum does not).
Paths reported over the file (plans and pbn_debug_mi_full groupings): counts only 46, full Gram 258, sorted 304, legacy 68; 81 distinct
launch forms.
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import mi_restatement as mr

pytestmark = pytest.mark.gpu

# ---- the kernels' constants, each with the line it restates ----------------------------------------------------------------------
STEP_D = ((64, 3), (32, 4))    # stats_kernels.hip gram_gring_kernel: RL = (double && NCT == 4) ? 2 : 4; D = RL == 2 ? 4 : 3; STEP = 16 * RL
SORTED_BLOCK = 256             # mi.hip moments_sorted_kernel: for (r = r0 + threadIdx.x; r < r1; r += 256)
PIECE = mr.MI_SORTED_ROWS      # mi.hip: #define MI_SORTED_ROWS 4096
SORTED_MAX_CONT = 16           # mi.hip: #define MI_SORTED_MAX_CONT 16
MAX_CONT = 24                  # mi.hip: #define MI_MAX_CONT 24
FULL_MAX_CONT, FULL_MAX_G = 64, 4096   # mi.hip full_applies: h->n_cont <= 64 && g.G <= 4096
PILOT_ROWS = 1024              # stats_kernels.hip pilot_mean_kernel: m = n < 1024 ? n : 1024
NCOL = 66
OFFS = np.array([(-1) ** j * (10 + j) for j in range(NCOL)], dtype=np.int64)   # s_j: distinct, tens in magnitude
CARDS = (7, 8)                 # d1 (fastest), d2: 56 configurations
CARD3 = 5                      # d3: (d3, d2) has 40

PATH = {0: "count", 1: "full", 2: "sorted", 3: "legacy"}
FIELDS = ("path", "c", "nulls", "bytes", "G", "windows", "nblocks", "chunks", "rows", "nct", "form", "nblk", "launched", "order", "grid_x", "batch")

SEEN = set()                   # ("full", bytes, nct, form, order) / ("sorted", bytes, C, nulls) / ("legacy", bytes, c, chunks > 1) / ("count",)
NOTES = {"frac": 0.0, "early_return": False, "padding": False}
PLANS = {k: 0 for k in PATH.values()}   # plans (and pbn_debug_mi_full groupings) served, by path


def lengths():
    L = {0, 1, 2, SORTED_BLOCK - 1, SORTED_BLOCK, SORTED_BLOCK + 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1}
    for step, d in STEP_D:
        for k in (1, 2, d - 1, d, 3 * d - 1, 3 * d, 3 * d + 1, 4 * d, 4 * d + 1):
            L |= {k * step - 1, k * step, k * step + 1}
    return sorted(L)


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def int_e(n, seed, null_cols=(), null_share=0.0):
    """e [n][NCOL] in [-15, 15] whose first min(n, 1024) rows sum to zero in every column; a column of null_cols instead gets a null mask
    and valid cells that sum to zero over the whole column.  Returns e and the mask (True = null)."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-15, 16, size=(n, NCOL)).astype(np.int64)
    m = min(n, PILOT_ROWS)
    h = m // 2
    e[h:2 * h] = -e[:h][rng.permutation(h)]
    if m % 2:
        e[m - 1] = 0
    mask = np.zeros((n, NCOL), dtype=bool)
    for j in null_cols:
        mask[:, j] = rng.random(n) < null_share
        valid = np.flatnonzero(~mask[:, j])
        h = len(valid) // 2
        e[valid[h:2 * h], j] = -e[valid[:h], j]
        if len(valid) % 2:
            e[valid[-1], j] = 0
        assert e[valid, j].sum() == 0
    assert np.all(e[:m][:, [j for j in range(NCOL) if j not in null_cols]].sum(axis=0) == 0)
    return e, mask


def main_codes(seed):
    """The prescribed configuration sizes on a 7 x 8 grid, shuffled rows: returns d1, d2 and the sizes by configuration id."""
    rng = np.random.default_rng(seed)
    L = [v for v in lengths() if v > 0]
    G = CARDS[0] * CARDS[1]
    assert len(lengths()) == 53 and len(L) + 4 == G
    interior = np.array(L + [0, 0])
    rng.shuffle(interior)
    size = np.concatenate([[0], interior, [0]])
    assert size[0] == 0 and size[-1] == 0 and (size[1:-1] == 0).sum() >= 1
    cfg = np.repeat(np.arange(G), size)
    perm = rng.permutation(len(cfg))
    assert not np.array_equal(perm, np.arange(len(cfg)))
    cfg = cfg[perm]
    return (cfg % CARDS[0]).astype(np.int32), (cfg // CARDS[0]).astype(np.int32), size


class Table:
    """values [n][NCOL] (int64 for the exact leg, float for the rounding leg), a null mask, and discrete columns name -> (codes, card)."""

    def __init__(self, values, mask, disc, families):
        self.values, self.mask, self.disc, self.families = values, mask, disc, families
        self.n = values.shape[0]
        self._fine = {}

    # the restatement, shared by every handle over a column subset of this table
    def _family(self, names):
        for fam in self.families:
            if set(names) <= set(fam):
                return fam
        raise KeyError(names)

    def fine(self, fam, shifted, real):
        """Moments of all columns per configuration of the family's variables, a null category as one more bucket."""
        if (fam, real) not in self._fine:
            codes = [np.where(self.disc[v][0] < 0, self.disc[v][1], self.disc[v][0]) for v in fam]
            key, G = mr.keys(codes, [self.disc[v][1] + 1 for v in fam])
            self._fine[(fam, real)] = (mr.real_moments if real else mr.int_moments)(shifted, key, G)
        return self._fine[(fam, real)]

    def index(self, fam, names):
        """fine configuration of the family -> configuration of the plan (first name fastest), -1 with a null category of a plan variable."""
        ecards = [self.disc[v][1] + 1 for v in fam]
        G = int(np.prod(ecards)) if fam else 1
        rem = np.arange(G)
        digit = {}
        for v, k in zip(fam, ecards):
            digit[v] = rem % k
            rem = rem // k
        idx = np.zeros(G, dtype=np.int64)
        bad = np.zeros(G, dtype=bool)
        stride = 1
        for v in names:
            bad |= digit[v] == self.disc[v][1]
            idx += digit[v] * stride
            stride *= self.disc[v][1]
        idx[bad] = -1
        return idx, stride

    def pooled(self, names, shifted, real=False):
        fam = self._family(names)
        parts = self.fine(fam, shifted, real)
        idx, G = self.index(fam, names)
        keep = idx >= 0
        out = []
        for a in parts:
            z = np.zeros((G,) + a.shape[1:], dtype=a.dtype)
            np.add.at(z, idx[keep], a[keep])
            out.append(z)
        return out

    def want(self, cont, names):
        """The int64 statistics of a plan, [G][stats]."""
        cont = list(cont)
        if self.mask[:, cont].any():   # rows valid in all of the plan's columns: counted directly
            key, G = mr.keys([self.disc[v][0] for v in names], [self.disc[v][1] for v in names])
            if not names:
                key = np.zeros(self.n, dtype=np.int64)
            key = np.where(self.mask[:, cont].any(axis=1), -1, key)
            count, S, P = mr.int_moments(self.shifted_int()[:, cont], key, G)
            return mr.layout(count, S, P)
        count, S, P = self.pooled(tuple(names), self.shifted_int())
        return mr.layout(count, S[:, cont], P[:, cont][:, :, cont])

    def shifted_int(self):
        return np.where(self.mask, 0, self.values - OFFS[:self.values.shape[1]])


class Handle:
    """pbn.MutualInformation over the first nc columns of a table, and the three test aids on its handle."""

    def __init__(self, pbn, table, nc, dtype, shifts=OFFS):
        from pybnesian_amd import _lib

        self.table, self.nc, self.bytes = table, nc, np.dtype(dtype).itemsize
        vals = table.values[:, :nc].astype(dtype)
        vals[table.mask[:, :nc]] = np.nan
        data = {f"x{j}": vals[:, j] for j in range(nc)}
        for name, (codes, card) in table.disc.items():
            data[name] = pd.Categorical.from_codes(codes, [f"l{i}" for i in range(card)])
        self.mi = pbn.MutualInformation(pd.DataFrame(data))
        self.did = {name: nc + i for i, name in enumerate(table.disc)}
        lib = _lib.load()
        self.f_mom, self.f_full, self.f_shift = lib.pbn_debug_mi_moments, lib.pbn_debug_mi_full, lib.pbn_debug_mi_shifts
        self.f_mom.restype = C.c_int64
        self.f_mom.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int64, C.c_void_p]
        self.f_full.restype = C.c_int64
        self.f_full.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        self.f_shift.restype = C.c_int
        self.f_shift.argtypes = [C.c_void_p, C.c_void_p]
        self.shift = np.zeros(nc)
        assert self.f_shift(self.mi._handle, self.shift.ctypes.data) == 0
        if shifts is not None:
            assert np.array_equal(self.shift, shifts[:nc].astype(np.float64)), "the pilot shift is not the column's integer offset"

    def moments(self, plans):
        """plans = [(continuous columns, discrete names)]: one pbn_debug_mi_moments call; returns ([G][stats] per plan, records)."""
        n = len(plans)
        coff = np.zeros(n + 1, dtype=np.int32)
        doff = np.zeros(n + 1, dtype=np.int32)
        coff[1:] = np.cumsum([len(p[0]) for p in plans])
        doff[1:] = np.cumsum([len(p[1]) for p in plans])
        cont = np.array([v for p in plans for v in p[0]] or [0], dtype=np.int32)
        disc = np.array([self.did[v] for p in plans for v in p[1]] or [0], dtype=np.int32)
        sizes = []
        for cs, ds in plans:
            G = int(np.prod([self.table.disc[v][1] for v in ds])) if ds else 1
            sizes.append((G, 1 + len(cs) + len(cs) * (len(cs) + 1) // 2))
        total = sum(g * s for g, s in sizes)
        out = np.full(total, np.nan)
        rec = np.zeros((n, len(FIELDS)), dtype=np.int64)
        got = self.f_mom(self.mi._handle, n, coff.ctypes.data, cont.ctypes.data, doff.ctypes.data, disc.ctypes.data, out.ctypes.data, total, rec.ctypes.data)
        assert got == total, (got, total)
        res, at = [], 0
        for g, s in sizes:
            res.append(out[at:at + g * s].reshape(g, s))
            at += g * s
        recs = [dict(zip(FIELDS, (int(v) for v in r))) for r in rec]
        for r, (cs, _), (g, _) in zip(recs, plans, sizes):
            assert (r["c"], r["bytes"], r["G"]) == (len(cs), self.bytes, g), r
            note(r)
        return res, recs

    def full(self, names):
        """pbn_debug_mi_full of the grouping of `names` (any order; the grouping's own is by variable id): S [G][nc], P [G][nc][nc], record."""
        names = sorted(names, key=lambda v: self.did[v])
        G = int(np.prod([self.table.disc[v][1] for v in names])) if names else 1
        S, P = np.full((G, self.nc), np.nan), np.full((G, self.nc, self.nc), np.nan)
        rec = np.zeros(5, dtype=np.int64)
        ids = np.array([self.did[v] for v in names] or [0], dtype=np.int32)
        got = self.f_full(self.mi._handle, len(names), ids.ctypes.data, S.ctypes.data, P.ctypes.data, rec.ctypes.data)
        assert got == G, (got, G)
        r = dict(zip(("nct", "form", "nblk", "launched", "order"), (int(v) for v in rec)))
        r.update(path=1, bytes=self.bytes)
        note(r)
        return names, S, P, r


def note(r):
    """Book a record's launch form for the final coverage check."""
    kind = PATH[r["path"]]
    PLANS[kind] += 1
    if kind == "count":
        SEEN.add(("count",))
    elif kind == "full":
        SEEN.add(("full", r["bytes"], r["nct"], r["form"], r["order"]))
        NOTES["padding"] |= r["order"] == 1 and r["launched"] > r["nblk"]
    elif kind == "sorted":
        SEEN.add(("sorted", r["bytes"], r["c"], r["nulls"]))
        NOTES["early_return"] |= r["nblk"] < r["grid_x"]
    else:
        SEEN.add(("legacy", r["bytes"], r["c"], r["chunks"] > 1))


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def main():
    """The main table: 46 052 rows in the prescribed configurations of (d1, d2), a third variable d3 and a one-category variable."""
    d1, d2, size = main_codes(11)
    n = len(d1)
    assert 40000 <= n <= 60000 and n % 64 != 0 and n > 32768
    rng = np.random.default_rng(12)
    e, mask = int_e(n, 13)
    disc = {"d1": (d1, CARDS[0]), "d2": (d2, CARDS[1]), "d3": (rng.integers(0, CARD3, n).astype(np.int32), CARD3), "one": (np.zeros(n, dtype=np.int32), 1)}
    t = Table(OFFS + e, mask, disc, [("d1", "d2", "d3", "one")])
    t.size = size
    # the counts are the prescribed sizes, in both orders of the variables
    key, G = mr.keys([d1, d2], CARDS)
    assert np.array_equal(np.bincount(key, minlength=G), size)
    return t


def spread(c, nc, start=0):
    """c distinct columns of a table of nc, out of order and across its 16-column tiles, the last column among them."""
    step = next(s for s in (5, 7, 3, 1) if np.gcd(s, nc) == 1)
    return [(nc - 1 - start - step * i) % nc for i in range(c)]


def check_exact(table, plans, res):
    for (cont, names), got in zip(plans, res):
        want = table.want(cont, names)
        assert got.shape == want.shape, (cont, names)
        if not np.array_equal(got, want.astype(np.float64)):
            g, s = np.argwhere(got != want)[0]
            raise AssertionError(f"plan {cont} | {names}: configuration {g} ({int(want[g, 0])} rows) statistic {s}: got {got[g, s]!r}, want {int(want[g, s])}; "
                                 f"{int((got != want).sum())} cells differ")


def check_full(table, names, S, P, cols):
    count, wS, wP = table.pooled(tuple(names), table.shifted_int())
    wS, wP = wS[:, :cols], wP[:, :cols, :cols]
    assert np.array_equal(S, wS.astype(np.float64)), (names, np.argwhere(S != wS)[:4].tolist())
    assert np.array_equal(P, wP.astype(np.float64)), (names, np.argwhere(P != wP)[:4].tolist(), count[np.argwhere(P != wP)[:4, 0]].tolist())
    return count


# ---- exact leg: the full Gram --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("nc", [1, 16, 17, 32, 33, 48, 49, 64])
def test_full_gram(pbn, main, nc, dtype):
    h = Handle(pbn, main, nc, dtype)
    nct = (nc + 15) // 16
    # every sum and every product of every configuration: the row list of (d1, d2) through the mirror
    names, S, P, r = h.full(("d1", "d2"))
    count = check_full(main, names, S, P, nc)
    assert np.array_equal(count, main.size)
    order, launched, nblk = mr.gram_launch(count)
    assert order == 0                                    # by ensure_full's formula this table is not aligned
    assert r == dict(r, nct=nct, form=1, nblk=nblk, launched=launched, order=0)
    # no discrete variable: the contiguous gram_glds kernels on pieces of the table; a one-category variable: G = 1 with a row list
    names, S, P, r = h.full(())
    check_full(main, names, S, P, nc)
    assert r == dict(r, nct=nct, form=2, nblk=-(-main.n // PIECE), launched=-(-main.n // PIECE), order=2)
    names, S, P, r = h.full(("one",))
    check_full(main, names, S, P, nc)
    assert r == dict(r, nct=nct, form=1, nblk=-(-main.n // PIECE), order=2)
    # a test's entries of them, in both orders of the variables (order_maps), over coarser groupings, and the counts alone
    c16, c3 = spread(min(16, nc), nc), spread(min(3, nc), nc, 1 if nc > 3 else 0)
    plans = [(c16, ("d1", "d2")), (c16, ("d2", "d1")), (c3, ("d1", "d2")), (c3, ("d2", "d1")), ([nc - 1], ("d1",)), (c3, ("d2",)), (c3, ()),
             (c16, ("one",)), (c3, ("one", "d1")), (c3, ("d3", "d2")), (c3, ("d2", "d3", "d1")), ([], ("d1", "d2")), ([], ("d2", "d1"))]
    res, recs = h.moments(plans)
    check_exact(main, plans, res)
    for (cont, ds), rec in zip(plans, recs):
        assert PATH[rec["path"]] == ("full" if cont else "count"), (cont, ds, rec)
        if cont:
            key, G = mr.keys([main.disc[v][0] for v in ds], [main.disc[v][1] for v in ds])
            cnt = np.bincount(key, minlength=G) if ds else np.array([main.n])
            order, launched, nblk = mr.gram_launch(cnt)
            assert rec == dict(rec, nct=nct, form=1 if ds else 2, nblk=nblk, launched=launched, order=order), (cont, ds)


def order_table(seed):
    """One configuration of 9 pieces beside 11 one-piece configurations (variable a: aligned, with padding blocks) and beside 12
    (variable b: plain stripe-major)."""
    big = 8 * PIECE + 5
    small_a = [1, 63, 64, 65, 257, 1023, 4096, 4095, 2, 31, 33]
    small_b = [1, 63, 64, 65, 257, 1023, 4096, 4095, 2, 31, 32, 1]
    assert sum(small_a) == sum(small_b) and max(small_a + small_b) <= PIECE
    rng = np.random.default_rng(seed)
    codes = {}
    for name, small in (("a", small_a), ("b", small_b)):
        size = np.array(small[:4] + [big] + small[4:])
        cfg = np.repeat(np.arange(len(size)), size)
        codes[name] = (cfg[rng.permutation(len(cfg))].astype(np.int32), len(size))
    n = big + sum(small_a)
    e, mask = int_e(n, seed + 1)
    return Table(OFFS + e, mask, codes, [("a",), ("b",)])


@pytest.fixture(scope="module")
def order_tab():
    return order_table(21)


@pytest.mark.parametrize("nc,dtype", [(64, "float64"), (33, "float32")])
def test_launch_order(pbn, order_tab, nc, dtype):
    h = Handle(pbn, order_tab, nc, dtype)
    for name, want_order in (("a", 1), ("b", 0)):
        names, S, P, r = h.full((name,))
        count = check_full(order_tab, names, S, P, nc)
        order, launched, nblk = mr.gram_launch(count)       # the switch restated: cells <= 2 nblk + 64
        assert order == want_order and nblk == 9 + len(count) - 1
        assert r == dict(r, form=1, nblk=nblk, launched=launched, order=want_order), name
        assert (r["launched"] > r["nblk"]) == (want_order == 1)
    plans = [(spread(min(16, nc), nc), ("a",)), (spread(2, nc), ("b",))]
    res, recs = h.moments(plans)
    check_exact(order_tab, plans, res)
    assert [rec["order"] for rec in recs] == [1, 0]


@pytest.fixture(scope="module")
def switch_tab():
    """G = 4096 (16 x 256: the last full Gram, 12 key bits) and G = 4097 (17 x 241: the sorted kernels, 13 key bits); the first and the last
    configuration of both are empty."""
    n = 20000
    rng = np.random.default_rng(31)
    e, mask = int_e(n, 32)
    k1, k2 = rng.integers(1, 4095, n), rng.integers(1, 4096, n)
    disc = {"p16": ((k1 % 16).astype(np.int32), 16), "p256": ((k1 // 16).astype(np.int32), 256),
            "q17": ((k2 % 17).astype(np.int32), 17), "q241": ((k2 // 17).astype(np.int32), 241)}
    return Table((OFFS + e)[:, :17], mask[:, :17], disc, [("p16", "p256"), ("q17", "q241")])   # 17 columns: 4097 x 66 x 66 would be 150 MB


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_configurations_at_the_switch(pbn, switch_tab, dtype):
    nc = 17
    assert 16 * 256 == FULL_MAX_G and 17 * 241 == FULL_MAX_G + 1
    h = Handle(pbn, switch_tab, nc, dtype)
    cols = [16, 0, 5]
    plans = [(cols, ("p16", "p256")), (cols, ("p256", "p16")), (cols, ("q17", "q241")), (cols, ("q241", "q17")), ([], ("q17", "q241"))]
    res, recs = h.moments(plans)
    check_exact(switch_tab, plans, res)
    assert [PATH[r["path"]] for r in recs] == ["full", "full", "sorted", "sorted", "count"]
    assert recs[0]["G"] == 4096 and recs[2]["G"] == 4097 and recs[2]["nulls"] == 0
    assert res[0][0, 0] == 0 and res[0][-1, 0] == 0 and res[2][0, 0] == 0 and res[2][-1, 0] == 0
    names, S, P, r = h.full(("p16", "p256"))
    check_full(switch_tab, names, S, P, nc)


# ---- exact leg: the per-test sorted kernels -------------------------------------------------------------------------------------------
GROUPINGS = (("d1", "d2"), ("d2", "d1"), ("d1",), ("d2",), (), ("one",), ("d3", "d2"))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sorted_kernels(pbn, main, dtype):
    """66 columns: no full Gram.  Every C, each plan with a column >= 64, one launch per C over groupings of different nblk."""
    assert NCOL > FULL_MAX_CONT
    h = Handle(pbn, main, NCOL, dtype)
    plans = [(spread(c, NCOL, c % 2), ds) for c in range(1, SORTED_MAX_CONT + 1) for ds in GROUPINGS]
    assert all(max(cont) >= 64 for cont, _ in plans)
    res, recs = h.moments(plans)
    check_exact(main, plans, res)
    nblk = {}
    for ds in GROUPINGS:
        key, G = mr.keys([main.disc[v][0] for v in ds], [main.disc[v][1] for v in ds])
        nblk[ds] = sum(mr.pieces(np.bincount(key, minlength=G) if ds else [main.n]))
    assert len(set(nblk.values())) > 2
    for (cont, ds), rec in zip(plans, recs):
        assert rec == dict(rec, path=2, c=len(cont), nulls=0, nblk=nblk[ds], grid_x=max(nblk.values()), batch=len(GROUPINGS)), (cont, ds)


NULL_COLS = (1, 4, 6, 10, 13)


@pytest.fixture(scope="module")
def null_tab(main):
    """The main table's configurations with NaN cells in five columns and a discrete column with null cells (code -1)."""
    n = main.n
    rng = np.random.default_rng(41)
    e, mask = int_e(n, 42, NULL_COLS, 0.1)
    dn = rng.integers(0, 4, n).astype(np.int32)
    dn[rng.random(n) < 0.15] = -1
    disc = {"d1": main.disc["d1"], "d2": main.disc["d2"], "dn": (dn, 4)}
    return Table(OFFS + e, mask, disc, [("d1", "d2", "dn")])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_sorted_kernels_with_nulls(pbn, null_tab, dtype):
    nc = 24
    h = Handle(pbn, null_tab, nc, dtype)     # the shifts of the null columns: the Python side's nanmean over the valid cells
    touching = {1: [4], 2: [4, 0], 7: list(range(7)), 16: list(range(15, -1, -1))}
    clean = [0, 2, 3]
    assert all(set(c) & set(NULL_COLS) for c in touching.values()) and not set(clean) & set(NULL_COLS)
    plans = []
    for ds in (("d1", "d2"), ("d2", "d1"), (), ("dn",), ("d1", "dn"), ("dn", "d2", "d1")):
        plans += [(cont, ds) for cont in touching.values()] + [(clean, ds), ([], ds)]
    res, recs = h.moments(plans)
    check_exact(null_tab, plans, res)
    for (cont, ds), rec, got in zip(plans, recs, res):
        if not cont:
            assert PATH[rec["path"]] == "count"
        elif cont is clean:
            assert PATH[rec["path"]] == "full", (cont, ds)
        else:
            assert rec == dict(rec, path=2, c=len(cont), nulls=1), (cont, ds)
            # fewer rows than the configuration holds wherever one of its rows has a null cell
            assert got[:, 0].sum() < null_tab.want([], ds)[:, 0].sum()
    # the null bucket of dn belongs to no configuration
    assert res[plans.index(([], ("dn",)))][:, 0].sum() == (null_tab.disc["dn"][0] >= 0).sum() < null_tab.n


# ---- exact leg: the LDS-cell kernel ----------------------------------------------------------------------------------------------------
def check_legacy(table, plans, recs):
    for (cont, ds), rec in zip(plans, recs):
        G = int(np.prod([table.disc[v][1] for v in ds])) if ds else 1
        windows = -(-G // mr.legacy_window(len(cont)))
        assert rec == dict(rec, path=3, c=len(cont), windows=windows), (cont, ds, rec)
        assert (rec["nblocks"], rec["chunks"]) == mr.legacy_launch(table.n, rec["rows"]), rec


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_legacy_kernel(pbn, main, dtype):
    assert (SORTED_MAX_CONT + 1, MAX_CONT) == (17, 24)       # the first and the last c the LDS-cell kernel serves
    assert (mr.legacy_window(17), mr.legacy_window(24)) == (37, 18)
    h = Handle(pbn, main, NCOL, dtype)
    # single plans: 56 configurations take 2 and 4 windows, the 40 of (d3, d2) take 2 and 3, one configuration takes one
    singles = [(spread(17, NCOL), ("d1", "d2")), (spread(24, NCOL), ("d1", "d2")), (spread(17, NCOL, 1), ("d3", "d2")), (spread(24, NCOL, 2), ("d3", "d2")),
               (spread(24, NCOL, 3), ("d2", "d1")), (spread(17, NCOL, 4), ()), (spread(24, NCOL, 5), ("one",))]
    seen_windows = set()
    for plan in singles:
        res, recs = h.moments([plan])
        check_exact(main, [plan], res)
        check_legacy(main, [plan], recs)
        assert recs[0]["rows"] == recs[0]["windows"]
        seen_windows.add((recs[0]["c"], recs[0]["G"], recs[0]["windows"]))
    assert {(17, 56, 2), (24, 56, 4), (17, 40, 2), (24, 40, 3), (17, 1, 1), (24, 1, 1)} <= seen_windows
    # batches of 8 plans and more: 512 blocks, two chunks each on this table - and the trailing blocks own no chunk
    for c in (17, 24):
        plans = [(spread(c, NCOL, s), ds) for s, ds in enumerate((("d1", "d2"), ("d2", "d1"), ("d3", "d2"), ("d2", "d3"), ("d1", "d2"), ("d2",), ("d2", "d1"),
                                                                   ("d1", "d2"), ("d3", "d2")))]
        res, recs = h.moments(plans)
        check_exact(main, plans, res)
        check_legacy(main, plans, recs)
        assert recs[0]["rows"] >= 8 and (recs[0]["nblocks"], recs[0]["chunks"]) == (512, 2)
        assert 512 * 2 * 64 - main.n >= 2 * 64 * 100          # over a hundred trailing blocks without a chunk


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fewer_rows_than_a_chunk(pbn, dtype):
    """N = 61 < 64: one chunk, one block of the legacy kernel; one piece per configuration everywhere else."""
    n = 61
    rng = np.random.default_rng(51)
    e, mask = int_e(n, 52)
    disc = {"d1": (rng.integers(0, 3, n).astype(np.int32), 3), "d2": (rng.integers(1, 4, n).astype(np.int32), 5)}
    t = Table(OFFS + e, mask, disc, [("d1", "d2")])
    h = Handle(pbn, t, NCOL, dtype)
    plans = [(spread(17, NCOL), ("d1", "d2")), (spread(24, NCOL, 1), ("d2", "d1")), (spread(24, NCOL, 2), ()), (spread(16, NCOL), ("d2", "d1")), (spread(3, NCOL), ())]
    res, recs = h.moments(plans)
    check_exact(t, plans, res)
    check_legacy(t, plans[:3], recs[:3])
    assert all((r["nblocks"], r["chunks"]) == (1, 1) for r in recs[:3]) and [PATH[r["path"]] for r in recs[3:]] == ["sorted", "sorted"]
    h = Handle(pbn, t, 64, dtype)
    for ds in (("d1", "d2"), ()):
        names, S, P, r = h.full(ds)
        check_full(t, names, S, P, 64)


# ---- rounding leg ------------------------------------------------------------------------------------------------------------------------
def real_table(main, dtype, seed):
    """Real values as wide() of tests/test_gram_paths_gpu.py builds them: mixed columns, scales 0.5 .. 2, offsets up to +-30."""
    rng = np.random.default_rng(seed)
    mix = np.eye(NCOL) + 0.15 * np.tril(rng.normal(size=(NCOL, NCOL)), -1)
    data = rng.normal(size=(main.n, NCOL)) @ mix.T * rng.uniform(0.5, 2.0, size=NCOL) + rng.uniform(-30, 30, size=NCOL)
    data = data.astype(dtype)
    return Table(data, np.zeros(data.shape, dtype=bool), {k: main.disc[k] for k in ("d1", "d2")}, [("d1", "d2")])


def check_bound(table, x, cont, names, got):
    """|got - want| <= (n_g + 2) 2^-53 sum |x_i x_j| per cell (sums: sum |x_i|); returns the worst fraction of the bound."""
    count, S, P, aS, aP = table.pooled(tuple(names), x, real=True)
    want = mr.layout(count, S[:, cont], P[:, cont][:, :, cont])
    mag = mr.layout(count, aS[:, cont], aP[:, cont][:, :, cont])
    assert np.array_equal(got[:, 0], count.astype(np.float64))
    bound = ((count[:, None] + 2) * 2.0 ** -53 * mag)[:, 1:].astype(np.longdouble)
    err = np.abs(got[:, 1:].astype(np.longdouble) - want[:, 1:])
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), (cont, names, "configuration", int(worst[0]), "rows", int(count[worst[0]]), "statistic", int(worst[1]) + 1,
                                  "error", float(err[worst]), "bound", float(bound[worst]))
    frac = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
    NOTES["frac"] = max(NOTES["frac"], frac)
    return frac


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rounding(pbn, main, dtype):
    t = real_table(main, dtype, 61)
    h66 = Handle(pbn, t, NCOL, dtype, shifts=None)
    x = t.values.astype(np.float64) - h66.shift          # fl64(x - shift), the kernels' own first operation
    fracs = {}
    # 64 columns: the full Gram of (d1, d2) through the mirror and of the whole table through the contiguous kernels
    h64 = Handle(pbn, t, 64, dtype, shifts=None)
    assert np.array_equal(h64.shift, h66.shift[:64])
    allc = list(range(64))
    iu = np.triu_indices(64)
    for ds in (("d1", "d2"), ()):
        names, S, P, r = h64.full(ds)
        count = t.pooled(tuple(names), x, real=True)[0]
        got = mr.layout(count.astype(np.float64), S, P)
        fracs[("full", ds)] = check_bound(t, x, allc, names, got)
    # 66 columns: the sorted kernels and the LDS-cell kernel
    plans = [(spread(c, NCOL), ds) for c in (1, 2, 7, 16, 17, 24) for ds in (("d1", "d2"), ("d2", "d1"), ())]
    res, recs = h66.moments(plans)
    for (cont, ds), rec, got in zip(plans, recs, res):
        assert PATH[rec["path"]] == ("sorted" if len(cont) <= SORTED_MAX_CONT else "legacy")
        key = (PATH[rec["path"]], ds)
        fracs[key] = max(fracs.get(key, 0.0), check_bound(t, x, cont, ds, got))
    print(f"\nworst fraction of the rounding bound ({dtype}): " + ", ".join(f"{k[0]} {'x'.join(k[1]) or 'none'} {v:.3f}" for k, v in fracs.items()))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def test_every_launch_form_was_seen():
    want = {("count",)}
    for b in (8, 4):
        for nct in (1, 2, 3, 4):
            want |= {("full", b, nct, 1, 0),     # row list through the mirror, plain stripe-major
                     ("full", b, nct, 1, 2),     # G = 1 with a row list (a one-category variable)
                     ("full", b, nct, 2, 2)}     # no discrete variable: the contiguous gram_glds kernels
        want |= {("sorted", b, c, 0) for c in range(1, SORTED_MAX_CONT + 1)}
        want |= {("sorted", b, c, 1) for c in (1, 2, 7, 16)}
        want |= {("legacy", b, c, chunked) for c in (17, 24) for chunked in (False, True)}
    want |= {("full", 8, 4, 1, 1), ("full", 4, 3, 1, 1)}          # the aligned order: (STEP, D) = (32, 4) and (64, 3)
    missing = sorted(want - SEEN, key=str)
    assert not missing, missing
    assert NOTES["padding"], "no aligned launch with padding blocks"
    assert NOTES["early_return"], "no sorted launch whose grid is wider than a test's nblk"
    assert not any(f[0] == "full" and f[3] == 0 for f in SEEN), "the column-gather form ran: the mirror was not built"
    print(f"\nplans by path: {PLANS}; launch forms seen: {len(SEEN)}; worst fraction of the rounding bound {NOTES['frac']:.3f}")
