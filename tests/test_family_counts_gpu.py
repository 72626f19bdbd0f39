"""GPU tier: the family-count pass of the score engine (csrc/family_counts.hip) at every launch shape, cell by cell.

One unit = (family, region): the joint counts of a variable and its parents (the variable fastest, the parents in ascending column order)
over one contiguous row range of the permuted table - a CV fold, the hold-out train / test part, or all rows.  The test aid
pbn_debug_family_counts returns the tables of a batch as the batch path of pbn_score_batch counts them, and which form served each unit
(0 host loop, 1 LDS on the byte mirror, 2 LDS on the int32 codes, 3 global atomics).  The reference is numpy.bincount on the codes permuted
with pbn_split_layout; every cell of every region must be EQUAL.

Reference routine: factors/discrete/discrete_indices.cpp:134-150 (joint_counts)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST, LDS_U8, LDS_I32, GLOBAL = 0, 1, 2, 3
BIC, CVLIK, HOLDOUT = 0, 2, 3
SPLIT_NONE, SPLIT_CV, SPLIT_HOLDOUT, SPLIT_VALIDATED = 0, 1, 2, 3
MAX_VARS, LDS_CELLS, MAX_CELLS = 8, 4096, 1 << 20

# column -> cardinality.  0-3 small, 4-10 binary (up to 7 parents), 11/12: 241 x 17 = 4 097 cells, 13-15: 16^3 = 4 096, 16-18: 13 x 15 x 21 = 4 095,
# 19 a one-category variable, 20 constant (every row in category 2 of 3); an optional column 21 of 300 categories takes the byte mirror away
CARDS = [2, 3, 4, 5, 2, 2, 2, 2, 2, 2, 2, 241, 17, 16, 16, 16, 13, 15, 21, 1, 3]
SMALL = [(0, []), (19, []), (4, [5]), (1, [0, 2]), (3, [2, 1, 0]), (20, []), (0, [20]), (4, [5, 6, 7, 8, 9, 10]), (0, [10, 9, 8, 7, 6, 5, 4]),
         (1, [0, 4, 5, 6, 7, 8, 9, 10])]
SWITCH = [(16, [17, 18]), (13, [14, 15]), (12, [11]), (11, [12])]
LARGE = [(13, [14, 15, 11]), (13, [14, 15, 11, 0])]   # 987 136 cells (global), 1 974 272 (above the cap: host)


@pytest.fixture(scope="module")
def lib():
    import pybnesian_amd
    from pybnesian_amd import _lib

    pybnesian_amd.load_library()
    L = _lib.load()
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_int64)
    L.pbn_debug_family_counts.restype = C.c_int
    L.pbn_debug_family_counts.argtypes = [C.c_void_p, C.c_int, C.c_int, ip, ip, ip, lp, lp, C.c_int64, ip]
    return L


class Data:
    """Discrete-only score data over random codes, with its numpy reference."""

    def __init__(self, lib, rows, split=SPLIT_NONE, k=0, ratio=0.0, seed=3, wide=False, fill=None):
        from pybnesian_amd import _lib
        from pybnesian_amd.dataset import default_context

        self.lib, self._lib, self.rows, self.k = lib, _lib, rows, k
        self.cards = CARDS + ([300] if wide else [])
        self.perm = np.zeros(rows, dtype=np.int32)
        self.limits = np.zeros(max(k, 0) + 1, dtype=np.int32)
        n_cv, n_hold = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.pbn_split_layout(rows, split, k, C.c_uint32(seed), ratio, self.perm.ctypes.data, self.limits.ctypes.data if k > 1 else None,
                                        C.byref(n_cv), C.byref(n_hold)))
        self.n_cv, self.n_hold = n_cv.value, n_hold.value
        rng = np.random.default_rng(rows * 7 + split)
        self.codes = [rng.integers(0, c, size=rows).astype(np.int32) for c in self.cards]
        self.codes[20][:] = 2
        if fill is not None:
            fill(self)
        self.ctx = default_context()
        h = C.c_void_p()
        _lib.check(lib.pbn_scoredata_create_discrete(self.ctx.handle, rows, split, k, C.c_uint32(seed), ratio, C.byref(h)))
        self.h = h
        ptrs = (C.c_void_p * len(self.codes))(*[c.ctypes.data for c in self.codes])
        _lib.check(lib.pbn_scoredata_set_discrete(h, len(self.codes), ptrs, _lib.int_array(self.cards)))
        self.permuted = [c[self.perm] for c in self.codes]
        self.wide = wide

    def close(self):
        self.lib.pbn_scoredata_destroy(self.h)

    def regions(self, kind):
        if kind == CVLIK:
            return [(int(self.limits[f]), int(self.limits[f + 1])) for f in range(self.k)]
        if kind == HOLDOUT:
            return [(0, self.n_cv), (self.n_cv, self.n_cv + self.n_hold)]
        return [(0, self.n_cv)]

    def cells(self, fam):
        return int(np.prod([self.cards[c] for c in [fam[0]] + list(fam[1])], dtype=np.int64))

    def expected(self, fam, region):
        cols = [fam[0]] + sorted(fam[1])
        key, stride = np.zeros(region[1] - region[0], dtype=np.int64), 1
        for c in cols:
            key += self.permuted[c][region[0]: region[1]].astype(np.int64) * stride
            stride *= self.cards[c]
        return np.bincount(key, minlength=stride)

    def form(self, fam):
        if 1 + len(fam[1]) > MAX_VARS or self.cells(fam) > MAX_CELLS:
            return HOST
        if self.cells(fam) > LDS_CELLS:
            return GLOBAL
        return LDS_I32 if self.wide else LDS_U8

    def counted(self, kind, fams):
        """[(table, form)] per unit, unit = family * regions + region."""
        R = len(self.regions(kind))
        var, off, par = [f[0] for f in fams], [0], []
        for f in fams:
            par.extend(f[1])
            off.append(len(par))
        total = sum(self.cells(f) for f in fams) * R
        out_off = np.zeros(len(fams) * R + 1, dtype=np.int64)
        out = np.full(total, -1, dtype=np.int64)
        form = np.full(len(fams) * R, -1, dtype=np.int32)
        i32 = self._lib.int_array
        self._lib.check(self.lib.pbn_debug_family_counts(self.h, kind, len(fams), i32(var), i32(off), i32(par or [0]),
                                                         out_off.ctypes.data_as(C.POINTER(C.c_int64)), out.ctypes.data_as(C.POINTER(C.c_int64)), total,
                                                         form.ctypes.data_as(C.POINTER(C.c_int))))
        assert out_off[-1] == total
        return [(out[out_off[u]: out_off[u + 1]], int(form[u])) for u in range(len(fams) * R)]

    def check(self, kind, fams):
        regions = self.regions(kind)
        got = self.counted(kind, fams)
        seen = set()
        for i, fam in enumerate(fams):
            for ri, region in enumerate(regions):
                table, form = got[i * len(regions) + ri]
                assert form == self.form(fam), (fam, region, form)
                want = self.expected(fam, region)
                assert table.shape == want.shape and np.array_equal(table, want), (fam, region, form, int(np.abs(table - want).sum()))
                assert int(table.sum()) == region[1] - region[0]
                seen.add(form)
        return seen

    def stats(self):
        d, h, l = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._lib.check(self.lib.pbn_scoredata_discrete_stats(self.h, C.byref(d), C.byref(h), C.byref(l)))
        return d.value, h.value, l.value


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 8193, 20000])
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "int32"])
def test_every_row_count_through_both_mirrors(lib, rows, wide):
    """No split: one region of all rows, around the workgroup (256), the byte form's slice (2 048) and 4 096 / 8 192 rows; tables of 1, 2, 4
    ... 256 cells with 0 - 8 parents, and 4 095 / 4 096 / 4 097 cells at the LDS / global switch.  `wide` adds a column of 300 categories to the
    score data: the same families are then counted from the int32 codes."""
    d = Data(lib, rows, wide=wide)
    try:
        fams = SMALL + SWITCH + ([(21, [0]), (0, [21])] if wide else [])
        assert d.check(BIC, fams) == {HOST, GLOBAL, LDS_I32 if wide else LDS_U8}
    finally:
        d.close()


@pytest.mark.parametrize("rows,split,k,ratio,kinds", [
    (1001, SPLIT_CV, 3, 0.0, (CVLIK, BIC)),
    (20000, SPLIT_CV, 10, 0.0, (CVLIK,)),
    (5003, SPLIT_VALIDATED, 3, 0.2, (CVLIK, HOLDOUT)),
    (5003, SPLIT_HOLDOUT, 0, 0.2, (HOLDOUT,)),
], ids=["cv3x1001", "cv10x20000", "validated", "holdout"])
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "int32"])
def test_unaligned_regions(lib, rows, split, k, ratio, kinds, wide):
    """Folds and hold-out parts start on rows that are no multiple of anything: every region's table against bincount on its own rows."""
    d = Data(lib, rows, split, k, ratio, wide=wide)
    try:
        assert rows % 8 == 0 or any(r0 % 8 for r0, _ in d.regions(kinds[0]))
        for kind in kinds:
            d.check(kind, SMALL + SWITCH)
    finally:
        d.close()


def test_tables_near_and_above_the_cap(lib):
    """987 136 cells go through the global form, 1 974 272 cells (and nine variables) through the host loop - with and without regions."""
    for args in ((20000,), (5003, SPLIT_VALIDATED, 3, 0.2)):
        d = Data(lib, *args)
        try:
            for kind in ((BIC,) if len(args) == 1 else (CVLIK, HOLDOUT)):
                got = d.counted(kind, LARGE)
                regions = d.regions(kind)
                for i, fam in enumerate(LARGE):
                    for ri, region in enumerate(regions):
                        table, form = got[i * len(regions) + ri]
                        assert form == (GLOBAL if i == 0 else HOST)
                        assert np.array_equal(table, d.expected(fam, region))
        finally:
            d.close()


def test_one_cell_holds_a_whole_region(lib):
    """Skew: column 0 is category 1 on every row of the first fold and category 0 elsewhere - one cell takes every add of one region and
    none of the others; the constant column 20 does the same to every region."""
    def fill(d):
        inside = np.zeros(d.rows, dtype=bool)
        inside[d.perm[d.limits[0]: d.limits[1]]] = True
        d.codes[0][:] = inside.astype(np.int32)

    d = Data(lib, 9001, SPLIT_CV, 3, fill=fill)
    try:
        got = d.counted(CVLIK, [(0, []), (0, [20]), (20, [0])])
        sizes = [r1 - r0 for r0, r1 in d.regions(CVLIK)]
        assert [t.tolist() for t, _ in got[:3]] == [[0, sizes[0]], [sizes[1], 0], [sizes[2], 0]]
        d.check(CVLIK, [(0, []), (0, [20]), (20, [0]), (1, [0, 20])])
    finally:
        d.close()


def distinct_families(n, rng):
    """n distinct (variable, parent set) over the small columns 0 - 10 (4 246 of them with up to 4 parents), parents given in random order."""
    out, seen = [], set()
    while len(out) < n:
        size = int(rng.integers(1, 6))
        cols = rng.choice(11, size=size, replace=False).tolist()
        key = (cols[0], tuple(sorted(cols[1:])))
        if key not in seen:
            seen.add(key)
            out.append((cols[0], cols[1:]))
    return out


@pytest.mark.parametrize("n_fam", [1, 2, 257, 3000])
def test_batch_sizes(lib, n_fam):
    d = Data(lib, 4097)
    try:
        before = d.stats()
        d.check(BIC, distinct_families(n_fam, np.random.default_rng(n_fam)))
        after = d.stats()
        assert after[0] - before[0] == n_fam and after[1] == before[1] and after[2] - before[2] == 1   # one launch for the whole batch
    finally:
        d.close()


def test_repeated_families_are_counted_once(lib):
    d = Data(lib, 5000, SPLIT_CV, 3)
    try:
        fams = [(1, [0, 2]), (1, [2, 0]), (3, []), (1, [0, 2]), (3, []), (12, [11]), (12, [11])]
        before = d.stats()
        d.check(CVLIK, fams)
        after = d.stats()
        assert after[0] - before[0] == 3 * 3    # three distinct families x three folds
    finally:
        d.close()


def test_chunked_batch_equals_its_parts(lib, monkeypatch):
    """A count buffer of 5 000 cells: the batch goes in several chunks (a 4 097-cell table in a chunk of its own) and returns what its parts
    return unchunked."""
    d = Data(lib, 6001, SPLIT_CV, 3)
    try:
        fams = distinct_families(60, np.random.default_rng(1)) + SWITCH + [(0, [10, 9, 8, 7, 6, 5, 4])]
        whole_launches = d.stats()[2]
        parts = [d.counted(CVLIK, fams[i: i + 7]) for i in range(0, len(fams), 7)]
        unchunked = [u for p in parts for u in p]
        monkeypatch.setenv("PBN_DISCRETE_CHUNK_CELLS", "5000")
        before = d.stats()[2]
        chunked = d.counted(CVLIK, fams)
        assert d.stats()[2] - before > 4 and before > whole_launches
        assert len(chunked) == len(unchunked)
        for (a, fa), (b, fb) in zip(chunked, unchunked):
            assert fa == fb and np.array_equal(a, b)
        d.check(CVLIK, fams)
    finally:
        d.close()


def test_knob_off_is_the_host_loop(lib, monkeypatch):
    d = Data(lib, 3000)
    try:
        monkeypatch.setenv("PBN_DISCRETE_COUNTS", "0")
        got = d.counted(BIC, SMALL + SWITCH)
        assert {f for _, f in got} == {HOST} and d.stats()[0] == 0
        for (table, _), fam in zip(got, SMALL + SWITCH):
            assert np.array_equal(table, d.expected(fam, (0, 3000)))
    finally:
        d.close()
