"""GPU tier: the device path of discrete networks through the C ABI (csrc/discrete_model.hip) at every launch shape.

pbn_dtable_family_counts: every cell of every family EQUAL to the restatement's null-aware joint counts, with the form that served
it (0 host loop, 1 LDS on the byte mirror, 2 LDS on the int32 codes, 3 global atomics).  pbn_dnet_logl: bit for bit the restatement's
node-order sum, NaN and -inf rows included.  pbn_dnet_slogl: within the derived bound of the exact (math.fsum) value, per node
(cells_n + 1) 2^-53 sum |count x logprob| - one rounding per product, recursive summation over the cells - and for the total the sum
of those plus (n_nodes - 1) 2^-53 sum_n |slogl_n|; exactly -inf where the exact value is; the same bits whatever the chunking and
on a second call.

Row tiles of dnet_logl_kernel: 2 048 rows on the byte mirror, 1 024 on the int32 codes - hence 1 023 / 1 024 / 1 025 next to the
row counts around 256 and 2 048.

Reference routines: factors/discrete/discrete_indices.cpp:134-150, learning/parameters/mle_DiscreteFactor.cpp:5-41,
factors/discrete/DiscreteFactor.cpp:91-171, models/BayesianNetwork.hpp:960-994."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_model_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

HOST, LDS_U8, LDS_I32, GLOBAL = 0, 1, 2, 3
MAX_VARS, LDS_CELLS, MAX_CELLS = 8, 4096, 1 << 20
ROWS = [0, 1, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097]
NULLS = ["none", "first", "last", "allnull", "parent"]

# column -> cardinality.  0-3 small, 4-11 binary (seven and eight parents), 12 one category, 13 255 categories, 14-16: 16^3 = 4 096 cells,
# 17/18: 241 x 17 = 4 097 cells; an optional column 19 of 300 categories takes the byte mirror away
CARDS = [2, 3, 4, 5, 2, 2, 2, 2, 2, 2, 2, 2, 1, 255, 16, 16, 16, 241, 17]
NO_PARENTS = [(0, []), (12, []), (13, [])]
SEVEN = (4, [5, 6, 7, 8, 9, 10, 11])            # eight variables: at the cap
EIGHT = (1, [4, 5, 6, 7, 8, 9, 10, 11])         # nine: the host loop for the counts, refused by pbn_dnet_create
SWITCH = [(14, [15, 16]), (17, [18]), (18, [17])]   # 4 096 cells (LDS), 4 097 (global), 4 097 the other way round
DESCENDING = [(3, [2, 1, 0]), (3, [0, 1, 2]), (1, [13, 0]), (0, [12])]
FAMILIES = NO_PARENTS + [SEVEN] + SWITCH + DESCENDING
WIDE = [(19, []), (19, [0]), (0, [19, 1])]
PARENT_ONLY = 5    # the "parent" null pattern puts its nulls here: a column that is a parent in SEVEN / EIGHT and nobody's variable


@pytest.fixture(scope="module")
def lib():
    import pybnesian_amd
    from pybnesian_amd import _lib

    pybnesian_amd.load_library()
    return _lib.load()


def make_codes(rows, cards, nulls, seed):
    rng = np.random.default_rng(seed * 100003 + rows)
    codes = [rng.integers(0, c, size=rows).astype(np.int32) for c in cards]
    if rows:
        if nulls == "first":
            for c in (0, 3, 5, 13, 15, len(cards) - 1):
                codes[c][0] = -1
        elif nulls == "last":
            for c in (0, 2, 6, 13, 16, len(cards) - 1):
                codes[c][-1] = -1
        elif nulls == "allnull":
            codes[1][:] = -1
        elif nulls == "parent":
            codes[PARENT_ONLY][rng.random(rows) < 0.25] = -1
            codes[PARENT_ONLY][rows // 2] = -1
    return codes


class Table:
    def __init__(self, lib, codes, cards):
        from pybnesian_amd import _lib
        from pybnesian_amd.dataset import default_context

        self.lib, self._lib, self.codes, self.cards = lib, _lib, codes, list(cards)
        self.rows = len(codes[0])
        self.ctx = default_context()
        ptrs = (C.c_void_p * len(codes))(*[c.ctypes.data for c in codes])
        h = C.c_void_p()
        _lib.check(lib.pbn_dtable_create(self.ctx.handle, self.rows, len(codes), ptrs, _lib.int_array(self.cards), C.byref(h)))
        self.h = h
        self.wide = max(self.cards) > 255

    def close(self):
        self.lib.pbn_dtable_destroy(self.h)

    def cells(self, fam):
        return R.strides_of(self.cards, fam)[2]

    def form(self, fam):
        if self.rows == 0 or 1 + len(fam[1]) > MAX_VARS or self.cells(fam) > MAX_CELLS:
            return HOST
        if self.cells(fam) > LDS_CELLS:
            return GLOBAL
        return LDS_I32 if self.wide else LDS_U8

    def counted(self, fams, cap=None):
        var, off, par = [f[0] for f in fams], [0], []
        for f in fams:
            par.extend(f[1])
            off.append(len(par))
        total = sum(self.cells(f) for f in fams)
        out_off = np.full(len(fams) + 1, -1, dtype=np.int64)
        out = np.full(max(total, 1), -1, dtype=np.int64)
        form = np.full(max(len(fams), 1), -1, dtype=np.int32)
        i32, lp = self._lib.int_array, C.POINTER(C.c_int64)
        self._lib.check(self.lib.pbn_dtable_family_counts(self.h, len(fams), i32(var), i32(off), i32(par or [0]), out_off.ctypes.data_as(lp),
                                                          out.ctypes.data_as(lp), total if cap is None else cap, form.ctypes.data_as(C.POINTER(C.c_int))))
        assert out_off[-1] == total
        return [(out[out_off[i]: out_off[i + 1]], int(form[i])) for i in range(len(fams))]

    def check_counts(self, fams):
        seen = set()
        for fam, (table, form) in zip(fams, self.counted(fams)):
            want = R.joint_counts_fast(self.codes, self.cards, fam)
            assert form == self.form(fam), (fam, form)
            assert table.shape == want.shape and np.array_equal(table, want), (fam, form, int(np.abs(table - want).sum()))
            seen.add(form)
        return seen


class Net:
    def __init__(self, lib, cards, fams, lps):
        from pybnesian_amd import _lib
        from pybnesian_amd.dataset import default_context

        self.lib, self._lib, self.n = lib, _lib, len(fams)
        var, off, par, cpt = [f[0] for f in fams], [0], [], [0]
        for f, lp in zip(fams, lps):
            par.extend(f[1])
            off.append(len(par))
            cpt.append(cpt[-1] + len(lp))
        self.lp = np.ascontiguousarray(np.concatenate(lps), dtype=np.float64)
        cpt = np.asarray(cpt, dtype=np.int64)
        h = C.c_void_p()
        i32 = _lib.int_array
        _lib.check(lib.pbn_dnet_create(default_context().handle, len(cards), i32(cards), len(fams), i32(var), i32(off), i32(par or [0]),
                                       cpt.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(self.lp), C.byref(h)))
        self.h = h

    def close(self):
        self.lib.pbn_dnet_destroy(self.h)

    def logl(self, table):
        out = np.full(table.rows, 12345.0)
        self._lib.check(self.lib.pbn_dnet_logl(self.h, table.h, _lib_dptr(out)))
        return out

    def slogl(self, table):
        total, per = C.c_double(12345.0), np.full(self.n, 12345.0)
        self._lib.check(self.lib.pbn_dnet_slogl(self.h, table.h, C.byref(total), _lib_dptr(per)))
        return total.value, per

    def stats(self):
        a, b = C.c_int64(-1), C.c_int64(-1)
        self._lib.check(self.lib.pbn_dnet_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def _lib_dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def fitted(codes, cards, fams):
    """The restatement's CPTs of the families on `codes`."""
    return [R.logprob(R.joint_counts_fast(codes, cards, f), cards[f[0]]) for f in fams]


def check_evaluation(lib, table, fams, lps):
    """logl bit for bit, slogl per node and in total within the derived bounds, -inf exactly; returns what was seen."""
    net = Net(lib, table.cards, fams, lps)
    try:
        got = net.logl(table)
        want = R.network_logl(table.codes, table.cards, fams, lps)
        assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True), (table.rows, int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want))))))
        assert net.stats() == ((1, table.rows) if table.rows else (0, 0))
        total, per = net.slogl(table)
        exact = [R.slogl_exact(table.codes, table.cards, f, lp) for f, lp in zip(fams, lps)]
        bound_total = 0.0
        for n, (value, magnitude, cells) in enumerate(exact):
            if value == -math.inf:
                assert per[n] == -math.inf, (fams[n], per[n])
            else:
                bound = R.slogl_bound(cells, magnitude)
                print(f"slogl node {n} {fams[n]}: |got - exact| = {abs(per[n] - value):.3e} bound {bound:.3e}")
                assert abs(per[n] - value) <= bound, (fams[n], per[n], value, bound)
                bound_total += bound
        values = [e[0] for e in exact]
        if -math.inf in values:
            assert total == -math.inf
        else:
            want_total = math.fsum(values)
            bound_total += (len(fams) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in values)
            print(f"slogl total: |got - exact| = {abs(total - want_total):.3e} bound {bound_total:.3e}")
            assert abs(total - want_total) <= bound_total, (total, want_total, bound_total)
        again_total, again_per = net.slogl(table)
        assert again_total == total and np.array_equal(again_per, per)
        return {"nan": bool(np.isnan(want).any()), "neg_inf": bool(np.isneginf(want).any()), "slogl_inf": total == -math.inf}
    finally:
        net.close()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "int32"])
def test_every_row_count_null_pattern_and_form(lib, rows, wide):
    """Counts, logl and slogl of a ten-node network (no parents, seven parents, 4 096 and 4 097 cells, parents in descending order,
    one-category and 255-category variables) and of its one-node networks, under every null pattern.  `wide` adds a column of 300
    categories: the same families then run on the int32 codes."""
    cards = CARDS + ([300] if wide else [])
    fams = FAMILIES + (WIDE if wide else [])
    for nulls in NULLS:
        table = Table(lib, make_codes(rows, cards, nulls, 1), cards)
        try:
            seen = table.check_counts(fams + [EIGHT] + fams[:2])   # (the last two: families repeated in the call)
            if rows:
                assert seen == {HOST, GLOBAL, LDS_I32 if wide else LDS_U8}
            # CPTs fitted on the table itself: every row falls on a cell with a count, slogl is finite
            own = check_evaluation(lib, table, fams, fitted(table.codes, cards, fams))
            assert not own["neg_inf"] and not own["slogl_inf"]
            assert own["nan"] == (rows > 0 and nulls != "none")
            # CPTs fitted on OTHER rows: rows on cells of probability zero give -inf (in logl, and exactly in slogl)
            other = check_evaluation(lib, table, fams, fitted(make_codes(max(rows, 64), cards, "none", 2), cards, fams))
            if rows >= 7:   # (on an all-null column every row is NaN before it can be -inf)
                assert other["slogl_inf"] and other["neg_inf"] == (nulls != "allnull")
            # one node: every family as a network of its own
            for f in (fams[0], SEVEN, SWITCH[1], DESCENDING[0]):
                check_evaluation(lib, table, [f], fitted(table.codes, cards, [f]))
        finally:
            table.close()


def random_families(n, rng):
    """n (variable, up to three parents in random order) over the small columns 0 - 11."""
    out = []
    for _ in range(n):
        cols = rng.choice(12, size=int(rng.integers(1, 5)), replace=False).tolist()
        out.append((cols[0], cols[1:]))
    return out


@pytest.mark.parametrize("rows", [257, 2049, 4097])
@pytest.mark.parametrize("nulls", ["none", "parent", "allnull"])
def test_forty_nodes(lib, rows, nulls):
    fams = random_families(40, np.random.default_rng(40))
    table = Table(lib, make_codes(rows, CARDS, nulls, 3), CARDS)
    try:
        table.check_counts(fams)
        seen = check_evaluation(lib, table, fams, fitted(table.codes, CARDS, fams))
        assert seen["nan"] == (nulls != "none") and not seen["slogl_inf"]
        # smoothed CPTs (no cell of probability zero) fitted elsewhere: a finite slogl that is not the table's own fit
        smooth = [np.log((R.joint_counts_fast(make_codes(500, CARDS, "none", 4), CARDS, f) + 0.5)) - 7.0 for f in fams]
        assert not check_evaluation(lib, table, fams, smooth)["slogl_inf"]
    finally:
        table.close()


def test_tables_above_the_device_cap_take_the_host_loop(lib):
    """255 x 241 x 17 = 1 044 735 cells still count on the device (global form); twice that goes through the host loop in the same call."""
    table = Table(lib, make_codes(4097, CARDS, "last", 5), CARDS)
    try:
        fams = [(13, [17, 18]), (13, [18, 17, 0]), (0, [])]
        got = table.counted(fams)
        assert [f for _, f in got] == [GLOBAL, HOST, LDS_U8]
        for fam, (t, _) in zip(fams, got):
            assert np.array_equal(t, R.joint_counts_fast(table.codes, CARDS, fam))
        with pytest.raises(ValueError):
            table.counted(fams, cap=1000)
    finally:
        table.close()


def test_slogl_does_not_depend_on_the_chunking(lib, monkeypatch):
    """A count buffer of 5 000 cells: the families go in several launch chunks; integer counts and one summation order - the same bits."""
    fams = FAMILIES + random_families(30, np.random.default_rng(7))
    table = Table(lib, make_codes(4097, CARDS, "parent", 6), CARDS)
    net = Net(lib, CARDS, fams, fitted(table.codes, CARDS, fams))
    try:
        whole = net.slogl(table)
        counts = [t.copy() for t, _ in table.counted(fams)]
        monkeypatch.setenv("PBN_DISCRETE_CHUNK_CELLS", "5000")
        chunked = net.slogl(table)
        assert chunked[0] == whole[0] and np.array_equal(chunked[1], whole[1])
        for a, (b, _) in zip(counts, table.counted(fams)):
            assert np.array_equal(a, b)
    finally:
        net.close()
        table.close()


def test_what_pbn_dnet_refuses(lib):
    from pybnesian_amd import _lib

    with pytest.raises(ValueError, match="more than 8 family variables"):
        Net(lib, CARDS, [EIGHT], [np.zeros(3 * 256)])
    with pytest.raises(ValueError, match="2\\^31 - 1 cells"):
        Net(lib, [300, 300, 300, 300], [(0, [1, 2, 3])], [np.zeros(4)])
    with pytest.raises(ValueError, match="offsets"):
        Net(lib, CARDS, [(0, [1]), (2, [])], [np.zeros(6), np.zeros(5)])
    with pytest.raises(ValueError):
        Net(lib, CARDS, [(0, [0])], [np.zeros(4)])            # the variable among its parents
    with pytest.raises(ValueError):
        Net(lib, CARDS, [(0, [len(CARDS)])], [np.zeros(4)])   # a column that does not exist
    # a table whose cardinalities are not the network's
    table = Table(lib, make_codes(9, CARDS[:4], "none", 8), CARDS[:4])
    net = Net(lib, [2, 3, 4, 6], [(0, [1])], [np.zeros(6)])
    try:
        with pytest.raises(ValueError, match="cardinalities"):
            net.logl(table)
        with pytest.raises(ValueError, match="cardinalities"):
            net.slogl(table)
        assert net.stats() == (0, 0)
    finally:
        net.close()
        table.close()
    # codes outside [-1, cardinality) never reach the device
    bad = make_codes(9, CARDS[:4], "none", 9)
    bad[2][4] = 4
    with pytest.raises(ValueError, match="outside"):
        Table(lib, bad, CARDS[:4])
    assert _lib.load() is lib
