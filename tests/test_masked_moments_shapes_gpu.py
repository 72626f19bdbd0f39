"""GPU tier: the masked moment pass of the score engine (csrc/masked_moments.hip) at every launch shape, through the test aid
pbn_debug_masked_moments: N, S and the upper triangle of G of a unit's columns over the rows that are valid in all of them.

Shapes: rows 1 ... 257 around the wave and workgroup sizes, one slice (16 384 rows) - 1 / + 0 / + 1, three slices + 5; units of 1 ... 8
columns that use the first and the last column of tables of 3, 64, 65 and 70 columns (65 and 70 need a second validity word; a table of 3
columns repeats columns inside a unit - the pass takes any column list); fp64 and fp32; the null patterns below; the segmented form.

N is compared exactly.  S and G: |got - want| <= (R + 2) 2^-53 sum_r |term_r| over the R valid rows, `want` and the terms from
math.fsum over float64(x) - shift with the shifts the aid reports.  That is the forward error of any summation order of terms that are
each rounded once; the kernel forms x_i x_j inside an fma, which rounds LESS than the separately rounded products of the restatement
(whose own rounding is one of the + 2), so the bound stands for its arithmetic as well.

Reference routine: DataFrame::combined_bitmap (dataset.cpp:208-235) + the moments MLE<LinearGaussianCPD> takes (mle_LinearGaussianCPD.hpp)."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

SLICE = 16384
SMALL_ROWS = [1, 63, 64, 65, 255, 256, 257]
BIG_ROWS = [SLICE - 1, SLICE, SLICE + 1, 3 * SLICE + 5]
WIDTHS = [3, 64, 65, 70]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def aid(pbn):
    from pybnesian_amd import _lib

    L = _lib.load()
    ip, lp, dp = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
    L.pbn_debug_masked_moments.restype = C.c_int
    L.pbn_debug_masked_moments.argtypes = [C.c_void_p, C.c_int, ip, ip, lp, C.POINTER(C.c_int32), ip, lp, C.c_int64, lp, dp, dp, dp]
    return L, _lib


def null_column(n):
    return 1 if n == 3 else n // 2


def unit_columns(n, d):
    """d columns: the first, the last, then columns of both validity words; a narrow table repeats the first and the last."""
    fill = [c for c in (2, 3, 63, 64, 5, 6, 7, 4) if c < n - 1 and c != null_column(n)]
    cols = ([0, n - 1] + fill)[:d]
    while len(cols) < d:
        cols.append([0, n - 1][len(cols) % 2])
    return cols


def make_table(rows, n, dtype, pattern, seed=0):
    """(values with NaN under the nulls, as float64 of what the table holds)."""
    rng = np.random.default_rng(seed + 7 * rows + n)
    x = (rng.normal(size=(rows, n)) * rng.uniform(0.5, 3.0, size=n) + rng.uniform(-5, 5, size=n)).astype(dtype)
    x = x.astype(np.float64)
    other = null_column(n)
    x[rng.integers(0, rows, size=max(1, rows // 10)), other] = np.nan   # every table holds a null somewhere outside the units
    if pattern == "first":
        x[0, 0] = np.nan
    elif pattern == "last":
        x[rows - 1, n - 1] = np.nan
    elif pattern == "column":
        x[:, n - 1] = np.nan
    elif pattern == "slice":   # one whole slice of the pass (a short table: all of it but the rows past the first slice)
        s0 = SLICE if rows > 2 * SLICE else 0
        x[s0: s0 + SLICE, 0] = np.nan
    elif pattern == "alternate":
        x[1::2, 0] = np.nan
        x[0::3, n - 1] = np.nan
    else:
        assert pattern == "other"
    return x


class Handle:
    def __init__(self, pbn, aid, x, dtype):
        self.lib, self._lib = aid
        self.x = x
        df = pd.DataFrame(x, columns=[f"c{i}" for i in range(x.shape[1])]).astype(dtype)
        self.score = pbn.BIC(df)
        self.h = self.score._handle

    def run(self, units, lists=None):
        """units: column lists; lists: None or per unit None / (rows, [segment offsets]).  -> per unit a list of (N, S, G, shifts) per segment."""
        i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
        i64 = lambda a: np.ascontiguousarray(a, dtype=np.int64)
        col_off = i32(np.concatenate([[0], np.cumsum([len(u) for u in units])]))
        cols = i32([c for u in units for c in u])
        ip, lp, dp = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        pairs = [1 if not lists or lists[k] is None else len(lists[k][1]) - 1 for k in range(len(units))]
        cap = int(sum(pairs))
        N, S, G = np.zeros(cap, dtype=np.int64), np.full((cap, 8), np.nan), np.full((cap, 36), np.nan)
        shift = np.zeros(len(cols))
        if lists:
            list_off, rows, seg_ptr, seg_off = [0], [], [0], []
            for entry in lists:
                if entry is not None:
                    rows.extend(entry[0])
                    seg_off.extend(entry[1])
                list_off.append(len(rows))
                seg_ptr.append(len(seg_off))
            list_off, rows, seg_ptr, seg_off = i64(list_off), i32(rows or [0]), i32(seg_ptr), i64(seg_off or [0])
            args = (list_off.ctypes.data_as(lp), rows.ctypes.data_as(C.POINTER(C.c_int32)), seg_ptr.ctypes.data_as(ip), seg_off.ctypes.data_as(lp))
        else:
            args = (None, None, None, None)
        self._lib.check(self.lib.pbn_debug_masked_moments(self.h, len(units), col_off.ctypes.data_as(ip), cols.ctypes.data_as(ip), *args, cap,
                                                          N.ctypes.data_as(lp), S.ctypes.data_as(dp), G.ctypes.data_as(dp), shift.ctypes.data_as(dp)))
        out, k = [], 0
        for u, unit in enumerate(units):
            sh = shift[col_off[u]: col_off[u + 1]]
            out.append([(int(N[k + s]), S[k + s].copy(), G[k + s].copy(), sh) for s in range(pairs[u])])
            k += pairs[u]
        return out


def check(x, cols, rows, got, where):
    """One (unit, segment): `rows` = the table rows of the segment, in list order."""
    N, S, G, shift = got
    d = len(cols)
    sub = x[np.asarray(rows, dtype=np.int64)][:, cols] if len(rows) else np.zeros((0, d))
    valid = ~np.isnan(sub).any(axis=1)
    R = int(valid.sum())
    assert N == R, (where, N, R)
    z = sub[valid] - shift   # float64(x) - shift, rounded once: the kernel's x
    pos = 0
    for i in range(d):
        want, mag = math.fsum(z[:, i]), math.fsum(np.abs(z[:, i]))
        assert abs(S[i] - want) <= (R + 2) * U * mag, (where, "S", i, S[i], want)
        for j in range(i, d):
            t = z[:, i] * z[:, j]
            want, mag = math.fsum(t), math.fsum(np.abs(t))
            assert abs(G[pos] - want) <= (R + 2) * U * mag, (where, "G", i, j, G[pos], want)
            pos += 1
    if R == 0:
        assert not S[:d].any() and not G[:pos].any(), where


def patterns_for(rows):
    return ["other", "first", "last", "column", "alternate"] + (["slice"] if rows >= SLICE else [])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", WIDTHS)
def test_small_tables(pbn, aid, n, dtype):
    for rows in SMALL_ROWS:
        for pattern in patterns_for(rows):
            x = make_table(rows, n, dtype, pattern)
            h = Handle(pbn, aid, x, dtype)
            units = [unit_columns(n, d) for d in range(1, 9)]
            for cols, res in zip(units, h.run(units)):
                check(x, cols, np.arange(rows), res[0], (rows, n, dtype, pattern, cols))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [3, 70])
@pytest.mark.parametrize("rows", BIG_ROWS)
def test_slice_boundaries(pbn, aid, rows, n, dtype):
    for pattern in patterns_for(rows):
        x = make_table(rows, n, dtype, pattern)
        h = Handle(pbn, aid, x, dtype)
        units = [unit_columns(n, d) for d in range(1, 9)]
        for cols, res in zip(units, h.run(units)):
            check(x, cols, np.arange(rows), res[0], (rows, n, dtype, pattern, cols))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("rows,n", [(257, 65), (3 * SLICE + 5, 70)])
def test_segmented_form(pbn, aid, rows, n, dtype):
    """Row lists in non-monotone order cut into 1, 2 and 7 segments, with an empty segment and a segment of one row; a plain unit between
    them in the same call."""
    x = make_table(rows, n, dtype, "alternate")
    h = Handle(pbn, aid, x, dtype)
    rng = np.random.default_rng(3)
    perm = rng.permutation(rows)
    L = len(perm)
    seven = sorted({0, L} | set(rng.integers(1, L, size=3).tolist()))
    seven = [0, 0, 1] + [v for v in seven if v > 1]   # an empty segment, a segment of one row ...
    while len(seven) < 8:
        seven.insert(3, seven[2])                     # ... and empty ones until there are seven
    lists = [(perm, [0, L]), None, (perm[: L // 2][::-1], [0, L // 4, L // 2]), (perm, seven), (perm[:1], [0, 1]), (perm[:0], [0, 0])]
    units = [unit_columns(n, d) for d in (2, 3, 8, 5, 1, 4)]
    res = h.run(units, lists)
    for k, (cols, entry) in enumerate(zip(units, lists)):
        if entry is None:
            check(x, cols, np.arange(rows), res[k][0], ("plain", k))
            continue
        r, off = entry
        assert len(res[k]) == len(off) - 1
        for s in range(len(off) - 1):
            check(x, cols, r[off[s]: off[s + 1]], res[k][s], ("segment", k, s))
    # the whole list as one segment = the plain unit over the same rows in another order: within the bound of either, N equal
    assert res[0][0][0] == h.run([units[0]])[0][0][0]


def same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_unit_does_not_depend_on_its_batch(pbn, aid, dtype):
    rows, n = 3 * SLICE + 5, 70
    x = make_table(rows, n, dtype, "alternate")
    h = Handle(pbn, aid, x, dtype)
    rng = np.random.default_rng(5)
    unit = [0, 69, 63, 64, 2]
    alone = h.run([unit])[0][0]
    others = [rng.choice(n, size=int(rng.integers(1, 9)), replace=False).tolist() for _ in range(500)]
    batch = others[:250] + [unit] + others[250:] + [unit]
    res = h.run(batch)
    assert same(res[250][0], alone) and same(res[-1][0], alone)   # among 500 others, and repeated in one call
    assert same(h.run([unit])[0][0], alone)                      # two calls
    check(x, unit, np.arange(rows), alone, "alone")
    for k in (0, 100, 499):
        check(x, others[k], np.arange(rows), res[k if k < 250 else k + 1][0], ("other", k))
    # a column permutation of the unit: the permuted numbers, each within its bound
    perm = [3, 0, 4, 2, 1]
    permuted = [unit[p] for p in perm]
    got = h.run([permuted])[0][0]
    check(x, permuted, np.arange(rows), got, "permuted")
    assert got[0] == alone[0]


def test_the_aid_refuses_bad_requests(pbn, aid):
    lib, _lib = aid
    x = make_table(64, 3, "float64", "first")
    h = Handle(pbn, aid, x, "float64")
    with pytest.raises(Exception, match="between 1 and 8 columns"):
        h.run([[0] * 9])
    with pytest.raises(Exception, match="column out of range"):
        h.run([[0, 3]])
    with pytest.raises(Exception, match="row out of range"):
        h.run([[0]], [([0, 64], [0, 2])])
    clean = pbn.BIC(pd.DataFrame(np.random.default_rng(0).normal(size=(64, 3)), columns=list("abc")))
    h.h = clean._handle
    with pytest.raises(Exception, match="no validity words"):
        h.run([[0]])
