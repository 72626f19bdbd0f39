"""The hybrid score engine's per-cell moment kernels (csrc/hybrid.hip group_moments, csrc/stats_kernels.hip) at every launch shape, against numpy.

Every hybrid local score - CLG BIC, the CV and hold-out likelihood of a continuous node with discrete parents - is host arithmetic on
per-cell moments: a cell is one configuration of the discrete parents in one region (all rows for BIC, a fold for CV, train / test for
hold-out), and per cell the engine takes a count N, the pilot-shifted column sums S and the products G.  The test aid
pbn_debug_hybrid_moments (layout at its definition in csrc/hybrid.hip) builds or fetches the handle's own grouping and calls group_moments
exactly as score_hybrid does; it hands back every cell's N, S, G and a record of what ran: the path - full (the grouping's Gram over all
continuous columns: gram_gring_kernel<T, NCT, false> through the grouped row list + gram_seg_reduce_kernel), seg (seg_moments_kernel<T, D>
+ seg_reduce_kernel) or own (the same Gram over the candidate's own columns) -, the cells, the pieces launched, NCT or D and the element
size.  pbn_debug_scoredata_shifts reports the pilot shifts, pbn_debug_gram_rows runs gram_raw through a device row list as the two null
paths of the engine do (the plain gathered ring + the 16-ary gram_reduce_kernel tree).

Cell sizes are prescribed, not drawn: lengths() of tests/test_mi_shapes_gpu.py - 0, 1, 2, k STEP + {-1, 0, 1} around the switch points of
gram_gring_kernel's ring for both of its (STEP, D) pairs, the 256-row stride of seg_moments_kernel and the 4096-row pieces of both paths
(53 lengths, 46 052 rows).  BIC handles take them as the configurations of a 7 x 8 grid (main_codes); for CV (k = 3) and hold-out handles
the fold / train-test membership of every row is read first from a score built on the same number of rows, then the discrete codes are
laid out so that the (configuration, region) cells take the prescribed sizes (one more configuration per region holds the rows left over).

Exact leg.  Column j is s_j + e, an integer offset plus integers in [-15, 15].  BIC handles are not permuted and the pilot rows sum to
zero, so the shift is exactly s_j (asserted).  CV / hold-out handles take the pilot over the first 1024 rows of the permuted table: the
shift is an exact multiple of 2^-10 (asserted), x - shift has at most 10 fractional bits and |x - shift| < 64, every product at most 20
fractional bits below 2^12, a sum over at most 2^16 rows stays below 2^48 - any order of FMAs or f64 MFMAs is exact, on float and double
tables alike.  N, S and G must EQUAL the numpy result over the same rows, which is formed on the integers 1024 (x - shift) (their
products and sums stay below 2^53, asserted: float64 matrix products of them are exact in any order).  No tolerance.

Rounding leg.  Real-valued tables (offsets up to +-30), same cells: |got - want| <= (N + 2) 2^-53 sum |x_i x_j| per cell and entry (S: sum
|x_i|), the bound of any summation order of N rounded products or FMAs, `want` from np.longdouble sums of the double-rounded x - shift
with the shifts as reported, for the candidate's columns only.  No measured constant.

What was reached is asserted at the end (test_every_launch_form_was_seen): every path x element size x NCT or D with a cell of more than
one piece and with an empty cell, the seg path by each of the three ways the full path is refused, every path under every kind of region,
and pbn_debug_gram_rows' forms.

Measured on an MI355X (this file alone, one pytest process; profiles/hybrid_moments/tests.txt): 4.0 s for the 40 tests, the slowest
(test_the_cells_take_the_prescribed_sizes, which builds the four tables and the two probe scores) 0.40 s, the slowest with device work
(test_rounding[float64-cv]) 0.30 s; 582 pbn_debug_hybrid_moments and 316 pbn_debug_gram_rows calls.  Worst fraction of the rounding bound
per path, float64 / float32 table: full 0.335 / 0.441, seg 0.385 / 0.389, own 0.335 / 0.355, gram_raw through row lists of 4 097 and
65 613 rows 0.001 / 0.002 (the bound grows with N, the error of a blocked sum does not).  Launch forms seen: 128 - 32 path x element size
x NCT or D, each with a cell of more than one piece and with an empty cell; 48 (refusal of the full path, element size, D); 48 (element
size, NCT, tree levels, dense or sparse list).
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import mi_restatement as mr
from test_mi_shapes_gpu import NCOL, OFFS, PILOT_ROWS, STEP_D, int_e, lengths, main_codes

pytestmark = pytest.mark.gpu

# ---- the kernels' constants, each with the line it restates ----------------------------------------------------------------------
assert STEP_D == ((64, 3), (32, 4))   # stats_kernels.hip gram_gring_kernel: RL = (sizeof(T) == 8 && NCT == 4) ? 2 : 4; D = RL == 2 ? 4 : 3; STEP = 16 * RL
SEG_STRIDE = 256               # hybrid.hip seg_moments_kernel: for (int r = r0 + (int)threadIdx.x; r < r1; r += 256)
SEG_PIECE = 4096               # hybrid.hip: constexpr int SEG_PIECE = 4096
PIECE = 4096                   # hybrid.hip cells_gram: constexpr int64_t PIECE = 4096
assert PILOT_ROWS == 1024      # stats_kernels.hip pilot_mean_kernel: m = n < 1024 ? n : 1024
FULL_MAX_COLS = 64             # hybrid.hip ensure_full_moments: n > 64 -> no full Gram
FULL_MAX_NUMBERS = 1 << 24     # hybrid.hip ensure_full_moments: cells * (n * n + n) > 2^24 -> no full Gram
SEG_MAX_D = 8                  # hybrid.hip group_moments: if (d <= 8 && batched && g.npieces > 0)
GRAM_ROWS_PER_BLOCK = 256      # scoring.hip gram_raw: nblocks = min(4 * num_cus, max(1, ceil_div(n, 256)))
REDUCE_ARITY = 16              # stats_kernels.hip launch_gram: while ((nblocks + stride - 1) / stride > 16)
K_FOLDS, HOLD_RATIO, SEED = 3, 0.2, 5
SPLIT_ROWS = 47123             # rows of the CV / hold-out tables: the 46 052 prescribed rows and 1 071 left over
U = 2.0 ** -53

PATH = {0: "full", 1: "seg", 2: "own", 3: "cellwise"}
FIELDS = ("path", "nc", "nregions", "pieces", "width", "bytes", "cells", "zero")

SEEN = {}                      # (path, bytes, NCT or D) -> [a cell of more than one piece seen, an empty cell seen]
SEG_WHY = set()                # (why the full path was refused, bytes, D)
KINDS = set()                  # (path, kind of regions)
GRAM_ROWS = set()              # (bytes, NCT, levels of the reduce tree, kind of list)
FRAC = {}                      # (path, bytes) -> worst fraction of the rounding bound
CALLS = {"hybrid": 0, "gram_rows": 0}


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def aids(pbn):
    from pybnesian_amd import _lib

    L = _lib.load()
    L.pbn_debug_hybrid_moments.restype = C.c_int64
    L.pbn_debug_hybrid_moments.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.pbn_debug_scoredata_shifts.restype = C.c_int
    L.pbn_debug_scoredata_shifts.argtypes = [C.c_void_p, C.c_void_p]
    L.pbn_debug_gram_rows.restype = C.c_int
    L.pbn_debug_gram_rows.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    return L, _lib


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def split_layout(pbn, kind, n):
    """Region of every source row and the rows in the permuted table's order, read from a score over n rows: membership depends on the
    row count, k, the seed and the ratio only.  The probe's one column holds the row number, so the tables the score hands out name
    their rows."""
    probe = pd.DataFrame({"row": np.arange(n, dtype=np.float64)})
    region = np.full(n, -1, dtype=np.int64)
    if kind == "cv":
        score = pbn.CVLikelihood(probe, k=K_FOLDS, seed=SEED)
        parts = [np.asarray(test) for _, test in score.cv.indices()]
        assert len(parts) == K_FOLDS
    else:
        score = pbn.HoldoutLikelihood(probe, test_ratio=HOLD_RATIO, seed=SEED)
        parts = [np.asarray(t.column("row").to_numpy()).astype(np.int64) for t in (score.training_data(), score.test_data())]
    for r, rows in enumerate(parts):
        region[rows] = r
    order = np.concatenate(parts).astype(np.int64)     # the folds one after the other / train then test: the permuted table
    assert np.array_equal(np.sort(order), np.arange(n)) and np.all(region >= 0)
    return region, order


def cell_codes(region, R, seed):
    """Discrete codes such that the (configuration, region) cells take the prescribed sizes: the lengths go, longest first, to the region
    with the most rows left; one configuration per region takes the rows left over, the remaining slots stay empty.  Returns the
    configuration of every source row, the number of configurations and the sizes [nc][R]."""
    rng = np.random.default_rng(seed)
    L = sorted((v for v in lengths() if v > 0), reverse=True)
    card2 = -(-(len(L) + 1 + R) // (7 * R))
    nc = 7 * card2
    left = np.bincount(region, minlength=R).astype(np.int64)
    assert left.sum() >= sum(L)
    size = [[] for _ in range(R)]
    for v in L:
        r = max((r for r in range(R) if len(size[r]) < nc - 1 and left[r] >= v), key=lambda r: left[r])
        size[r].append(v)
        left[r] -= v
    sizes = np.zeros((nc, R), dtype=np.int64)
    config = np.full(len(region), -1, dtype=np.int64)
    for r in range(R):
        col = np.array(size[r] + [left[r]] + [0] * (nc - 1 - len(size[r])))
        col = col[rng.permutation(nc)]
        sizes[:, r] = col
        rows = np.flatnonzero(region == r)
        config[rows[rng.permutation(len(rows))]] = np.repeat(np.arange(nc), col)
    assert np.all(config >= 0)
    got = sorted(sizes.ravel().tolist())
    for v in lengths():                                  # every prescribed length is the size of a cell (0 included)
        assert v in got, v
    return config, nc, sizes, card2


class Table:
    """values [n][NCOL] (int64 for the exact leg, float64 of what a real table holds for the rounding leg), discrete columns name ->
    (codes, card) in the order the handle numbers them, the region of every source row and the pilot rows (source row ids)."""

    def __init__(self, kind, values, disc, region, pilot):
        self.kind, self.values, self.disc, self.region, self.pilot = kind, values, disc, region, pilot
        self.n = values.shape[0]
        self.R = int(region.max()) + 1
        self.names = list(disc)
        self._cache = {}
        if values.dtype == np.int64:
            # 1024 * shift as the pilot defines it: 1024 s_j + the sum of e over the PILOT_ROWS pilot rows
            self.shift1024 = OFFS * 1024 + (values[pilot] - OFFS).sum(axis=0)
            self.y = values * 1024 - self.shift1024   # 1024 (x - shift): an integer
            assert np.abs(self.y).max() < 64 * 1024 and self.n <= 1 << 16
            assert float(np.abs(self.y).max()) ** 2 * self.n < 2.0 ** 53    # float64 products and sums of y are exact in any order

    def key(self, names):
        """Cell of every row, canonical: the parents in the handle's column order, the first the fastest, the region the minor index;
        -1 where a parent's code is null."""
        names = sorted(names, key=self.names.index)
        cfg, nc = mr.keys([self.disc[v][0] for v in names], [self.disc[v][1] for v in names])
        if not names:
            cfg, nc = np.zeros(self.n, dtype=np.int64), 1
        return np.where(cfg >= 0, cfg * self.R + self.region, -1), nc

    def exact(self, names):
        """count [cells], S [cells][NCOL], P [cells][NCOL][NCOL] of y, as float64 holding integers."""
        tag = ("exact",) + tuple(sorted(names))
        if tag not in self._cache:
            key, nc = self.key(names)
            cells = nc * self.R
            order, b, count = mr.segments(key, cells)
            ys = self.y[order].astype(np.float64)
            S, P = np.zeros((cells, NCOL)), np.zeros((cells, NCOL, NCOL))
            for g in np.flatnonzero(count):
                seg = ys[b[g]:b[g + 1]]
                S[g] = seg.sum(axis=0)
                P[g] = seg.T @ seg
            self._cache[tag] = (count, S, P)
        return self._cache[tag]


def bic_table(seed, null_rows=0):
    """The MI test's main table: the prescribed sizes as the configurations of (d1, d2), rows shuffled.  null_rows: that many more rows
    with a null code in d1 or d2 - they belong to no cell, so the cells keep their sizes."""
    d1, d2, size = main_codes(seed)
    rng = np.random.default_rng(seed + 1)
    if null_rows:
        pos = np.sort(rng.integers(0, len(d1) + 1, null_rows))
        which = rng.integers(0, 2, null_rows)
        d1 = np.insert(d1, pos, np.where(which == 0, -1, rng.integers(0, 7, null_rows))).astype(np.int32)
        d2 = np.insert(d2, pos, np.where(which == 1, -1, rng.integers(0, 8, null_rows))).astype(np.int32)
        assert ((d1 < 0) | (d2 < 0)).sum() == null_rows and (d1 < 0).any() and (d2 < 0).any()
    n = len(d1)
    e, _ = int_e(n, seed + 2)
    d3 = rng.integers(0, 3, n).astype(np.int32)
    t = Table("bicnull" if null_rows else "bic", OFFS + e, {"d1": (d1, 7), "d2": (d2, 8), "d3": (d3, 3)}, np.zeros(n, dtype=np.int64), np.arange(PILOT_ROWS))
    t.size = size
    return t


def split_table(pbn, kind, seed):
    region, order = split_layout(pbn, kind, SPLIT_ROWS)
    R = K_FOLDS if kind == "cv" else 2
    config, nc, sizes, card2 = cell_codes(region, R, seed)
    e, _ = int_e(SPLIT_ROWS, seed + 2)
    d1, d2 = (config % 7).astype(np.int32), (config // 7).astype(np.int32)
    t = Table(kind, OFFS + e, {"d1": (d1, 7), "d2": (d2, card2)}, region, order[:PILOT_ROWS])
    t.size, t.order = sizes, order
    return t


@pytest.fixture(scope="module")
def tables(pbn):
    """One table per kind of regions, built when first asked for."""
    made = {}

    def get(kind):
        if kind not in made:
            if kind == "bic":
                made[kind] = bic_table(11)
            elif kind == "bicnull":
                made[kind] = bic_table(15, null_rows=1500)
            else:
                made[kind] = split_table(pbn, kind, 21 if kind == "cv" else 31)
        return made[kind]

    return get


def test_the_cells_take_the_prescribed_sizes(tables):
    assert len(lengths()) == 53
    for step, d in STEP_D:
        for k in (1, 2, d - 1, d, 3 * d - 1, 3 * d, 3 * d + 1, 4 * d, 4 * d + 1):
            assert {k * step - 1, k * step, k * step + 1} <= set(lengths())
    assert {0, 1, 2, SEG_STRIDE - 1, SEG_STRIDE, SEG_STRIDE + 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1} <= set(lengths())
    assert SEG_PIECE == PIECE
    for kind in ("bic", "bicnull", "cv", "ho"):
        t = tables(kind)
        key, nc = t.key(["d1", "d2"])
        count = np.bincount(key[key >= 0], minlength=nc * t.R)
        assert np.array_equal(count.reshape(nc, t.R), np.asarray(t.size).reshape(nc, t.R)), kind
        assert set(lengths()) <= set(count.tolist()), kind
        if kind != "bic":
            assert t.n <= 1 << 16
        if kind == "bicnull":
            assert (key < 0).sum() == 1500


# ---- handles ---------------------------------------------------------------------------------------------------------------------------
class Handle:
    """A score over the first nc columns of a table (float64 / float32) and its discrete columns; mask_col: that column gets nulls (BIC: a
    validity mask; the column stays outside every candidate)."""

    def __init__(self, pbn, aids, table, nc, dtype, mask_col=None, values=None, exact=True):
        self.lib, self._lib = aids
        self.table, self.nc, self.bytes, self.mask_col = table, nc, np.dtype(dtype).itemsize, mask_col
        vals = (table.values if values is None else values)[:, :nc].astype(dtype)
        if mask_col is not None:
            assert table.kind.startswith("bic")
            vals[3::7, mask_col] = np.nan
        data = {f"x{j}": vals[:, j] for j in range(nc)}
        for name, (codes, card) in table.disc.items():
            data[name] = pd.Categorical.from_codes(codes, [f"l{i}" for i in range(card)])
        df = pd.DataFrame(data)
        if table.kind == "cv":
            self.score, self.kind = pbn.CVLikelihood(df, k=K_FOLDS, seed=SEED), self._lib.PBN_SCORE_CVLIK
        elif table.kind == "ho":
            self.score, self.kind = pbn.HoldoutLikelihood(df, test_ratio=HOLD_RATIO, seed=SEED), self._lib.PBN_SCORE_HOLDOUT
        else:
            self.score, self.kind = pbn.BIC(df), self._lib.PBN_SCORE_BIC
        self.h = self.score._handle
        self.did = {name: nc + i for i, name in enumerate(table.disc)}
        self.shift = np.full(nc, np.nan)
        self._lib.check(self.lib.pbn_debug_scoredata_shifts(self.h, self.shift.ctypes.data))
        if table.kind in ("cv", "ho"):                    # the same rows in the same regions as the probe's
            perm, _, n_cv, n_hold = self.score._layout()
            assert np.array_equal(perm, table.order) and n_cv + n_hold == table.n
        if exact:
            live = [j for j in range(nc) if j != mask_col]
            s1024 = self.shift * 1024
            assert np.array_equal(s1024[live], np.round(s1024[live])), "1024 * shift is not an integer"
            assert np.array_equal(s1024[live].astype(np.int64), table.shift1024[:nc][live]), "the shift is not the pilot rows' mean"
            if table.kind.startswith("bic"):
                assert np.array_equal(self.shift[live], OFFS[:nc][live].astype(np.float64)), "the pilot shift is not the column's integer offset"

    def moments(self, names, cols):
        """One pbn_debug_hybrid_moments call: (N [cells], S [cells][d], G [cells][d][d] with G[c][j][i] = entry i + j d, the record)."""
        d = len(cols)
        nc = int(np.prod([self.table.disc[v][1] for v in names])) if names else 1
        cells = nc * self.table.R
        per = 1 + d + d * d
        dpar = np.array([self.did[v] for v in names] or [0], dtype=np.int32)
        cc = np.array(cols, dtype=np.int32)
        rec = np.full(len(FIELDS), -7, dtype=np.int64)
        need = self.lib.pbn_debug_hybrid_moments(self.h, self.kind, len(names), dpar.ctypes.data, d, cc.ctypes.data, None, 0, None)
        assert need == cells * per, (need, cells, per)
        out = np.full(need, np.nan)
        got = self.lib.pbn_debug_hybrid_moments(self.h, self.kind, len(names), dpar.ctypes.data, d, cc.ctypes.data, out.ctypes.data, need, rec.ctypes.data)
        assert got == need
        CALLS["hybrid"] += 1
        out = out.reshape(cells, per)
        r = dict(zip(FIELDS, (int(v) for v in rec)))
        assert (r["nc"], r["nregions"], r["cells"], r["bytes"], r["zero"]) == (nc, self.table.R, cells, self.bytes, 0), r
        return out[:, 0], out[:, 1:1 + d], out[:, 1 + d:].reshape(cells, d, d), r

    def expected(self, names, d, count):
        """(path, NCT or D, pieces) by the rules of ensure_full_moments / group_moments, restated."""
        pieces = int(sum(-(-int(c) // PIECE) for c in count))
        full = self.nc <= FULL_MAX_COLS and self.mask_col is None and len(count) * (self.nc * self.nc + self.nc) <= FULL_MAX_NUMBERS
        if full:
            return "full", (self.nc + 15) // 16, pieces
        if d <= SEG_MAX_D and pieces > 0:
            return "seg", d, pieces
        return "own", (d + 15) // 16, pieces

    def why_not_full(self, cells):
        if self.nc > FULL_MAX_COLS:
            return "columns"
        if self.mask_col is not None:
            return "mask"
        assert cells * (self.nc * self.nc + self.nc) > FULL_MAX_NUMBERS
        return "cells"


def note(h, r, count, path):
    multi, empty = bool((count > PIECE).any()), bool((count == 0).any())
    flags = SEEN.setdefault((path, h.bytes, r["width"]), [False, False])
    flags[0] |= multi
    flags[1] |= empty
    KINDS.add((path, h.table.kind))
    if path == "seg":
        SEG_WHY.add((h.why_not_full(len(count)), h.bytes, r["width"]))


def run_exact(h, names, cols, want_path=None):
    """One candidate of the exact leg: every cell's N, S and G equal the integers' result; the record says what the rules predict."""
    t = h.table
    N, S, G, r = h.moments(names, cols)
    count, wS, wP = t.exact(names)
    path, width, pieces = h.expected(names, len(cols), count)
    assert (PATH[r["path"]], r["width"], r["pieces"]) == (path, width, pieces), (names, cols, r)
    assert want_path is None or path == want_path, (path, want_path)
    where = f"{t.kind} {h.nc} columns {h.bytes} B, {path} {width}, parents {names}, columns {cols}"
    assert np.array_equal(N, count.astype(np.float64)), where
    cols = list(cols)
    wantS = wS[:, cols] / 1024.0
    wantG = np.transpose(wP[:, cols][:, :, cols], (0, 2, 1)) / float(1 << 20)
    if not np.array_equal(S, wantS):
        g, i = np.argwhere(S != wantS)[0]
        raise AssertionError(f"{where}: cell {g} ({int(count[g])} rows) S[{i}]: got {S[g, i]!r}, want {wantS[g, i]!r}; {int((S != wantS).sum())} entries differ")
    if not np.array_equal(G, wantG):
        g, j, i = np.argwhere(G != wantG)[0]
        bad = sorted({int(count[c]) for c in np.argwhere(G != wantG)[:, 0]})
        raise AssertionError(f"{where}: cell {g} ({int(count[g])} rows) G[{i}, {j}]: got {G[g, j, i]!r}, want {wantG[g, j, i]!r}; "
                             f"{int((G != wantG).sum())} entries differ, in cells of {bad[:12]} rows")
    note(h, r, count, path)
    return r


def spread(c, nc, start=0):
    """c distinct columns of a table of nc, out of order and across its 16-column tiles, the last column among them (start = 0)."""
    step = next(s for s in (5, 7, 3, 1) if np.gcd(s, nc) == 1)
    return [(nc - 1 - start - step * i) % nc for i in range(c)]


# ---- exact leg: the full path ------------------------------------------------------------------------------------------------------
FULL_HANDLES = [("bic", n, dt) for n in (7, 16, 17, 33, 48, 49, 64) for dt in ("float64", "float32")] + \
               [("cv", 64, "float64"), ("cv", 33, "float32"), ("ho", 17, "float64"), ("ho", 64, "float32"), ("bicnull", 64, "float64"), ("bicnull", 49, "float32")]


@pytest.mark.parametrize("kind,nc,dtype", FULL_HANDLES)
def test_full_path(pbn, aids, tables, kind, nc, dtype):
    """At most 64 columns, no mask: one gathered Gram of ALL columns per grouping; candidates are entries of it - subsets in the engine's
    order (the variable, then ascending parents) and scrambled, over the prescribed cells and over coarser groupings."""
    t = tables(kind)
    h = Handle(pbn, aids, t, nc, dtype)
    allc = list(range(nc))
    sub = spread(min(8, nc), nc)
    cands = [[nc - 1], [0, nc - 1], [sub[0]] + sorted(sub[1:]), sub, spread(min(16, nc), nc, 1 if nc > 16 else 0), allc, spread(nc, nc)]
    for cols in cands:
        run_exact(h, ["d1", "d2"], cols, "full")
    run_exact(h, ["d2", "d1"], sub, "full")              # the parents in the other order: the same canonical cells
    for names in (["d2"], ["d1"], []):                  # coarser groupings: cells of many pieces, the whole region as one cell
        run_exact(h, names, sub, "full")
    if kind.startswith("bic"):
        run_exact(h, ["d3", "d1"], sub[:3], "full")


# ---- exact leg: the register kernel and the candidate's own Gram -------------------------------------------------------------------------
OWN_D = (9, 16, 17, 32, 33, 48, 49, 64)


def seg_and_own(h, names_list, own_d, ncols):
    for D in range(1, SEG_MAX_D + 1):
        cols = spread(D, ncols, D % 2)
        for names in names_list:
            run_exact(h, names, cols, "seg")
        if D in (3, 8):
            run_exact(h, names_list[0], [cols[0]] + sorted(cols[1:]), "seg")
    for d in own_d:
        cols = spread(d, ncols, d % 3)
        assert ncols < 64 or (min(cols) < 32 <= max(cols))          # the list straddles the two 32-column halves
        run_exact(h, names_list[0], cols, "own")
    run_exact(h, names_list[-1], spread(own_d[0], ncols), "own")
    run_exact(h, names_list[0], sorted(spread(own_d[1], ncols)), "own")


@pytest.mark.parametrize("kind,dtype", [(k, dt) for k in ("bic", "cv", "ho", "bicnull") for dt in ("float64", "float32")])
def test_wide_table_seg_and_own(pbn, aids, tables, kind, dtype):
    """66 continuous columns: no full Gram.  seg_moments_kernel<T, D> for D = 1 .. 8 (every D with a column >= 64), the candidate's own Gram
    for 9 .. 64 columns."""
    assert NCOL > FULL_MAX_COLS
    t = tables(kind)
    h = Handle(pbn, aids, t, NCOL, dtype)
    assert all(max(spread(D, NCOL, D % 2)) >= 64 for D in range(1, 9))
    seg_and_own(h, [["d1", "d2"], ["d2"], []] if dtype == "float64" else [["d2", "d1"], []], OWN_D, NCOL)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_masked_table_seg_and_own(pbn, aids, tables, dtype):
    """64 columns and a validity mask on a column outside the candidates: a row that is null there still counts for the candidate, so
    the full Gram is refused and the candidate's own moments are taken."""
    t = tables("bic")
    mask_col = 40
    h = Handle(pbn, aids, t, 64, dtype, mask_col=mask_col)

    def without(cols):
        return [c if c != mask_col else 41 for c in cols]

    for D in range(1, SEG_MAX_D + 1):
        cols = without(spread(D, 64, D % 2))
        assert len(set(cols)) == D
        run_exact(h, ["d1", "d2"], cols, "seg")
    for d in (9, 17, 33, 49, 63):
        cols = [c for c in spread(64, 64) if c != mask_col][:d]
        run_exact(h, ["d1", "d2"], cols, "own")
    # a candidate that holds the masked column goes through the masked pass in the engine: the aid refuses it
    bad = np.array([mask_col, 0], dtype=np.int32)
    dpar = np.array([h.did["d1"]], dtype=np.int32)
    assert h.lib.pbn_debug_hybrid_moments(h.h, h.kind, 1, dpar.ctypes.data, 2, bad.ctypes.data, None, 0, None) == -1


@pytest.fixture(scope="module")
def many_tab():
    """Three parents of 16 values: 4096 configurations, of which some 1400 hold 1 to 3 rows and the rest - the first and the last among
    them - none."""
    rng = np.random.default_rng(41)
    G = 16 ** 3
    live = rng.choice(np.arange(1, G - 1), 1400, replace=False)
    size = np.zeros(G, dtype=np.int64)
    size[live] = rng.integers(1, 4, len(live))
    cfg = np.repeat(np.arange(G), size)
    cfg = cfg[rng.permutation(len(cfg))]
    n = len(cfg)
    assert n >= PILOT_ROWS and set(size.tolist()) == {0, 1, 2, 3}
    e, _ = int_e(n, 42)
    disc = {"p": ((cfg % 16).astype(np.int32), 16), "q": ((cfg // 16 % 16).astype(np.int32), 16), "r": ((cfg // 256).astype(np.int32), 16)}
    t = Table("bic", OFFS + e, disc, np.zeros(n, dtype=np.int64), np.arange(PILOT_ROWS))
    t.size = size
    return t


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_many_configurations(pbn, aids, many_tab, dtype):
    """64 columns, 4096 cells: 4096 x (64 x 64 + 64) numbers are more than 2^24, so no full Gram; both reduce kernels run over cells
    without a piece.  Two parents (256 cells) still take the full Gram."""
    assert 4096 * (64 * 64 + 64) > FULL_MAX_NUMBERS >= 4032 * (64 * 64 + 64)
    h = Handle(pbn, aids, many_tab, 64, dtype)
    three = ["r", "p", "q"]
    for D in range(1, SEG_MAX_D + 1):
        r = run_exact(h, three, spread(D, 64, D % 2), "seg")
        assert r["cells"] == 4096 and r["pieces"] == 1400
    for d in (9, 17):
        run_exact(h, three, spread(d, 64, 1), "own")
    run_exact(h, ["q", "p"], spread(5, 64), "full")
    N = h.moments(three, [0])[0]
    assert N[0] == 0 and N[-1] == 0 and np.array_equal(N, many_tab.size.astype(np.float64))


# ---- pbn_debug_gram_rows: gram_raw through a row list -----------------------------------------------------------------------------------
LIST_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 16 * 256 + 1, 256 * 256 + 77)
ROWS_D = (1, 15, 16, 17, 31, 33, 47, 49, 64)           # NCT 1 .. 4, last tiles of 1, 15 and 16 live columns


def tree_levels(n, num_blocks_cap=None):
    """Levels of launch_gram's 16-ary tree over gram_raw's blocks (one block per 256 rows while 4 x CUs allows: every GPU this runs on has
    more than 64 CUs, so the lists up to 65 613 rows get ceil(n / 256) blocks rounded by the 64-row alignment of rows_per_block)."""
    nblocks = max(1, -(-n // GRAM_ROWS_PER_BLOCK))
    rpb = -(-(-(-n // nblocks)) // 64) * 64
    nblocks = max(1, -(-n // rpb))
    levels, stride = 1, 1
    while -(-nblocks // stride) > REDUCE_ARITY:
        levels, stride = levels + 1, stride * REDUCE_ARITY
    return levels


def row_lists(n_table, seed):
    """Per length a dense increasing list and a sparse shuffled one in which the first row comes again."""
    rng = np.random.default_rng(seed)
    out = []
    for n in LIST_LENGTHS:
        if n <= n_table - 7:
            dense = 7 + np.arange(n)
        else:   # longer than the table: increasing with every row taken once or twice
            dense = np.sort(np.concatenate([np.arange(n_table), rng.choice(n_table, n - n_table, replace=False)]))
        sparse = rng.choice(n_table, n, replace=n > n_table)
        if n > 2:
            sparse[[n // 2, n - 1]] = sparse[0]
        out.append((n, "dense", dense.astype(np.int32)))
        out.append((n, "sparse", sparse.astype(np.int32)))
    return out


def gram_rows(h, cols, rows, shift):
    d = len(cols)
    S, G = np.full(d, np.nan), np.full(d * d, np.nan)
    cc = np.array(cols, dtype=np.int32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    shift = np.ascontiguousarray(shift, dtype=np.float64)
    assert len(shift) == h.nc
    h._lib.check(h.lib.pbn_debug_gram_rows(h.score._table.handle, d, cc.ctypes.data, rows.ctypes.data, len(rows), shift.ctypes.data, S.ctypes.data, G.ctypes.data))
    CALLS["gram_rows"] += 1
    return S, G.reshape(d, d)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gram_rows(pbn, aids, tables, dtype):
    """The plain gathered ring and the reduce tree of one, two and three levels.  The shifts handed in are the integer offsets: x - shift
    is an integer in [-15, 15] and every sum far below 2^53."""
    t = tables("bic")
    h = Handle(pbn, aids, t, 64, dtype)
    assert {tree_levels(n) for n in LIST_LENGTHS} == {1, 2, 3}
    assert [tree_levels(n) for n in (256, 257, 16 * 256, 16 * 256 + 1, 256 * 256, 256 * 256 + 77)] == [1, 1, 1, 2, 2, 3]
    e = (t.values - OFFS).astype(np.float64)
    shift = OFFS[:64].astype(np.float64)
    for n, kind, rows in row_lists(t.n, 51):
        assert len(rows) == n and (kind == "sparse" or np.all(np.diff(rows) >= 0))
        for d in (ROWS_D if n < 60000 else (15, 17, 33, 49)):
            cols = spread(d, 64, d % 2)
            S, G = gram_rows(h, cols, rows, shift)
            x = e[rows][:, cols]
            wantS, wantG = x.sum(axis=0), x.T @ x          # integers below 2^24: exact
            assert np.array_equal(S, wantS), (n, kind, d, np.argwhere(S != wantS)[:4].tolist())
            assert np.array_equal(G, wantG.T), (n, kind, d, np.argwhere(G != wantG.T)[:4].tolist())
            GRAM_ROWS.add((h.bytes, (d + 15) // 16, tree_levels(n), kind))


# ---- rounding leg ----------------------------------------------------------------------------------------------------------------------
def real_values(n, dtype, seed):
    """Real values as wide() of tests/test_gram_paths_gpu.py builds them: mixed columns, scales 0.5 .. 2, offsets up to +-30; returned as
    float64 of what a table of `dtype` holds."""
    rng = np.random.default_rng(seed)
    mix = np.eye(NCOL) + 0.15 * np.tril(rng.normal(size=(NCOL, NCOL)), -1)
    data = rng.normal(size=(n, NCOL)) @ mix.T * rng.uniform(0.5, 2.0, size=NCOL) + rng.uniform(-30, 30, size=NCOL)
    return data.astype(dtype).astype(np.float64)


def check_bound(N, S, G, x, key, cells, where):
    """|got - want| <= (N + 2) 2^-53 sum |x_i x_j| per cell and entry (S: sum |x_i|), x = fl64(value - shift) of the candidate's
    columns; returns the worst fraction of the bound."""
    count, wS, wP, aS, aP = mr.real_moments(x, key, cells)
    assert np.array_equal(N, count.astype(np.float64)), where
    scale = ((count + 2) * U).astype(np.longdouble)
    frac = 0.0
    for got, want, mag, what in ((S, wS, aS, "S"), (G, np.transpose(wP, (0, 2, 1)), np.transpose(aP, (0, 2, 1)), "G")):
        bound = scale.reshape((-1,) + (1,) * (mag.ndim - 1)) * mag
        err = np.abs(got.astype(np.longdouble) - want)
        if not np.all(err <= bound):
            w = np.unravel_index(np.argmax(err - bound), err.shape)
            raise AssertionError(f"{where}: {what}{tuple(int(v) for v in w[1:])} of cell {int(w[0])} ({int(count[w[0]])} rows): error {float(err[w])}, bound {float(bound[w])}")
        frac = max(frac, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    return frac


@pytest.mark.parametrize("kind", ["bic", "cv"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_rounding(pbn, aids, tables, dtype, kind):
    t = tables(kind)
    vals = real_values(t.n, dtype, 61)
    fracs = {}
    for nc, plans in ((64, [("full", ["d1", "d2"], spread(8, 64)), ("full", ["d2"], spread(3, 64)), ("full", [], [63, 0])]),
                      (33, [("full", ["d1", "d2"], spread(8, 33))]),
                      (NCOL, [("seg", ["d1", "d2"], spread(1, NCOL)), ("seg", ["d1", "d2"], spread(3, NCOL)), ("seg", ["d2", "d1"], spread(8, NCOL)),
                              ("seg", [], spread(4, NCOL)), ("own", ["d1", "d2"], spread(9, NCOL)), ("own", ["d1", "d2"], spread(17, NCOL))])):
        h = Handle(pbn, aids, t, nc, dtype, values=vals, exact=False)
        for want_path, names, cols in plans:
            N, S, G, r = h.moments(names, cols)
            key, ncfg = t.key(names)
            count = np.bincount(key[key >= 0], minlength=ncfg * t.R)
            path, width, pieces = h.expected(names, len(cols), count)
            assert (PATH[r["path"]], r["width"], r["pieces"]) == (path, width, pieces) and path == want_path, (names, cols, r)
            x = vals[:, cols] - h.shift[cols]             # fl64(x - shift), the kernels' own first operation
            f = check_bound(N, S, G, x, key, ncfg * t.R, f"{kind} {nc} columns {dtype}, {path}, parents {names}, columns {cols}")
            fracs[(path, nc)] = max(fracs.get((path, nc), 0.0), f)
            FRAC[(path, h.bytes)] = max(FRAC.get((path, h.bytes), 0.0), f)
            note(h, r, count, path)
        if nc == 64:   # gram_raw through row lists of two and three tree levels, shifts = the handle's own
            for n, lkind, rows in row_lists(t.n, 71):
                if n < 4097 or lkind == "dense" and n > 60000:
                    continue
                cols = spread(17, 64)
                S, G = gram_rows(h, cols, rows, h.shift)
                x = (vals[:, cols] - h.shift[cols])[rows]
                f = check_bound(np.array([float(n)]), S[None], G[None], x, np.zeros(n, dtype=np.int64), 1, f"gram_rows {n} {lkind} {dtype}")
                FRAC[("gram_rows", h.bytes)] = max(FRAC.get(("gram_rows", h.bytes), 0.0), f)
    print(f"\nworst fraction of the rounding bound ({kind}, {dtype}): " + ", ".join(f"{k[0]} of {k[1]} columns {v:.3f}" for k, v in fracs.items()))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------
def test_every_launch_form_was_seen():
    want = set()
    for b in (8, 4):
        want |= {("full", b, nct) for nct in (1, 2, 3, 4)}
        want |= {("seg", b, D) for D in range(1, SEG_MAX_D + 1)}
        want |= {("own", b, nct) for nct in (1, 2, 3, 4)}
    missing = sorted(want - set(SEEN), key=str)
    assert not missing, missing
    assert not [k for k in SEEN if k[0] == "cellwise"]
    one_piece_only = sorted((k for k in want if not SEEN[k][0]), key=str)
    assert not one_piece_only, ("never with a cell of more than one piece", one_piece_only)
    never_empty = sorted((k for k in want if not SEEN[k][1]), key=str)
    assert not never_empty, ("never with an empty cell", never_empty)
    why = {(w, b, D) for w in ("columns", "mask", "cells") for b in (8, 4) for D in range(1, SEG_MAX_D + 1)}
    assert not why - SEG_WHY, sorted(why - SEG_WHY)
    kinds = {(p, k) for p in ("full", "seg", "own") for k in ("bic", "cv", "ho", "bicnull")}
    assert not kinds - KINDS, sorted(kinds - KINDS)
    rows = {(b, nct, lv, k) for b in (8, 4) for nct in (1, 2, 3, 4) for lv in (1, 2, 3) for k in ("dense", "sparse")}
    assert not rows - GRAM_ROWS, sorted(rows - GRAM_ROWS)
    forms = len(SEEN) + len(SEG_WHY) + len(GRAM_ROWS)
    print(f"\ncalls: {CALLS}; launch forms seen: {forms} ({len(SEEN)} path x size x width, {len(SEG_WHY)} refusals, {len(GRAM_ROWS)} row-list forms); "
          "worst fraction of the rounding bound: " + ", ".join(f"{k[0]} {k[1]} B {v:.3f}" for k, v in sorted(FRAC.items())))
