"""The contiguous Gram kernels (csrc/stats_kernels.hip gram_glds_kernel / gram_glds_f32_kernel) at every ring state, exactly.

The two kernels stream a table's rows through a per-wave ring of two LDS stages filled by LDS-DMA two chunks ahead, with s_waitcnt vmcnt(N)
counted by hand: a prologue, a steady loop that runs only while a block has more than four whole chunks in front of it, a drain whose waits
depend on what is left, and a cut last chunk through registers.  Which of these a block executes is decided by nfull, its number of whole
chunks, and by the rows of the cut chunk; tests/gram_restatement.py restates that arithmetic and plans the cases below so that every such
state is reached in both forms of the kernels:
 * plain form - pbn_table_sse / DataFrame::means, ::cov, ::sse (capi.hip table_gram -> launch_gram, the 16-ary gram_reduce_kernel tree):
   blocks interleave their chunks; a block owns more than four chunks only once the grid is capped at 2 x CUs blocks, which takes
   4 x 2 CUs x 64 (128 on float tables) rows and more.  The test aid pbn_debug_table_gram returns the raw result of that one launch.
 * segmented form - the moments of a score handle (scoring.hip compute_stats_segments -> launch_gram_segments, gram_seg_reduce_kernel):
   a segment is cut into pieces of 4 096 rows, one block each.  The test aid pbn_debug_scoredata_segments runs it on given row ranges.

Exact leg.  Column j is s_j + e with an integer offset s_j and integers e in [-15, 15], and the shift is exactly s_j (uploaded in the plain
form; in the segmented form the first 1 024 rows sum to zero per column, asserted through pbn_debug_scoredata_shifts).  Then x - shift is a
small integer, every product and partial sum is an integer far below 2^53, and whatever the order of the f64 FMAs and MFMAs, S and G must
EQUAL the integer result.  No tolerance.  Plain form: d in (1, 15, 16, 17, 31, 33, 47, 49, 64) as permuted column subsets, n in
gram_restatement.N_UNCAPPED at row0 in (0, 1, 2, 3, 37), and the capped cases n = k B C + r (k = 4 .. 8, B = 2 CUs, C = 64 / 128) at
d in (1, 49) and (16, 48), row0 in (0, 3).  (At d = 1 and 49 the last tile has one live column: the eight columns a stage's LAST DMA
instruction moves are all dead and zeroed, so a wait that lets that instruction slip shows only where the last tile is full.)  Segmented
form: tables of 1, 17, 33, 49, 64, 65, 70 and 97 columns, one aid call each with the 495 (float: 585) ranges of
gram_restatement.segment_cases: every length at five starts.

Rounding leg.  Real-valued tables (wide() of test_gram_paths_gpu.py, offsets up to +-1000 on double tables), the pilot as in production:
|got - want| <= (N + 2) 2^-53 sum |x_i x_j| per entry of G and (N + 2) 2^-53 sum |x_i| per entry of S, with want from np.longdouble sums of
the float64 values x = fl(value - shift) for the reported shift: the bound of ANY order of N rounded products or FMAs.  No measured
constant.  The pilot: |shift - mean of the first m = min(n, 1024) rows| <= (m + 2) 2^-53 sum |x| / m.

pbn_table_sse on top: bit for bit the two host expressions (means = shift + S / N, sse = G - S_r S_c / N) applied in numpy to the aid's
output, and above 64 columns (the 32-column block pairs) a derived bound, see test_table_sse_above_64_columns.

The score handles' own segments (BIC, CVLikelihood(k = 3), HoldoutLikelihood): the reported ranges are the super-blocks of add_region, and
the installed moments equal a recomputation of the same ranges through the aid, bit for bit.

What was reached is asserted at the end (test_every_ring_state_was_seen) from the aids' records held against the restatement.

Measured on an MI355X (256 CUs; this file alone, one pytest process; profiles/gram_shapes/tests.txt): 7.5 s for the 87 tests, the slowest
(test_segments_rounding[70-8400-float32]) 0.64 s, most of it the longdouble references; the slowest exact test 0.29 s
(test_plain_exact_capped[4-float32], which also builds its table).  2 198 pbn_debug_table_gram, 28 pbn_debug_scoredata_segments and 144
pbn_table_sse calls; 484 states seen, 477 required.  Worst fraction of the rounding bound: plain form 0.345 (float64) and 0.075 (float32),
segmented form 0.329 and 0.332, the pilot 0.008 and 0.003, pbn_table_sse above 64 columns 0.663 and 0.145 (both in the means of the 129-row
range).  No test fails: the kernels are correct at every planned shape.
"""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import gram_restatement as gr
from test_gram_paths_gpu import wide
from test_mi_shapes_gpu import OFFS, int_e, spread

pytestmark = pytest.mark.gpu

U = np.longdouble(2.0) ** -53
ES = {"float64": 8, "float32": 4}
SEEN = set()
CALLS = {"pbn_debug_table_gram": 0, "pbn_debug_scoredata_segments": 0, "pbn_table_sse": 0}
FRAC = {(form, es): 0.0 for form in ("plain", "segmented", "pilot", "sse>64") for es in (8, 4)}


def offs(nc):
    """s_j of test_mi_shapes_gpu.py's OFFS, continued past its 66 columns."""
    s = np.array([(-1) ** j * (10 + j) for j in range(nc)], dtype=np.int64)
    assert np.array_equal(s[:min(nc, len(OFFS))], OFFS[:min(nc, len(OFFS))])
    return s


def int_cols(n, nc, seed):
    """int_e for any number of columns: blocks of its 66 columns side by side (the pilot rows of every column sum to zero)."""
    parts = [int_e(n, seed + 1000 * b)[0] for b in range(gr.ceil_div(nc, OFFS.size))]
    return np.hstack(parts)[:, :nc]


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib(pbn):
    from pybnesian_amd import _lib

    L = _lib.load()
    L.pbn_debug_table_gram.restype = C.c_int
    L.pbn_debug_table_gram.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 5
    L.pbn_debug_scoredata_segments.restype = C.c_int
    L.pbn_debug_scoredata_segments.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5
    L.pbn_debug_scoredata_shifts.restype = C.c_int
    L.pbn_debug_scoredata_shifts.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def num_cus():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class Plain:
    """A device table and the plain form's aid on it."""

    def __init__(self, pbn, lib, values, dtype):
        from pybnesian_amd import _lib

        self._lib, self.lib, self.es = _lib, lib, ES[dtype]
        self.nc = values.shape[1]
        names = [f"x{j}" for j in range(self.nc)]
        self.stored = np.asfortranarray(values.astype(dtype))            # what the device holds
        self.table, _ = pbn.DeviceTable.from_dataframe(pbn.default_context(), pd.DataFrame({n: self.stored[:, j] for j, n in enumerate(names)}), names)

    def gram(self, cols, row0, n, shift_in=None):
        d = len(cols)
        cc = np.ascontiguousarray(cols, dtype=np.int32)
        shift_out, S, G, rec = np.full(d, np.nan), np.full(d, np.nan), np.full((d, d), np.nan, order="F"), np.full(4, -1, dtype=np.int64)
        sin = None if shift_in is None else np.ascontiguousarray(shift_in, dtype=np.float64)
        assert sin is None or sin.size == self.nc
        self._lib.check(self.lib.pbn_debug_table_gram(self.table.handle, d, cc.ctypes.data, row0, n, None if sin is None else sin.ctypes.data,
                                                      shift_out.ctypes.data, S.ctypes.data, G.ctypes.data, rec.ctypes.data))
        CALLS["pbn_debug_table_gram"] += 1
        return shift_out, S, G, rec.tolist()

    def sse(self, cols, row0, n):
        d = len(cols)
        means, sse = np.full(d, np.nan), np.full((d, d), np.nan, order="F")
        self._lib.check(self._lib.load().pbn_table_sse(self.table.handle, self._lib.int_array([int(c) for c in cols]), d, row0, n, self._lib.dptr(means),
                                                       self._lib.dptr(sse)))
        CALLS["pbn_table_sse"] += 1
        return means, sse


class Segmented:
    """A score handle over a table and the segmented form's aid on it."""

    def __init__(self, pbn, lib, values, dtype, make=None):
        from pybnesian_amd import _lib

        self._lib, self.lib, self.es = _lib, lib, ES[dtype]
        self.nc = values.shape[1]
        self.stored = values.astype(dtype)
        df = pd.DataFrame({f"x{j}": self.stored[:, j] for j in range(self.nc)})
        self.score = pbn.BIC(df) if make is None else make(df)
        self.h = self.score._handle
        self.shift = np.full(self.nc, np.nan)
        _lib.check(lib.pbn_debug_scoredata_shifts(self.h, self.shift.ctypes.data))

    def segments(self, segs):
        m, n = len(segs), self.nc
        r0 = np.array([s[0] for s in segs], dtype=np.int64)
        r1 = np.array([s[1] for s in segs], dtype=np.int64)
        S, G, rec = np.full((m, n), np.nan), np.full((m, n, n), np.nan), np.full(4 + m, -1, dtype=np.int64)
        self._lib.check(self.lib.pbn_debug_scoredata_segments(self.h, m, r0.ctypes.data, r1.ctypes.data, S.ctypes.data, G.ctypes.data, rec.ctypes.data))
        CALLS["pbn_debug_scoredata_segments"] += 1
        return rec[4:].copy(), S, G, rec[:4].tolist()

    def own(self):
        """The handle's own segments: (region, r0, r1) rows and the installed S, G."""
        n = self.nc
        head = np.full(1, -1, dtype=np.int64)
        self._lib.check(self.lib.pbn_debug_scoredata_segments(self.h, 0, None, None, None, None, head.ctypes.data))
        m = int(head[0])
        S, G, rec = np.full((m, n), np.nan), np.full((m, n, n), np.nan), np.full(1 + 3 * m, -1, dtype=np.int64)
        self._lib.check(self.lib.pbn_debug_scoredata_segments(self.h, 0, None, None, S.ctypes.data, G.ctypes.data, rec.ctypes.data))
        assert rec[0] == m
        return rec[1:].reshape(m, 3), S, G


def first_diff(got, want):
    i = tuple(np.argwhere(got != want)[0])
    return f"entry {i}: got {got[i]!r}, want {want[i]!r}; {int((got != want).sum())} entries differ"


def check_plain_exact(t, bg, s, d, cases, num_cus):
    cols = spread(d, t.nc)
    assert cols != list(range(d)) and (d == 1 or sorted(cols) != cols) and len(set(cols)) == d    # a permuted subset, never 0 .. d - 1 in order
    for n, row0 in cases:
        shift_out, S, G, rec = t.gram(cols, row0, n, shift_in=s)
        plan = gr.plain_call(n, d, row0, t.es, num_cus)
        assert rec == plan["rec"], (d, n, row0, rec, plan["rec"])
        SEEN.update(plan["states"])
        wS, wG = bg.range(row0, row0 + n)
        wS, wG = wS[cols], wG[np.ix_(cols, cols)]
        where = f"{t.es}-byte table, d = {d}, n = {n}, row0 = {row0}, grid {rec[1]}"
        assert np.array_equal(shift_out, s[cols].astype(np.float64)), where
        assert np.array_equal(S, wS), f"{where}: S {first_diff(S, wS)}"
        assert np.array_equal(G, wG), f"{where}: G {first_diff(G, wG)}"


def worst_fraction(err, bound):
    """max err / bound; an entry whose bound is zero (all x zero) must be exact."""
    assert np.all(err[bound == 0] == 0)
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def check_rounding(key, where, N, S, G, wS, wG, aS, aG):
    """got S, G against longdouble sums wS, wG; aS = sum |x_i|, aG = sum |x_i x_j|."""
    fS = worst_fraction(np.abs(S.astype(np.longdouble) - wS), (N + 2) * U * aS)
    fG = worst_fraction(np.abs(G.astype(np.longdouble) - wG), (N + 2) * U * aG)
    print(f"rounding {key} {where}: S {fS:.3f} G {fG:.3f} of the bound")
    FRAC[key] = max(FRAC[key], fS, fG)
    assert fS <= 1.0 and fG <= 1.0, (where, fS, fG)


def moments_ld(x):
    """longdouble (S, G, sum |x|, sum |x x|) of the float64 rows x."""
    xl = x.astype(np.longdouble)
    ax = np.abs(xl)
    return xl.sum(axis=0), np.einsum("ri,rj->ij", xl, xl), ax.sum(axis=0), np.einsum("ri,rj->ij", ax, ax)


# ---- exact leg, plain form ------------------------------------------------------------------------------------------------------------------
_uncapped, _capped, _real = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def release_tables():
    """The shared tables (up to 124 MiB each on the device, their references on the host) go when the file is done."""
    yield
    for cache in (_uncapped, _capped, _real):
        cache.clear()


def uncapped_table(pbn, lib, dtype):
    if dtype not in _uncapped:
        rows = gr.uncapped_table_rows()
        e = int_e(rows, 21)[0][:, :gr.NCOL_PLAIN]
        s = offs(gr.NCOL_PLAIN)
        _uncapped[dtype] = (Plain(pbn, lib, s + e, dtype), gr.BlockGram(e, np.float64), s.astype(np.float64))
    return _uncapped[dtype]


def capped_table(pbn, lib, dtype, num_cus):
    if dtype not in _capped:
        rows = gr.capped_table_rows(num_cus, ES[dtype])
        assert rows * gr.NCOL_CAPPED * ES[dtype] <= gr.MAX_TABLE_BYTES and gr.exact_headroom(rows) < 2 ** 53
        e = np.random.default_rng(22).integers(-15, 16, size=(rows, gr.NCOL_CAPPED), dtype=np.int8).astype(np.float64)   # (no pilot here: nothing to balance)
        s = offs(gr.NCOL_CAPPED).astype(np.float64)
        _capped[dtype] = (Plain(pbn, lib, s + e, dtype), gr.BlockGram(e, np.float64), s)
    return _capped[dtype]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", gr.D_ALL)
def test_plain_exact_uncapped(pbn, lib, num_cus, d, dtype):
    t, bg, s = uncapped_table(pbn, lib, dtype)
    assert np.array_equal(t.stored.astype(np.int64), (s + bg.X).astype(np.int64))     # the offsets and integers are exact in the table's type
    check_plain_exact(t, bg, s, d, gr.uncapped_cases(), num_cus)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("k", gr.K_CAPPED)
def test_plain_exact_capped(pbn, lib, num_cus, k, dtype):
    t, bg, s = capped_table(pbn, lib, dtype, num_cus)
    for d in gr.D_CAPPED:
        check_plain_exact(t, bg, s, d, gr.capped_cases(num_cus, t.es, k), num_cus)


# ---- exact leg, segmented form --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("width", gr.SEG_WIDTHS)
def test_segments_exact(pbn, lib, width, dtype):
    e = int_cols(gr.SEG_TABLE_ROWS, width, 31 + width)
    s = offs(width)
    h = Segmented(pbn, lib, s + e, dtype)
    assert np.array_equal(h.shift, s.astype(np.float64)), "the pilot shift is not the column's integer offset"
    bg = gr.BlockGram(e, np.float64)
    segs = gr.segment_cases(h.es)
    N, S, G, rec = h.segments(segs)
    plan = gr.segment_call(segs, width, h.es)
    assert rec == plan["rec"], (rec, plan["rec"])
    SEEN.update(plan["states"])
    assert np.array_equal(N, [r1 - r0 for r0, r1 in segs])
    for i, (r0, r1) in enumerate(segs):
        wS, wG = bg.range(r0, r1)
        where = f"{h.es}-byte table of {width} columns, segment [{r0}, {r1}): {r1 - r0} rows, {len(gr.pieces(r0, r1))} pieces"
        assert np.array_equal(S[i], wS), f"{where}: S {first_diff(S[i], wS)}"
        assert np.array_equal(G[i], wG), f"{where}: G {first_diff(G[i], wG)}"
        assert np.array_equal(G[i], G[i].T)
        if r1 == r0:
            assert not S[i].any() and not G[i].any()


# ---- rounding leg -------------------------------------------------------------------------------------------------------------------------
def real_table(rows, cols, seed, dtype):
    v = wide(rows, cols, seed, dtype).to_numpy().astype(np.float64)
    if dtype == "float64":
        v = v + np.random.default_rng(seed + 1).uniform(-1000.0, 1000.0, size=cols)
    return v


def real_plain(pbn, lib, dtype):
    if dtype not in _real:
        _real[dtype] = Plain(pbn, lib, real_table(max(gr.uncapped_table_rows(), max(gr.PILOT_N) + 3), gr.NCOL_PLAIN, 41, dtype), dtype)
    return _real[dtype]


ROUNDING_CASES = ((1, 0), (2, 1), (65, 1), (191, 2), (257, 3), (513, 37), (4097, 3))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", gr.D_ALL)
def test_plain_rounding_and_table_sse(pbn, lib, num_cus, d, dtype):
    t = real_plain(pbn, lib, dtype)
    cols = spread(d, t.nc)
    for n, row0 in ROUNDING_CASES:
        shift, S, G, rec = t.gram(cols, row0, n)
        assert rec == gr.plain_call(n, d, row0, t.es, num_cus)["rec"]
        x = t.stored[row0:row0 + n][:, cols].astype(np.float64) - shift          # fl64(value - shift), as the kernels form it
        check_rounding(("plain", t.es), f"d = {d}, n = {n}, row0 = {row0}", n, S, G, *moments_ld(x))
        assert np.array_equal(G, G.T)
        # the decode and the host centring: the same launches give the same bits, and the two host expressions applied to them
        means, sse = t.sse(cols, row0, n)
        assert np.array_equal(means, shift + S / float(n)), (d, n, row0)
        assert np.array_equal(sse, G - np.outer(S, S) / float(n)), (d, n, row0)
        assert np.array_equal(sse, sse.T)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_plain_rounding_capped(pbn, lib, num_cus, dtype):
    """One capped case per element size: k = 5 chunks per block and half a grid more, so blocks of 5 and 6 whole chunks (one and one trip of the
    steady loop, 3 and 4 chunks left to the drain) and a cut chunk in the middle of the grid.  17 columns: NCT 2 with one live column in the
    last tile; the longdouble reference is what bounds the time."""
    es, d = ES[dtype], 17
    B, C = gr.GD_BLOCKS_PER_CU * num_cus, gr.chunk_rows(es)
    n, row0 = 5 * B * C + B * C // 2 + 17, 3
    t = Plain(pbn, lib, real_table(n + row0, d, 43, dtype), dtype)
    cols = spread(d, d)
    shift, S, G, rec = t.gram(cols, row0, n)
    plan = gr.plain_call(n, d, row0, es, num_cus)
    assert rec == plan["rec"] and rec[1] == B < rec[0]
    x = t.stored[row0:row0 + n][:, cols].astype(np.float64) - shift
    check_rounding(("plain", es), f"capped, d = {d}, n = {n}, row0 = {row0}", n, S, G, *moments_ld(x))
    means, sse = t.sse(cols, row0, n)
    assert np.array_equal(means, shift + S / float(n)) and np.array_equal(sse, G - np.outer(S, S) / float(n))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_pilot_shift(pbn, lib, dtype):
    t = real_plain(pbn, lib, dtype)
    cols = spread(17, t.nc)
    for n in gr.PILOT_N:
        for row0 in (0, 3):
            shift, _, _, _ = t.gram(cols, row0, n)
            m = min(n, gr.PILOT_ROWS)
            v = t.stored[row0:row0 + m][:, cols].astype(np.longdouble)
            err = np.abs(shift.astype(np.longdouble) - v.sum(axis=0) / m)
            f = worst_fraction(err, (m + 2) * U * np.abs(v).sum(axis=0) / m)
            print(f"pilot {t.es}-byte n = {n} row0 = {row0}: {f:.3f} of the bound")
            FRAC[("pilot", t.es)] = max(FRAC[("pilot", t.es)], f)
            assert f <= 1.0, (n, row0, f)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("width,rows", [(17, gr.SEG_TABLE_ROWS), (33, gr.SEG_TABLE_ROWS), (70, 8400)])
def test_segments_rounding(pbn, lib, width, rows, dtype):
    """All multi-piece segments (2 .. 9 pieces, every shape of gram_seg_reduce_kernel's four runs) and the short ones around one and five
    chunks, on real values.  70 columns take the three block-pair launches; the longdouble reference is what bounds the time, so that table
    has 8 400 rows and its segments one or two pieces.  sum |x_i x_j| is taken in float64 and the bound lowered by 1e-9 of itself for it."""
    h = Segmented(pbn, lib, real_table(rows, width, 47 + width, dtype), dtype)
    C_ = gr.chunk_rows(h.es)
    lengths = [ln for ln in gr.multi_piece_lengths() + [gr.SEG_ROWS, 1, C_ - 1, C_ + 1, 5 * C_ + C_ - 1, 8 * C_] if ln + 64 + max(gr.SEG_STARTS) <= rows]
    assert len(lengths) >= 8 and (rows < gr.SEG_TABLE_ROWS or set(gr.multi_piece_lengths()) <= set(lengths))
    segs = gr.segment_cases(h.es, lengths, rows)
    N, S, G, rec = h.segments(segs)
    assert rec == gr.segment_call(segs, width, h.es)["rec"]
    x = h.stored.astype(np.float64) - h.shift
    bx, ba = gr.BlockGram(x, np.longdouble), gr.BlockGram(np.abs(x), np.float64)
    worst = 0.0
    for i, (r0, r1) in enumerate(segs):
        (wS, wG), (aS, aG) = bx.range(r0, r1), ba.range(r0, r1)
        n = r1 - r0
        fS = worst_fraction(np.abs(S[i].astype(np.longdouble) - wS), (n + 2) * U * aS * (1 - 1e-9))
        fG = worst_fraction(np.abs(G[i].astype(np.longdouble) - wG), (n + 2) * U * aG * (1 - 1e-9))
        worst = max(worst, fS, fG)
        assert fS <= 1.0 and fG <= 1.0, (width, r0, r1, fS, fG)
        assert np.array_equal(G[i], G[i].T)
    print(f"rounding segmented {h.es}-byte {width} columns, {len(segs)} segments: {worst:.3f} of the bound")
    FRAC[("segmented", h.es)] = max(FRAC[("segmented", h.es)], worst)


# ---- pbn_table_sse above 64 columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", gr.D_WIDE)
def test_table_sse_above_64_columns(pbn, lib, d, dtype):
    """pbn_table_sse on 65, 70, 97 and 130 columns: every pair I <= J of 32-column blocks is one launch over I u J.  Bound, with u = 2^-53,
    x = fl64(value - shift) for the pilot shift of the column and range (the same in every launch; read through the aid), a_r = sum |x_r|,
    A_rc = sum |x_r x_c|, and the launch's S, G within the rounding leg's bounds dS_r = (N + 2) u a_r, dG_rc = (N + 2) u A_rc:
      sse_rc = fl(G_rc - fl(fl(S_r S_c) / N)).  The true value is G*_rc - S*_r S*_c / N.  |S_r S_c - S*_r S*_c| <= a_r dS_c + a_c dS_r + dS_r dS_c
      since |S*| <= a; the product and the division round once each, 2 u |S_r S_c| / N to first order, and the subtraction once, u |sse_rc|.  So
      |sse_rc - sse*_rc| <= u [ (N + 2) (A_rc + 2 a_r a_c / N) + 2 a_r a_c / N + |sse*_rc| ] (1 + 1e-9),
      the last factor covering every second-order term ((N + 2) u < 1e-11 here).  Likewise mean_r = fl(shift_r + fl(S_r / N)):
      |mean_r - mean*_r| <= u [ (N + 2) a_r / N + a_r / N + |mean*_r| ] (1 + 1e-9).
    The result is prefilled with NaN: every diagonal and cross block must be written, and the matrix must be symmetric bit for bit."""
    es = ES[dtype]
    rows = 1503
    t = Plain(pbn, lib, real_table(rows, d, 53 + d, dtype), dtype)
    cols = spread(d, d)
    for n, row0 in ((1500, 3), (129, 1)):
        means, sse = t.sse(cols, row0, n)
        assert not np.isnan(means).any() and not np.isnan(sse).any(), "a block pair was not filled"
        assert np.array_equal(sse, sse.T)
        shift = np.concatenate([t.gram(cols[c0:c0 + 64], row0, n)[0] for c0 in range(0, d, 64)])
        x = t.stored[row0:row0 + n][:, cols].astype(np.float64) - shift
        wS, wG, aS, aG = moments_ld(x)
        want = wG - np.outer(wS, wS) / n
        aa = np.outer(aS, aS) / n
        f = worst_fraction(np.abs(sse.astype(np.longdouble) - want), U * ((n + 2) * (aG + 2 * aa) + 2 * aa + np.abs(want)) * (1 + 1e-9))
        wmean = shift.astype(np.longdouble) + wS / n
        fm = worst_fraction(np.abs(means.astype(np.longdouble) - wmean), U * ((n + 2) * aS / n + aS / n + np.abs(wmean)) * (1 + 1e-9))
        print(f"pbn_table_sse {es}-byte d = {d} n = {n}: sse {f:.3f} means {fm:.3f} of the bound")
        FRAC[("sse>64", es)] = max(FRAC[("sse>64", es)], f, fm)
        assert f <= 1.0 and fm <= 1.0, (d, n, f, fm)
        for i, j, pos in gr.sse_pairs(d):   # the block pairs, one by one: filled and finite
            blk = sse[np.ix_(pos, pos)]
            assert np.isfinite(blk).all(), (i, j)


# ---- the handles' own segments --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("kind", ["bic", "cv", "holdout"])
def test_own_segments(pbn, lib, kind, dtype):
    make = {"bic": None, "cv": lambda df: pbn.CVLikelihood(df, k=3, seed=7), "holdout": lambda df: pbn.HoldoutLikelihood(df, test_ratio=0.2, seed=7)}[kind]
    h = Segmented(pbn, lib, real_table(5000, 17, 61, dtype), dtype, make)
    own, S, G = h.own()
    if kind == "bic":
        regions = [(0, 5000)]
    else:
        _, limits, n_cv, n_hold = h.score._layout()
        assert n_cv + n_hold == 5000
        regions = [(int(a), int(b)) for a, b in zip(limits[:-1], limits[1:])] if kind == "cv" else [(0, n_cv), (n_cv, n_cv + n_hold)]
        assert len(regions) == (3 if kind == "cv" else 2)
    want = [(reg, start + lo, start + hi) for reg, (start, end) in enumerate(regions) for lo, hi in gr.super_blocks(end - start)]
    assert own.tolist() == [list(w) for w in want]
    for reg, (start, end) in enumerate(regions):        # the ranges tile the region; inner boundaries are multiples of 64 from its start
        mine = own[own[:, 0] == reg]
        assert mine[0, 1] == start and mine[-1, 2] == end and np.array_equal(mine[1:, 1], mine[:-1, 2])
        assert all((b - start) % 64 == 0 for b in mine[:-1, 2] if b < end)
    segs = [(int(a), int(b)) for _, a, b in own]
    N, S2, G2, rec = h.segments(segs)
    assert rec == gr.segment_call(segs, 17, h.es)["rec"]
    assert np.array_equal(S, S2) and np.array_equal(G, G2), "the installed moments are not what the same ranges give again"
    assert np.array_equal(N, own[:, 2] - own[:, 1])


# ---- what was reached -------------------------------------------------------------------------------------------------------------------------
def test_every_ring_state_was_seen(num_cus):
    missing = sorted(gr.required_states(num_cus) - SEEN, key=str)
    assert not missing, missing
    print(f"\n{num_cus} CUs; states seen: {len(SEEN)} (required {len(gr.required_states(num_cus))}); aid calls: {CALLS}")
    print("worst fraction of the rounding bound: " + ", ".join(f"{form} {es}-byte {v:.3f}" for (form, es), v in sorted(FRAC.items())))
