"""GPU tier: the partial sums of the d = 8 far pass, cell by cell against fp64 (kde_sweep_far32_d8_kernel, csrc/kde_far32_d8.inc).

tests/test_far32_d8_gpu.py holds the far WORDS; what the far kernel then writes was held against nothing but the launch's slogl, of which
the far blocks of the suite's tables carry 1e-13.  Here every (split, query column) cell of the launch's partial rows (pbn_debug_d8_masks,
what = 8: rows 0 .. nsplit - 1 the fp64 sweep's, rows nsplit .. 2 nsplit - 1 the far pass's; a pair (o, s) is s 2^o, base 2) is compared
with a plain fp64 sum over the blocks the dumped words name.  For sorted training row t and sorted query q the exponent is
x = z_t.z_q - |z_t|^2/2 - |z_q|^2/2 (Dump.column_maxima's); both sides of every comparison are scaled by 2^-m_q, m_q = ceil of the query's
largest exponent, so nothing underflows in fp64.

a. Far cells.  F_ref = sum of 2^x over the 16 rows of every tile whose far bit is set for the query's tile in the split; F_dev from far
   row nsplit + split.  |F_dev - F_ref| <= eps F_ref + n_terms 2^(-126 + o): eps = the kernel's proven per-term bound
   (pbn_debug_far32_rule, 1.94e-3; all terms are positive, so it carries to sums), the second summand the terms v_exp_f32 flushes below
   2^-126 on the biased scale.  A non-empty cell's offset: o + BIAS an integer in [thr + margin, thr + margin + 1) - off = ceil(qrow_thr),
   what makes kde_finish_kernel's scale factors exact powers of two.  A cell without a far block holds exactly (-1e300, 0); the row array
   has nqtiles * 16 columns and no more (the second group of an odd last wave writes nothing); padding columns are left out of the sums.
   CELL_TOL, test_lincor_batch_gpu.py's convention: 8 x the largest |F_dev / F_ref - 1| measured on the MI355X over every non-empty cell
   clear of the flush term, asserted as measured <= CELL_TOL / 8 and CELL_TOL <= eps.  At eps one dropped or doubled tile in a cell of more
   than 500 far tiles would pass; at CELL_TOL / 8 = 2.75e-05 a tile of its cell's average weight cannot in any cell that a split of at
   most 1 024 tiles holds.  MEASURED 2.696e-05 at the largest (CELL_TOL below, profiles/far32_cells/tests.txt).
b. Coverage of the ring, counted from the far words alone (test_ring_classes_occur): far-tile counts 0, 1, R - 1, R, R + 1, 8 R, 8 R + 1
   and more than 16 R (R = PBN_FAR32_RING; the reload past the end, the `go` flag, the 8-turn carry into the double), both per cell and
   per list the ring walks (the union of a wave's two groups); far tiles in two 64-tile batches of one split; a wave whose groups differ on
   a tile (gsel 1, 2 and 3 in one walk); a last split shorter than the others; an odd number of query tiles.  The launches: the sizes of
   tests/test_far32_d8_gpu.py (32 768, 32 769, 65 537, 131 087 rows x 17, 33, 1 025 queries; splits of 64 or 65 tiles at these sizes) and
   the two tables of part d - more than 16 R far tiles in a cell takes a whole split of 65 tiles far, which only "shell65" has.  A split
   never exceeds PBN_PRUNE_MAX_TILES = 1 024 tiles in a shipped build (compiled in), so the kernel's second 4 096-tile super-batch cannot
   be reached and is not reached for.
c. The fp64 sweep's cells: the same reference over live & ~far against sweep row `split`, relative BUDGET (3e-7, the sum-only budget) where
   the reference is non-zero, a zero sum where the cell has no such block: a far block evaluated twice or by neither kernel shows in its cell.
   MEASURED: at most 1.06e-07 in any cell (2^f on the fp32 unit), so the sweep's own fp32 tail (PBN_FAR_SPAN) gets no slack of its own.
d. Tables on which the far mass is visible (shell_tables): isolated queries on a spot beside a dense shell - the far blocks hold 1e-7 and
   more of at least 8 queries' sums (MEASURED: "shell" 11 queries at 4.2e-07, S = 4.7e-06; "shell65" 32 at 2.3e-06, S = 7.3e-05), so the
   launch's slogl sees the far rows: within 2 eps S of the switch at 0, within S / 8 of it and of the unpruned sweep (S = the queries' far
   shares added up), every query's 2 nsplit rows together its fp64 sum over the live blocks (every launch of a. is held to that), and the
   three screen kernels the same far rows bit for bit.
profiles/far32_cells/tests.txt has every figure, and which assertion caught each of three deliberate faults in the kernel."""
import ctypes as C
import re

import numpy as np
import pandas as pd
import pytest

from helpers import CSRC
from test_far32_d8_gpu import NCAP, FarDump, header_constant, theta_of
from test_prune_d8_screen_gpu import margin_of
from test_prune_d8_screen_rowthr_gpu import env
from test_prune_d8_screen_stream_gpu import fetch
from test_prune_d8_screen_stream_gpu import lib, pbn  # noqa: F401  (fixtures)
from test_prune_d8_sweep_gpu import BUDGET, frames

pytestmark = pytest.mark.gpu

BIAS = header_constant("PBN_FAR32_BIAS")
with open(f"{CSRC}/kde_far32_d8.inc") as _f:
    R = int(re.search(r"^#define PBN_FAR32_RING (\d+)", _f.read(), flags=re.M).group(1))

# 8 x the largest |F_dev / F_ref - 1| over the non-empty far cells of every launch below (MI355X, against the fp64 reference of this file):
# MEASURED 2.696e-05 (32 769 x 1 025, column 90 of split 14, one far tile; per launch 8.5e-06 ... 2.7e-05 on the correlated tables, 4.0e-06 and 1.5e-06 on
# the shell tables, whose cells hold up to 65 tiles of much the same weight) -> CELL_TOL = 2.2e-04, an eighth of it 2.75e-05
CELL_TOL = 2.2e-4
FLUSH_CLEAR = 2.0 ** -40   # a cell counts towards the measured maximum when its flush term is below this share of its reference

NATURAL = [(n_train, n_test) for n_train in (32_768, 32_769, 65_537, 131_087) for n_test in (17, 33, 1_025)]


def eps_of(lib):
    eps = C.c_double()
    lib.pbn_debug_far32_rule.argtypes = [C.c_double, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.pbn_debug_far32_rule.restype = None
    lib.pbn_debug_far32_rule(NCAP, 1_000_000, C.byref(eps), None)
    return eps.value


class CellDump(FarDump):
    """... and the launch's partial rows (what = 8): [rows][nqt * 16][2], rows = nsplit, or 2 nsplit where the far pass ran."""

    def __init__(self, lib, k, test, stream="2", **kv):
        super().__init__(lib, k, test, stream, **kv)
        part = fetch(lib, 8, np.float64)
        lib.pbn_debug_d8_masks(0, None, 0, 0)
        rows = self.nsplit * (2 if self.far is not None else 1)
        assert part.size == rows * self.nqt * 16 * 2, (part.size, rows, self.nqt)
        self.part = part.reshape(rows, self.nqt * 16, 2)


def shell_tables(n=32_768, outer=0.05, radius=2.5, seed=1616, spot_queries=16, shell_queries=17):
    """d = 8: 16 training rows within 1e-3 of the origin (the spot), `outer` of the rows on the sphere of `radius`, the rest on the unit
    sphere with 2 % radial jitter; queries: 16 within 1e-3 of the origin and 17 from the shell (33: an odd number of query tiles).  With the
    diagonal normal-reference bandwidth the shell lies 30 to 39 bits below a spot query's sum of 16 spot terms - inside the far window
    (theta 30.07, margin 38.07 at 32 768 rows) - and the largest 1/2|z|^2 stays below the cap.
    How much of that window a spot query's far blocks cover depends on its bound, and the window pass centres a query tile's window on the
    tile's FIRST query: spot queries in a tile that a shell query leads get a bound well below their sum.  Of these 16, 11 sit in a tile of
    their own kind (far share 4.2e-7 each); "shell65" asks 48 spot queries beside the 17, of which whole tiles are spot queries whatever
    the order (2.3e-6 each), on 32 784 rows: splits of 65 tiles, and whole splits far.  (Seventeen shell queries, not fewer: a spot
    query's log-density is near 0, and a slogl below 0.33 per query is evaluated once more at full precision, kde_sum_needs_precision -
    it would not come from the rows held here.)"""
    rng = np.random.default_rng(seed)
    d = 8

    def sphere(count, r):
        v = rng.normal(size=(count, d))
        return v / np.linalg.norm(v, axis=1, keepdims=True) * np.reshape(r, (-1, 1))

    n_out = int(round(outer * n))
    n_shell = n - 16 - n_out
    train = np.vstack([sphere(16, rng.uniform(0.0, 1e-3, 16)), sphere(n_out, np.full(n_out, radius)),
                       sphere(n_shell, 1.0 + 0.02 * rng.normal(size=n_shell))])
    train = train[rng.permutation(n)]
    test = np.vstack([sphere(spot_queries, rng.uniform(0.0, 1e-3, spot_queries)), sphere(shell_queries, 1.0 + 0.02 * rng.normal(size=shell_queries))])
    names = [f"v{i}" for i in range(d)]
    return names, pd.DataFrame(train, columns=names), pd.DataFrame(test, columns=names)


def reference(d):
    """fp64, per sorted query column (padding columns: all zero), scaled by 2^-m_q: the block sums T[column][training tile] and m_q."""
    zt = np.zeros((d.ntiles * 16, 8))
    zt[:len(d.zt)] = d.zt
    nt = -0.5 * np.sum(zt * zt, axis=1)
    nt[len(d.zt):] = -np.inf
    T = np.zeros((d.nqt * 16, d.ntiles))
    m = np.zeros(d.nqt * 16)
    for i in range(0, d.nq, 64):
        q = d.zq[i:i + 64]
        x = q @ zt.T + nt[None, :] - 0.5 * np.sum(q * q, axis=1)[:, None]
        mq = np.ceil(x.max(axis=1))
        m[i:i + len(q)] = mq
        T[i:i + len(q)] = np.exp2(x - mq[:, None]).reshape(len(q), d.ntiles, 16).sum(axis=2)
    return T, m


def by_split(d, a):
    """[..., ntiles] -> [..., nsplit, tps], the tiles past the table's end zero."""
    out = np.zeros(a.shape[:-1] + (d.nsplit * d.tps,), dtype=a.dtype)
    out[..., :d.ntiles] = a
    return out.reshape(a.shape[:-1] + (d.nsplit, d.tps))


def ring_classes(d):
    """What the far words alone say about the lists the ring walks and the cells it fills: names of the classes of 2b that occur."""
    far = d.tile_bits(d.far)
    cells = by_split(d, far).sum(axis=-1)                                 # [query tile][split]: far tiles of a cell
    b = d.bits(d.far)                                                     # [wave][split][batch][group][64]
    g0, g1 = b[:, :, :, 0, :], b[:, :, :, 1, :]
    if d.nqt % 2:                                                         # (the absent second group of an odd last wave: whatever its words say, it has no cells)
        g1 = g1.copy()
        g1[-1] = g0[-1]
    lists = (g0 | g1).sum(axis=(2, 3))                                    # [wave][split]: tiles of the wave's one list
    seen = set()
    for name, counts in (("cell", cells), ("list", lists)):
        for label, hit in (("0", counts == 0), ("1", counts == 1), ("R-1", counts == R - 1), ("R", counts == R), ("R+1", counts == R + 1),
                           ("8R", counts == 8 * R), ("8R+1", counts == 8 * R + 1), (">16R", counts > 16 * R)):
            if hit.any():
                seen.add(f"{name} of {label} far tiles")
    if ((g0 | g1).any(axis=3).sum(axis=2) >= 2).any():
        seen.add("far tiles in two batches of a split")
    if ((g0 & ~g1).any(axis=(2, 3)) & (~g0 & g1).any(axis=(2, 3)) & (g0 & g1).any(axis=(2, 3))).any():
        seen.add("gsel 1, 2 and 3 in one walk")
    last = d.ntiles - (d.nsplit - 1) * d.tps
    if 0 < last < d.tps and cells[:, -1].any():
        seen.add("far tiles in a short last split")
    if d.nqt % 2:
        seen.add("an odd number of query tiles")
    return seen, np.bincount(cells.ravel(), minlength=1), np.bincount(lists.ravel(), minlength=1)


CLASSES = {f"{name} of {label} far tiles" for name in ("cell", "list") for label in ("0", "1", "R-1", "R", "R+1", "8R", "8R+1", ">16R")} | {
    "far tiles in two batches of a split", "gsel 1, 2 and 3 in one walk", "far tiles in a short last split", "an odd number of query tiles"}


def check_cells(d, eps, margin, label):
    """2a and 2c on one launch's dump; returns the figures (the measured maxima, the far shares, the per-query combination's error)."""
    assert d.far is not None and d.part.shape[0] == 2 * d.nsplit
    T, m = reference(d)
    cols = d.nqt * 16
    valid = np.arange(cols) < d.nq
    far, live = d.tile_bits(d.far), d.tile_bits(d.live)
    assert not np.any(far & ~live)
    fbits = np.repeat(by_split(d, far), 16, axis=0)                      # [column][split][tile of the split]
    sbits = np.repeat(by_split(d, live & ~far), 16, axis=0)
    Ts = by_split(d, T)
    F_ref, n_far = (Ts * fbits).sum(axis=-1), fbits.sum(axis=-1)         # [column][split]
    W_ref, n_sw = (Ts * sbits).sum(axis=-1), sbits.sum(axis=-1)
    total = T.sum(axis=1)

    # ---- a. the far rows
    o, s = d.part[d.nsplit:, :, 0].T, d.part[d.nsplit:, :, 1].T          # [column][split]
    empty = n_far == 0
    assert np.all(o[empty] == -1e300) and np.all(s[empty] == 0.0), f"{label}: a cell without a far block holds {o[empty][s[empty] != 0.0][:4]}, {s[empty][s[empty] != 0.0][:4]}"
    assert np.all((s > 0.0) | ((o == -1e300) & (s == 0.0))), f"{label}: a far pair that is neither a positive sum nor (-1e300, 0)"
    raw = (d.thr + margin)[:, None]                                      # (what = 6 is the bound less the margin)
    filled = (s > 0.0) & valid[:, None]
    ob = o + BIAS
    assert np.all(ob[filled] == np.round(ob[filled])), f"{label}: a far offset that is no integer"
    gap = (ob - raw)[filled]
    assert np.all((gap >= -1e-9) & (gap < 1.0 + 1e-9)), f"{label}: a far offset that is not ceil(qrow_thr): o + BIAS - bound in [{gap.min()}, {gap.max()}]"
    check = valid[:, None] & ~empty
    o_use = np.where(s > 0.0, o, np.ceil(np.where(np.isfinite(raw), raw, 0.0)) - BIAS)   # (a cell flushed to nothing: the offset it would have had)
    flush = 16.0 * n_far * np.exp2(np.where(check, -126.0 + o_use - m[:, None], 0.0))
    F_dev = s * np.exp2(np.where(s > 0.0, o - m[:, None], 0.0))
    err = np.abs(F_dev - F_ref)
    bad = check & ~(err <= eps * F_ref + flush)
    assert not bad.any(), (f"{label}: {int(bad.sum())} far cells beyond eps; the first (column, split) {np.argwhere(bad)[0]}: device {F_dev[bad][0]!r} "
                           f"reference {F_ref[bad][0]!r}, {n_far[bad][0]} far tiles")
    clear = check & (F_ref > 0.0) & (flush <= FLUSH_CLEAR * F_ref)
    rel = np.where(clear, err / np.where(F_ref > 0.0, F_ref, 1.0), 0.0)
    at = np.unravel_index(np.argmax(rel), rel.shape)
    worst = float(rel[at])
    print(f"{label}: far cells {int(check.sum())} non-empty ({int(clear.sum())} clear of the flush term) of {int(valid.sum()) * d.nsplit}; "
          f"largest |F_dev / F_ref - 1| {worst:.3e} at column {at[0]} split {at[1]} ({n_far[at]} far tiles); eps {eps:.3e}")

    # ---- c. the fp64 sweep's rows
    o2, s2 = d.part[:d.nsplit, :, 0].T, d.part[:d.nsplit, :, 1].T
    W_dev = s2 * np.exp2(np.where(s2 != 0.0, o2 - m[:, None], 0.0))
    none = valid[:, None] & (n_sw == 0)
    stray = none & (s2 != 0.0)
    some = valid[:, None] & (W_ref > 0.0)
    rel2 = np.where(some, np.abs(W_dev - W_ref) / np.where(some, W_ref, 1.0), 0.0)
    share2 = np.where(some, np.abs(W_dev - W_ref) / total[:, None].clip(min=1e-300), 0.0)   # ... as a share of the query's whole sum
    at2 = np.unravel_index(np.argmax(rel2), rel2.shape)
    print(f"{label}: sweep cells {int(some.sum())} non-empty, largest relative error {rel2[at2]:.3e} at column {at2[0]} split {at2[1]} (as a share of the "
          f"query's sum {share2[at2]:.3e}; largest such share {share2.max():.3e}); {int(none.sum())} cells without a block, {int(stray.sum())} of them non-zero"
          + (f" (largest {float((W_dev / total[:, None].clip(min=1e-300))[stray].max()):.3e} of its query's sum)" if stray.any() else ""))
    assert not stray.any(), f"{label}: {int(stray.sum())} sweep cells without a block of live & ~far hold a sum; the first (column, split) {np.argwhere(stray)[0]}"
    over = some & ~(np.abs(W_dev - W_ref) <= BUDGET * W_ref)
    assert not over.any(), (f"{label}: {int(over.sum())} sweep cells beyond BUDGET; the first (column, split) {np.argwhere(over)[0]}: device "
                            f"{W_dev[over][0]!r} reference {W_ref[over][0]!r}")

    # ---- per query: all 2 nsplit rows together against the fp64 sum over its live blocks
    both = (F_dev + W_dev).sum(axis=1)
    live_ref = (Ts * np.repeat(by_split(d, live), 16, axis=0)).sum(axis=(1, 2))
    ok = valid & (live_ref > 0.0)
    comb = float(np.max(np.abs(both - live_ref)[ok] / live_ref[ok]))
    share = np.where(total > 0.0, F_ref.sum(axis=1) / np.where(total > 0.0, total, 1.0), 0.0)[:d.nq]   # per sorted query: the far blocks' share of its whole sum
    print(f"{label}: rows combined against the live blocks: largest relative error {comb:.3e}; far shares: largest {share.max():.3e}, "
          f"{int((share >= 1e-7).sum())} queries at 1e-7 or more, sum {share.sum():.3e}")
    assert comb <= BUDGET, f"{label}: a query's rows together miss its live blocks by {comb:.3e}"
    return dict(worst=worst, cells=int(check.sum()), share=share, comb=comb, sweep=float(rel2[at2]))


@pytest.fixture(scope="module")
def models(pbn):
    """Per training size the model of tests/test_far32_d8_gpu.py (same table, same seed) and its queries; fitted once."""
    done = {}

    def get(n_train):
        if n_train not in done:
            names, train, test = frames("correlated", 8, 1600 + n_train % 1000, n_train, 3_200)
            k = pbn.ProductKDE(names)
            k.fit(train)
            done[n_train] = (k, test)
        return done[n_train]

    return get


SHELLS = {"shell": dict(), "shell65": dict(n=32_784, spot_queries=48)}
CASES = NATURAL + list(SHELLS)


@pytest.fixture(scope="module")
def shell(pbn):
    """The tables of part d: per name the model, the same fitted with pruning off (the switch is read at the fit), the queries and the
    number of training rows; fitted once."""
    done = {}

    def get(name):
        if name not in done:
            names, train, test = shell_tables(**SHELLS[name])
            k = pbn.ProductKDE(names)
            k.fit(train)
            with env(PBN_SWEEP_PRUNE="0"):
                k0 = pbn.ProductKDE(names)
                k0.fit(train)
            done[name] = (k, k0, test, len(train))
        return done[name]

    return get


@pytest.fixture(scope="module")
def dumps(lib, models, shell):
    """One launch's dump per case, taken once: (n_train, n_test) of the natural sizes, or the name of a shell table."""
    done = {}

    def get(case):
        if case not in done:
            if case in SHELLS:
                k, _, test, n = shell(case)
                done[case] = (CellDump(lib, k, test), n)
            else:
                k, test = models(case[0])
                done[case] = (CellDump(lib, k, test.iloc[:case[1]]), case[0])
        return done[case]

    return get


@pytest.mark.parametrize("case", CASES, ids=lambda c: c if isinstance(c, str) else f"{c[0]}x{c[1]}")
def test_cells_against_fp64(lib, dumps, case):
    d, n = dumps(case)
    eps = eps_of(lib)
    assert d.passes == 1
    got = check_cells(d, eps, margin_of(n), str(case))
    assert got["cells"] >= 1, "the far rows are exercised"
    print(f"{case}: MEASURED largest far cell error {got['worst']:.3e} (CELL_TOL / 8 = {CELL_TOL / 8:.3e}, eps {eps:.3e})")
    assert CELL_TOL <= eps
    assert got["worst"] <= CELL_TOL / 8


def test_ring_classes_occur(dumps):
    seen = set()
    cells, lists = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
    for case in CASES:
        d, _ = dumps(case)
        s, c, l = ring_classes(d)
        print(f"{case}: nsplit {d.nsplit}, {d.tps} tiles a split (the last {d.ntiles - (d.nsplit - 1) * d.tps}), {d.nqt} query tiles; classes new here: {sorted(s - seen)}")
        seen |= s
        n = max(len(cells), len(c), len(l))
        cells = np.pad(cells, (0, n - len(cells))) + np.pad(c, (0, n - len(c)))
        lists = np.pad(lists, (0, n - len(lists))) + np.pad(l, (0, n - len(l)))
    pick = [0, 1, R - 1, R, R + 1, 8 * R, 8 * R + 1]
    print("far tiles: cells / lists of that count: " + ", ".join(f"{v}: {cells[v] if v < len(cells) else 0} / {lists[v] if v < len(lists) else 0}" for v in pick)
          + f", > {16 * R}: {int(cells[16 * R + 1:].sum())} / {int(lists[16 * R + 1:].sum())}")
    assert not CLASSES - seen, f"classes of cell no launch reaches: {sorted(CLASSES - seen)}"


@pytest.mark.parametrize("name", list(SHELLS))
def test_far_mass_is_visible(lib, shell, dumps, name):
    """Part d: the table's far blocks hold a share of the sums that slogl can see, and slogl sees the far rows right."""
    k, k0, test, n = shell(name)
    on, _ = dumps(name)
    eps, theta, margin = eps_of(lib), theta_of(lib, n), margin_of(n)
    assert on.passes == 1 and on.nqt % 2 == 1 and (on.nqt == 3 or name != "shell"), "an odd number of query tiles; 33 queries: three"
    assert abs(on.slogl) >= 0.33 * on.nq, "slogl comes from the screened launch (kde_sum_needs_precision: no second, precise evaluation)"
    n_t, n_q = 0.5 * np.sum(on.zt * on.zt, axis=1), 0.5 * np.sum(on.zq * on.zq, axis=1)
    assert n_t.max() <= NCAP and n_q.max() <= NCAP, (n_t.max(), n_q.max())
    T, m = reference(on)
    total = T.sum(axis=1)[:on.nq]
    far = np.repeat(on.tile_bits(on.far), 16, axis=0)[:on.nq]
    share = (T[:on.nq] * far).sum(axis=1) / total
    assert np.allclose(np.log2(total) + m[:on.nq], on.log2_sums(), rtol=0, atol=1e-9), "the reference's whole sums are Dump.log2_sums'"
    S = float(share.sum())
    print(f"{name}: theta {theta:.2f} margin {margin:.2f}, largest 1/2|z|^2 {max(n_t.max(), n_q.max()):.1f}; far shares of the {on.nq} sums: largest {share.max():.3e}, "
          f"{int((share >= 1e-7).sum())} at 1e-7 or more, S = {S:.3e}")
    assert (share >= 1e-7).sum() >= 8, "the far mass is visible in at least 8 sums"
    off = FarDump(lib, k, test, PBN_D8_FAR32="0")
    assert off.far is None and off.passes == 0
    plain = k0.slogl(test)
    print(f"{name}: slogl far {on.slogl!r} fp64 {off.slogl!r} unpruned {plain!r}: |far - fp64| {abs(on.slogl - off.slogl):.3e} (2 eps S = {2 * eps * S:.3e}, "
          f"S / 8 = {S / 8:.3e}), |far - unpruned| {abs(on.slogl - plain):.3e}")
    assert abs(on.slogl - off.slogl) <= 2.0 * eps * S, "both launches evaluate the same blocks, each within eps"
    assert abs(on.slogl - off.slogl) < S / 8 and abs(on.slogl - plain) < S / 8, "the far rows reach the merge once"


@pytest.mark.parametrize("name", list(SHELLS))
def test_three_screen_kernels_give_the_same_far_rows(lib, shell, dumps, name):
    k, _, test, _ = shell(name)
    on, _ = dumps(name)
    for stream in ("0", "1"):
        other = CellDump(lib, k, test, stream)
        assert np.array_equal(on.far, other.far)
        assert other.part.shape == on.part.shape and on.part[on.nsplit:].tobytes() == other.part[on.nsplit:].tobytes(), f"far rows of screen kernel {stream}"
        assert on.slogl == other.slogl
