"""KMutualInformation's device kernels (csrc/kmi.hip) at every launch form, row by row against brute force.

The kernels produce integers: per row the k-th neighbour's Chebyshev distance eps and the strict counts n_xz, n_yz, n_z on ordinal ranks, and
per row the m nearest rows in the conditioning values.  The test aid pbn_debug_kmi captures, for every evaluation, the launch form
(all-pairs kmi_eps_kernel / kmi_count_kernel<D, TILE> with `slices`, or kmi_window_kernel<O>), the host ranks (a permuted sample's uploaded
x ranks included) and the integers copied back from the device, and for every conditional p-value the neighbour table.  They are held to
EXACT equality with tests/kmi_restatement.py - numpy on the captured ranks, sharing nothing with the library or its CPU checker - so there
is no tolerance to choose; the estimate the library returns is held to the restatement's digamma mean over the captured integers at the bar
of tests/test_kmi_gpu.py (MI_REL, MI_ABS: both sides add the same N digammas in double).

What is covered, and asserted at the end (test_every_launch_form_was_seen): every D instantiation at TILE = 64 and TILE = 256, slices == 1
and > 1, every O.  On a 256-CU card kmi.hip's `slices` = min(16, 1024 / blocks) is > 1 for every table of the small grid (4999 rows: 79
blocks, 12 slices) and for 65 537 rows (257 blocks of 256, 3 slices); it is 1 only above 512 blocks, which with TILE = 64 needs more than
32 768 rows: the 33 000-row table with the all-pairs form forced (516 blocks) is the slices == 1 launch.  The expectation is computed from
the device's CU count; should a card have so few CUs that no launch of these tables slices, the final assertion says so.

Ranks are an input of the restatement, and have checks of their own: on tie-free tables they equal numpy's; on tied tables they are a
permutation per column, consistent with the values, equal between a float32 table and its widened copy, and the estimate equals the CPU
checker's, which chains its sorts as rank_data does.

Not asserted: WHICH rows the neighbour table names where distances tie (the reference's kd-tree order there is pinned by neither the
library nor the checker) - only their distances, in order, that they are distinct and in range, and on tie-free values that the first is
the row itself.  P-values above 65 536 rows are held only to pipelined == serial at small N (PBN_KMI_PIPELINE_MIN_ROWS forces the worker
thread), where both equal the CPU checker exactly.

Run time, measured on the MI355X box (this file alone, one pytest process): 13 s, 7 s of it numpy brute force (the 4999-row tables of the
small grid: 4 s); the budget is a minute - past it the row samples of the large tables shrink, never the grid.
"""
import ctypes as C
import time

import numpy as np
import pandas as pd
import pytest

import kmi_restatement as kr

pytestmark = pytest.mark.gpu

MI_REL, MI_ABS = 1e-10, 1e-12          # tests/test_kmi_gpu.py's bar for the estimate

DIMS = (2, 3, 4, 5, 6, 7, 8, 11, 16)
NS = (63, 64, 65, 255, 256, 257, 1025, 4999)
KS = (1, 2, 10, 63, 64)
HUGE = str(10 ** 9)

SEEN = set()                           # launch forms the tests met: ("pairs", D, TILE, slices > 1) / ("window", O)
BRUTE = {}                             # (table key, dims) -> {k: (eps, cnt)}: the all-pairs and the window run share one brute force
SPENT = {"brute": 0.0}


# ---- the capture hook ----------------------------------------------------------------------------------------------------------
class Capture:
    def __init__(self):
        from pybnesian_amd import _lib

        self.fn = _lib.load().pbn_debug_kmi
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_void_p, C.c_int64]

    def arm(self):
        self.fn(1, None, 0)

    def disarm(self):
        self.fn(0, None, 0)

    def take(self):
        """The records since arm(), parsed (the layout is at pbn_debug_kmi's definition); the capture is cleared and stays armed."""
        n = self.fn(2, None, 0)
        buf = np.zeros(n, dtype=np.int64)
        self.fn(2, buf.ctypes.data, n)
        self.arm()
        recs, i = [], 0
        while i < n:
            if buf[i] == 1:
                window, form, tile, slices, dims, rows, k, permuted = (int(v) for v in buf[i + 1:i + 9])
                i += 9
                r = {"kind": "eval", "window": window, "form": form, "tile": tile, "slices": slices, "dims": dims, "n": rows, "k": k,
                     "permuted": permuted, "vars": buf[i:i + dims].tolist()}
                i += dims
                r["R"] = buf[i:i + dims * rows].reshape(dims, rows).T
                i += dims * rows
                r["eps"] = buf[i:i + rows]
                i += rows
                r["cnt"] = None
                if dims > 2:
                    r["cnt"] = buf[i:i + 3 * rows].reshape(3, rows)
                    i += 3 * rows
            else:
                assert buf[i] == 2
                nz, rows, m = (int(v) for v in buf[i + 1:i + 4])
                i += 4
                r = {"kind": "nbr", "nz": nz, "n": rows, "m": m, "vars": buf[i:i + nz].tolist()}
                i += nz
                r["nbr"] = buf[i:i + rows * m].reshape(rows, m)
                i += rows * m
            recs.append(r)
        assert i == n
        return recs


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def cap(pbn):
    c = Capture()
    c.arm()
    yield c
    c.disarm()
    print(f"\nbrute force took {SPENT['brute']:.1f} s of this file")


@pytest.fixture(scope="module")
def num_cus(pbn):
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def names(d):
    return [f"c{j}" for j in range(d)]


def mixed(n, seed, d=16):
    """Tie-free; neighbouring columns dependent, distant ones nearly independent."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, d))
    v[:, 1] += 0.8 * v[:, 0]
    for j in range(2, d):
        v[:, j] += 0.6 * np.tanh(v[:, j - 2])
    return pd.DataFrame(v, columns=names(d))


def independent(n, seed, d=8):
    """Every column independent of all others: the window walk is as long as it gets."""
    return pd.DataFrame(np.random.default_rng(seed).normal(size=(n, d)), columns=names(d))


def monotone(n, seed, d=8):
    """Every column a strictly monotone function of one latent: ranks equal or reversed, the distance of two rows is their step along the
    window axis and the walk ends at once."""
    t = np.sort(np.random.default_rng(seed).uniform(0.5, 2.0, size=n))
    np.random.default_rng(seed + 1).shuffle(t)
    fns = [lambda u: u, lambda u: -u, np.exp, lambda u: -np.log(u), lambda u: u ** 3, np.sqrt, lambda u: 1 / u, lambda u: 2 * u + 1]
    v = np.stack([fns[j % 8](t) for j in range(d)], axis=1)
    return pd.DataFrame(v, columns=names(d))


def numpy_ranks(values):
    """Ordinal ranks of tie-free columns: no sorting routine can disagree."""
    r = np.empty(values.shape, np.int64)
    for j in range(values.shape[1]):
        assert len(np.unique(values[:, j])) == len(values)
        r[np.argsort(values[:, j]), j] = np.arange(len(values))
    return r


# ---- expectations and comparisons --------------------------------------------------------------------------------------------------
def expected_pairs_form(dims, n, cus):
    """Kmi::launch / launch_d and the `slices` formula of Kmi::evaluate."""
    tile = 64 if n < 64 * 1024 else 256
    blocks = -(-n // tile)
    return (dims if dims <= 6 else 0), tile, max(1, min(16, cus * 4 // blocks))


def check_form(rec, cus, window):
    dims, n = rec["dims"], rec["n"]
    if window:
        others = dims - 1
        want = (1, others if others <= 3 else 0, 256, 0)
        SEEN.add(("window", want[1]))
    else:
        d, tile, slices = expected_pairs_form(dims, n, cus)
        want = (0, d, tile, slices)
        SEEN.add(("pairs", d, tile, slices > 1))
    got = (rec["window"], rec["form"], rec["tile"], rec["slices"])
    assert got == want, f"launch form (window, D or O, TILE, slices) {got}, expected {want} at dims {dims}, N {n}"


def brute(key, R, ks, rows=None):
    """eps and counts of R by brute force for every k of ks, remembered under `key` (the same table and columns give the same ranks in
    both forms; the caller has compared R)."""
    have = BRUTE.setdefault(key, {})
    need = [k for k in ks if k not in have]
    if need:
        t0 = time.perf_counter()
        have.update(kr.eps_counts(R, need, rows))
        SPENT["brute"] += time.perf_counter() - t0
    return have


def assert_integers(rec, want, rows=None, what=""):
    """Every row (or the rows given) of a captured evaluation equals the brute force (eps, cnt)."""
    eps, cnt = want
    sel = slice(None) if rows is None else rows
    got = rec["eps"][sel]
    bad = np.flatnonzero(got != eps)
    assert bad.size == 0, f"{what}: eps differs at {bad.size} rows, first row {bad[0]}: device {got[bad[0]]}, brute force {eps[bad[0]]}"
    if rec["dims"] == 2:
        assert rec["cnt"] is None and cnt is None
        return
    for c, name in enumerate(("n_xz", "n_yz", "n_z")):
        got = rec["cnt"][c][sel]
        bad = np.flatnonzero(got != cnt[c])
        assert bad.size == 0, f"{what}: {name} differs at {bad.size} rows, first row {bad[0]}: device {got[bad[0]]}, brute force {cnt[c][bad[0]]}"


def assert_mi(value, rec, what=""):
    want = kr.mi_from_integers(rec["R"], rec["k"], rec["eps"], rec["cnt"])
    assert value == pytest.approx(want, rel=MI_REL, abs=MI_ABS), what


def evaluate(pbn, cap, df, k, dims_list, **kw):
    """mi(c0, c1 | c2 ...) for every dims of dims_list on one handle: ({dims: value}, {dims: record})."""
    test = pbn.KMutualInformation(df, k, seed=0, **kw)
    cols = list(df.columns)
    cap.take()
    values = {d: test.mi(cols[0], cols[1], cols[2:d] or None) for d in dims_list}
    recs = cap.take()
    assert [r["kind"] for r in recs] == ["eval"] * len(dims_list)
    for d, r in zip(dims_list, recs):
        assert (r["dims"], r["n"], r["k"], r["permuted"], r["vars"]) == (d, len(df), k, 0, list(range(d)))
    return values, dict(zip(dims_list, recs))


# ---- the small grid, both forms: every row against brute force ------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form", ["pairs", "window"])
def test_small_grid_every_row(pbn, cap, num_cus, monkeypatch, form, n):
    """dims x N x k of the issue's grid (k < N; k = N - 1 at 63 rows: every row is a neighbour), once through the all-pairs kernels and once
    with the window form forced: the launch form logged is the expected one, the captured ranks are numpy's, every row's integers equal
    brute force, the estimate equals the restatement's on them.  257 rows is a second block of one thread in the window form; ranks 0
    and N - 1 are its one-sided walks (every row is checked, so they are)."""
    monkeypatch.setenv("PBN_KMI_WINDOW_MIN_ROWS", "0" if form == "window" else HUGE)
    df = mixed(n, 1000 + n)
    ranks = numpy_ranks(df.to_numpy())
    ks = [k for k in KS if k < n] + ([n - 1] if n == 63 else [])
    assert len(ks) >= 3
    got = {k: evaluate(pbn, cap, df, k, DIMS) for k in ks}
    parities = set()
    for dims in DIMS:
        for k in ks:
            assert np.array_equal(got[k][1][dims]["R"], ranks[:, :dims]), (dims, k)
        want = brute(("mixed", n, dims), ranks[:, :dims], ks)
        for k in ks:
            value, rec = got[k][0][dims], got[k][1][dims]
            what = f"{form} form, N {n}, dims {dims}, k {k}"
            check_form(rec, num_cus, form == "window")
            assert_integers(rec, want[k], what=what)
            assert_mi(value, rec, what)
            if dims == 3:
                parities |= set((rec["eps"] % 2).tolist())
    if n == 63:
        eps = got[62][1][3]["eps"]
        assert (eps == np.maximum(ranks[:, :3], 62 - ranks[:, :3]).max(axis=1)).all()      # the farthest row
    # the window form's second walk stops at step eps - 1; with one conditioning column (dims 3) the rows at steps eps - 1 and eps are in z
    # whatever they are, so a walk one step short or long miscounts n_z: both parities of eps (two steps per trip) must have occurred
    assert parities == {0, 1}


# ---- tables that take TILE = 256, slices == 1, and the window form by default: all rows form against form, a sample against brute force ----
def sampled(key, recs, what):
    """The row sample of captured evaluations of the same columns (one per k) against brute force."""
    first = recs[0]
    rows = kr.row_sample(first["R"], 1 if first["dims"] == 2 else 2, seed=first["n"] + first["dims"])
    want = brute(key, first["R"], [r["k"] for r in recs], rows)
    for r in recs:
        assert np.array_equal(r["R"], first["R"])
        assert_integers(r, want[r["k"]], rows, f"{what}, k {r['k']}")


@pytest.mark.parametrize("n,dims_list", [(65_537, (2, 3, 4, 5, 6, 7)), (33_000, (3, 7))])
def test_large_tables_all_pairs(pbn, cap, num_cus, monkeypatch, n, dims_list):
    """65 537 rows: TILE = 256 at every D (the issue asks for dims 3 and 7; the others cost a launch each).  33 000 rows with the all-pairs
    form forced: the slices == 1 launch of a 256-CU card at TILE = 64 (516 blocks).  k = 10.  Every captured row equals the window form's
    of the same table (both from the device: equality of the two forms); the row sample (first and last 64 rows, the window axis's four
    lowest and highest ranks, 128 random rows) equals brute force."""
    df = mixed(n, 7 + n, 8)
    ranks = numpy_ranks(df.to_numpy())
    monkeypatch.setenv("PBN_KMI_WINDOW_MIN_ROWS", HUGE)
    pairs_v, pairs = evaluate(pbn, cap, df, 10, dims_list)
    monkeypatch.delenv("PBN_KMI_WINDOW_MIN_ROWS")
    window_v, window = evaluate(pbn, cap, df, 10, dims_list)
    for dims in dims_list:
        what = f"N {n}, dims {dims}"
        a, w = pairs[dims], window[dims]
        check_form(a, num_cus, False)
        check_form(w, num_cus, True)
        assert np.array_equal(a["R"], ranks[:, :dims]) and np.array_equal(w["R"], ranks[:, :dims])
        assert np.array_equal(a["eps"], w["eps"]), what
        assert dims == 2 or np.array_equal(a["cnt"], w["cnt"]), what
        sampled(("large", n, dims), [a], what)
        assert_mi(pairs_v[dims], a, what)
        assert window_v[dims] == pairs_v[dims]


@pytest.mark.parametrize("n,make", [(32_768, mixed), (40_001, mixed), (40_001, monotone), (40_001, independent)])
def test_window_form_by_default(pbn, cap, num_cus, n, make):
    """Tables of 32 768 (the threshold itself) and 40 001 rows take the window form without being told to: every O, k = 1, 10 and 64, the row
    sample against brute force (it holds the rows at ranks 0-3 and N-4 to N-1 of the window axis: one-sided walks).  `monotone`: the walk
    ends at once; `independent`: the longest walk."""
    df = make(n, 11 + n, 8)
    ranks = numpy_ranks(df.to_numpy())
    dims_list = (2, 3, 4, 5, 8)
    got = {k: evaluate(pbn, cap, df, k, dims_list) for k in (1, 10, 64)}
    for dims in dims_list:
        what = f"{make.__name__}, N {n}, dims {dims}"
        assert np.array_equal(got[1][1][dims]["R"], ranks[:, :dims])
        sampled(("default", make.__name__, n, dims), [recs[dims] for _, recs in got.values()], what)
        for k, (values, recs) in got.items():
            check_form(recs[dims], num_cus, True)
            assert_mi(values[dims], recs[dims], f"{what}, k {k}")
            if make is monotone:       # the distance of two rows is their step: the k-th neighbour is ceil(k / 2) steps away, k at the ends
                assert recs[dims]["eps"].max() == k and recs[dims]["eps"].min() == (k + 1) // 2


# ---- ties ---------------------------------------------------------------------------------------------------------------------------
def tied(n, seed):
    """Columns in the order [x, y, z...] the test uses them in, so that the library (which ranks the whole table, one index vector sorted
    column after column as rank_data does) and the CPU checker (which is given the columns of one call) chain the same sorts."""
    rng = np.random.default_rng(seed)
    a = np.round(rng.normal(size=n) * 4) / 4                          # rounded to quarters
    b = rng.poisson(6.0, size=n).astype(np.float64)                   # integer-valued
    c = np.zeros(n)
    c[n // 3] = 1.0                                                   # constant but for one row
    d = np.round((0.7 * a + rng.normal(size=n)) * 2) / 2              # a coarser grid, dependent on a
    e = rng.normal(size=n)                                            # continuous
    return pd.DataFrame({"a": a, "b": b, "c": c, "d": d, "a2": a.copy(), "e": e})


@pytest.mark.parametrize("n,k", [(257, 3), (1201, 5), (1201, 64)])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tied_values(pbn, cap, num_cus, monkeypatch, n, k, dtype):
    """Ranks of tied columns: a permutation per column, consistent with the values, the same for a float32 table and its widened copy; the
    integers of both forms equal brute force on them; the estimate equals the CPU checker's.  (This test found the checker ranking every
    column from the identity instead of chaining the sorts: 257 rows, k = 3, the first two columns: 0.1304 against the library's 0.4632.)"""
    from oracle import oracle

    df = tied(n, n + k).astype(dtype)
    wide = df.astype("float64")                                       # float32 widens exactly
    values = wide.to_numpy()
    dims_list = (2, 3, 4, 5, 6)
    monkeypatch.setenv("PBN_KMI_WINDOW_MIN_ROWS", HUGE)
    pairs_v, pairs = evaluate(pbn, cap, df, k, dims_list)
    _, of_wide = evaluate(pbn, cap, wide, k, dims_list)
    monkeypatch.setenv("PBN_KMI_WINDOW_MIN_ROWS", "0")
    window_v, window = evaluate(pbn, cap, df, k, dims_list)
    R = pairs[6]["R"]
    for j in range(6):
        assert np.array_equal(np.sort(R[:, j]), np.arange(n)), f"column {j}: the ranks are not a permutation of 0..N-1"
        by_rank = values[np.argsort(R[:, j]), j]
        assert (np.diff(by_rank) >= 0).all(), f"column {j}: a smaller value holds a larger rank"
    assert len(np.unique(values[:, 0])) < n / 4 and np.array_equal(values[:, 0], values[:, 4])
    for dims in dims_list:
        what = f"N {n}, k {k}, dims {dims}, {dtype}"
        assert np.array_equal(pairs[dims]["R"], R[:, :dims]) and np.array_equal(window[dims]["R"], R[:, :dims])
        assert np.array_equal(of_wide[dims]["R"], R[:, :dims]), what + ": the float32 table ranks differently from its widened copy"
        check_form(pairs[dims], num_cus, False)
        check_form(window[dims], num_cus, True)
        want = brute(("tied", n, k, dtype, dims), R[:, :dims], [k])[k]
        assert_integers(pairs[dims], want, what=what + " (all-pairs)")
        assert_integers(window[dims], want, what=what + " (window)")
        assert_mi(pairs_v[dims], pairs[dims], what)
        assert window_v[dims] == pairs_v[dims]
        checker, _ = oracle.kmi(values[:, :dims], k)
        assert pairs_v[dims] == pytest.approx(checker, rel=MI_REL, abs=MI_ABS), what


# ---- the conditional shuffle's neighbour table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 600])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_neighbour_table(pbn, cap, n, m):
    """z of 1, 2, 3, 7 and 14 columns, tie-free and with tied values.  Per row the captured neighbours' distances, in captured order, ARE the
    sorted m smallest distances (doubles from fmax / fabs of differences on both sides: no rounding differs); the indices are distinct and
    in range; on tie-free z the first is the row itself.  Which rows are named where distances tie is not asserted: the reference's kd-tree
    order there is pinned by neither the library nor its checker."""
    for label, df in (("tie-free", mixed(n, 50 + n + m)), ("tied", mixed(n, 60 + n + m).round(1))):
        test = pbn.KMutualInformation(df, 3, seed=1, shuffle_neighbors=m, samples=1)
        cols = list(df.columns)
        for nz in (1, 2, 3, 7, 14):
            cap.take()
            test.pvalue(cols[0], cols[1], cols[2:2 + nz])
            recs = [r for r in cap.take() if r["kind"] == "nbr"]
            assert len(recs) == 1
            rec = recs[0]
            assert (rec["nz"], rec["n"], rec["m"], rec["vars"]) == (nz, n, m, list(range(2, 2 + nz)))
            nbr = rec["nbr"]
            assert nbr.min() >= 0 and nbr.max() < n
            assert all(len(set(row)) == m for row in nbr.tolist()), "a row is named twice"
            z = df[cols[2:2 + nz]].to_numpy()
            got = kr.chebyshev(z, np.arange(n)[:, None], nbr)
            want = kr.neighbor_distances(z, m)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"{label}, N {n}, m {m}, nz {nz}: {bad.size} rows, first {bad[0]}: {got[bad[0]]} against {want[bad[0]]}"
            if label == "tie-free":
                assert (nbr[:, 0] == np.arange(n)).all()


# ---- permutation p-values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 257, 513])
@pytest.mark.parametrize("nz", [0, 1, 3, 6])
def test_permutation_pvalues(pbn, cap, monkeypatch, n, nz):
    """The p-value equals the CPU checker's exactly (same permutations, same integers) with 1 and 64 shuffle neighbours, in the all-pairs and
    the window form, serial and with the worker thread forced (PBN_KMI_PIPELINE_MIN_ROWS); every uploaded permuted x column is a
    permutation of 0..N-1, its integers equal brute force, and the pipelined run captures what the serial run captures, sample by sample.
    A dependent pair (c0, c1: p = 0 whatever is permuted) and a nearly independent one (c0, c7: the p-value moves with the permutations)."""
    from oracle import oracle

    df = mixed(n, 300 + n + nz, 8)
    k, seed, samples = 4, 5 + nz, 12
    wanted = []
    for m, cols in ((1, names(8)), (64, names(8)), (1, ["c0", "c7"] + names(7)[1:]), (64, ["c0", "c7"] + names(7)[1:])):
        data = df[cols[:2 + nz]].to_numpy()
        _, want = oracle.kmi(data, k, seed, m, samples)
        wanted.append(want)
        captured = {}
        for window in (False, True):
            for pipelined in (False, True):
                monkeypatch.setenv("PBN_KMI_WINDOW_MIN_ROWS", "0" if window else HUGE)
                monkeypatch.setenv("PBN_KMI_PIPELINE_MIN_ROWS", "0" if pipelined else HUGE)
                test = pbn.KMutualInformation(df, k, seed=seed, shuffle_neighbors=m, samples=samples)
                cap.take()
                got = test.pvalue(cols[0], cols[1], cols[2:2 + nz] or None)
                recs = [r for r in cap.take() if r["kind"] == "eval"]
                what = f"N {n}, nz {nz}, m {m}, window {window}, pipelined {pipelined}"
                assert got == want, what
                assert len(recs) == samples + 1 and [r["permuted"] for r in recs] == [0] + [1] * samples, what
                assert recs[0]["vars"] == [df.columns.get_loc(c) for c in cols[:2 + nz]]
                for r in recs:
                    assert r["window"] == int(window)
                    assert np.array_equal(np.sort(r["R"][:, 0]), np.arange(n)), what + ": the permuted x is not a permutation"
                    assert np.array_equal(r["R"][:, 1:], recs[0]["R"][:, 1:])
                captured[window, pipelined] = recs
        first = captured[False, False]
        for key, recs in captured.items():
            for s, (a, b) in enumerate(zip(first, recs)):
                assert np.array_equal(a["R"], b["R"]) and np.array_equal(a["eps"], b["eps"]), (key, s)
                assert nz == 0 or np.array_equal(a["cnt"], b["cnt"]), (key, s)
        for s in (0, 1, samples):                        # the original and two permuted samples against brute force
            r = first[s]
            assert_integers(r, kr.eps_counts(r["R"], [k])[k], what=f"N {n}, nz {nz}, m {m}, sample {s}")
    assert 0.0 < wanted[3] < 1.0            # (the checker's value: the equalities above had a p-value that moves with the permutations)


# ---- argument checks at the caps ------------------------------------------------------------------------------------------------------
def test_argument_checks_at_the_caps(pbn, cap):
    df = mixed(70, 3, 17)
    cols = list(df.columns)
    test = pbn.KMutualInformation(df, 64, seed=0, samples=3)                                  # k = 64: the cap, accepted
    good = test.mi(cols[0], cols[1], cols[2:16])                                               # 16 variables: the cap, accepted
    with pytest.raises(ValueError, match="conditioning set too large"):
        test.mi(cols[0], cols[1], cols[2:17])                                                  # 17
    with pytest.raises(ValueError, match="conditioning set too large"):
        test.pvalue(cols[0], cols[1], cols[2:17])
    with pytest.raises(ValueError, match="repeated variable"):
        test.mi(cols[0], cols[0])
    with pytest.raises(ValueError, match="repeated variable"):
        test.mi(cols[0], cols[1], [cols[2], cols[1]])
    with pytest.raises(ValueError, match="repeated variable"):
        test.pvalue(cols[0], cols[1], [cols[2], cols[2]])
    assert test.mi(cols[0], cols[1], cols[2:16]) == good                                       # the handle is usable afterwards
    assert 0.0 <= test.pvalue(cols[0], cols[1], cols[2:16]) <= 1.0
    with pytest.raises(ValueError, match=r"k must be between 1 and min\(64, rows - 1\)"):
        pbn.KMutualInformation(df, 65)
    small = df.iloc[:40]
    with pytest.raises(ValueError, match=r"k must be between 1 and min\(64, rows - 1\)"):
        pbn.KMutualInformation(small, 40)                                                      # k = N
    with pytest.raises(ValueError, match=r"k must be between 1 and min\(64, rows - 1\)"):
        pbn.KMutualInformation(small, 0)
    edge = pbn.KMutualInformation(small, 39, seed=0)                                           # k = N - 1
    cap.take()
    value = edge.mi(cols[0], cols[1], cols[2])
    (rec,) = cap.take()
    assert_integers(rec, kr.eps_counts(rec["R"], [39])[39], what="k = N - 1 at 40 rows")
    assert_mi(value, rec)


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------
def test_every_launch_form_was_seen(cap):
    """The launch forms the tests above met are the ones the dispatch (Kmi::launch, launch_d, the window switch of Kmi::evaluate) can
    produce: an instantiation added there and reached by no test fails here.  (Needs the whole file to have run.)"""
    ds = {2, 3, 4, 5, 6, 0}
    pairs = {f for f in SEEN if f[0] == "pairs"}
    assert {(f[1], f[2]) for f in pairs} == {(d, t) for d in ds for t in (64, 256)}
    assert {f[3] for f in pairs} == {False, True}, "no launch with slices == 1, or none with slices > 1, on this card"
    assert {f[1] for f in SEEN if f[0] == "window"} == {1, 2, 3, 0}
