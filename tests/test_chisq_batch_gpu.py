"""GPU tier: the batch form of ChiSquare (csrc/chisq.hip behind pbn_chisq_pvalue_batch).

The contract has no tolerance in it.  The integer table the kernel counts must equal np.bincount of the keys over the rows valid in the
test's variables, and the p-value - the scalar routine's own arithmetic on those integers - must equal ChiSquare.pvalue of the same
test on the same handle bit for bit, whether the test was counted on the device or looped on the host.  The test aid pbn_debug_chisq
(layout at its definition in csrc/chisq.hip) says where every test ran, with which code width, in how many slices and LDS copies, and hands
back the table as it came off the device.

One case cannot go through ChiSquare.pvalue: a one-category x or y has zero degrees of freedom, where the scalar routine answers 1 or -
when rounding leaves its statistic a few ulps above 0 - NaN without pbn_last_error, and pvalue() raises.  The batch returns that same
NaN silently in its slot; check() compares those slots with pbn_chisq_pvalue itself, NaN equal to NaN."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib
from pybnesian_amd.constraint import pc_estimate_indices
from pybnesian_amd.independences import mmpc_cpcs

pytestmark = pytest.mark.gpu


def discrete_table(n, rows, seed):
    rng = np.random.default_rng(seed)
    cards = rng.integers(2, 5, n)
    cols = []
    for v in range(n):
        k = min(v, int(rng.integers(0, 3)))
        pa = sorted(rng.choice(v, k, replace=False)) if k else []
        cfg = np.zeros(rows, dtype=np.int64); m = 1
        for p in pa:
            cfg += cols[p] * m; m *= cards[p]
        cpt = rng.dirichlet(np.full(cards[v], 0.35), size=m)
        u = rng.random(rows)
        cols.append((u[:, None] > np.cumsum(cpt[cfg], axis=1)).sum(1).clip(0, cards[v] - 1))
    return np.stack(cols), cards        # columns -> pd.Categorical.from_codes


def frame(codes, cards, extra=None):
    """Categorical columns v0, v1, ... from a [columns][rows] code matrix (-1 = null)."""
    data = {f"v{i}": pd.Categorical.from_codes(codes[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(len(cards))}
    data.update(extra or {})
    return pd.DataFrame(data)


def uniform_codes(cards, rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, c, rows) for c in cards])


class Capture:
    def __init__(self):
        self.fn = _lib.load().pbn_debug_chisq
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_void_p, C.c_int64]

    def __enter__(self):
        self.fn(1, None, 0)
        return self

    def __exit__(self, *exc):
        self.fn(0, None, 0)

    def take(self):
        """The batch calls since the last take(): per call a dict with the grouping counter before / after and the per-test records."""
        n = self.fn(2, None, 0)
        buf = np.zeros(max(n, 1), dtype=np.int64)
        self.fn(2, buf.ctypes.data, n)
        self.fn(1, None, 0)
        calls, i = [], 0
        while i < n:
            assert buf[i] == 3
            n_tests, g0, g1 = (int(v) for v in buf[i + 1:i + 4])
            i += 4
            tests = []
            for _ in range(n_tests):
                where, width, slices, copies, cells, held = (int(v) for v in buf[i:i + 6])
                i += 6
                tests.append({"where": where, "width": width, "slices": slices, "R": copies, "G": cells, "table": buf[i:i + held].copy()})
                i += held
            calls.append({"groups_before": g0, "groups_after": g1, "tests": tests})
        assert i == n
        return calls


def run_batch(chi, tests):
    """pbn_chisq_pvalue_batch called directly; tests = [(x, y, [z...])] in the index space set on the handle."""
    n = len(tests)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t[2]) for t in tests])
    cond = np.array([v for t in tests for v in t[2]] or [0], dtype=np.int32)
    v1 = np.array([t[0] for t in tests], dtype=np.int32)
    v2 = np.array([t[1] for t in tests], dtype=np.int32)
    out = np.full(n, -1.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _lib.load().pbn_chisq_pvalue_batch(chi._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
    return out


def expected_table(codes, cards, test):
    vs = [test[0], test[1]] + list(test[2])
    valid = np.all(codes[vs] >= 0, axis=0)
    key = np.zeros(int(valid.sum()), dtype=np.int64)
    stride = 1
    for v in vs:
        key += codes[v][valid] * stride
        stride *= int(cards[v])
    return np.bincount(key, minlength=stride)


def check(chi, codes, cards, tests, cap, device=None):
    """One direct batch call at threshold 0 against bincount and against the scalar routine; returns the per-test capture records.
    device: per test, whether it must have been counted on the device (None = all of them)."""
    chi.set_batch_threshold(0)
    _lib.check(_lib.load().pbn_mi_set_order(chi._handle, 0, None))
    before = chi.batch_stats()
    out = run_batch(chi, tests)
    calls = cap.take()
    assert len(calls) == 1 and len(calls[0]["tests"]) == len(tests)
    recs = calls[0]["tests"]
    device = [True] * len(tests) if device is None else device
    for t, rec, p, dev in zip(tests, recs, out, device):
        assert rec["where"] == (1 if dev else 0), (t, rec["where"])
        if dev:
            want = expected_table(codes, cards, t)
            assert rec["G"] == len(want) and np.array_equal(rec["table"], want), t
        else:
            assert len(rec["table"]) == 0
        name = lambda v: f"v{v}"
        args = (name(t[0]), name(t[1]), [name(z) for z in t[2]])
        if min(cards[t[0]], cards[t[1]]) > 1:
            scalar = chi.pvalue(*args)
            assert p == scalar, (t, p, scalar)           # bit for bit
        else:
            # a one-category x or y: zero degrees of freedom, where the scalar routine answers 1 when its statistic is exactly 0 and
            # NaN when rounding left it a few ulps above (pvalue() then raises).  The batch must give that very answer.
            a = chi._args(*args)
            scalar = _lib.load().pbn_chisq_pvalue(chi._handle, a[0], a[1], a[2], a[3])
            assert p == scalar or (np.isnan(p) and np.isnan(scalar)), (t, p, scalar)
    moved = tuple(a - b for a, b in zip(chi.batch_stats(), before))
    assert moved == (sum(device), len(device) - sum(device))
    return recs


@pytest.fixture(scope="module")
def cap():
    with Capture() as c:
        yield c


@pytest.fixture(scope="module")
def caps():
    lib = _lib.load()
    max_cells, max_cond = lib.pbn_chisq_batch_max_cells(), lib.pbn_chisq_batch_max_cond()
    assert max_cells >= 4096 and max_cond >= 6
    return max_cells, max_cond


ROW_CARDS = [2, 3, 7, 2, 2, 2, 2, 2, 2, 3]
SLICE_ROWS = 4096                       # a test is cut into at most rows // max(SLICE_ROWS, 8 G) slices ...
SLICE_ALIGN = 2048                      # ... whose length is rounded up to a multiple of this (256 lanes x 8 rows of one load)


def slicing(rows, cells):
    """(slices, rows per slice) of one test by the host's rule, for calls of so few tests that the chip asks for more slices than the
    rule allows (a handful of tests, rows <= a few SLICE_ROWS: true of every chip with five compute units or more)."""
    s = max(1, rows // max(SLICE_ROWS, 8 * cells))
    per = -(-(-(-rows // s)) // SLICE_ALIGN) * SLICE_ALIGN
    return -(-rows // per), per


ONE_ROW_TAIL = 2 * 3 * SLICE_ALIGN + 1     # 12 289 rows of a 6-cell table: three slices asked for, 4 097 rows each rounded up to 6 144, one row left


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 2 * SLICE_ROWS + 1, ONE_ROW_TAIL, 3 * SLICE_ROWS + 5])
def test_counts_at_every_row_shape(cap, caps, rows):
    """Block, wave and load-width edges of the row loop, one slice, two slices (6 144 + 2 049 rows), two slices and ONE row (the tail of
    the 8-byte load path: a last slice of a single row), three slices with a tail of five (the atomic flush), and every conditioning-set
    size 0 ... max_cond on the device with max_cond + 1 looping on the host."""
    max_cells, max_cond = caps
    codes = uniform_codes(ROW_CARDS, rows, rows)
    chi = pbn.ChiSquare(frame(codes, ROW_CARDS))
    others = [3, 4, 5, 6, 7, 8, 9, 2]
    assert max_cond + 1 <= len(others)
    tests = [(0, 1, others[:k]) for k in range(max_cond + 2)] + [(2, 1, [0]), (9, 2, [1, 0, 3]), (1, 0, []), (4, 3, [2, 1])]
    device = [len(t[2]) <= max_cond for t in tests]
    assert device.count(False) == 1
    recs = check(chi, codes, ROW_CARDS, tests, cap, device)
    slices = max(r["slices"] for r in recs)
    widths = {r["width"] for r in recs if r["where"] == 1}
    assert widths == {1}
    for r in recs:
        if r["where"] == 1:
            assert r["slices"] == slicing(rows, r["G"])[0], (r["G"], r["slices"])
    if rows <= SLICE_ROWS + 1:
        assert slices == 1
    elif rows == 2 * SLICE_ROWS + 1:
        assert slices == 2
    else:
        assert slices >= 3
    if rows == ONE_ROW_TAIL:
        assert ONE_ROW_TAIL == 12289
        n, per = slicing(rows, recs[0]["G"])
        assert recs[0]["slices"] == n == 3 and rows - (n - 1) * per == 1       # the last slice of (v0, v1) holds exactly one row


def test_cardinalities_code_widths_and_caps(cap, caps):
    """Cardinalities 1, 2, 3, 7, 255 on the byte mirror, a 300-category column on int32 codes, tables of exactly max_cells cells (one LDS
    copy) and above it (host), 2 x 2 tables (32 copies)."""
    max_cells, max_cond = caps
    rows = 5003
    cards = [1, 2, 3, 7, 255, 8, 8, 8, 8, 2, 2]
    codes = uniform_codes(cards, rows, 11)
    # a table of exactly max_cells cells out of the 8-category columns, whatever the cap is
    full = [5, 6]
    cells = 64
    fill = [7, 8]
    while cells * 8 <= max_cells and fill:
        full.append(fill.pop(0)); cells *= 8
    pad_cards = []
    while cells < max_cells:
        step = min(8, max_cells // cells)
        pad_cards.append(step); cells *= step
    assert cells == max_cells and len(full) + len(pad_cards) <= max_cond + 2
    for c in pad_cards:
        cards.append(c); full.append(len(cards) - 1)
    codes = uniform_codes(cards, rows, 11)
    tests = [(0, 1, []), (1, 0, [2]), (0, 0 + 9, [10]), (1, 2, []), (2, 3, [1]), (4, 1, []), (4, 3, []), (3, 4, [1]), (9, 10, []),
             (full[0], full[1], full[2:]),                         # max_cells cells: device
             (full[0], full[1], full[2:] + [9]),                   # twice that: host
             (4, 3, [2])]                                          # 255 * 7 * 3 = 5 355 cells: host when the cap is 4 096
    device = [int(np.prod([cards[v] for v in [t[0], t[1]] + list(t[2])])) <= max_cells for t in tests]
    assert device[-3] and not device[-2]
    chi = pbn.ChiSquare(frame(codes, cards))
    recs = check(chi, codes, cards, tests, cap, device)
    on_device = [r for r in recs if r["where"] == 1]
    assert {r["width"] for r in on_device} == {1}
    copies = {r["R"] for r in on_device}
    assert min(copies) == 1 and max(copies) == 32, copies          # the fullest table and the 2 x 2 one
    assert recs[-3]["G"] == max_cells and recs[-3]["R"] == 1 and recs[8]["R"] == 32

    # one 300-category column: every code column of the handle is read as int32
    wide_cards = [2, 3, 300, 7, 2]
    wide = uniform_codes(wide_cards, rows, 12)
    chi = pbn.ChiSquare(frame(wide, wide_cards))
    tests = [(0, 1, []), (2, 0, []), (2, 1, [0]), (0, 1, [2]), (3, 4, [0, 1]), (1, 3, [4])]
    recs = check(chi, wide, wide_cards, tests, cap)
    assert {r["width"] for r in recs} == {4}


@pytest.mark.parametrize("card, nulls, width", [(255, True, 1), (256, True, 4), (256, False, 1)])
def test_null_bucket_at_the_byte_limit(cap, card, nulls, width):
    """A column with nulls holds one more code, the null bucket (code == cardinality): 255 still fits a byte, 256 does not.  Without
    nulls 256 categories are the codes 0 ... 255 and fit: code 255 is then a category, the same byte that pads the mirror past N."""
    rows = 4099
    cards = [card, 2, 3]
    codes = uniform_codes(cards, rows, card)
    codes[0, ::2] = card - 1                                       # the top category next to the bucket is well filled
    if nulls:
        codes[0, 5::7] = -1
    chi = pbn.ChiSquare(frame(codes, cards))
    recs = check(chi, codes, cards, [(0, 1, []), (1, 0, [2]), (1, 2, [0]), (1, 2, [])], cap)
    assert {r["width"] for r in recs} == {width}
    assert recs[0]["table"].sum() == (codes[0] >= 0).sum() and ((codes[0] >= 0).sum() < rows) == nulls


@pytest.mark.parametrize("value", [0, 1])
def test_constant_columns_put_every_row_in_one_cell(cap, value):
    rows = 3 * SLICE_ROWS + 77
    cards = [2, 2, 3]
    codes = uniform_codes(cards, rows, 5)
    codes[0, :] = value
    codes[1, :] = value
    chi = pbn.ChiSquare(frame(codes, cards))
    recs = check(chi, codes, cards, [(0, 1, []), (1, 0, [2]), (0, 2, [1])], cap)
    assert recs[0]["table"][value * 3] == rows and recs[0]["table"].sum() == rows
    assert recs[0]["R"] == 32 and recs[0]["slices"] >= 3


def test_nulls_in_x_y_z_and_all(cap):
    """A test counts exactly the rows valid in all of ITS variables."""
    rows = 2 * SLICE_ROWS + 501
    cards = [3, 2, 4, 2, 3, 2]
    rng = np.random.default_rng(8)
    codes = uniform_codes(cards, rows, 7)
    for col, rate in ((0, 0.2), (1, 0.1), (2, 0.3), (4, 0.05)):
        codes[col, rng.random(rows) < rate] = -1
    chi = pbn.ChiSquare(frame(codes, cards))
    tests = [(0, 3, []), (0, 3, [5]),           # x only
             (3, 1, []), (5, 1, [3]),           # y only
             (3, 5, [2]), (5, 3, [2]),          # one Z column
             (0, 1, [2, 4]), (1, 0, [4, 2, 3]), (4, 2, [0, 1]),   # all of them
             (3, 5, [])]                        # none
    recs = check(chi, codes, cards, tests, cap)
    assert recs[-1]["table"].sum() == rows
    assert recs[6]["table"].sum() == np.all(codes[[0, 1, 2, 4]] >= 0, axis=0).sum() < rows


def test_order_set_through_the_callback(cap):
    """The index space of the batch is the node list handed to _ci_callback."""
    rows = 6001
    cards = [2, 3, 4, 2, 3]
    codes = uniform_codes(cards, rows, 21)
    chi = pbn.ChiSquare(frame(codes, cards))
    chi.set_batch_threshold(0)
    perm = [3, 0, 4, 2, 1]                      # external index i stands for column perm[i]
    keep = chi._ci_callback([f"v{p}" for p in perm])
    tests = [(0, 1, []), (1, 2, [0]), (4, 3, [2, 0]), (2, 4, [1, 3, 0])]
    out = run_batch(chi, tests)
    recs = cap.take()[0]["tests"]
    del keep
    for t, rec, p in zip(tests, recs, out):
        real = (perm[t[0]], perm[t[1]], [perm[z] for z in t[2]])
        assert rec["where"] == 1 and np.array_equal(rec["table"], expected_table(codes, cards, real)), t
        assert p == chi.pvalue(f"v{real[0]}", f"v{real[1]}", [f"v{z}" for z in real[2]])


def test_batch_equals_scalar_at_scale(cap):
    """1e6 rows x 12 columns, 2 000 distinct tests with at most three conditioning variables in one call."""
    rows, n_tests = 1_000_000, 2000
    rng = np.random.default_rng(3)
    cards = rng.integers(2, 5, 12)
    codes = uniform_codes(cards, rows, 4)
    codes[1] = (codes[0] + (rng.random(rows) < 0.4) * codes[2]) % cards[1]      # some dependence
    codes[5] = (codes[4] * (rng.random(rows) < 0.7)) % cards[5]
    chi = pbn.ChiSquare(frame(codes, cards))
    chi.set_batch_threshold(0)
    seen, tests = set(), []
    while len(tests) < n_tests:
        k = int(rng.integers(0, 4))
        vs = rng.choice(12, 2 + k, replace=False).tolist()
        key = (vs[0], vs[1], tuple(vs[2:]))
        if key not in seen:
            seen.add(key); tests.append((vs[0], vs[1], vs[2:]))
    _lib.check(_lib.load().pbn_mi_set_order(chi._handle, 0, None))
    passes, stats = chi.passes(), chi.batch_stats()
    out = run_batch(chi, tests)
    call = cap.take()[0]
    assert tuple(a - b for a, b in zip(chi.batch_stats(), stats)) == (n_tests, 0)
    assert chi.passes() == passes and call["groups_before"] == call["groups_after"] == 0      # no row grouping, no sort
    assert all(r["where"] == 1 and r["width"] == 1 for r in call["tests"])
    for i in (0, 999, 1999):
        assert np.array_equal(call["tests"][i]["table"], expected_table(codes, cards, tests[i]))
    name = lambda v: f"v{v}"
    scalar = np.array([chi.pvalue(name(a), name(b), [name(z) for z in zs]) for a, b, zs in tests])
    assert np.array_equal(out, scalar)
    assert 0 < (out < 0.05).sum() < n_tests


@pytest.fixture(scope="module")
def pc_table():
    cols, cards = discrete_table(16, 20000, 1)
    return frame(cols, cards)


def same(a, b):
    assert a["arcs"] == b["arcs"] and a["edges"] == b["edges"]
    assert a["sepsets"] == b["sepsets"]            # sets AND p-values
    assert a["serial_tests"] == b["serial_tests"]


def test_pc_end_to_end(pc_table):
    chi = pbn.ChiSquare(pc_table)
    names = chi.variable_names()
    serial = pc_estimate_indices(chi, names, batched=False)
    assert chi.batch_stats() == (0, 0)
    print(f"serial tests {serial['serial_tests']}, arcs {len(serial['arcs'])}, edges {len(serial['edges'])}")
    assert serial["serial_tests"] == 855 and len(serial["arcs"]) == 9 and len(serial["edges"]) == 6
    same(pc_estimate_indices(chi, names), serial)           # the default threshold
    chi.set_batch_threshold(0)
    before = chi.batch_stats()
    batched = pc_estimate_indices(chi, names)
    same(batched, serial)
    dev, host = (a - b for a, b in zip(chi.batch_stats(), before))
    assert dev > 0 and host == 0                             # at most 4^6 cells and four conditioning variables: nothing too large
    graph = pbn.PC().estimate(chi)
    idx = {v: i for i, v in enumerate(names)}
    assert sorted((idx[a], idx[b]) for a, b in graph.arcs()) == serial["arcs"]
    assert sorted(tuple(sorted((idx[a], idx[b]))) for a, b in graph.edges()) == serial["edges"]


def test_mmpc_with_and_without_the_batch(pc_table):
    chi = pbn.ChiSquare(pc_table)
    chi.set_batch_threshold(0)
    names = chi.variable_names()
    batched = mmpc_cpcs(chi, names, 0.05)
    assert chi.batch_stats()[0] > 0
    plain = pbn.ChiSquare(pc_table)
    plain._ci_batch_callback = lambda: None
    serial = mmpc_cpcs(plain, names, 0.05)
    assert plain.batch_stats() == (0, 0)
    assert batched == serial                                 # the sets of every node and the number of tests


def test_dynamic_chi_square_gets_the_batch(pc_table):
    dyn = pbn.DynamicChiSquare(pbn.DynamicDataFrame(pc_table.iloc[:4000, :4], 1))
    static = dyn.static_tests()
    assert isinstance(static, pbn.ChiSquare) and static._ci_batch_callback()
    static.set_batch_threshold(0)
    g = pbn.PC().estimate(static)
    assert isinstance(g, pbn.PartiallyDirectedGraph) and g.num_nodes() == len(static.variable_names())
    assert static.batch_stats()[0] > 0
    assert isinstance(pbn.PC().estimate(dyn.transition_tests()), pbn.PartiallyDirectedGraph)


class HybridChi(pbn.ChiSquare):
    """A ChiSquare whose handle also holds the continuous columns, so that a continuous variable can be asked for."""

    def __init__(self, df):
        pbn.MutualInformation.__init__(self, df, True)


def test_a_continuous_variable_is_refused():
    rows = 3000
    cards = [2, 3, 2]
    codes = uniform_codes(cards, rows, 2)
    rng = np.random.default_rng(2)
    chi = HybridChi(frame(codes, cards, {"x": rng.normal(size=rows)}))      # variable ids: x = 0, v0 ... v2 = 1 ... 3
    chi.set_batch_threshold(0)
    _lib.check(_lib.load().pbn_mi_set_order(chi._handle, 0, None))
    out = run_batch(chi, [(1, 2, []), (0, 2, []), (1, 2, [0]), (2, 3, [1]), (1, 9, [])])
    assert np.isnan(out[[1, 2, 4]]).all() and not np.isnan(out[[0, 3]]).any()
    assert out[0] == chi.pvalue("v0", "v1") and out[3] == chi.pvalue("v1", "v2", ["v0"])
    with pytest.raises(ValueError):
        chi.pvalue("x", "v1")
    with pytest.raises(ValueError):
        pbn.PC().estimate(chi)
    with pytest.raises(ValueError):
        pc_estimate_indices(chi, chi.variable_names(), batched=False)
