"""GPU tier: the count-only tests of pbn_mi_pvalue_batch - x, y and Z all categorical - counted by the joint-count kernel (csrc/mi.hip on
mi::count_tables of csrc/chisq.hip).

The contract has no tolerance in it.  The integer table the kernel counts must equal np.bincount of the keys over the rows valid in the
test's variables, and the p-value - pbn_mi_pvalue's own host arithmetic on those integers - must equal pbn_mi_pvalue of the same test on
a SECOND, fresh handle bit for bit (a fresh one, so that the batch cannot have read a grouping the scalar call left behind).  The test
aid pbn_debug_mi_discrete (layout at its definition in csrc/mi.hip) says where every test ran, with which code width, in how many slices
and LDS copies, and hands back the table as it came off the device.

The scalar side is pbn_mi_pvalue itself, not MutualInformation.pvalue: a one-category x or y has zero degrees of freedom, where the
routine answers NaN and pvalue() raises.  The batch must give that very answer in its slot, NaN equal to NaN."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib

pytestmark = pytest.mark.gpu

DEVICE, CACHED, GROUPED, HYBRID = 1, 2, 0, -1     # `where` of a capture record
LDS_CELLS = 4096                                  # tables up to here take the LDS form, larger ones the global form
MAX_COND = 6
GROUPING_CELLS = 1 << 22                         # the sort path's own limit: larger tables take the LDS-cell kernel, which refuses tables with nulls


def uniform_codes(cards, rows, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, c, rows) for c in cards])


def frame(codes, cards, extra=None):
    """Categorical columns v0, v1, ... from a [columns][rows] code matrix (-1 = null)."""
    data = {f"v{i}": pd.Categorical.from_codes(codes[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(len(cards))}
    data.update(extra or {})
    return pd.DataFrame(data)


class Capture:
    def __init__(self):
        self.fn = _lib.load().pbn_debug_mi_discrete
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


@pytest.fixture(scope="module")
def cap():
    with Capture() as c:
        yield c


@pytest.fixture(scope="module")
def max_cells():
    v = _lib.load().pbn_mi_discrete_batch_max_cells()
    assert v >= LDS_CELLS
    return v


def pack(tests):
    n = len(tests)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t[2]) for t in tests])
    cond = np.array([v for t in tests for v in t[2]] or [0], dtype=np.int32)
    v1 = np.array([t[0] for t in tests], dtype=np.int32)
    v2 = np.array([t[1] for t in tests], dtype=np.int32)
    return n, v1, v2, off, cond


def run_batch(test, tests):
    """pbn_mi_pvalue_batch called directly; tests = [(x, y, [z...])] as variable ids (the identity order)."""
    _lib.check(_lib.load().pbn_mi_set_order(test._handle, 0, None))
    n, v1, v2, off, cond = pack(tests)
    out = np.full(n, -1.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    _lib.load().pbn_mi_pvalue_batch(test._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
    return out


def scalar(test, tests):
    """pbn_mi_pvalue of every test, one call each."""
    lib = _lib.load()
    _lib.check(lib.pbn_mi_set_order(test._handle, 0, None))
    return np.array([lib.pbn_mi_pvalue(test._handle, t[0], t[1], len(t[2]), _lib.int_array(list(t[2]) or [0])) for t in tests])


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def expected_table(codes, cards, test):
    vs = [test[0], test[1]] + list(test[2])
    valid = np.all(codes[vs] >= 0, axis=0)
    key = np.zeros(int(valid.sum()), dtype=np.int64)
    stride = 1
    for v in vs:
        key += codes[v][valid] * stride
        stride *= int(cards[v])
    return np.bincount(key, minlength=stride)


def cells_of(cards, t):
    return int(np.prod([int(cards[v]) for v in [t[0], t[1]] + list(t[2])], dtype=np.int64))


def eligible(cards, t, max_cells):
    """The rule of the issue: at most 6 conditioning variables, no variable named twice, at most max_cells cells (rows > 0 everywhere here)."""
    vs = [t[0], t[1]] + list(t[2])
    return len(t[2]) <= MAX_COND and len(set(vs)) == len(vs) and cells_of(cards, t) <= max_cells


# columns of the bit-identity table
ONE, TWO, THREE, SEVEN, BIG, BIG2 = 0, 1, 2, 3, 4, 5       # cardinalities 1, 2, 3, 7, 256, 256
B = [6, 7, 8, 9, 10, 11]                                   # six binary columns
TRI, CONST = 12, 13                                        # cardinality 3; a binary column that holds one value only
NX, NY, NZ = 14, 15, 16                                    # columns with nulls, cardinalities 3, 2, 4
WIDE = 17                                                  # 257 categories: only in the int32 table
CARDS = [1, 2, 3, 7, 256, 256, 2, 2, 2, 2, 2, 2, 3, 2, 3, 2, 4]


def identity_table(rows, wide):
    cards = CARDS + ([257] if wide else [])
    codes = uniform_codes(cards, rows, 100 + rows)
    rng = np.random.default_rng(rows)
    codes[TWO] = (codes[THREE] + (rng.random(rows) < 0.5) * codes[B[0]]) % 2          # some dependence
    codes[CONST, :] = 1
    for col, rate in ((NX, 0.2), (NY, 0.1), (NZ, 0.3)):
        codes[col, rng.random(rows) < rate] = -1
    if rows >= 7:
        codes[NX, 0] = codes[NY, 1] = codes[NZ, 2] = -1                                # nulls at every size but the one-row table
    return codes, cards


def identity_tests(cards, max_cells, wide):
    """(tests, indices of those expected OFF the kernel - enumerated by hand, checked against the rule)."""
    tests = [(TWO, THREE, B[:k]) for k in range(MAX_COND + 1)]                          # k = 0 ... 6
    off_kernel = [len(tests)]
    tests.append((TWO, THREE, B + [TRI]))                                              # k = 7
    tests += [(THREE, TWO, B[:2]), (TWO, THREE, [B[1], B[0]]), (SEVEN, THREE, [TWO, B[0]]), (B[0], SEVEN, [THREE, TWO]),   # x / y swapped, Z permuted
              (ONE, TWO, []), (TWO, ONE, [THREE]), (THREE, SEVEN, [ONE]),                # a one-category column
              (BIG, TWO, []), (TWO, BIG, []), (BIG, SEVEN, []), (SEVEN, TRI, [BIG]),     # 256 categories, the last 7 * 3 * 256 = 5 376 cells
              (BIG, B[0], B[1:4]),                                                      # 4 096 cells exactly
              (CONST, TWO, []), (TWO, CONST, []), (B[0], CONST, [THREE]), (THREE, TWO, [CONST, B[1]]),   # every row in one x / y / z slice
              (NX, TWO, []), (NX, THREE, [B[0]]), (TWO, NY, []), (B[0], NY, [THREE]),    # nulls in x, in y,
              (TWO, THREE, [NZ]), (THREE, TWO, [NZ, B[0]]), (NX, NY, [NZ]), (NY, NX, [NZ, TWO])]   # in one Z column, in all of them
    off_kernel.append(len(tests))
    tests.append((TWO, THREE, [B[0], TWO]))                                            # a repeated variable
    # G above the cap, while the cap leaves room for such a table on the grouping path: with nulls in the table that path ends at 2^22
    # cells (test_a_table_above_the_cap_stays_on_the_grouping_path has the case on a table without nulls, whatever the cap)
    big = [BIG, BIG2, SEVEN, THREE, TRI, B[0], B[1], B[2]]
    m = 2
    while m < 8 and cells_of(cards, (big[0], big[1], big[2:m])) <= max_cells:
        m += 1
    if cells_of(cards, (big[0], big[1], big[2:m])) <= GROUPING_CELLS:
        off_kernel.append(len(tests))
        tests.append((big[0], big[1], big[2:m]))
    else:
        assert max_cells * 2 > GROUPING_CELLS
    if wide:
        tests += [(WIDE, TWO, []), (THREE, WIDE, [B[0]]), (TWO, THREE, [WIDE])]
    rule = [i for i, t in enumerate(tests) if not eligible(cards, t, max_cells)]
    assert rule == off_kernel, (rule, off_kernel)
    return tests, off_kernel


def check_records(recs, codes, cards, tests, off_kernel, width):
    for i, (t, rec) in enumerate(zip(tests, recs)):
        if i in off_kernel:
            assert rec["where"] == GROUPED and len(rec["table"]) == 0, (t, rec["where"])
            continue
        assert rec["where"] == DEVICE, (t, rec["where"])          # no other test may fall back
        assert rec["width"] == width, (t, rec["width"])
        want = expected_table(codes, cards, t)
        assert rec["G"] == len(want) and np.array_equal(rec["table"], want), t
        assert (rec["R"] >= 1) == (rec["G"] <= LDS_CELLS) and rec["slices"] >= 1, (t, rec["R"], rec["slices"])


@pytest.mark.parametrize("wide", [False, True], ids=["bytes", "int32"])
@pytest.mark.parametrize("rows", [1, 7, 2047, 2048, 2049, 4097, 50000])
def test_batch_is_bit_identical_to_the_scalar_routine(cap, max_cells, rows, wide):
    """Rows around SLICE_ALIGN (2 048) and the 4 096-row slice floor; cardinalities 1, 2, 3, 7, 256; k = 0 ... 6; both layouts of one
    variable set; a constant column; nulls in x, y, one Z column and all of them; both asymptotic_df values; the byte mirror and - with a
    257-category column in the table - the int32 codes."""
    codes, cards = identity_table(rows, wide)
    df = frame(codes, cards)
    tests, off_kernel = identity_tests(cards, max_cells, wide)
    for asymptotic in (True, False):
        bat, ref = pbn.MutualInformation(df, asymptotic_df=asymptotic), pbn.MutualInformation(df, asymptotic_df=asymptotic)
        bat.set_batch_threshold(0)
        out = run_batch(bat, tests)
        calls = cap.take()
        assert len(calls) == 1 and len(calls[0]["tests"]) == len(tests)
        check_records(calls[0]["tests"], codes, cards, tests, off_kernel, 4 if wide else 1)
        assert bat.batch_stats() == (len(tests) - len(off_kernel), 0, len(off_kernel))
        assert calls[0]["groups_after"] - calls[0]["groups_before"] <= len(off_kernel)
        want = scalar(ref, tests)
        bad = [(t, a, b) for t, a, b in zip(tests, out, want) if not same_bits(a, b)]
        assert not bad, bad[:5]
        if rows >= 2047:
            assert np.isfinite(out).sum() > len(tests) // 2 and (out < 0.05).any() and (out > 0.05).any()


def test_tables_at_the_form_boundary_and_the_cap(cap, max_cells):
    """G = 4 096 exactly (the fullest LDS table: one copy), 4 097 = 17 * 241 (the smallest global one) and the cap itself."""
    rows = 5003
    cards = [17, 241, 256, 256, 2, 2, 2, 2, 2, 2]
    codes = uniform_codes(cards, rows, 41)
    codes[4, np.random.default_rng(4).random(rows) < 0.15] = -1
    df = frame(codes, cards)
    tests = [(2, 5, [6, 7, 8]), (5, 2, [8, 7, 6]), (2, 4, [6, 7, 8])]                   # 4 096 cells, the last with nulls
    if max_cells > LDS_CELLS:
        tests += [(0, 1, []), (1, 0, [])]                                               # 4 097 cells
        at_cap = [2, 3] if max_cells >= 65536 else [2]
        g, fill = (65536 if max_cells >= 65536 else 256), [5, 6, 7, 8, 9, 4]
        while g * 2 <= max_cells and fill:
            at_cap.append(fill.pop(0)); g *= 2
        assert g == max_cells, "the cap is not a power of two >= 256 that this table can build"
        tests += [(at_cap[0], at_cap[1], at_cap[2:]), (at_cap[1], at_cap[0], at_cap[:1:-1])]
    bat, ref = pbn.MutualInformation(df), pbn.MutualInformation(df)
    bat.set_batch_threshold(0)
    out = run_batch(bat, tests)
    recs = cap.take()[0]["tests"]
    check_records(recs, codes, cards, tests, [], 1)
    assert [r["G"] for r in recs[:3]] == [LDS_CELLS] * 3 and all(r["R"] == 1 for r in recs[:3])
    if max_cells > LDS_CELLS:
        assert recs[3]["G"] == recs[4]["G"] == 4097 and recs[3]["R"] == 0
        assert recs[-1]["G"] == recs[-2]["G"] == max_cells and recs[-1]["R"] == 0
    assert recs[2]["table"].sum() == (codes[4] >= 0).sum() < rows
    assert same_bits(out, scalar(ref, tests))


def test_a_table_above_the_cap_stays_on_the_grouping_path(cap, max_cells):
    """Few rows, no nulls: above 2^22 cells the grouping path is the LDS-cell kernel in windows, which costs per cell, not per row."""
    rows = 64
    cards = [256, 256, 7, 3, 3, 2, 2, 2]
    codes = uniform_codes(cards, rows, 77)
    vs = [0, 1]
    while cells_of(cards, (vs[0], vs[1], vs[2:])) <= max_cells:
        vs.append(len(vs))
    tests = [(vs[0], vs[1], vs[2:]), (5, 6, [7]), (vs[0], vs[1], vs[2:-1])]
    assert len(vs) <= MAX_COND + 2 and max_cells < cells_of(cards, tests[0]) <= 1 << 24 and cells_of(cards, tests[2]) <= max_cells
    df = frame(codes, cards)
    bat, ref = pbn.MutualInformation(df), pbn.MutualInformation(df)
    bat.set_batch_threshold(0)
    out = run_batch(bat, tests)
    recs = cap.take()[0]["tests"]
    assert [r["where"] for r in recs] == [GROUPED, DEVICE, DEVICE] and bat.batch_stats() == (2, 0, 1)
    assert np.array_equal(recs[2]["table"], expected_table(codes, cards, tests[2]))
    assert same_bits(out, scalar(ref, tests)) and np.isfinite(out[1])


def small_table(rows=4099, seed=9):
    cards = [2, 3, 4, 2, 3, 2]
    codes = uniform_codes(cards, rows, seed)
    codes[1] = (codes[0] + codes[2] * (np.random.default_rng(seed).random(rows) < 0.3)) % 3
    tests = [(0, 1, []), (1, 2, [0]), (3, 4, [5, 0]), (2, 0, [1, 3, 4]), (5, 4, [])]
    return codes, cards, tests


def test_no_grouping_is_built(cap):
    """Fails on the parent commit: there every one of these tests builds a DiscGroup, and none of these entry points exists."""
    codes, cards, tests = small_table()
    df = frame(codes, cards)
    test = pbn.MutualInformation(df)
    out = run_batch(test, tests)                                                        # the default threshold
    call = cap.take()[0]
    assert call["groups_before"] == call["groups_after"] == 0
    assert all(r["where"] == DEVICE for r in call["tests"])
    assert test.batch_stats() == (len(tests), 0, 0)
    assert test.passes() == (len(tests), 0)                                             # pbn_mi_stats: one device pass per test served
    # a scalar mi() leaves the grouping of its variable set behind: the same call then reads that test off it
    again = pbn.MutualInformation(df)
    again.mi("v1", "v2", ["v0"])
    out2 = run_batch(again, tests)
    call = cap.take()[0]
    assert [r["where"] for r in call["tests"]] == [DEVICE, CACHED, DEVICE, DEVICE, DEVICE]
    assert call["groups_before"] == call["groups_after"] == 1
    assert again.batch_stats() == (len(tests) - 1, 1, 0)
    assert same_bits(out, out2) and np.isfinite(out).all()


def hybrid_table(n, seed, nulls=False):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 3, size=n)
    d2 = (d1 + rng.integers(0, 2, size=n) * (rng.random(n) < 0.6)) % 2
    d3 = rng.integers(0, 4, size=n)
    d4 = (d3 + rng.integers(0, 2, size=n)) % 3
    c1 = rng.normal(size=n) + 0.8 * d1
    c2 = 0.7 * c1 + rng.normal(scale=0.6, size=n) - 0.5 * d2
    c3 = rng.normal(size=n) * (1 + 0.3 * d3)
    df = pd.DataFrame({"c1": c1, "c2": c2, "c3": c3})
    if nulls:
        d3 = np.where(rng.random(n) < 0.1, -1, d3)
        df.loc[rng.random(n) < 0.05, "c2"] = np.nan
    for name, codes, k in (("d1", d1, 3), ("d2", d2, 2), ("d3", d3, 4), ("d4", d4, 3)):
        df[name] = pd.Categorical.from_codes(codes, [f"{name}_{i}" for i in range(k)])
    return df


@pytest.mark.parametrize("nulls", [False, True])
def test_mixed_batch_on_a_hybrid_table(cap, nulls):
    """Count-only and hybrid tests in one call: every slot equals the same call on a fresh handle with the switch at 0."""
    df = hybrid_table(6001, 3, nulls)
    c1, c2, c3, d1, d2, d3, d4 = range(7)                                               # variable ids: continuous columns first
    tests = [(d1, d2, []), (d1, c1, []), (d2, d1, [d3]), (c1, c2, []), (d1, d2, [c1]), (d3, d4, [d1, d2]), (c2, d1, [d2]),
             (c1, c3, [d1, c2]), (d4, d1, [d3, c3]), (d2, d4, []), (c3, c1, [d4, d3]), (d1, d2, [d3])]
    count_only = [all(v >= d1 for v in [t[0], t[1]] + list(t[2])) for t in tests]
    on = pbn.MutualInformation(df)
    on.set_batch_threshold(0)
    out = run_batch(on, tests)
    recs = cap.take()[0]["tests"]
    assert [r["where"] for r in recs] == [DEVICE if c else HYBRID for c in count_only]
    assert on.batch_stats() == (sum(count_only), 0, 0)
    os.environ["PBN_MI_DISCRETE_BATCH"] = "0"
    try:
        off = pbn.MutualInformation(df)
        off.set_batch_threshold(0)
        want = run_batch(off, tests)
        recs = cap.take()[0]["tests"]
    finally:
        del os.environ["PBN_MI_DISCRETE_BATCH"]
    assert [r["where"] for r in recs] == [GROUPED if c else HYBRID for c in count_only]
    assert off.batch_stats() == (0, 0, sum(count_only))
    assert np.isfinite(out).all() and np.array_equal(out, want)
    only = [t for t, c in zip(tests, count_only) if c]
    assert same_bits(out[np.array(count_only)], scalar(pbn.MutualInformation(df), only))


def oracle_table():
    """20 000 rows, six dependent categorical columns.  The oracle (oracle/mi_oracle.py) is finite for every case of oracle_cases() on it -
    checked on the CPU when this test was written."""
    rows = 20000
    rng = np.random.default_rng(17)
    cards = [3, 2, 4, 2, 3, 2]
    codes = uniform_codes(cards, rows, 18)
    codes[1] = (codes[0] + (rng.random(rows) < 0.6) * rng.integers(0, 2, rows)) % 2
    codes[4] = (codes[2] + codes[3] * (rng.random(rows) < 0.5)) % 3
    codes[5] = (codes[4] + (rng.random(rows) < 0.2)) % 2
    return codes, cards


def oracle_cases():
    return [(0, 1, []), (1, 0, []), (2, 4, []), (0, 5, []), (0, 1, [2]), (2, 4, [3]), (4, 5, [2]), (3, 4, [2, 0]), (1, 5, [4, 0]),
            (0, 2, [1, 3, 5]), (5, 4, [3, 2, 1]), (3, 0, [4])]


@pytest.mark.parametrize("asymptotic", [True, False])
def test_against_the_oracle(asymptotic):
    from oracle.mi_oracle import MIOracle

    codes, cards = oracle_table()
    name = lambda v: f"v{v}"
    orc = MIOracle({name(i): (codes[i].astype(np.int64), int(cards[i])) for i in range(len(cards))}, asymptotic)
    test = pbn.MutualInformation(frame(codes, cards), asymptotic_df=asymptotic)
    test.set_batch_threshold(0)
    cases = oracle_cases()
    out = run_batch(test, cases)
    assert test.batch_stats() == (len(cases), 0, 0)
    for t, p in zip(cases, out):
        z = tuple(name(v) for v in t[2])
        want = orc.pvalue(name(t[0]), name(t[1]), z)
        assert np.isfinite(want)
        assert p == pytest.approx(want, rel=1e-6, abs=1e-300), t
        want_mi = orc.mi(name(t[0]), name(t[1]), z)
        assert np.isfinite(want_mi)
        assert test.mi(name(t[0]), name(t[1]), list(z)) == pytest.approx(want_mi, rel=1e-9, abs=1e-12), t


def test_threshold_and_switch(cap):
    codes, cards, tests = small_table(5000, 10)
    df = frame(codes, cards)
    dev = pbn.MutualInformation(df)
    dev.set_batch_threshold(len(tests))                                                 # the call size itself: still the kernel
    want = run_batch(dev, tests)
    assert dev.batch_stats() == (len(tests), 0, 0) and cap.take()[0]["groups_after"] == 0

    high = pbn.MutualInformation(df)
    high.set_batch_threshold(len(tests) + 1)
    got = run_batch(high, tests)
    call = cap.take()[0]
    assert high.batch_stats() == (0, 0, len(tests)) and all(r["where"] == GROUPED for r in call["tests"])
    assert call["groups_after"] == len(tests) and np.array_equal(got, want)

    os.environ["PBN_MI_DISCRETE_BATCH"] = "0"
    try:
        off = pbn.MutualInformation(df)
        off.set_batch_threshold(0)
        got = run_batch(off, tests)
        assert off.batch_stats()[0] == 0 and np.array_equal(got, want)
    finally:
        del os.environ["PBN_MI_DISCRETE_BATCH"]
    cap.take()
    got = run_batch(off, tests)                                                         # read per call: back on, and everything cached
    assert [r["where"] for r in cap.take()[0]["tests"]] == [CACHED] * len(tests)
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        dev.set_batch_threshold(-1)
    # the default: a call of ONE eligible test keeps it on the grouping path, two go to the kernel
    default = pbn.MutualInformation(df)
    assert run_batch(default, tests[:1])[0] == want[0] and default.batch_stats() == (0, 0, 1)
    assert np.array_equal(run_batch(default, tests[1:3]), want[1:3]) and default.batch_stats() == (2, 0, 1)
