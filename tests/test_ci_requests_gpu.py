"""GPU tier: how the entry points over a pbn_mi handle read a request - the index order set by pbn_mi_set_order, and what they refuse.

Six entry points map external indices through the handle's order: pbn_mi_pvalue, pbn_mi_pvalue_batch, pbn_mi_lincor_pvalue,
pbn_chisq_pvalue, pbn_chisq_pvalue_batch and pbn_mi_counts.  Under a non-identity order each must answer exactly (==, NaN equal to NaN)
what it answers under the identity order for the mapped variable ids; the batch forms must answer what their scalar forms answer, and the
counts must be np.bincount of the codes.  Their refusals differ from one entry point to the next, and callers rely on the differences:

 * an index outside a set order: pbn_mi_pvalue answers NaN and leaves pbn_last_error alone; pbn_mi_pvalue_batch fails the whole call;
   pbn_chisq_pvalue_batch refuses that slot only; the others answer NaN (pbn_mi_counts: a status) with their own message;
 * no order set and an index that is no variable id: pbn_mi_pvalue and its batch say "variable index out of range"; the routines that
   want one kind of variable see no variable of that kind and say so ("is not continuous" / "is not categorical");
 * a variable of the wrong kind: the same "is not ..." messages.

The table is small (257 rows: no multiple of a wave, so the tail of every kernel runs) - this file is about requests, not about sizes."""
import ctypes as C
import itertools

import numpy as np
import pandas as pd
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib

pytestmark = pytest.mark.gpu

ROWS = 257
CARDS = (2, 3, 2)
FLOATS, CATS = ["c0", "c1", "c2"], ["d0", "d1", "d2"]
# variable ids of the mixed handle: the float columns 0 1 2, then the categorical ones 3 4 5
PERM6 = [4, 2, 5, 0, 3, 1]      # external index i stands for variable PERM6[i]
PERM3 = [2, 0, 1]
SHORT = [4, 0, 5, 3]            # an order over four of the six variables: ids 1 and 2 are valid ids and valid nowhere in it


def same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def requests(eligible):
    """every (x, y | z), x != y, |z| in {0, 1, 2}, over the given indices"""
    out = []
    for x, y in itertools.permutations(eligible, 2):
        rest = [v for v in eligible if v not in (x, y)]
        for k in range(3):
            out.extend((x, y, list(z)) for z in itertools.combinations(rest, k))
    return out


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(20261)
    codes = np.stack([rng.integers(0, c, ROWS) for c in CARDS])
    codes[1] = (codes[1] + codes[0] * (rng.random(ROWS) < 0.5)) % CARDS[1]
    z = rng.normal(size=(ROWS, 3))
    z[:, 1] += 0.6 * z[:, 0] + 0.5 * codes[0]
    z[:, 2] += 0.4 * z[:, 1] - 0.3 * codes[1]
    data = {n: z[:, i] for i, n in enumerate(FLOATS)}
    data.update({n: pd.Categorical.from_codes(codes[i], [f"l{j}" for j in range(CARDS[i])]) for i, n in enumerate(CATS)})
    df = pd.DataFrame(data)
    w = {"codes": codes, "mi": pbn.MutualInformation(df), "chi": pbn.ChiSquare(df), "lin": pbn.MutualInformation(df[FLOATS])}
    yield w
    for k in ("mi", "chi", "lin"):
        _lib.check(_lib.load().pbn_mi_set_order(w[k]._handle, 0, None))


def set_order(t, ids):
    _lib.check(_lib.load().pbn_mi_set_order(t._handle, len(ids), _lib.int_array(ids) if ids else None))


def scalar(fn_name, t, x, y, z):
    return getattr(_lib.load(), fn_name)(t._handle, x, y, len(z), _lib.int_array(list(z) or [0]))


def batch(fn_name, t, tests):
    n = len(tests)
    off = np.zeros(n + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(q[2]) for q in tests])
    cond = np.array([v for q in tests for v in q[2]] or [0], dtype=np.int32)
    v1 = np.array([q[0] for q in tests], dtype=np.int32)
    v2 = np.array([q[1] for q in tests], dtype=np.int32)
    out = np.full(n, -1.0)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    getattr(_lib.load(), fn_name)(t._handle, n, ip(v1), ip(v2), ip(off), ip(cond), _lib.dptr(out))
    return out


def counts(t, vs, cells):
    out = np.full(cells, -1.0)
    rc = _lib.load().pbn_mi_counts(t._handle, len(vs), _lib.int_array(vs), _lib.dptr(out))
    return rc, out


def last_error():
    return _lib.load().pbn_last_error()


def poison():
    """leave a known message in pbn_last_error, so that a call that must not touch it can be seen not to"""
    h = C.c_void_p()
    assert _lib.load().pbn_lincor_from_cov(1, 10, None, C.byref(h)) != _lib.PBN_OK
    assert last_error() == b"pbn_lincor_from_cov: bad argument"


def mapped(q, perm):
    return perm[q[0]], perm[q[1]], [perm[v] for v in q[2]]


# ---- order equivalence -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn_name, key, perm, eligible", [
    ("pbn_mi_pvalue", "mi", PERM6, range(6)),
    ("pbn_mi_lincor_pvalue", "lin", PERM3, range(3)),
    ("pbn_chisq_pvalue", "chi", PERM3, range(3)),
    ("pbn_chisq_pvalue", "mi", PERM6, [0, 2, 4]),      # the external indices of the categorical variables of the mixed handle
])
def test_scalar_under_an_order_equals_identity_on_the_mapped_ids(world, fn_name, key, perm, eligible):
    t, reqs = world[key], requests(list(eligible))
    set_order(t, [])
    want = [scalar(fn_name, t, *mapped(q, perm)) for q in reqs]
    set_order(t, perm)
    got = [scalar(fn_name, t, *q) for q in reqs]
    set_order(t, [])
    again = [scalar(fn_name, t, *mapped(q, perm)) for q in reqs]     # pbn_mi_set_order(h, 0, NULL) restores the identity
    assert sum(np.isfinite(want)) > len(want) // 2
    for q, g, w, a in zip(reqs, got, want, again):
        assert same(g, w) and same(a, w), (fn_name, q, g, w, a)


@pytest.mark.parametrize("batch_name, fn_name, key, perm, eligible", [
    ("pbn_mi_pvalue_batch", "pbn_mi_pvalue", "mi", PERM6, range(6)),
    ("pbn_chisq_pvalue_batch", "pbn_chisq_pvalue", "chi", PERM3, range(3)),
    ("pbn_chisq_pvalue_batch", "pbn_chisq_pvalue", "mi", PERM6, [0, 2, 4]),
])
def test_batch_under_an_order_equals_the_scalar_form(world, batch_name, fn_name, key, perm, eligible):
    t, reqs = world[key], requests(list(eligible))
    set_order(t, perm)
    got = batch(batch_name, t, reqs)
    want = [scalar(fn_name, t, *q) for q in reqs]
    set_order(t, [])
    ident = batch(batch_name, t, [mapped(q, perm) for q in reqs])
    assert sum(np.isfinite(want)) > len(want) // 2
    for q, g, w, i in zip(reqs, got, want, ident):
        assert same(g, w) and same(i, w), (batch_name, q, g, w, i)


@pytest.mark.parametrize("key, perm, eligible", [("chi", PERM3, range(3)), ("mi", PERM6, [0, 2, 4])])
def test_counts_under_an_order_are_bincount_of_the_codes(world, key, perm, eligible):
    t, codes = world[key], world["codes"]
    first = 3 if key == "mi" else 0                     # id of d0 on this handle
    for order in (perm, []):
        set_order(t, order)
        for k in (1, 2, 3):
            for vs in itertools.permutations(list(eligible), k):
                ids = [perm[v] for v in vs]
                ask = list(vs) if order else ids
                key_, stride = np.zeros(ROWS, dtype=np.int64), 1
                for v in ids:
                    key_ += codes[v - first] * stride
                    stride *= CARDS[v - first]
                rc, got = counts(t, ask, stride)
                assert rc == _lib.PBN_OK and np.array_equal(got, np.bincount(key_, minlength=stride)), (key, order, vs)
    set_order(t, [])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

OUTSIDE = [4, 5, -1]     # under SHORT: past the order (though 4 and 5 are variable ids), and negative


def test_index_outside_a_set_order(world):
    mi, chi, lin = world["mi"], world["chi"], world["lin"]
    set_order(mi, SHORT)
    good = [(0, 2, []), (0, 2, [3]), (2, 3, [0])]                      # categorical variables 4, 5, 3: fit both MI and ChiSquare
    mi_good = [scalar("pbn_mi_pvalue", mi, *q) for q in good]
    chi_good = [scalar("pbn_chisq_pvalue", mi, *q) for q in good]
    assert np.all(np.isfinite(mi_good)) and np.all(np.isfinite(chi_good))
    for bad in OUTSIDE:
        for q in ((bad, 0, []), (0, bad, []), (0, 2, [bad]), (0, 2, [3, bad])):
            # pbn_mi_pvalue: NaN, and pbn_last_error is byte for byte what it was
            poison()
            before = last_error()
            assert np.isnan(scalar("pbn_mi_pvalue", mi, *q))
            assert last_error() == before
            # pbn_mi_pvalue_batch: the call fails as a whole
            poison()
            out = batch("pbn_mi_pvalue_batch", mi, good[:2] + [q] + good[2:])
            assert np.all(np.isnan(out)), (q, out)
            assert last_error() == b"MutualInformation: variable index out of range"
            # pbn_chisq_pvalue: NaN and its message
            poison()
            assert np.isnan(scalar("pbn_chisq_pvalue", mi, *q))
            assert last_error() == b"ChiSquare: variable index out of range"
            # pbn_chisq_pvalue_batch: that slot only
            out = batch("pbn_chisq_pvalue_batch", mi, good[:2] + [q] + good[2:])
            assert np.isnan(out[2]) and [out[0], out[1], out[3]] == chi_good, (q, out)
        for vs in ([bad], [0, bad], [bad, 2, 0]):
            poison()
            rc, _ = counts(mi, vs, 64)
            assert rc != _lib.PBN_OK and last_error() == b"pbn_mi_counts: variable index out of range"
    set_order(mi, [])
    set_order(chi, PERM3)
    for q in ((3, 0, []), (0, -1, []), (0, 1, [3])):
        poison()
        assert np.isnan(scalar("pbn_chisq_pvalue", chi, *q))
        assert last_error() == b"ChiSquare: variable index out of range"
    set_order(chi, [])
    set_order(lin, [2, 0])                                              # variable 1 is in the table and not in the order
    assert np.isfinite(scalar("pbn_mi_lincor_pvalue", lin, 0, 1, []))
    for q in ((2, 0, []), (0, 2, []), (-1, 0, []), (0, 1, [2]), (0, 1, [-1])):
        poison()
        assert np.isnan(scalar("pbn_mi_lincor_pvalue", lin, *q))
        assert last_error() == b"LinearCorrelation: variable index out of range"
    set_order(lin, [])


def test_no_order_and_an_index_that_is_no_variable(world):
    mi, lin = world["mi"], world["lin"]
    set_order(mi, [])
    set_order(lin, [])
    good = [(3, 4, []), (3, 5, [4])]
    chi_good = [scalar("pbn_chisq_pvalue", mi, *q) for q in good]
    assert np.all(np.isfinite(chi_good))
    for bad in (6, 1000, -1):
        for q in ((bad, 3, []), (3, bad, []), (3, 4, [bad]), (3, 4, [5, bad])):
            poison()
            assert np.isnan(scalar("pbn_mi_pvalue", mi, *q))
            assert last_error() == b"MutualInformation: variable index out of range"
            poison()
            out = batch("pbn_mi_pvalue_batch", mi, [good[0], q, good[1]])
            assert np.all(np.isnan(out))
            assert last_error() == b"MutualInformation: variable index out of range"
            poison()
            assert np.isnan(scalar("pbn_chisq_pvalue", mi, *q))
            assert last_error() == b"ChiSquare: variable is not categorical"
            out = batch("pbn_chisq_pvalue_batch", mi, [good[0], q, good[1]])
            assert np.isnan(out[1]) and [out[0], out[2]] == chi_good, (q, out)
        poison()
        rc, _ = counts(mi, [3, bad], 64)
        assert rc != _lib.PBN_OK and last_error() == b"pbn_mi_counts: variable is not categorical"
    for bad in (3, 1000, -1):
        for q in ((bad, 0, []), (0, bad, []), (0, 1, [bad])):
            poison()
            assert np.isnan(scalar("pbn_mi_lincor_pvalue", lin, *q))
            assert last_error() == b"LinearCorrelation: variable is not continuous"


def test_a_variable_of_the_wrong_kind(world):
    mi = world["mi"]
    good = [(0, 2, []), (2, 4, [0])]                                    # under PERM6: categorical 4, 5 / 5, 3 | 4
    for order, cat, cont, cont2 in ((PERM6, 0, 1, 3), ([], 3, 2, 0)):  # a categorical index and two continuous ones of that index space
        set_order(mi, order)
        tests = good if order else [mapped(q, PERM6) for q in good]
        chi_good = [scalar("pbn_chisq_pvalue", mi, *q) for q in tests]
        assert np.all(np.isfinite(chi_good))
        other = tests[0][1]
        for q in ((cat, cont, []), (cont, cat, []), (cat, other, [cont])):
            poison()
            assert np.isnan(scalar("pbn_chisq_pvalue", mi, *q))
            assert last_error() == b"ChiSquare: variable is not categorical"
            out = batch("pbn_chisq_pvalue_batch", mi, [tests[0], q, tests[1]])
            assert np.isnan(out[1]) and [out[0], out[2]] == chi_good, (q, out)
        for q in ((cont, cat, []), (cat, cont, []), (cont, cont2, [cat])):
            poison()
            assert np.isnan(scalar("pbn_mi_lincor_pvalue", mi, *q))
            assert last_error() == b"LinearCorrelation: variable is not continuous"
        for vs in ([cont], [cat, cont]):
            poison()
            rc, _ = counts(mi, vs, 64)
            assert rc != _lib.PBN_OK and last_error() == b"pbn_mi_counts: variable is not categorical"
    set_order(mi, [])
