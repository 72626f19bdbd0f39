"""GPU tier: ChiSquare's batch and the family tables of a pbn_dtable count with one kernel (csrc/joint_counts.hip).

The same joint table is asked for twice - as the ChiSquare test (x, y, Z) through pbn_chisq_pvalue_batch with the capture on, and as the
family (x; y, Z) through pbn_dtable_family_counts, which lays out the variable fastest and the parents as given - and the two integer
tables must be equal to each other and to np.bincount over the rows valid in the table's columns.  A null is -1 in the dtable and the
null bucket (code == cardinality) in the pbn_mi handle: two encodings, one validity rule in the kernel."""
import numpy as np
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib
from test_chisq_batch_gpu import Capture, expected_table, frame, run_batch, uniform_codes
from test_discrete_model_shapes_gpu import LDS_I32, LDS_U8, Table

pytestmark = pytest.mark.gpu

CARDS = [3, 2, 4, 2]            # every cardinality <= 4: byte mirrors on both sides
WIDE = 300                      # one such column more: int32 codes on both sides
NULL_COLUMNS = {"none": [], "x": [0], "z": [2], "all": [0, 1, 2, 3, 4]}


@pytest.fixture(scope="module")
def cap():
    with Capture() as c:
        yield c


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("nulls", list(NULL_COLUMNS))
@pytest.mark.parametrize("rows", [257, 4097, 12289])
def test_both_callers_count_the_same_table(cap, rows, nulls, wide):
    cards = CARDS + ([WIDE] if wide else [])
    codes = uniform_codes(cards, rows, rows + len(cards))
    rng = np.random.default_rng(rows)
    for c in NULL_COLUMNS[nulls]:
        if c < len(cards):
            codes[c, rng.random(rows) < 0.15] = -1
            codes[c, [0, rows - 1]] = -1                       # the first and the last row of the table as well
    # y and Z in ascending column order: the family's table then has the ChiSquare test's layout
    tests = [(0, 1, []), (0, 1, [2, 3]), (1, 2, [3])] + ([(0, 1, [4]), (4, 3, [])] if wide else [])
    want = [expected_table(codes, cards, t) for t in tests]

    chi = pbn.ChiSquare(frame(codes, cards))
    chi.set_batch_threshold(0)
    _lib.check(_lib.load().pbn_mi_set_order(chi._handle, 0, None))
    run_batch(chi, tests)
    calls = cap.take()
    assert len(calls) == 1
    recs = calls[0]["tests"]
    assert [r["where"] for r in recs] == [1] * len(tests)
    assert {r["width"] for r in recs} == {4 if wide else 1}

    table = Table(_lib.load(), [np.ascontiguousarray(c, dtype=np.int32) for c in codes], cards)
    try:
        fams = table.counted([(t[0], [t[1]] + list(t[2])) for t in tests])
    finally:
        table.close()
    for t, rec, (fam, form), w in zip(tests, recs, fams, want):
        assert form == (LDS_I32 if wide else LDS_U8), (t, form)
        assert w.sum() == np.all(codes[[t[0], t[1]] + list(t[2])] >= 0, axis=0).sum()
        assert np.array_equal(rec["table"], w), t
        assert np.array_equal(fam, w), t
        assert np.array_equal(rec["table"], fam), t
