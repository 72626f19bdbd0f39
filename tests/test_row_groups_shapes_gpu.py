"""GPU tier: the device partition of a code table's rows by configuration (csrc/row_groups.hip: pbn_dtable_group_rows,
pbn_rowgroups_offsets, pbn_rowgroups_rows, pbn_table_take_group) alone, through ctypes, compared EXACTLY.

Comparator: numpy.  The keys are adaptator_group.keys - the restatement tests/test_adaptator_group_cpu.py holds against
_DiscreteAdaptator._config (factors/discrete/DiscreteAdaptator.hpp:201-260, factors/discrete/discrete_indices.cpp:93-204) - the rows are
the grouped rows in np.argsort(key, kind="stable") order and the offsets the cumulative bincount (adaptator_group.grouping).  `offsets`
and `rows` must be equal as integers: the partition is stable, so there is one right answer.

Launch shapes.  A workgroup of 256 threads steps through its chunk in tiles of TILE = 256 rows; the grid is min(256, ceil(n / TILE))
workgroups at the most, each chunk a multiple of the tile.  So the row counts are: 0, 1, 63 / 64 / 65 (a wave), 255 / 256 / 257 (one row
less than, equal to and one more than the tile; 257 is the first with two workgroups), 100 (fewer rows than the grid's cap of 256
workgroups - the grid is never larger than the tiles, so this is one partly filled workgroup), 65 537 = 256 x 256 + 1 (one more than
workgroups x tile: 129 chunks of 512 rows, the last holding ONE row - uneven chunks) and 131 073 (171 workgroups of 768 rows, the last
of 513: EVERY workgroup walks three tiles, so the running counters carry from tile to tile everywhere)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE, MAX_BLOCKS, CAP = 256, 256, 8192
ROWS = [0, 1, 63, 64, 65, 100, TILE - 1, TILE, TILE + 1, MAX_BLOCKS * TILE + 1, 131073]
# the key columns' cardinalities, first fastest: G = 1, 2, 3, 63, 64, 65 and the cap, from one to seven columns of unequal cardinalities
SPECS = {"G1_m1": (1,), "G2_m1": (2,), "G3_m2": (3, 1), "G63_m3": (7, 3, 3), "G64_m4": (2, 4, 2, 4), "G65_m2": (5, 13), "G72_m5": (3, 2, 2, 3, 2),
         "G96_m6": (2, 3, 2, 2, 2, 2), "Gcap_m7": (2, 4, 2, 8, 4, 4, 4), "Gcap_m1": (CAP,)}


@pytest.fixture(scope="module")
def env():
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib, adaptator_group

    pbn.load_library()
    assert adaptator_group.MAX_CONFIGS == CAP
    return adaptator_group, _lib, _lib.load(), pbn.Context(0)


class Codes:
    """A pbn_dtable whose key columns lie, reversed, between decoy columns: cols = the key columns' places in the table."""

    def __init__(self, env, key_codes, cards):
        _, _lib, lib, ctx = env
        self.lib = lib
        rows = len(key_codes[0])
        m = len(cards)
        decoy = np.zeros(rows, dtype=np.int32)
        self.arrays = [decoy] + [np.ascontiguousarray(a, dtype=np.int32) for a in reversed(key_codes)] + [decoy]
        self.cards = [1] + list(reversed(cards)) + [1]
        self.cols = [m - j for j in range(m)]
        ptrs = (C.c_void_p * len(self.arrays))(*[a.ctypes.data for a in self.arrays])
        self.handle = C.c_void_p()
        _lib.check(lib.pbn_dtable_create(ctx.handle, rows, len(self.arrays), ptrs, _lib.int_array(self.cards), C.byref(self.handle)))

    def close(self):
        self.lib.pbn_dtable_destroy(self.handle)


def group(env, dt, cols, bitmap=None):
    """(return code, handle) of pbn_dtable_group_rows"""
    _, _lib, lib, _ = env
    h = C.c_void_p()
    rc = lib.pbn_dtable_group_rows(dt.handle, len(cols), _lib.int_array(list(cols) or [0]), None if bitmap is None else bitmap.ctypes.data, C.byref(h))
    return rc, h


def read_groups(env, h):
    _, _lib, lib, _ = env
    n = C.c_int64(-1)
    _lib.check(lib.pbn_rowgroups_offsets(h, C.byref(n), None))
    offsets = np.full(n.value + 1, -7, dtype=np.int64)
    _lib.check(lib.pbn_rowgroups_offsets(h, C.byref(n), offsets.ctypes.data_as(C.POINTER(C.c_int64))))
    rows = np.full(int(offsets[-1]), -7, dtype=np.int32)
    _lib.check(lib.pbn_rowgroups_rows(h, rows.ctypes.data if rows.size else None))
    return offsets, rows


def check_partition(env, key_codes, cards, valid=None):
    """Group on the device, compare with numpy, group again and compare the bytes.  Returns (offsets, rows)."""
    ag, _lib, lib, _ = env
    key, grouped = ag.keys(key_codes, cards, valid)
    cells = int(np.prod(cards))
    want_offsets, want_rows = ag.grouping(key, grouped, cells)
    bitmap = None if valid is None else np.packbits(valid, bitorder="little")
    dt = Codes(env, key_codes, cards)
    try:
        rc, h = group(env, dt, dt.cols, bitmap)
        _lib.check(rc)
        try:
            offsets, rows = read_groups(env, h)
        finally:
            lib.pbn_rowgroups_destroy(h)
        assert offsets.shape == (cells + 1,) and np.array_equal(offsets, want_offsets)
        assert np.array_equal(rows, want_rows)
        rc, h = group(env, dt, dt.cols, bitmap)
        _lib.check(rc)
        try:
            again = read_groups(env, h)
        finally:
            lib.pbn_rowgroups_destroy(h)
        assert again[0].tobytes() == offsets.tobytes() and again[1].tobytes() == rows.tobytes()
    finally:
        dt.close()
    return offsets, rows


def codes_of(key, cards):
    """The key columns' codes of the configurations `key`: its mixed-radix digits, the first column fastest."""
    out, rest = [], np.asarray(key, dtype=np.int64)
    for card in cards:
        out.append((rest % card).astype(np.int32))
        rest = rest // card
    assert (rest == 0).all()
    return out


@pytest.mark.parametrize("spec", list(SPECS))
@pytest.mark.parametrize("rows", ROWS)
def test_every_launch_shape(env, rows, spec):
    """Random configurations; a -1 here and there in the first key column, and for every second shape a validity bitmap."""
    cards = SPECS[spec]
    rng = np.random.default_rng(rows * 31 + len(cards) * 7 + int(np.prod(cards)))
    key_codes = [rng.integers(0, c, size=rows).astype(np.int32) for c in cards]
    key_codes[0][rng.random(rows) < 0.05] = -1
    valid = (rng.random(rows) < 0.9) if (rows + len(cards)) % 2 else None
    offsets, _ = check_partition(env, key_codes, cards, valid)
    assert offsets[-1] <= rows


PATTERN_ROWS = 1003   # four workgroups, the last partly filled; no multiple of 8


def pattern(name):
    """(key codes, cardinalities, validity or None) of a named pattern"""
    n = PATTERN_ROWS
    rng = np.random.default_rng(5)
    cards = (5, 13)
    G = 65
    valid = None
    if name == "all_in_the_first":
        key = np.zeros(n, dtype=np.int64)
    elif name == "all_in_the_last":
        key = np.full(n, G - 1, dtype=np.int64)
    elif name == "distinct_descending":
        cards, n = (2, 4, 2, 8, 4, 4, 4), CAP
        key = np.arange(CAP - 1, -1, -1, dtype=np.int64)
    elif name == "two_alternating":
        key = np.where(np.arange(n) % 2 == 0, 40, 7).astype(np.int64)
    elif name == "only_in_the_last_row":
        key = rng.integers(0, G - 1, size=n).astype(np.int64)
        key[-1] = G - 1
    elif name == "empty_at_start_middle_end":
        key = rng.choice([2, 3, 30, 31, 62], size=n).astype(np.int64)
    elif name in ("null_first_and_last_row", "null_every_row", "bitmap_across_bytes", "bitmap_and_nulls"):
        key = rng.integers(0, G, size=n).astype(np.int64)
    else:
        raise KeyError(name)
    codes = codes_of(key, cards)
    if name == "null_first_and_last_row":
        codes[0][0] = -1
        codes[1][-1] = -1
    if name == "null_every_row":
        codes[1][:] = -1
    if name in ("bitmap_across_bytes", "bitmap_and_nulls"):
        valid = np.ones(n, dtype=bool)
        valid[5:19] = False          # bytes 0, 1 and 2
        valid[255:258] = False       # the last row of a tile and the first of the next workgroup
        valid[999:1002] = False      # in the last, partial byte; row 1002 stays
        valid[rng.random(n) < 0.2] = False
    if name == "bitmap_and_nulls":
        codes[0][rng.random(n) < 0.2] = -1
        codes[1][6] = -1             # excluded twice
    return codes, cards, valid


@pytest.mark.parametrize("name", ["all_in_the_first", "all_in_the_last", "distinct_descending", "two_alternating", "only_in_the_last_row",
                                  "empty_at_start_middle_end", "null_first_and_last_row", "null_every_row", "bitmap_across_bytes", "bitmap_and_nulls"])
def test_key_patterns(env, name):
    codes, cards, valid = pattern(name)
    offsets, rows = check_partition(env, codes, cards, valid)
    n = len(codes[0])
    if name == "null_every_row":
        assert offsets[-1] == 0 and not offsets.any()
    if name == "distinct_descending":
        assert np.array_equal(rows, np.arange(n - 1, -1, -1)) and np.array_equal(offsets, np.arange(n + 1))
    if name == "only_in_the_last_row":
        assert offsets[-1] - offsets[-2] == 1 and rows[-1] == n - 1
    if name == "all_in_the_last":
        assert np.array_equal(rows, np.arange(n)) and offsets[-2] == 0
    if name == "null_first_and_last_row":
        assert offsets[-1] == n - 2 and 0 not in rows and n - 1 not in rows


def test_refusals(env):
    """PBN_ERR_INVALID, and no handle: the arguments are checked before anything is launched."""
    _, _lib, lib, _ = env
    rows = 300
    cards = [3, 2, 64, 64, 2, 2, 2, 2, 2]
    arrays = [np.zeros(rows, dtype=np.int32) for _ in cards]
    ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
    dt = C.c_void_p()
    ctx = env[3]
    _lib.check(lib.pbn_dtable_create(ctx.handle, rows, len(arrays), ptrs, _lib.int_array(cards), C.byref(dt)))

    class Holder:
        handle = dt

    try:
        for cols in ([], list(range(8)), [0, 1, 0], [0, 9], [-1]):     # m = 0, m = 8, a column twice, out of range at either end
            rc, h = group(env, Holder, cols)
            assert rc == _lib.PBN_ERR_INVALID, cols
            assert not h.value
        rc, h = group(env, Holder, [2, 3, 0])     # 64 x 64 x 3 = 12 288: above the cap
        assert rc == _lib.PBN_ERR_INVALID and not h.value
        rc, h = group(env, Holder, [2, 3, 1])     # 64 x 64 x 2: the cap itself
        _lib.check(rc)
        offsets, got = read_groups(env, h)
        lib.pbn_rowgroups_destroy(h)
        assert offsets.shape == (CAP + 1,) and offsets[0] == 0 and (offsets[1:] == rows).all() and np.array_equal(got, np.arange(rows))
        assert lib.pbn_dtable_group_rows(None, 1, _lib.int_array([0]), None, C.byref(h)) == _lib.PBN_ERR_INVALID
        assert lib.pbn_dtable_group_rows(dt, 1, None, None, C.byref(h)) == _lib.PBN_ERR_INVALID
        assert lib.pbn_dtable_group_rows(dt, 1, _lib.int_array([0]), None, None) == _lib.PBN_ERR_INVALID
    finally:
        lib.pbn_dtable_destroy(dt)


# ---- the gather --------------------------------------------------------------------------------------------------------------------------

def read_table(env, h, n_cols, dtype):
    _, _lib, lib, _ = env
    rows = lib.pbn_table_rows(h)
    assert lib.pbn_table_cols(h) == n_cols
    out = np.full((n_cols, rows), 77, dtype=dtype)
    if rows:
        _lib.check(lib.pbn_table_read(h, _lib.int_array(range(n_cols)), n_cols, out.ctypes.data))
    return out


@pytest.mark.parametrize("borrowed", [False, True], ids=["owned", "borrowed_ld_1031"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_gather_equals_the_numpy_gather(env, dtype, borrowed):
    """Every configuration's table - a column subset in permuted order - read back and compared with the numpy gather; the source an
    uploaded table, or a borrowed allocation whose leading dimension is no multiple of 64.  Configurations 0, 4 and 9 are empty."""
    import torch

    ag, _lib, lib, ctx = env
    rows, n_cols, take = 1003, 5, [3, 0, 4]
    rng = np.random.default_rng(11)
    cards = (2, 5)
    key = rng.choice([1, 2, 3, 5, 6, 7, 8], size=rows).astype(np.int64)
    codes = codes_of(key, cards)
    codes[0][rng.random(rows) < 0.1] = -1
    valid = rng.random(rows) < 0.9
    data = rng.normal(size=(n_cols, rows)).astype(dtype)
    code = _lib.PBN_F64 if dtype == "float64" else _lib.PBN_F32
    src, dev = C.c_void_p(), None
    if borrowed:
        ld = 1031
        host = np.zeros((n_cols, ld), dtype=dtype)
        host[:, :rows] = data
        dev = torch.from_numpy(host).to(torch.device("cuda", 0))
        torch.cuda.synchronize()
        _lib.check(lib.pbn_table_from_device(ctx.handle, C.c_void_p(dev.data_ptr()), ld, n_cols, rows, code, C.byref(src)))
    else:
        cols = [np.ascontiguousarray(data[c]) for c in range(n_cols)]
        ptrs = (C.c_void_p * n_cols)(*[c.ctypes.data for c in cols])
        _lib.check(lib.pbn_table_create(ctx.handle, ptrs, n_cols, rows, code, None, 0, C.byref(src)))
    k, grouped = ag.keys(codes, cards, valid)
    offsets, order = ag.grouping(k, grouped, 10)
    dt = Codes(env, codes, cards)
    try:
        rc, h = group(env, dt, dt.cols, np.packbits(valid, bitorder="little"))
        _lib.check(rc)
        try:
            got_offsets, got_rows = read_groups(env, h)
            assert np.array_equal(got_offsets, offsets) and np.array_equal(got_rows, order)
            for c in range(10):
                piece = C.c_void_p()
                _lib.check(lib.pbn_table_take_group(src, _lib.int_array(take), len(take), h, c, C.byref(piece)))
                try:
                    sel = order[offsets[c]: offsets[c + 1]]
                    assert lib.pbn_table_rows(piece) == sel.size
                    if c in (0, 4, 9):
                        assert sel.size == 0
                    got = read_table(env, piece, len(take), dtype)
                    assert got.dtype == data.dtype and np.array_equal(got, data[take][:, sel])
                finally:
                    lib.pbn_table_destroy(piece)
            # refusals: a configuration or a column that is not there, a table of other rows
            piece = C.c_void_p()
            for cols_, c in (([0], 10), ([0], -1), ([5], 1), ([-1], 1), ([], 1)):
                assert lib.pbn_table_take_group(src, _lib.int_array(cols_ or [0]), len(cols_), h, c, C.byref(piece)) == _lib.PBN_ERR_INVALID
                assert not piece.value
            short = C.c_void_p()
            one = np.zeros(8, dtype=dtype)
            _lib.check(lib.pbn_table_create(ctx.handle, (C.c_void_p * 1)(one.ctypes.data), 1, 8, code, None, 0, C.byref(short)))
            assert lib.pbn_table_take_group(short, _lib.int_array([0]), 1, h, 1, C.byref(piece)) == _lib.PBN_ERR_INVALID
            lib.pbn_table_destroy(short)
        finally:
            lib.pbn_rowgroups_destroy(h)
    finally:
        dt.close()
        lib.pbn_table_destroy(src)
    del dev


def test_a_table_without_rows(env):
    _, _lib, lib, ctx = env
    offsets, rows = check_partition(env, [np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)], (3, 2))
    assert offsets.shape == (7,) and not offsets.any() and rows.size == 0
