"""GPU tier: pbn_clg_fit (csrc/clg_fit.hip) - the per-cell moments and fits of conditional linear Gaussian nodes in one device pass -
through the C ABI at every launch shape.

The tables are lg_exact.make_table(..., shift=8) with at most 4 097 rows (the launch shapes go to 2 R + 1 = 2 049, R = the kernel's
1 024 rows per tile; the node at the cap of 256 configurations takes 4 097 so that its cells hold 16 rows): every value is an integer
times 2^-8 with |integer| < 2^15 (in fact below 2^13).  The pilot shift of a column is a value of that column (its first row), so every
shifted value is an integer below 2^16 in grid units, every product below 2^32 and every moment of at most 4 097 rows below 2^45 <
2^53: exact in fp64 in ANY order of additions.  rows / shift / moments are therefore compared with tolerance ZERO against integers
computed here - a wrong key or stride, a null row counted, a row of the tail dropped or read twice, a column of another node's
family, a cell's partial landing in a neighbour's record: all miss by whole units.  The precondition is asserted per table.

The fitted parameters are compared with entry points that were there before - pbn_table_take of the cell's rows, then
pbn_lg_fit_table - within 1e-10 (max|beta - ref| / max|ref|, relative variance): the project's tolerance for a slice fit against a
factor fitted alone on well-conditioned data.  EVERY status-1 cell of at least 2 D rows is held to it, at every D, for the nodes of 1,
2 and 7 discrete parents and for the two nodes of 256 configurations; the parameter tests shape their codes so that the cells that have
rows at all have that many (`populated`).  Why 2 D rows: both sides solve fp64 normal equations, and their variances carry eps S_yy /
RSS.  With k = N - D residual degrees of freedom RSS / S_yy of a cell falls below t with probability of order t^(k / 2): at k = 1
a few hundred cells reach 1e-5 and below - 1e-11 ... 1e-10 of disagreement that neither side is right about, down to lg_fit's own
suspect threshold RSS / S_yy = 1e-8 - while at k >= D >= 3 they stay above 1e-2.  (For D <= 2 the fits are closed forms and the same
count is kept.)  Status-1 cells of fewer rows are compared too and recorded, not asserted; measured on one MI355X: 9.7e-12 at worst on
these tables, and over tables of the same construction with other seeds 1.95e-10 at worst (D = 8, p + 2 rows), 3 cells of 143 with
p + 2 rows above 1e-10, every cell with two residual degrees of freedom or more below 1e-11.  Each path's error against exact rational least squares (lg_exact.exact_fit) is printed and the worst per family
recorded (PBN_CLG_FIT_ERRORS=<file> writes them), not asserted.

Reference routines: factors/discrete/DiscreteAdaptator.hpp:201-276, learning/parameters/mle_LinearGaussianCPD.hpp."""
import ctypes as C
import os

import numpy as np
import pytest

import lg_exact

pytestmark = pytest.mark.gpu

SHIFT = 8
WIDTH = 11            # columns of the device tables: 8 of data and noise between them
TOL = 1e-10
INVALID = 1           # PBN_ERR_INVALID


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib(pbn):
    from pybnesian_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def cf(pbn):
    from pybnesian_amd import clg_fit

    return clg_fit


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    lines = [f"{family:<64s} {err:.3g}" for family, err in sorted(w.items())]
    for line in lines:
        print("\nclg_fit gpu " + line)
    path = os.environ.get("PBN_CLG_FIT_ERRORS")
    if path and lines:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def grid_table(seed, n, d, dtype):
    """n rows of d columns on the 2^-8 grid; lg_exact.make_table cannot make the d = 1 float32 table (it scales the response by the
    parents' magnitude), that one is made by hand."""
    if d == 1 and np.dtype(dtype) == np.float32:
        xi = np.rint(np.ldexp(0.5 * np.random.default_rng(seed).normal(size=(n, 1)), SHIFT)).astype(np.int64)
        t = lg_exact.Table(xi, SHIFT, dtype, 1.0, ())
    else:
        t = lg_exact.make_table(seed, n, d, dtype=dtype, shift=SHIFT)
    # the exactness precondition of the module docstring
    assert t.shift == SHIFT and n <= 4097 and int(np.abs(t.xi).max()) < 2 ** 15
    return t


class Case:
    """A grid table inside a WIDTH-column device table (data column j in table column pos[j]) and a code table of the same rows."""

    def __init__(self, lib, table, code_arrays, cards, seed=0, ctx=None):
        from pybnesian_amd import _lib
        from pybnesian_amd.dataset import default_context
        from pybnesian_amd.network_pass import CodeTable

        self._lib, self.lib, self.table = _lib, lib, table
        n, d = table.data.shape
        self.n, self.d = n, d
        rng = np.random.default_rng(1000 + seed)
        self.pos = [int(c) for c in rng.permutation(WIDTH)[:d]]
        self.columns = [np.ascontiguousarray(rng.normal(size=n).astype(table.data.dtype)) for _ in range(WIDTH)]
        for j, c in enumerate(self.pos):
            self.columns[c] = np.ascontiguousarray(table.data[:, j])
        self.ctx = ctx or default_context()
        ptrs = (C.c_void_p * WIDTH)(*[a.ctypes.data if a.size else None for a in self.columns])
        h = C.c_void_p()
        dtype = _lib.PBN_F32 if table.data.dtype == np.float32 else _lib.PBN_F64
        _lib.check(lib.pbn_table_create(self.ctx.handle, ptrs, WIDTH, n, dtype, None, 0, C.byref(h)))
        self.h = h
        self.codes = [np.ascontiguousarray(c, dtype=np.int32) for c in code_arrays]
        self.cards = [int(c) for c in cards]
        self.ctable = CodeTable(self.ctx, self.codes, self.cards, n)

    def close(self):
        self.ctable.close()
        self.lib.pbn_table_destroy(self.h)

    # a node here: (data columns [variable, continuous parents...], code columns [discrete parents...])
    def configs(self, node):
        return int(np.prod([self.cards[c] for c in node[1]]))

    def keys(self, node):
        key = np.zeros(self.n, dtype=np.int64)
        valid = np.ones(self.n, dtype=bool)
        stride = 1
        for c in node[1]:
            valid &= self.codes[c] >= 0
            key += np.where(self.codes[c] >= 0, self.codes[c], 0).astype(np.int64) * stride
            stride *= self.cards[c]
        return key, valid

    def args(self, nodes):
        """Every argument of pbn_clg_fit for `nodes`, by name: a refusal test replaces one."""
        ip, i64p, dp = C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_double)
        dpar_off, dparents, cpar_off, cparents, cell_off, param_off, n_mom, n_shift = [0], [], [0], [], [0], [0], 0, 0
        for cont, disc in nodes:
            D, G = len(cont), self.configs((cont, disc))
            dparents += list(disc)
            dpar_off.append(len(dparents))
            cparents += [self.pos[j] for j in cont[1:]]
            cpar_off.append(len(cparents))
            cell_off.append(cell_off[-1] + G)
            param_off.append(param_off[-1] + G * (D + 1))
            n_mom += G * (D + D * (D + 1) // 2)
            n_shift += G * D
        keep = dict(cell_off=np.array(cell_off, dtype=np.int64), param_off=np.array(param_off, dtype=np.int64),
                    rows=np.full(max(cell_off[-1], 1), -7, dtype=np.int64), params=np.full(max(param_off[-1], 1), np.nan),
                    status=np.full(max(cell_off[-1], 1), 9, dtype=np.uint8), shift=np.full(max(n_shift, 1), np.nan),
                    moments=np.full(max(n_mom, 1), np.nan), launches=C.c_int64(-1))
        a = dict(ctx=self.ctx.handle, dt=self.ctable.handle, t=self.h, n_nodes=len(nodes), var=self._lib.int_array([self.pos[c[0]] for c, _ in nodes]),
                 dpar_off=self._lib.int_array(dpar_off), dparents=self._lib.int_array(dparents or [0]), cpar_off=self._lib.int_array(cpar_off),
                 cparents=self._lib.int_array(cparents or [0]), cell_off=keep["cell_off"].ctypes.data_as(i64p),
                 param_off=keep["param_off"].ctypes.data_as(i64p), rows=keep["rows"].ctypes.data_as(i64p), params=keep["params"].ctypes.data_as(dp),
                 status=keep["status"].ctypes.data_as(C.POINTER(C.c_ubyte)), shift=keep["shift"].ctypes.data_as(dp),
                 moments=keep["moments"].ctypes.data_as(dp), launches=C.byref(keep["launches"]))
        return a, keep

    def call(self, nodes):
        a, keep = self.args(nodes)
        self._lib.check(self.lib.pbn_clg_fit(*a.values()))
        return keep

    def expected(self, node):
        """(rows, shift, moments) of the node's cells in integers: [(N, shift[D], sums[D] + upper triangle)], in grid units."""
        cont, disc = node
        X = self.table.xi[:, cont]
        key, valid = self.keys(node)
        sh = X[0]
        Z = X - sh
        D = len(cont)
        out = []
        for c in range(self.configs(node)):
            Zc = Z[valid & (key == c)]
            mom = [int(Zc[:, i].sum()) for i in range(D)] + [int((Zc[:, i] * Zc[:, j]).sum()) for i in range(D) for j in range(i, D)]
            assert all(abs(v) < 2 ** 53 for v in mom)
            out.append((len(Zc), [int(v) for v in sh], mom))
        return out

    def take_fit(self, node, rows):
        """The comparator: pbn_table_take of the rows, then pbn_lg_fit_table."""
        cols = [self.pos[j] for j in node[0]]
        idx = np.ascontiguousarray(rows, dtype=np.int32)
        sub = C.c_void_p()
        self._lib.check(self.lib.pbn_table_take(self.h, idx.ctypes.data, len(idx), C.byref(sub)))
        beta, var = np.full(len(cols), np.nan), C.c_double(np.nan)
        try:
            self._lib.check(self.lib.pbn_lg_fit_table(sub, self._lib.int_array(cols), len(cols), 0, len(idx), beta.ctypes.data_as(C.POINTER(C.c_double)),
                                                      C.byref(var)))
        finally:
            self.lib.pbn_table_destroy(sub)
        return beta, var.value


def unpack(node_list, case, keep):
    """[(node, cell, rows, status, beta, variance, shift[D], moments)] of a call's outputs, cell by cell"""
    out, cell, po, so, mo = [], 0, 0, 0, 0
    for node in node_list:
        D = len(node[0])
        S = D + D * (D + 1) // 2
        for c in range(case.configs(node)):
            rec = keep["params"][po: po + D + 1]
            out.append((node, c, int(keep["rows"][cell]), int(keep["status"][cell]), rec[:D].copy(), float(rec[D]), keep["shift"][so: so + D].copy(),
                        keep["moments"][mo: mo + S].copy()))
            cell, po, so, mo = cell + 1, po + D + 1, so + D, mo + S
    return out


def check_moments(case, nodes, keep):
    """rows, shift and moments against the integers, tolerance zero; status 0 exactly for the cells without rows"""
    cells = unpack(nodes, case, keep)
    want = [(node, e) for node in nodes for e in case.expected(node)]
    assert len(cells) == len(want)
    for (node, c, rows, status, _, _, shift, moments), (_, (N, sh, mom)) in zip(cells, want):
        D = len(node[0])
        assert rows == N, (node, c, rows, N)
        assert (status == 0) == (N == 0), (node, c, status, N)
        assert np.array_equal(shift, np.ldexp(np.array(sh, dtype=np.float64), -SHIFT)), (node, c)
        exact = np.array([np.ldexp(float(v), -SHIFT) for v in mom[:D]] + [np.ldexp(float(v), -2 * SHIFT) for v in mom[D:]])
        assert np.array_equal(moments, exact), (node, c, moments, exact)
    return cells


def rel_errors(beta, var, ref_beta, ref_var):
    """(max|beta - ref| / max|ref|, relative error of the variance); a NaN coefficient (0 / 0 in a cell of one row, whose variance is
    infinite) must be NaN in both"""
    nan = np.isnan(ref_beta)
    if not np.array_equal(np.isnan(beta), nan):
        return np.inf, np.inf
    if nan.all():
        e_beta = 0.0
    else:
        scale = np.max(np.abs(ref_beta[~nan]))
        e_beta = float(np.max(np.abs(beta[~nan] - ref_beta[~nan])) / (scale if scale > 0 else 1.0))
    if np.isinf(ref_var) or np.isinf(var) or ref_var == 0.0:
        e_var = 0.0 if var == ref_var else np.inf
    else:
        e_var = abs(var - ref_var) / ref_var
    return e_beta, e_var


def check_parameters(case, nodes, cells, worst=None, family=None):
    """Every status-1 cell of at least 2 D rows (module docstring) against take + pbn_lg_fit_table within 1e-10; returns how many.  With
    `worst`: the cells of fewer rows are recorded against the comparator, and both paths against exact least squares"""
    checked = 0
    for node, c, rows, status, beta, var, _, _ in cells:
        if status != 1 or not any(node is m for m in nodes):
            continue
        D = len(node[0])
        key, valid = case.keys(node)
        idx = np.nonzero(valid & (key == c))[0]
        assert len(idx) == rows
        ref_beta, ref_var = case.take_fit(node, idx)
        e_beta, e_var = rel_errors(beta, var, ref_beta, ref_var)
        if rows < 2 * D:
            if worst is not None:
                lg_exact.note(worst, f"d {D}: status-1 cells of fewer than 2 D rows against take + pbn_lg_fit_table (not asserted)", max(e_beta, e_var))
            continue
        assert e_beta <= TOL and e_var <= TOL, (node, c, rows, beta, var, ref_beta, ref_var)
        checked += 1
        if worst is not None and family is not None and len(node[1]) <= 2:
            try:
                x_beta, x_var = lg_exact.exact_fit(case.table.xi[idx][:, node[0]], SHIFT)
            except ZeroDivisionError:
                continue
            if not x_var > 0:
                continue
            ours, theirs = max(rel_errors(beta, var, x_beta, x_var)), max(rel_errors(ref_beta, ref_var, x_beta, x_var))
            print(f"{family} cell {c} rows {rows}: pbn_clg_fit {ours:.3g}, take + pbn_lg_fit_table {theirs:.3g} (against exact least squares)")
            lg_exact.note(worst, f"{family}: pbn_clg_fit", ours)
            lg_exact.note(worst, f"{family}: take + pbn_lg_fit_table", theirs)
    return checked


CARDS = [3, 2, 3, 2, 2, 2, 2, 2, 2]


def codes_for(n, seed, populated=False):
    """Nine code columns: 0 card 3; 1 card 2; 2 card 3 with -1s (from two rows on); 3..8 card 2.  Row 0 is never null in column 2 only by
    chance - the shift does not depend on it.  populated: the rows take one of 6 joint patterns of the nine codes, so that a cell that
    has rows at all has about n / 6 of them (n / 7.5 where column 2 is read), whatever the number of parents."""
    rng = np.random.default_rng(seed)
    if populated:
        patterns = np.stack([rng.integers(0, card, size=6) for card in CARDS])     # [column][pattern]
        cols = list(patterns[:, rng.integers(0, 6, size=n)])
    else:
        cols = [rng.integers(0, card, size=n) for card in CARDS]
    if n >= 2:
        cols[2][rng.random(n) < 0.2] = -1
        cols[2][n - 1] = -1   # the last row of the tail is a null row
    return cols, list(CARDS)


def nodes_for(d):
    """Three nodes over the same d columns with 1, 2 and 7 discrete parents; the second takes the first's first parent as its variable
    (d >= 2: a column shared as variable and as parent) and reads the code column with nulls."""
    first = list(range(d))
    second = first[1:] + first[:1] if d >= 2 else first
    return [(first, [0]), (second, [2, 1]), (first, [1, 2, 3, 4, 5, 6, 7])]


def row_counts(R):
    return [1, 2, 63, 64, 65, 255, 256, 257, R - 1, R, R + 1, 2 * R + 1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_moments_are_exact_at_every_row_count(lib, cf, d, dtype):
    """Fails without pbn_clg_fit: the library has no such symbol."""
    assert cf.TILE_ROWS == 1024
    for n in row_counts(cf.TILE_ROWS):
        codes, cards = codes_for(n, 7 * n + d)
        case = Case(lib, grid_table(n + d, n, d, dtype), codes, cards, seed=n)
        try:
            nodes = nodes_for(d)
            keep = case.call(nodes)
            check_moments(case, nodes, keep)
            assert keep["launches"].value >= 3    # the shifts, at least one moment launch, the chunk sum
            if n in (257, 2 * cf.TILE_ROWS + 1):  # two calls, the same bits
                again = case.call(nodes)
                for name in ("rows", "params", "status", "shift", "moments"):
                    assert keep[name].tobytes() == again[name].tobytes(), name
        finally:
            case.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_parameters_match_take_and_fit_table(lib, cf, worst, d, dtype):
    R = cf.TILE_ROWS
    for n in (257, R + 1, 2 * R + 1):
        # populated cells: every status-1 cell of the three nodes is held to 1e-10
        codes, cards = codes_for(n, 11 * n + d, populated=True)
        case = Case(lib, grid_table(100 + n + d, n, d, dtype), codes, cards, seed=n + 1)
        try:
            nodes = nodes_for(d)
            cells = check_moments(case, nodes, case.call(nodes))
            fitted = [sum(1 for c in cells if c[0] is node and c[3] == 1) for node in nodes]
            record = worst if n == 2 * R + 1 else None
            checked = [check_parameters(case, [node], cells, record, f"d {d} {np.dtype(dtype).name} n {n}") for node in nodes]
            assert checked == fitted, (checked, fitted)        # no status-1 cell is left out: each has its 2 D rows
            assert min(checked) >= 2 and checked[2] >= 3, checked
        finally:
            case.close()
        # independent codes: the 192 cells of the third node hold a handful of rows each; those of 2 D rows are held to 1e-10, the
        # others recorded
        codes, cards = codes_for(n, 13 * n + d)
        case = Case(lib, grid_table(200 + n + d, n, d, dtype), codes, cards, seed=n + 2)
        try:
            cells = check_moments(case, nodes, case.call(nodes))
            assert check_parameters(case, nodes, cells, worst) >= 9    # (the cells of the first two nodes all have rows enough)
        finally:
            case.close()


@pytest.mark.parametrize("d", [2, 4, 8])
def test_nodes_with_the_cap_configurations(lib, cf, worst, d):
    """256 configurations as 16 x 16 and as one parent of 256, 16 rows in every cell (fewer where a code is null): the moments of all 512
    cells exact, every status-1 cell of 2 D rows within 1e-10 - at D = 8 the cells are short of that and are recorded"""
    n = 4 * cf.TILE_ROWS + 1
    rng = np.random.default_rng(5 + d)
    assert cf.MAX_CONFIGS == 256
    key = rng.permutation(n) % 256       # balanced
    codes, cards = [key % 16, key // 16, rng.permutation(n) % 256], [16, 16, 256]
    codes[1] = codes[1].copy()
    codes[1][::97] = -1
    case = Case(lib, grid_table(9 + d, n, d, np.float64), codes, cards)
    try:
        cols = list(range(d))
        nodes = [(cols, [0, 1]), (cols[-2:], [2])]
        cells = check_moments(case, nodes, case.call(nodes))
        assert len(cells) == 512 and all(c[2] >= 14 for c in cells)
        checked = check_parameters(case, nodes, cells, worst)
        fitted = sum(1 for c in cells if c[3] == 1 and c[2] >= 2 * len(c[0][0]))
        assert checked == fitted and checked >= (500 if d <= 4 else 256)
    finally:
        case.close()


@pytest.mark.parametrize("d", [1, 2, 3, 4, 8])
def test_cells_of_0_1_p_plus_1_and_p_plus_2_rows(lib, d, monkeypatch):
    """status 0, then an infinite variance twice, then a finite one - with the guard off for p >= 3, where a fit through p + 1 points
    (or of one row) is what lg_fit marks suspect: those two cells are then status 2, exactly pbn_lg_fit_table's refits."""
    p = d - 1
    n = 600
    code = np.full(n, 4, dtype=np.int32)
    code[10:11] = 1
    code[20:20 + p + 1] = 2
    code[40:40 + p + 2] = 3
    case = Case(lib, grid_table(30 + d, n, d, np.float64), [code], [5])
    try:
        nodes = [(list(range(d)), [0])]
        cells = check_moments(case, nodes, case.call(nodes))
        assert [c[2] for c in cells] == [0, 1, p + 1, p + 2, n - 2 * p - 4]
        if p >= 3:
            assert [c[3] for c in cells] == [0, 2, 2, 1, 1]
            check_parameters(case, nodes, cells)
            monkeypatch.setenv("PBN_LG_GUARD", "0")
            cells = check_moments(case, nodes, case.call(nodes))
        assert [c[3] for c in cells] == [0, 1, 1, 1, 1]
        assert np.all(cells[0][4] == 0.0) and cells[0][5] == 0.0     # a cell without rows leaves its record zero
        assert cells[1][5] == np.inf and cells[2][5] == np.inf
        assert np.isfinite(cells[3][5]) and cells[3][5] > 0 and np.isfinite(cells[4][5])
        if p < 3:
            check_parameters(case, nodes, cells)
        else:   # the guard is off: the variances of the comparator, which takes the same path
            for cell in cells[1:]:
                key, valid = case.keys(nodes[0])
                _, ref_var = case.take_fit(nodes[0], np.nonzero(valid & (key == cell[1]))[0])
                assert rel_errors(cell[4], cell[5], cell[4], ref_var)[1] <= TOL
    finally:
        case.close()


def test_a_cell_whose_variable_is_constant(lib):
    n = 300
    t = grid_table(41, n, 4, np.float64)
    code = (np.arange(n) % 3).astype(np.int32)
    t.xi[code == 1, 0] = 517          # 517 * 2^-8 in every row of configuration 1
    t = lg_exact.Table(t.xi, SHIFT, np.float64, 1.0, ())
    case = Case(lib, t, [code], [3])
    try:
        nodes = [([0], [0]), ([0, 1], [0]), ([0, 1, 2, 3], [0])]
        cells = check_moments(case, nodes, case.call(nodes))
        by = {(len(c[0][0]), c[1]): c for c in cells}
        value = 517 * 2.0 ** -SHIFT
        assert by[(1, 1)][3] == 1 and by[(1, 1)][5] == 0.0 and by[(1, 1)][4][0] == value        # p = 0: the mean, variance 0
        assert by[(2, 1)][3] == 1 and by[(2, 1)][5] == 0.0 and list(by[(2, 1)][4]) == [value, 0.0]
        assert by[(4, 1)][3] == 2                                                                 # p = 3: RSS = 0 is a suspect fit
        assert all(by[(d, c)][3] == 1 and by[(d, c)][5] > 0 for d in (1, 2, 4) for c in (0, 2))
        check_parameters(case, nodes, [c for c in cells if c[1] != 1])    # (a variance of exactly 0 has no relative error)
    finally:
        case.close()


def test_a_nearly_collinear_family_is_reported(lib):
    n = 1500
    t = lg_exact.make_table(3, n, 4, kappa=1e7)     # p = 3, the last parent a copy of the first up to 1e-7
    code = (np.arange(n) % 2).astype(np.int32)
    case = Case(lib, t, [code], [2])
    try:
        keep = case.call([([0, 1, 2, 3], [0])])
        assert list(keep["rows"]) == [750, 750]
        assert list(keep["status"]) == [2, 2]
        assert np.all(keep["params"] == 0.0)
        # without the last parent the same rows are an ordinary fit
        keep = case.call([([0, 1, 2], [0])])
        assert list(keep["status"]) == [1, 1]
    finally:
        case.close()


def test_tables_without_rows(lib):
    t = lg_exact.Table(np.zeros((1, 2), dtype=np.int64), SHIFT, np.float64, 1.0, ())
    t.data, t.xi = t.data[:0], t.xi[:0]
    case = Case(lib, t, [np.zeros(0, dtype=np.int32)], [3])
    try:
        keep = case.call([([0, 1], [0])])
        assert list(keep["rows"]) == [0, 0, 0] and list(keep["status"]) == [0, 0, 0] and keep["launches"].value == 0
        assert np.all(keep["params"] == 0.0) and np.all(keep["moments"] == 0.0)
    finally:
        case.close()


def test_refusals(lib, pbn):
    n = 100
    codes = [np.zeros(n, dtype=np.int32)] * 9 + [np.zeros(n, dtype=np.int32)]
    cards = [3, 2, 2, 2, 2, 2, 2, 2, 2, 257]
    case = Case(lib, grid_table(1, n, 8, np.float64), codes, cards)
    short = Case(lib, grid_table(2, n - 1, 8, np.float64), [c[:n - 1] for c in codes], cards)
    other = Case(lib, grid_table(3, n, 8, np.float64), codes, cards, ctx=pbn.Context(0))
    good = [(list(range(8)), [0, 1])]

    def refused(nodes=good, **replace):
        a, keep = case.args(nodes)
        a.update(replace)
        rc = lib.pbn_clg_fit(*a.values())
        if rc == INVALID:
            assert np.all(keep["status"] == 9), "a refused call wrote an output"
        return rc == INVALID

    try:
        a, _ = case.args(good)
        assert lib.pbn_clg_fit(*a.values()) == 0
        for name in ("ctx", "dt", "t", "var", "dpar_off", "dparents", "cpar_off", "cparents", "cell_off", "param_off", "rows", "params", "status"):
            assert refused(**{name: None}), name
        a, _ = case.args(good)
        a.update(shift=None, moments=None, launches=None)     # the three nullable ones
        assert lib.pbn_clg_fit(*a.values()) == 0
        assert refused(n_nodes=0)
        assert refused(dt=short.ctable.handle)                # tables of different row counts
        assert refused(t=short.h)
        assert refused(dt=other.ctable.handle)                # ... of different contexts
        assert refused(t=other.h)
        assert refused(ctx=other.ctx.handle)
        i = case._lib.int_array
        assert refused(var=i([WIDTH])) and refused(var=i([-1]))                      # a column outside its table
        assert refused(cparents=i([case.pos[j] for j in range(1, 7)] + [WIDTH]))
        assert refused(dparents=i([0, 10])) and refused(dparents=i([-1, 1]))
        assert refused(dparents=i([1, 1]))                                           # ... twice among the discrete parents
        assert refused([(list(range(8)), [])])                                       # no discrete parent
        assert refused([(list(range(8)), [0, 1, 2, 3, 4, 5, 6, 7])])                 # 8 discrete parents
        assert not refused([(list(range(8)), [0, 1, 2, 3, 4, 5, 6])])
        assert refused([(list(range(8)), [9])])                                      # 257 configurations
        assert refused([(list(range(8)), [9, 0])])
        a, _ = case.args([(list(range(8)) + [0], [0])])                              # 9 continuous columns
        assert lib.pbn_clg_fit(*a.values()) == INVALID
        keepalive = [np.array(v, dtype=np.int64) for v in ([0, 5], [1, 7], [0, 6 * 9 + 1], [1, 6 * 9 + 1])]
        for arr, name in zip(keepalive, ("cell_off", "cell_off", "param_off", "param_off")):   # offsets that do not match the cardinalities
            assert refused(**{name: arr.ctypes.data_as(C.POINTER(C.c_int64))}), (name, arr)
        assert refused(dpar_off=i([1, 3])) and refused(cpar_off=i([1, 8]))           # offsets that do not start at 0
    finally:
        case.close()
        short.close()
        other.close()
