"""GPU tier: the one-pass evaluation of CLG networks through the C ABI (csrc/clg_model.hip) at every launch shape.

The comparator is built from entry points that were there before: per CLG node and configuration of its discrete parents, pbn_lg_logl
on a table of that configuration's rows (pbn_table_take) with that configuration's coefficients and variance - the per-slice call of
_DiscreteAdaptator.logl; per discrete node the numpy CPT gather of DiscreteFactor.logl; the nodes' rows added in node order.
pbn_clgnet_logl must EQUAL that, bit for bit, NaN rows included.  pbn_clgnet_slogl sums in another order than any host routine, so
each per-node sum is held to the worst-case bound of ANY fp64 summation order of n terms v_i around their exact sum,
(n - 1) u sum|v_i| / (1 - (n - 1) u) with u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)), the exact sum
being math.fsum of the non-NaN reference values: derived, not measured.

clgnet_logl_kernel's row tile is 1 024 rows in four groups of 256: hence the row counts.

Reference routines: models/BayesianNetwork.hpp:997-1022, factors/discrete/DiscreteAdaptator.hpp:327-348,
factors/discrete/DiscreteFactor.cpp:91-171, factors/continuous/LinearGaussianCPD.cpp:92-149."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]
DTYPES = ["float64", "float32"]
INVALID = 1
U = 2.0 ** -53


class Net:
    """cards: cardinalities of the code columns; nodes in node order:
    ("d", variable code column, [parent code columns], CPT flat - the variable fastest)
    ("g", variable continuous column, [discrete parents], [continuous parents], [None | (beta, variance)] per configuration - the
          first discrete parent fastest)
    null_cols: code columns that get -1 codes."""

    def __init__(self, cards, n_ccols, nodes, null_cols=()):
        self.cards, self.n_ccols, self.nodes, self.null_cols = list(cards), n_ccols, nodes, null_cols
        self.kind, self.var, self.dparents, self.dpar_off, self.cparents, self.cpar_off = [], [], [], [0], [], [0]
        self.cfg_off, self.present, self.param_off, params = [0], [], [0], []
        for nd in nodes:
            clg = nd[0] == "g"
            self.kind.append(1 if clg else 0)
            self.var.append(nd[1])
            self.dparents += list(nd[2])
            self.dpar_off.append(len(self.dparents))
            if clg:
                self.cparents += list(nd[3])
                n_cfg = int(np.prod([cards[c] for c in nd[2]], dtype=np.int64)) if nd[2] else 1
                assert len(nd[4]) == n_cfg
                for rec in nd[4]:
                    self.present.append(0 if rec is None else 1)
                    beta, variance = ([7.0] * (len(nd[3]) + 1), 7.0) if rec is None else rec      # a missing record's values are not read
                    assert len(beta) == len(nd[3]) + 1
                    params += list(beta) + [variance]
                self.cfg_off.append(self.cfg_off[-1] + n_cfg)
            else:
                assert len(nd[3]) == int(np.prod([cards[c] for c in [nd[1]] + list(nd[2])], dtype=np.int64))
                params += list(nd[3])
                self.cfg_off.append(self.cfg_off[-1])
            self.cpar_off.append(len(self.cparents))
            self.param_off.append(len(params))
        self.params = np.asarray(params, dtype=np.float64)


def _cpt(rng, card, n_parent_cfg):
    """log of strictly positive probabilities: no zero-count cell, so no -inf sum"""
    p = rng.uniform(0.2, 1.0, size=(n_parent_cfg, card))
    return np.log(p / p.sum(axis=1, keepdims=True)).reshape(-1).tolist()


def _records(rng, n_cfg, p, missing=()):
    return [None if c in missing else (rng.normal(size=p + 1).tolist(), float(rng.uniform(0.3, 2.5))) for c in range(n_cfg)]


def _a():
    rng = np.random.default_rng(1)
    return Net([2], 1, [("g", 0, [0], [], _records(rng, 2, 0))])


def _b():
    # discrete parents of cardinalities 3 and 2 IN THAT ORDER: a swapped stride reads another record for every code pair but (0, 0), (1, 1)
    rng = np.random.default_rng(2)
    return Net([2, 3], 3, [("g", 1, [1, 0], [2, 0], _records(rng, 6, 2))])


def _c():
    # interleaved kinds: a discrete child, a CLG node, a discrete root, a plain LG node (one configuration), a second CLG node
    rng = np.random.default_rng(3)
    return Net([3, 2], 3, [("d", 1, [0], _cpt(rng, 2, 3)), ("g", 2, [1], [0], _records(rng, 2, 1)), ("d", 0, [], _cpt(rng, 3, 1)),
                           ("g", 0, [], [], _records(rng, 1, 0)), ("g", 1, [0, 1], [0, 2], _records(rng, 6, 2))])


def _d():
    # a parent of 300 categories: codes above a byte select records and CPT rows; the records of configurations 8 .. 249 are missing
    rng = np.random.default_rng(4)
    missing = set(range(8, 250))
    return Net([300, 2], 2, [("g", 0, [0], [1], _records(rng, 300, 1, missing)), ("d", 1, [0], _cpt(rng, 2, 300)), ("g", 1, [], [], _records(rng, 1, 0))])


def _e():
    # configurations 1 and 4 of 6 have no factor, and rows fall into them
    rng = np.random.default_rng(5)
    return Net([3, 2], 2, [("g", 0, [0, 1], [1], _records(rng, 6, 1, {1, 4})), ("d", 0, [], _cpt(rng, 3, 1))])


def _f():
    # -1 codes in a CLG node's discrete parent (column 0) and in a discrete node's own column (column 2)
    rng = np.random.default_rng(6)
    return Net([3, 2, 4], 2, [("g", 0, [0], [1], _records(rng, 3, 1)), ("d", 2, [1], _cpt(rng, 4, 2)), ("d", 1, [], _cpt(rng, 2, 1)),
                              ("g", 1, [1], [], _records(rng, 2, 0))], null_cols=(0, 2))


def _g():
    # degenerate variances in ONE configuration each: 0 (inv_std = inf: NaN or -inf rows) and 1e-300 (z ~ 1e150, finite)
    rng = np.random.default_rng(7)
    r0, r1 = _records(rng, 3, 1), _records(rng, 3, 1)
    r0[1] = (r0[1][0], 0.0)
    r1[2] = (r1[2][0], 1e-300)
    return Net([3], 2, [("g", 0, [0], [1], r0), ("g", 1, [0], [0], r1)])


NETS = {"a_one_binary_parent": _a, "b_strides_3_2": _b, "c_interleaved": _c, "d_card_300": _d, "e_missing_config": _e, "f_null_codes": _f,
        "g_degenerate_variance": _g}


@pytest.fixture(scope="module")
def env():
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    pbn.load_library()
    return pbn, _lib, _lib.load(), pbn.Context(0)


def make_data(net, rows, dtype, seed=0):
    rng = np.random.default_rng(seed * 7919 + rows + 31 * len(net.cards) + net.n_ccols)
    codes = [np.ascontiguousarray(rng.integers(0, c, size=rows), dtype=np.int32) for c in net.cards]
    for c in net.null_cols:
        codes[c][rng.random(rows) < 0.2] = -1
    cols = [np.ascontiguousarray(rng.normal(size=rows).astype(dtype)) for _ in range(net.n_ccols)]
    return codes, cols


class Table:
    def __init__(self, env, cols, rows, dtype):
        _, _lib, lib, ctx = env
        self.lib, self.cols = lib, cols
        ptrs = (C.c_void_p * len(cols))(*[c.ctypes.data if c.size else None for c in cols])
        self.handle = C.c_void_p()
        code = _lib.PBN_F64 if dtype == "float64" else _lib.PBN_F32
        _lib.check(lib.pbn_table_create(ctx.handle, ptrs, len(cols), rows, code, None, 0, C.byref(self.handle)))
        self.rows = rows

    def close(self):
        self.lib.pbn_table_destroy(self.handle)


class CodeTable:
    def __init__(self, env, codes, cards, rows, ctx=None):
        _, _lib, lib, ctx0 = env
        self.lib, self.codes = lib, codes
        ptrs = (C.c_void_p * len(codes))(*[c.ctypes.data for c in codes])
        self.handle = C.c_void_p()
        _lib.check(lib.pbn_dtable_create((ctx or ctx0).handle, rows, len(codes), ptrs, _lib.int_array(cards), C.byref(self.handle)))

    def close(self):
        self.lib.pbn_dtable_destroy(self.handle)


def create(env, net, **override):
    """(return code, handle) of pbn_clgnet_create for `net`, fields replaced by `override`"""
    _, _lib, lib, ctx = env
    a = dict(ctx=ctx.handle, n_dcols=len(net.cards), cards=net.cards, n_ccols=net.n_ccols, n_nodes=len(net.var), kind=net.kind, var=net.var,
             dpar_off=net.dpar_off, dparents=net.dparents, cpar_off=net.cpar_off, cparents=net.cparents, cfg_off=net.cfg_off, present=net.present,
             param_off=net.param_off, params=net.params)
    a.update(override)

    def ints(v):
        return None if v is None else _lib.int_array(list(v) or [0])

    present = None if a["present"] is None else np.ascontiguousarray(list(a["present"]) or [0], dtype=np.uint8)
    param_off = None if a["param_off"] is None else np.ascontiguousarray(a["param_off"], dtype=np.int64)
    params = None if a["params"] is None else np.ascontiguousarray(a["params"] if len(a["params"]) else [0.0], dtype=np.float64)
    h = C.c_void_p()
    rc = lib.pbn_clgnet_create(a["ctx"], a["n_dcols"], ints(a["cards"]), a["n_ccols"], a["n_nodes"], ints(a["kind"]), ints(a["var"]), ints(a["dpar_off"]),
                               ints(a["dparents"]), ints(a["cpar_off"]), ints(a["cparents"]), ints(a["cfg_off"]),
                               None if present is None else present.ctypes.data_as(C.POINTER(C.c_ubyte)),
                               None if param_off is None else param_off.ctypes.data_as(C.POINTER(C.c_int64)), None if params is None else _lib.dptr(params),
                               C.byref(h))
    return rc, h


class CLGNet:
    def __init__(self, env, net):
        _, _lib, lib, _ = env
        self._lib, self.lib, self.net = _lib, lib, net
        rc, self.handle = create(env, net)
        _lib.check(rc)

    def logl(self, dt, t, rows):
        out = np.full(rows, 123.0)
        self._lib.check(self.lib.pbn_clgnet_logl(self.handle, dt, t, self._lib.dptr(out)))
        return out

    def slogl(self, dt, t):
        out = np.full(len(self.net.var), 123.0)
        self._lib.check(self.lib.pbn_clgnet_slogl(self.handle, dt, t, self._lib.dptr(out)))
        return out

    def stats(self):
        launches, rows = C.c_int64(-1), C.c_int64(-1)
        self._lib.check(self.lib.pbn_clgnet_stats(self.handle, C.byref(launches), C.byref(rows)))
        return launches.value, rows.value

    def close(self):
        self.lib.pbn_clgnet_destroy(self.handle)


def per_factor(env, net, codes, table_handle, rows):
    """(the node-order sum of the nodes' reference rows, the list of those rows per node)"""
    _, _lib, lib, _ = env
    total, per_node = None, []
    for nd in net.nodes:
        keys = ([nd[1]] if nd[0] == "d" else []) + list(nd[2])
        idx, valid, stride = np.zeros(rows, dtype=np.int64), np.ones(rows, dtype=bool), 1
        for c in keys:
            valid &= codes[c] >= 0
            idx += np.where(codes[c] >= 0, codes[c], 0).astype(np.int64) * stride
            stride *= net.cards[c]
        ll = np.full(rows, np.nan)
        if nd[0] == "d":
            ll[valid] = np.asarray(nd[3], dtype=np.float64)[idx[valid]]              # DiscreteFactor.logl
        else:
            cols = [nd[1]] + list(nd[3])
            for c, rec in enumerate(nd[4]):                                        # _DiscreteAdaptator.logl
                sel = np.nonzero(valid & (idx == c))[0].astype(np.int32)
                if rec is None or sel.size == 0:
                    continue
                piece = C.c_void_p()
                _lib.check(lib.pbn_table_take(table_handle, sel.ctypes.data, sel.size, C.byref(piece)))
                try:
                    vals = np.full(sel.size, 321.0)
                    b = np.ascontiguousarray(rec[0], dtype=np.float64)
                    _lib.check(lib.pbn_lg_logl(piece, _lib.int_array(cols), len(cols), 0, sel.size, _lib.dptr(b), float(rec[1]), _lib.dptr(vals), None))
                finally:
                    lib.pbn_table_destroy(piece)
                ll[sel] = vals
        per_node.append(ll)
        total = ll if total is None else total + ll
    return total, per_node


def check_sums(got, per_node, where):
    for i, (s, ll) in enumerate(zip(got, per_node)):
        v = ll[~np.isnan(ll)]
        if v.size == 0:
            assert s == 0.0 and not np.signbit(s), (where, i, s)     # nothing but NaN rows (or no rows): exactly +0.0
            continue
        try:
            exact, mass = math.fsum(v), math.fsum(np.abs(v))
        except OverflowError:
            exact, mass = -np.inf, np.inf
        if not np.isfinite(mass):
            assert s == exact, (where, i, s, exact)                  # an infinite sum must be that infinity
            continue
        n = v.size
        bound = (n - 1) * U * mass / (1.0 - (n - 1) * U)
        print(f"slogl {where} node {i}: n={n} |got - fsum|={abs(s - exact):.3e} bound={bound:.3e}")
        assert abs(s - exact) <= bound, (where, i, s, exact, bound)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(NETS))
def test_equals_the_per_factor_calls_at_every_row_count(env, name, dtype):
    net = NETS[name]()
    g = CLGNet(env, net)
    try:
        for rows in ROWS:
            codes, cols = make_data(net, rows, dtype)
            t = Table(env, cols, rows, dtype)
            dt = CodeTable(env, codes, net.cards, rows)
            try:
                want, per_node = per_factor(env, net, codes, t.handle, rows)
                got = g.logl(dt.handle, t.handle, rows)
                assert got.shape == (rows,)
                if rows:
                    assert np.array_equal(got, want, equal_nan=True), (name, dtype, rows, np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[:8])
                sums = g.slogl(dt.handle, t.handle)
                check_sums(sums, per_node, (name, dtype, rows))
                if rows == 0:
                    assert list(sums) == [0.0] * len(net.var)
            finally:
                dt.close()
                t.close()
    finally:
        g.close()


def test_the_networks_hold_what_they_are_there_for(env):
    rows = 1025
    out = {}
    for name in NETS:
        net = NETS[name]()
        codes, cols = make_data(net, rows, "float64")
        t, dt, g = Table(env, cols, rows, "float64"), CodeTable(env, codes, net.cards, rows), CLGNet(env, net)
        try:
            out[name] = (net, codes, per_factor(env, net, codes, t.handle, rows)[1], g.logl(dt.handle, t.handle, rows))
        finally:
            g.close()
            dt.close()
            t.close()
    for name in ("a_one_binary_parent", "b_strides_3_2", "c_interleaved"):
        assert np.isfinite(out[name][3]).all()
    net, codes, per_node, got = out["d_card_300"]
    assert (codes[0] > 255).any() and np.isfinite(got[codes[0] >= 250]).all() and np.isnan(got[(codes[0] >= 8) & (codes[0] < 250)]).all()
    net, codes, per_node, got = out["e_missing_config"]
    cfg = codes[0] + 3 * codes[1]
    fell = (cfg == 1) | (cfg == 4)
    assert fell.sum() > 100 and np.isnan(got[fell]).all() and np.isfinite(got[~fell]).all()
    net, codes, per_node, got = out["f_null_codes"]
    null = (codes[0] < 0) | (codes[2] < 0)
    assert null.any() and (~null).any() and np.array_equal(np.isnan(got), null)
    assert (np.isnan(per_node[0]) != np.isnan(per_node[1])).any()     # the two null columns hit different nodes
    net, codes, per_node, got = out["g_degenerate_variance"]
    assert not np.isfinite(per_node[0][codes[0] == 1]).any() and np.isfinite(per_node[0][codes[0] != 1]).all()     # variance 0 in configuration 1 only
    assert np.isfinite(per_node[1]).all() and (per_node[1][codes[0] == 2] < -1e290).any() and (np.abs(per_node[1][codes[0] != 2]) < 1e6).all()
    assert np.isfinite(got[codes[0] == 0]).all()


def test_interleaved_network_against_the_closed_form(env):
    """Independent of every kernel of this library: the CPT cell, or -0.5 ((y - X beta) / sigma)^2 - 0.5 log sigma^2 - 0.5 log 2 pi, in numpy."""
    net = _c()
    rows = 1025
    codes, cols = make_data(net, rows, "float64")
    t, dt, g = Table(env, cols, rows, "float64"), CodeTable(env, codes, net.cards, rows), CLGNet(env, net)
    try:
        want = np.zeros(rows)
        for nd in net.nodes:
            keys = ([nd[1]] if nd[0] == "d" else []) + list(nd[2])
            idx, stride = np.zeros(rows, dtype=np.int64), 1
            for c in keys:
                idx += codes[c].astype(np.int64) * stride
                stride *= net.cards[c]
            if nd[0] == "d":
                want += np.asarray(nd[3])[idx]
                continue
            beta = np.asarray([nd[4][c][0] for c in idx])
            variance = np.asarray([nd[4][c][1] for c in idx])
            mean = beta[:, 0] + sum(beta[:, 1 + j] * cols[p] for j, p in enumerate(nd[3]))
            want += -0.5 * (cols[nd[1]] - mean) ** 2 / variance - 0.5 * np.log(variance) - 0.5 * np.log(2 * np.pi)
        np.testing.assert_allclose(g.logl(dt.handle, t.handle, rows), want, rtol=1e-7, atol=1e-9)
    finally:
        g.close()
        dt.close()
        t.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_borrowed_table_at_an_odd_leading_dimension(env, dtype):
    import torch

    pbn, _lib, lib, ctx = env
    net = _c()
    rows, ld = 1025, 1031
    codes, cols = make_data(net, rows, dtype)
    host = np.zeros((net.n_ccols, ld), dtype=dtype)
    host[:, :rows] = np.stack(cols)
    dev = torch.from_numpy(host).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    borrowed = C.c_void_p()
    code = _lib.PBN_F64 if dtype == "float64" else _lib.PBN_F32
    _lib.check(lib.pbn_table_from_device(ctx.handle, C.c_void_p(dev.data_ptr()), ld, net.n_ccols, rows, code, C.byref(borrowed)))
    owned, dt, g = Table(env, cols, rows, dtype), CodeTable(env, codes, net.cards, rows), CLGNet(env, net)
    try:
        want, per_node = per_factor(env, net, codes, owned.handle, rows)
        got = g.logl(dt.handle, borrowed, rows)
        assert np.array_equal(got, want, equal_nan=True)
        assert np.array_equal(got, g.logl(dt.handle, owned.handle, rows))
        sums = g.slogl(dt.handle, borrowed)
        check_sums(sums, per_node, ("borrowed", dtype, rows))
        assert sums.tobytes() == g.slogl(dt.handle, owned.handle).tobytes()
    finally:
        g.close()
        dt.close()
        owned.close()
        lib.pbn_table_destroy(borrowed)
    del dev


def test_second_call_gives_the_same_bits_and_stats_count_launches(env):
    net = _c()
    rows = 2049
    codes, cols = make_data(net, rows, "float64")
    t, dt, g = Table(env, cols, rows, "float64"), CodeTable(env, codes, net.cards, rows), CLGNet(env, net)
    try:
        assert g.stats() == (0, 0)
        first = g.logl(dt.handle, t.handle, rows)
        assert g.stats() == (1, rows)                  # one evaluation launch per logl call, for all five nodes
        second = g.logl(dt.handle, t.handle, rows)
        assert g.stats() == (2, 2 * rows)
        assert first.tobytes() == second.tobytes()
        s1 = g.slogl(dt.handle, t.handle)
        assert g.stats() == (3, 3 * rows)
        assert s1.tobytes() == g.slogl(dt.handle, t.handle).tobytes()
    finally:
        g.close()
        dt.close()
        t.close()


def test_a_group_of_nan_rows_sums_to_zero(env):
    """Rows 256 .. 511 - one whole 256-row group - carry a -1 code: the group's partial of the nodes that read the column is +0.0, and the
    sums are those of the other rows alone."""
    net = _f()
    rows = 1025
    codes, cols = make_data(net, rows, "float64")
    codes[0][:] = np.abs(codes[0])
    codes[2][:] = np.abs(codes[2])
    codes[0][256:512] = -1
    t, dt, g = Table(env, cols, rows, "float64"), CodeTable(env, codes, net.cards, rows), CLGNet(env, net)
    keep = np.r_[0:256, 512:rows]
    t2, dt2 = Table(env, [np.ascontiguousarray(c[keep]) for c in cols], keep.size, "float64"), CodeTable(env, [np.ascontiguousarray(c[keep]) for c in codes], net.cards, keep.size)
    try:
        _, per_node = per_factor(env, net, codes, t.handle, rows)
        assert np.isnan(per_node[0][256:512]).all() and not np.isnan(per_node[0][keep]).any()
        sums = g.slogl(dt.handle, t.handle)
        check_sums(sums, per_node, ("nan group", rows))
        # node 0 without the NaN group: the same 256-row groups in the same order, so the same bits
        assert sums[0] == g.slogl(dt2.handle, t2.handle)[0]
    finally:
        g.close()
        for h in (dt, dt2, t, t2):
            h.close()


def test_refusals(env):
    pbn, _lib, lib, ctx = env
    net = _c()

    def refused(**override):
        rc, h = create(env, override.pop("net", net), **override)
        if rc == 0:
            lib.pbn_clgnet_destroy(h)
        return (rc, h.value) == (INVALID, None)

    rc, h = create(env, net)
    assert rc == 0
    lib.pbn_clgnet_destroy(h)
    for field in ("ctx", "cards", "kind", "var", "dpar_off", "dparents", "cpar_off", "cparents", "cfg_off", "present", "param_off", "params"):
        assert refused(**{field: None}), field                                             # a null argument
    assert refused(n_nodes=0)
    assert refused(var=[2, 2, 2, 0, 1])                                                    # a discrete variable = n_dcols
    assert refused(var=[1, 3, 0, 0, 1])                                                    # a continuous variable = n_ccols
    assert refused(dparents=[2, 1, 0, 1])                                                  # a discrete parent = n_dcols
    assert refused(cparents=[0, 3, 2])                                                     # a continuous parent = n_ccols
    assert refused(cparents=[0, -1, 2])
    two = [2] * 9
    # caps: served at the cap, refused one beyond
    at_cap = Net(two, 1, [("d", 0, list(range(1, 8)), [0.0] * 256), ("g", 0, list(range(7)), [], [([0.0], 1.0)] * 128)])
    rc, h = create(env, at_cap)
    assert rc == 0
    lib.pbn_clgnet_destroy(h)
    assert refused(net=Net(two, 1, [("d", 0, list(range(1, 9)), [0.0] * 512), ("g", 0, [], [], [([0.0], 1.0)])]))          # 9 discrete family variables
    assert refused(net=Net(two, 1, [("g", 0, list(range(8)), [], [([0.0], 1.0)] * 256)]))                                   # 8 discrete parents
    assert refused(net=Net([2], 70, [("g", 0, [0], list(range(1, 65)), [([0.0] * 65, 1.0)] * 2)]))                          # 65 continuous family columns
    rc, h = create(env, Net([2], 70, [("g", 0, [0], list(range(1, 64)), [([0.0] * 64, 1.0)] * 2)]))
    assert rc == 0
    lib.pbn_clgnet_destroy(h)
    # counts and offsets that are not the cardinalities'
    assert refused(cfg_off=[0, 0, 2, 2, 3, 8])                                             # 5 marks for a node of 6 configurations
    assert refused(cfg_off=[0, 1, 3, 3, 4, 10])                                            # marks for a discrete node
    assert refused(param_off=[p + (1 if i >= 2 else 0) for i, p in enumerate(net.param_off)])
    assert refused(cards=[3, 3])                                                           # every CPT and record count off
    assert refused(cards=[3, 0])
    # a node beyond PBN_CLGNET_MAX_CONFIGS, parameters beyond PBN_CLGNET_MAX_PARAMS: refused before any parameter is read
    one = dict(n_nodes=1, kind=[1], var=[0], dpar_off=[0, 2], dparents=[0, 1], cpar_off=[0, 0], cparents=[], present=[1], params=[0.0])
    assert refused(n_dcols=2, cards=[1024, 1025], n_ccols=1, cfg_off=[0, 1024 * 1025], param_off=[0, 1024 * 1025 * 2], **one)
    five = dict(n_nodes=5, kind=[1] * 5, var=[0] * 5, dpar_off=[0, 2, 4, 6, 8, 10], dparents=[0, 1] * 5, cpar_off=[61 * i for i in range(6)],
                cparents=list(range(1, 62)) * 5, present=[1], params=[0.0])
    assert refused(n_dcols=2, cards=[1024, 1024], n_ccols=62, cfg_off=[i << 20 for i in range(6)], param_off=[i * 63 << 20 for i in range(6)], **five)
    # evaluation: nothing is launched for any of these
    rows = 300
    codes, cols = make_data(net, rows, "float64")
    g = CLGNet(env, net)
    other = pbn.Context(0)
    t, dt = Table(env, cols, rows, "float64"), CodeTable(env, codes, net.cards, rows)
    short = Table(env, [c[:299] for c in map(np.ascontiguousarray, cols)], 299, "float64")
    narrow = Table(env, cols[:2], rows, "float64")
    wrong_cards = CodeTable(env, [codes[0], np.zeros(rows, dtype=np.int32)], [3, 3], rows)
    one_col = CodeTable(env, codes[:1], net.cards[:1], rows)
    foreign = CodeTable(env, codes, net.cards, rows, ctx=other)
    out, sums = np.zeros(rows), np.zeros(len(net.var))
    try:
        for bad_dt, bad_t in ((dt.handle, short.handle), (dt.handle, narrow.handle), (wrong_cards.handle, t.handle), (one_col.handle, t.handle),
                              (foreign.handle, t.handle), (None, t.handle), (dt.handle, None)):
            assert lib.pbn_clgnet_logl(g.handle, bad_dt, bad_t, _lib.dptr(out)) == INVALID
            assert lib.pbn_clgnet_slogl(g.handle, bad_dt, bad_t, _lib.dptr(sums)) == INVALID
        assert lib.pbn_clgnet_logl(None, dt.handle, t.handle, _lib.dptr(out)) == INVALID
        assert lib.pbn_clgnet_logl(g.handle, dt.handle, t.handle, None) == INVALID
        assert lib.pbn_clgnet_slogl(g.handle, dt.handle, t.handle, None) == INVALID
        assert g.stats() == (0, 0)
        assert lib.pbn_clgnet_logl(g.handle, dt.handle, t.handle, _lib.dptr(out)) == 0       # and the good pair is served
        assert g.stats() == (1, rows)
    finally:
        g.close()
        for h in (t, dt, short, narrow, wrong_cards, one_col, foreign):
            h.close()
