"""GPU tier: networks of DiscreteFactors and (C)LinearGaussianCPDs evaluated in one device pass (pybnesian_amd/clg_model.py,
csrc/clg_model.hip) through the public interface.  The comparator is the same fitted model under PBN_CLG_MODEL=0 - the per-factor loop
of BayesianNetwork.logl / slogl and DynamicBayesianNetwork.logl / slogl: rows EQUAL (NaN positions included); sums within the
worst-case bound of any fp64 summation order, (n - 1) u sum|v_i| / (1 - (n - 1) u) per node with u = 2^-53 over the node's non-NaN
rows v_i, added over the nodes (the device sums 256-row trees, the loop sums per configuration: two orders of the same terms).

Reference routines: models/BayesianNetwork.hpp:997-1022, models/DynamicBayesianNetwork.cpp:71-151,
factors/discrete/DiscreteAdaptator.hpp:327-348, factors/discrete/DiscreteFactor.cpp:91-171,
factors/continuous/LinearGaussianCPD.cpp:92-149."""
import math

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

CONT = ["x", "y", "z", "w"]
NODES = ["z", "D2", "w", "x", "D1", "y"]                      # node order differs from column order, the kinds interleaved
ARCS = [("D1", "D2"), ("D1", "y"), ("x", "y"), ("D1", "z"), ("D2", "z"), ("x", "z"), ("y", "z"), ("y", "w")]
# x: no parents; w: a continuous parent only; y: one discrete parent; z: two discrete parents
CNODES, CINTERFACE = ["z", "y", "D2"], ["D1", "x"]            # D1, x: columns without a node
CARCS = [("D1", "D2"), ("D1", "y"), ("x", "y"), ("D1", "z"), ("D2", "z"), ("y", "z")]
DVARS = ["D", "x", "y"]
U = 2.0 ** -53


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def cm():
    from pybnesian_amd import clg_model

    return clg_model


def make_frame(rows, seed, dtype="float64"):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 3, size=rows)
    d2 = (rng.random(rows) < np.array([0.3, 0.5, 0.8])[d1]).astype(int)
    x = rng.normal(size=rows)
    y = np.array([-1.0, 0.5, 2.0])[d1] + np.array([0.5, -0.7, 1.2])[d1] * x + rng.normal(size=rows) * np.array([0.5, 1.0, 1.5])[d1]
    z = 0.3 * x - 0.6 * y + np.array([0.0, 1.0])[d2] * (1 + d1) + 0.8 * rng.normal(size=rows)
    w = 1.5 - 0.4 * y + 0.3 * rng.normal(size=rows)
    df = pd.DataFrame({"D1": pd.Categorical.from_codes(d1, ["a", "b", "c"]), "D2": pd.Categorical.from_codes(d2, ["u", "v"]),
                       "x": x, "y": y, "z": z, "w": w})
    return df.astype({c: dtype for c in CONT})


def discrete_types(pbn):
    """(given, not left to the data: a discrete child is typed before its parent in this node order)"""
    return [("D1", pbn.DiscreteFactorType()), ("D2", pbn.DiscreteFactorType())]


def make_series(rows, seed):
    rng = np.random.default_rng(seed)
    d = np.zeros(rows, dtype=int)
    x, y = np.zeros(rows), np.zeros(rows)
    for i in range(1, rows):
        d[i] = d[i - 1] if rng.random() < 0.8 else 1 - d[i - 1]
        x[i] = 0.6 * x[i - 1] + (1.0 if d[i] else -1.0) + 0.5 * rng.normal()
        y[i] = 0.5 * x[i] + (0.3 if d[i] else 1.0) * rng.normal()
    return pd.DataFrame({"D": pd.Categorical.from_codes(d, ["lo", "hi"]), "x": x, "y": y})


@pytest.fixture(scope="module")
def models(pbn):
    """Each network fitted once, on float64 data (a LinearGaussianCPD's parameters are doubles whatever the table's type)."""
    train = make_frame(3000, 1)
    clg = pbn.CLGNetwork(NODES, ARCS, discrete_types(pbn))
    ccl = pbn.ConditionalCLGNetwork(CNODES, CINTERFACE, CARCS, discrete_types(pbn)[1:])
    clg.fit(train)
    ccl.fit(train)
    dbn = pbn.DynamicCLGNetwork(DVARS, 1)
    for s, t in (("D_t_1", "D_t_0"), ("D_t_0", "x_t_0"), ("x_t_1", "x_t_0"), ("x_t_0", "y_t_0"), ("D_t_1", "y_t_0")):
        dbn.transition_bn().add_arc(s, t)
    dbn.fit(make_series(2000, 2))
    return {"clg": clg, "ccl": ccl, "dbn": dbn}


def both(monkeypatch, cm, model, df):
    """((logl, slogl) in one pass, (logl, slogl) of the per-factor loop, the counters the first pair moved)"""
    monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
    before = dict(cm.counters)
    one = (model.logl(df), model.slogl(df))
    took = {k: cm.counters[k] - before[k] for k in before}
    monkeypatch.setenv("PBN_CLG_MODEL", "0")
    before = dict(cm.counters)
    loop = (model.logl(df), model.slogl(df))
    assert cm.counters == before
    monkeypatch.delenv("PBN_CLG_MODEL")
    return one, loop, took


def sum_bound(rows_per_node):
    """The bound of the module docstring, added over the nodes, from the nodes' own per-row values."""
    total = 0.0
    for ll in rows_per_node:
        v = np.asarray(ll, dtype=np.float64)
        v = v[~np.isnan(v)]
        if v.size > 1:
            total += (v.size - 1) * U * math.fsum(np.abs(v)) / (1.0 - (v.size - 1) * U)
    return total


def check(one, loop, bound, rows):
    assert one[0].shape == (rows,) and one[0].dtype == np.float64
    assert np.array_equal(one[0], loop[0], equal_nan=True)
    print(f"slogl one pass {one[1]!r} loop {loop[1]!r} |difference| {abs(one[1] - loop[1]):.3e} bound {bound:.3e}")
    assert abs(one[1] - loop[1]) <= bound


def test_clg_network_equals_the_loop(pbn, cm, models, monkeypatch):
    """Fails without the one-pass path: the counters do not move."""
    model = models["clg"]
    types = {n: type(model.cpd(n)).__name__ for n in NODES}
    assert types == {"z": "CLinearGaussianCPD", "D2": "DiscreteFactor", "w": "LinearGaussianCPD", "x": "LinearGaussianCPD", "D1": "DiscreteFactor",
                     "y": "CLinearGaussianCPD"}
    assert sorted(model.cpd("z")._disc) == ["D1", "D2"] and sorted(model.cpd("z")._cont) == ["x", "y"]
    rows = 2049
    df = make_frame(rows, 3)
    one, loop, took = both(monkeypatch, cm, model, df)
    assert took == {"clgnet_created": 2, "launches": 2, "rows_evaluated": 2 * rows}     # one handle and one launch for logl, the same for slogl
    per_node = [model.cpd(n).logl(df) for n in NODES]
    check(one, loop, sum_bound(per_node), rows)
    assert not np.isnan(one[0]).any()
    # the network's rows are the factors' own, added in node order
    total = per_node[0]
    for ll in per_node[1:]:
        total = total + ll
    assert np.array_equal(one[0], total)


def test_nulls_in_a_continuous_column(pbn, cm, models, monkeypatch):
    model = models["clg"]
    df = make_frame(1025, 4)
    df.loc[np.random.default_rng(5).random(len(df)) < 0.2, "y"] = np.nan
    df.loc[0, "x"] = np.nan
    monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
    before = dict(cm.counters)
    got = model.logl(df)
    assert cm.counters["clgnet_created"] == before["clgnet_created"] + 1 and cm.counters["launches"] == before["launches"] + 1
    mid = dict(cm.counters)
    got_s = model.slogl(df)
    assert cm.counters == mid                                # slogl over such nulls: each factor sums its own family's valid rows - the loop
    monkeypatch.setenv("PBN_CLG_MODEL", "0")
    want, want_s = model.logl(df), model.slogl(df)
    assert np.isnan(want).any() and not np.isnan(want).all()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got, want, equal_nan=True)
    assert got_s == want_s


def test_nulls_in_a_discrete_column(pbn, cm, models, monkeypatch):
    model = models["clg"]
    rows = 1025
    df = make_frame(rows, 6)
    rng = np.random.default_rng(7)
    df.loc[rng.random(rows) < 0.15, "D1"] = np.nan
    df.loc[rng.random(rows) < 0.15, "D2"] = np.nan
    df.loc[rows - 1, "D2"] = np.nan
    one, loop, took = both(monkeypatch, cm, model, df)
    assert took["launches"] == 2                            # logl and slogl both on the device
    assert np.isnan(loop[0]).any() and not np.isnan(loop[0]).all()
    check(one, loop, sum_bound([model.cpd(n).logl(df) for n in NODES]), rows)


def outcome(fn):
    try:
        return ("value", fn())
    except Exception as e:   # noqa: BLE001 - the exception is what is compared
        return ("raised", type(e), str(e))


def same_outcome(a, b):
    if a[0] != b[0]:
        return False
    if a[0] == "raised":
        return a[1:] == b[1:]
    return np.array_equal(np.asarray(a[1]), np.asarray(b[1]), equal_nan=True)


@pytest.mark.parametrize("case", ["switched_off", "all_discrete", "all_lg", "hckde_node", "python_subclass"])
def test_staying_out(pbn, cm, models, monkeypatch, case):
    from pybnesian_amd.factors import CLinearGaussianCPD

    train, df = make_frame(800, 8), make_frame(500, 9)
    monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
    if case == "switched_off":
        model = models["clg"]
        monkeypatch.setenv("PBN_CLG_MODEL", "0")
    elif case == "all_discrete":
        model = pbn.CLGNetwork(["D2", "D1"], [("D1", "D2")], discrete_types(pbn))
        model.fit(train)
    elif case == "all_lg":
        model = pbn.CLGNetwork(["y", "x", "w"], [("x", "y"), ("y", "w")])
        model.fit(train)
    elif case == "hckde_node":
        model = pbn.SemiparametricBN(NODES, ARCS, discrete_types(pbn) + [("y", pbn.CKDEType())])
        model.fit(train)
        assert type(model.cpd("y")).__name__ == "HCKDE" and type(model.cpd("z")) is CLinearGaussianCPD
    else:
        class MyCPD(CLinearGaussianCPD):
            pass

        model = pbn.CLGNetwork(NODES, ARCS, discrete_types(pbn))
        model.fit(train)
        mine = MyCPD("y", model.cpd("y").evidence())
        mine.fit(train)
        model._cpds["y"] = mine
        assert model.fitted() and not cm.clg_factors(model)
    before = dict(cm.counters)
    got = outcome(lambda: model.logl(df)), outcome(lambda: model.slogl(df))
    assert cm.counters == before
    monkeypatch.setenv("PBN_CLG_MODEL", "0")
    want = outcome(lambda: model.logl(df)), outcome(lambda: model.slogl(df))
    assert got[0][0] == "value" and got[1][0] == "value"
    assert same_outcome(got[0], want[0]) and same_outcome(got[1], want[1])


def test_a_category_mismatch_raises_what_the_loop_raises(pbn, cm, models, monkeypatch):
    model = models["clg"]
    df = make_frame(300, 10)
    df["D2"] = pd.Categorical.from_codes(df["D2"].cat.codes, categories=["u", "other"])
    for knob in (None, "0"):
        if knob is None:
            monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
        else:
            monkeypatch.setenv("PBN_CLG_MODEL", knob)
        before = dict(cm.counters)
        for call in (model.logl, model.slogl):
            with pytest.raises(ValueError, match="Variable D2 does not contain the same categories"):
                call(df)
        assert cm.counters == before


def test_float32_table_is_served(pbn, cm, models, monkeypatch):
    model = models["clg"]
    rows = 1025
    df = make_frame(rows, 11, "float32")
    one, loop, took = both(monkeypatch, cm, model, df)
    assert took["launches"] == 2
    check(one, loop, sum_bound([model.cpd(n).logl(df) for n in NODES]), rows)


def test_conditional_network(pbn, cm, models, monkeypatch):
    model = models["ccl"]
    rows = 1025
    df = make_frame(rows, 12)
    one, loop, took = both(monkeypatch, cm, model, df)
    assert took["launches"] == 2
    check(one, loop, sum_bound([model.cpd(n).logl(df) for n in CNODES]), rows)


def test_dynamic_network_logl(pbn, cm, models, monkeypatch):
    dbn = models["dbn"]
    tr = dbn.transition_bn()
    assert cm.clg_factors(tr) and list(tr.nodes()) == ["D_t_0", "x_t_0", "y_t_0"]
    rows = 1025
    df = make_series(rows, 13)
    monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
    before = dict(cm.counters)
    got = dbn.logl(df)
    assert cm.counters["launches"] == before["launches"] + 1 and cm.counters["rows_evaluated"] == before["rows_evaluated"] + rows - 1
    monkeypatch.setenv("PBN_CLG_MODEL", "0")
    before = dict(cm.counters)
    want = dbn.logl(df)
    assert cm.counters == before
    assert got.shape == (rows,) and np.isfinite(want).all()
    assert np.array_equal(got, want)
