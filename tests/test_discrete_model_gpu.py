"""GPU tier: BayesianNetwork.fit / logl / slogl of networks whose factors are all DiscreteFactor, device path
(PBN_DISCRETE_MODEL=1, the default: csrc/discrete_model.hip) against the per-factor loop (PBN_DISCRETE_MODEL=0) and the restatement.

Fitted CPTs and logl must be the same bits on both settings; slogl within the derived bound of the exact (math.fsum) value on both:
per node (cells_n + 1) 2^-53 sum |count x logprob|, for the total the sum of those plus (n_nodes - 1) 2^-53 sum_n |slogl_n|.

Reference routines: models/BayesianNetwork.hpp:960-994, factors/discrete/DiscreteFactor.cpp:34-171,
learning/parameters/mle_DiscreteFactor.cpp:5-41."""
import math
import os
import pickle
import sys

import numpy as np
import pandas as pd
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_model_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 3001   # above the 2 048-row tile of the logl kernel, no multiple of anything
CATS = {"a": ["a0", "a1"], "b": ["b0", "b1", "b2"], "c": ["c0", "c1", "c2", "c3"], "d": ["d0", "d1", "d2"], "e": ["e0", "e1"]}
ARCS = [("a", "b"), ("a", "c"), ("b", "c"), ("c", "d"), ("a", "d"), ("b", "d")]   # d has three parents


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


def frame(rows, seed, nulls):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, rows)
    b = (a + (rng.random(rows) < 0.3) * rng.integers(0, 3, rows)) % 3
    c = (a + 2 * b + (rng.random(rows) < 0.2) * rng.integers(0, 4, rows)) % 4
    d = (a + b + c + (rng.random(rows) < 0.4) * rng.integers(0, 3, rows)) % 3
    e = rng.integers(0, 2, rows)
    codes = {"a": a, "b": b, "c": c, "d": d, "e": e}
    if nulls:
        for name, share in (("b", 0.05), ("d", 0.03), ("e", 0.01)):
            codes[name] = np.where(rng.random(rows) < share, -1, codes[name])
        codes["a"][0] = -1
        codes["d"][-1] = -1
    return pd.DataFrame({n: pd.Categorical.from_codes(codes[n], categories=CATS[n]) for n in CATS})


@pytest.fixture(scope="module", params=[False, True], ids=["complete", "nulls"])
def data(request):
    return frame(ROWS, 11, request.param), frame(ROWS - 500, 12, request.param)


def with_knob(monkeypatch, value, fn):
    monkeypatch.setenv("PBN_DISCRETE_MODEL", value)
    try:
        return fn()
    finally:
        monkeypatch.delenv("PBN_DISCRETE_MODEL")


def codes_of(df, columns):
    return [df[c].cat.codes.to_numpy().astype(np.int32) for c in columns], [len(df[c].cat.categories) for c in columns]


def check_slogl(model, df, got):
    """`got` against the exact sum over the model's own fitted CPTs."""
    nodes = model.nodes()
    columns = list(df.columns)
    codes, cards = codes_of(df, columns)
    bound, values = 0.0, []
    for n in nodes:
        f = model.cpd(n)
        fam = (columns.index(n), [columns.index(e) for e in f.evidence()])
        value, magnitude, cells = R.slogl_exact(codes, cards, fam, f._logprob)
        values.append(value)
        if value != -math.inf:
            bound += R.slogl_bound(cells, magnitude)
    if -math.inf in values:
        assert got == -math.inf
        return
    want = math.fsum(values)
    bound += (len(nodes) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in values)
    print(f"slogl: |got - exact| = {abs(got - want):.3e} bound {bound:.3e}")
    assert abs(got - want) <= bound, (got, want, bound)


def check_fit_against_restatement(model, df):
    """Counts are integers and the CPT is two logarithms and a subtraction: the fitted table against the restatement's, each logarithm of
    either side within 4 ulp (the vector and scalar logs differ in their last bits), so 8 x 2^-52 (|log count| + |log sum|) + one rounding."""
    columns = list(df.columns)
    codes, cards = codes_of(df, columns)
    for n in model.nodes():
        f = model.cpd(n)
        fam = (columns.index(n), [columns.index(e) for e in f.evidence()])
        counts = R.joint_counts_fast(codes, cards, fam)
        want = R.logprob(counts, cards[fam[0]])
        got = np.asarray(f._logprob)
        assert got.shape == want.shape
        sums = np.repeat(counts.reshape(-1, cards[fam[0]]).sum(axis=1), cards[fam[0]])
        finite = np.isfinite(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(want))
        scale = np.abs(np.log(np.maximum(counts, 1))) + np.abs(np.log(np.maximum(sums, 1))) + np.abs(want, where=finite, out=np.zeros_like(want)) + 2.0
        assert np.all(np.abs(got[finite] - want[finite]) <= 8 * 2.0 ** -52 * scale[finite])


def both_settings(monkeypatch, make, train, test, fit=lambda m, df: m.fit(df)):
    from pybnesian_amd import discrete_model as dm

    before = dict(dm.counters)
    on = make()
    with_knob(monkeypatch, "1", lambda: fit(on, train))
    after_fit = dict(dm.counters)
    assert after_fit["dtable_created"] > before["dtable_created"] and after_fit["dnet_created"] == before["dnet_created"]
    off = make()
    with_knob(monkeypatch, "0", lambda: fit(off, train))
    assert dict(dm.counters) == after_fit   # with the knob off the Python layer creates no handle
    return on, off


def same_factors(on, off):
    assert on.fitted() and off.fitted()
    for n in on.nodes():
        f, g = on.cpd(n), off.cpd(n)
        assert type(f) is type(g) and f.evidence() == g.evidence()
        assert f._cards == g._cards and f._categories == g._categories and f.fitted() and g.fitted()
        assert f._logprob.dtype == g._logprob.dtype and np.array_equal(f._logprob, g._logprob, equal_nan=True), n
        assert np.array_equal(np.signbit(f._logprob), np.signbit(g._logprob))


def test_discrete_bn(pbn, data, monkeypatch):
    from pybnesian_amd import discrete_model as dm

    train, test = data
    on, off = both_settings(monkeypatch, lambda: pbn.DiscreteBN(list(CATS), ARCS), train, test)
    same_factors(on, off)
    check_fit_against_restatement(on, train)
    for df in (train, test):
        before = dict(dm.counters)
        ll_on = with_knob(monkeypatch, "1", lambda: on.logl(df))
        mid = dict(dm.counters)
        # pbn_dnet_stats: one launch evaluated every row
        assert mid["dnet_created"] == before["dnet_created"] + 1 and mid["logl_launches"] == before["logl_launches"] + 1
        assert mid["rows_evaluated"] == before["rows_evaluated"] + len(df)
        ll_off = with_knob(monkeypatch, "0", lambda: on.logl(df))
        assert dict(dm.counters) == mid
        assert ll_on.dtype == np.float64 and ll_on.shape == (len(df),)
        assert np.array_equal(ll_on, ll_off, equal_nan=True)
        assert np.isnan(ll_on).any() == bool(df.isna().any().any())
        check_slogl(on, df, with_knob(monkeypatch, "1", lambda: on.slogl(df)))
        check_slogl(on, df, with_knob(monkeypatch, "0", lambda: on.slogl(df)))
    assert np.isneginf(with_knob(monkeypatch, "1", lambda: on.logl(test))).any() == np.isneginf(with_knob(monkeypatch, "0", lambda: off.logl(test))).any()


def test_conditional_discrete_bn(pbn, data, monkeypatch):
    train, test = data
    make = lambda: pbn.ConditionalDiscreteBN(["c", "d"], ["a", "b"], [("a", "c"), ("b", "c"), ("c", "d"), ("a", "d")])
    on, off = both_settings(monkeypatch, make, train, test)
    same_factors(on, off)
    check_fit_against_restatement(on, train)
    ll_on = with_knob(monkeypatch, "1", lambda: on.logl(test))
    assert np.array_equal(ll_on, with_knob(monkeypatch, "0", lambda: on.logl(test)), equal_nan=True)
    check_slogl(on, test, with_knob(monkeypatch, "1", lambda: on.slogl(test)))
    check_slogl(on, test, with_knob(monkeypatch, "0", lambda: on.slogl(test)))


def test_homogeneous_bn_of_discrete_factors(pbn, data, monkeypatch):
    train, test = data
    on, off = both_settings(monkeypatch, lambda: pbn.HomogeneousBN(pbn.DiscreteFactorType(), list(CATS), ARCS), train, test)
    same_factors(on, off)
    assert np.array_equal(with_knob(monkeypatch, "1", lambda: on.logl(test)), with_knob(monkeypatch, "0", lambda: on.logl(test)), equal_nan=True)


def test_dynamic_discrete_bn(pbn, data, monkeypatch):
    train, test = data
    variables = ["a", "b", "c"]

    def make():
        dbn = pbn.DynamicDiscreteBN(variables, 1)
        dbn.static_bn().add_arc("a_t_1", "b_t_1")
        dbn.transition_bn().add_arc("a_t_1", "a_t_0")
        dbn.transition_bn().add_arc("a_t_0", "b_t_0")
        dbn.transition_bn().add_arc("c_t_1", "b_t_0")
        return dbn

    on, off = both_settings(monkeypatch, make, train[variables], test[variables])
    same_factors(on.static_bn(), off.static_bn())
    same_factors(on.transition_bn(), off.transition_bn())
    ll_on = with_knob(monkeypatch, "1", lambda: on.logl(test[variables]))
    ll_off = with_knob(monkeypatch, "0", lambda: off.logl(test[variables]))
    assert np.array_equal(ll_on, ll_off, equal_nan=True)
    assert with_knob(monkeypatch, "1", lambda: on.slogl(test[variables])) == with_knob(monkeypatch, "0", lambda: off.slogl(test[variables]))
    # the transition network evaluated as a network of its own takes the device path and keeps the per-factor bits
    from pybnesian_amd.dynamic import DynamicDataFrame

    tdf = DynamicDataFrame(test[variables], 1).transition_df()
    assert np.array_equal(with_knob(monkeypatch, "1", lambda: on.transition_bn().logl(tdf)),
                          with_knob(monkeypatch, "0", lambda: on.transition_bn().logl(tdf)), equal_nan=True)


def test_category_mismatch_is_still_a_value_error(pbn, data, monkeypatch):
    train, test = data
    model = pbn.DiscreteBN(list(CATS), ARCS)
    model.fit(train)
    other = test.copy()
    other["b"] = pd.Categorical.from_codes(test["b"].cat.codes, categories=["b0", "bX", "b2"])
    for knob in ("1", "0"):
        for call in (model.logl, model.slogl):
            with pytest.raises(ValueError, match="Variable b does not contain the same categories"):
                with_knob(monkeypatch, knob, lambda: call(other))


def test_a_clg_network_keeps_the_per_factor_loop(pbn, data, monkeypatch):
    from pybnesian_amd import discrete_model as dm

    train, test = data
    rng = np.random.default_rng(5)
    mixed = train[["a", "b"]].dropna().reset_index(drop=True)
    mixed["x"] = rng.normal(size=len(mixed)) + mixed["a"].cat.codes.to_numpy()
    before = dict(dm.counters)
    net = pbn.CLGNetwork(["a", "b", "x"], [("a", "b"), ("a", "x")])
    net.fit(mixed)
    assert np.all(np.isfinite(net.logl(mixed))) and np.isfinite(net.slogl(mixed))
    assert dict(dm.counters) == before


def test_a_python_subclass_of_the_factor_stays_out(pbn, data, monkeypatch):
    from pybnesian_amd import discrete_model as dm
    from pybnesian_amd.factors import DiscreteFactor

    class Mine(DiscreteFactor):
        pass

    train, test = data
    model = pbn.DiscreteBN(["a", "b"], [("a", "b")])
    model.fit(train)
    assert dm.all_discrete_factors(model)
    mine = Mine("b", ["a"])
    mine.fit(train)
    model._cpds["b"] = mine
    assert not dm.all_discrete_factors(model)
    before = dict(dm.counters)
    model.logl(test)
    assert dict(dm.counters) == before


def test_a_pickled_network_gives_the_same_logl(pbn, data):
    train, test = data
    model = pbn.DiscreteBN(list(CATS), ARCS)
    model.fit(train)
    model.include_cpd = True
    again = pickle.loads(pickle.dumps(model, protocol=2))
    assert again.fitted()
    assert np.array_equal(again.logl(test), model.logl(test), equal_nan=True)
    assert again.slogl(test) == model.slogl(test)
