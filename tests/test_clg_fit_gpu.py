"""GPU tier: BayesianNetwork.fit with the conditional linear Gaussian nodes fitted in one device pass (pybnesian_amd/clg_fit.py,
csrc/clg_fit.hip) through the public interface.  The comparator is the same network fitted under PBN_CLG_FIT=0 - the per-factor loop,
_DiscreteAdaptator.fit per node: the same configurations dropped, a served configuration's coefficients and variance within 1e-10
(max|beta - loop| / max|loop|, relative variance: the project's tolerance for a slice fit against a factor fitted alone), everything
the pass does not compute in floating point EQUAL - DiscreteFactor tables, plain LinearGaussianCPDs, HCKDE slices, a refitted
configuration, a node the pass leaves to the loop.

Reference routines: models/BayesianNetwork.hpp:960-994, factors/discrete/DiscreteAdaptator.hpp:201-276,
learning/parameters/mle_LinearGaussianCPD.hpp, learning/parameters/mle_DiscreteFactor.cpp:5-41."""
import numpy as np
import pandas as pd
import pytest

import test_clg_model_gpu as base

pytestmark = pytest.mark.gpu

TOL = 1e-10


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def modules(pbn):
    from pybnesian_amd import clg_fit, clg_model, discrete_model, gaussian_model

    return {"clg_fit": clg_fit, "discrete_model": discrete_model, "gaussian_model": gaussian_model, "clg_model": clg_model}


def sparse_frame(seed=1):
    """About 3 000 rows of test_clg_model_gpu.make_frame in which the configuration (D1 = c, D2 = u) keeps two rows: with z's two continuous
    parents that is a fit of infinite variance, which is dropped."""
    df = base.make_frame(3100, seed)
    rare = np.nonzero(((df["D1"] == "c") & (df["D2"] == "u")).to_numpy())[0]
    return df.drop(index=df.index[rare[2:]]).reset_index(drop=True)


def sparse_series(rows=3000, seed=2):
    """test_clg_model_gpu.make_series with a third state of D that two time steps take"""
    df = base.make_series(rows, seed)
    d = df["D"].cat.codes.to_numpy().copy()
    d[[700, 1900]] = 2
    df["D"] = pd.Categorical.from_codes(d, ["lo", "hi", "rare"])
    return df


def snapshot(modules):
    return {k: dict(m.counters) for k, m in modules.items()}


def fit_both(monkeypatch, modules, make, df):
    """(the network fitted in one pass, the network fitted by the loop, what the first fit added to clg_fit.counters); the other
    modules' counters move in neither fit, clg_fit's only in the first"""
    monkeypatch.delenv("PBN_CLG_FIT", raising=False)
    one = make()
    before = snapshot(modules)
    one.fit(df)
    after = snapshot(modules)
    took = {k: after["clg_fit"][k] - before["clg_fit"][k] for k in before["clg_fit"]}
    assert all(after[m] == before[m] for m in ("discrete_model", "gaussian_model", "clg_model"))
    monkeypatch.setenv("PBN_CLG_FIT", "0")
    loop = make()
    before = snapshot(modules)
    loop.fit(df)
    assert snapshot(modules) == before
    monkeypatch.delenv("PBN_CLG_FIT")
    assert one.fitted() and loop.fitted()
    return one, loop, took


def equal_lg(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a.beta, b.beta) and a.variance == b.variance
                                         and a.evidence() == b.evidence() and a.fitted() and b.fitted())


def compare_factor(pbn, f, g, exact=False):
    """f: fitted in one pass (or left to the loop by it), g: fitted by the loop.  Returns the number of configurations compared within
    1e-10 (0 for a factor that must be equal)."""
    assert type(f) is type(g) and f.variable() == g.variable() and f.evidence() == g.evidence() and f.fitted() and g.fitted()
    if isinstance(f, pbn.DiscreteFactor):
        assert f._categories == g._categories and f._cards == g._cards
        assert np.array_equal(f._logprob, g._logprob)
        return 0
    if isinstance(f, pbn.LinearGaussianCPD):
        assert equal_lg(f, g)
        return 0
    assert f._disc == g._disc and f._cont == g._cont and f._categories == g._categories and len(f._factors) == len(g._factors)
    assert [s is None for s in f._factors] == [s is None for s in g._factors]      # the same configurations dropped
    if isinstance(f, pbn.HCKDE):
        for s, t in zip(f._factors, g._factors):
            assert s is None or (s.num_instances() == t.num_instances() and np.array_equal(s.bandwidth, t.bandwidth))
        return 0
    compared = 0
    for s, t in zip(f._factors, g._factors):
        if s is None:
            continue
        assert type(s) is pbn.LinearGaussianCPD and s.fitted() and s.variable() == t.variable() and s.evidence() == t.evidence()
        assert isinstance(s.beta, np.ndarray) and s.beta.dtype == np.float64 and s.beta.shape == t.beta.shape and isinstance(s.variance, float)
        if exact:
            assert equal_lg(s, t)
            continue
        e_beta = np.max(np.abs(s.beta - t.beta)) / np.max(np.abs(t.beta))
        e_var = abs(s.variance - t.variance) / t.variance
        print(f"{f.variable()} | {f._disc}: beta {e_beta:.3g} variance {e_var:.3g}")
        assert e_beta <= TOL and e_var <= TOL, (f.variable(), s.beta, t.beta, s.variance, t.variance)
        compared += 1
    return compared


def compare_networks(pbn, one, loop, exact=()):
    return sum(compare_factor(pbn, one.cpd(n), loop.cpd(n), n in exact) for n in one.nodes())


def check_slogl(one, loop, df):
    per_node = [loop.cpd(n).logl(df) for n in loop.nodes()]
    a, b = one.slogl(df), loop.slogl(df)
    bound = base.sum_bound(per_node)
    print(f"slogl(train): one pass {a!r} loop {b!r} |difference| {abs(a - b):.3e} bound {bound:.3e}")
    assert np.isfinite(a) and abs(a - b) <= bound


def test_clg_network(pbn, modules, monkeypatch):
    """Fails without the one-pass fit: the module is missing."""
    df = sparse_frame()
    assert 2900 < len(df) < 3100
    one, loop, took = fit_both(monkeypatch, modules, lambda: pbn.CLGNetwork(base.NODES, base.ARCS, base.discrete_types(pbn)), df)
    # y | D1 (3 configurations) and z | D1, D2 (6, one of them dropped); D1 and D2 from the same code table; x and w by the loop
    assert took["calls"] == 1 and took["nodes_served"] == 2 and took["cells_fitted"] == 9 and took["cells_refitted"] == 0
    assert took["discrete_nodes_fitted"] == 2 and took["launches"] >= 3
    assert [s is None for s in one.cpd("z")._factors].count(True) == 1
    assert one.cpd("z").conditional_factor(pbn.Assignment({"D1": "c", "D2": "u"})) is None
    assert compare_networks(pbn, one, loop) == 3 + 5
    check_slogl(one, loop, df)
    # a second fit finds every factor fitted: no pass
    before = snapshot(modules)
    one.fit(df)
    assert snapshot(modules) == before


def test_float32_columns(pbn, modules, monkeypatch):
    df = sparse_frame(4).astype({c: "float32" for c in base.CONT})
    one, loop, took = fit_both(monkeypatch, modules, lambda: pbn.CLGNetwork(base.NODES, base.ARCS, base.discrete_types(pbn)), df)
    assert took["nodes_served"] == 2
    assert compare_networks(pbn, one, loop) == 3 + 5


def test_conditional_clg_network(pbn, modules, monkeypatch):
    df = sparse_frame(5)
    make = lambda: pbn.ConditionalCLGNetwork(base.CNODES, base.CINTERFACE, base.CARCS, base.discrete_types(pbn)[1:])
    one, loop, took = fit_both(monkeypatch, modules, make, df)
    assert took["calls"] == 1 and took["nodes_served"] == 2 and took["discrete_nodes_fitted"] == 1     # D1 and x are interface columns
    assert compare_networks(pbn, one, loop) == 3 + 5
    check_slogl(one, loop, df)


def test_dynamic_clg_network(pbn, modules, monkeypatch):
    df = sparse_series()

    def make():
        dbn = pbn.DynamicCLGNetwork(base.DVARS, 1)
        for s, t in (("D_t_1", "D_t_0"), ("D_t_0", "x_t_0"), ("x_t_1", "x_t_0"), ("x_t_0", "y_t_0"), ("D_t_1", "y_t_0")):
            dbn.transition_bn().add_arc(s, t)
        return dbn

    one, loop, took = fit_both(monkeypatch, modules, make, df)
    # the transition network's x_t_0 | D_t_0 and y_t_0 | D_t_1; the static network has no arc, so no served node and no pass
    assert took["calls"] == 1 and took["nodes_served"] == 2 and took["discrete_nodes_fitted"] == 1
    assert compare_networks(pbn, one.static_bn(), loop.static_bn()) == 0
    compared = compare_networks(pbn, one.transition_bn(), loop.transition_bn())
    assert compared == 4      # two states of D with rows enough, in both nodes; the rare one is dropped
    for n in ("x_t_0", "y_t_0"):
        assert one.transition_bn().cpd(n)._factors[2] is None
    # the static networks are equal, so the two fits differ in the transition network alone: its slogl over its own training table
    from pybnesian_amd.dataset import as_record_batch
    from pybnesian_amd.dynamic import transition_table

    check_slogl(one.transition_bn(), loop.transition_bn(), transition_table(as_record_batch(df), 1))
    assert np.isfinite(one.slogl(df)) and np.isfinite(loop.slogl(df))


def test_semiparametric_network_with_an_hckde_node(pbn, modules, monkeypatch):
    df = sparse_frame(6)[["D1", "x", "y", "z"]]
    make = lambda: pbn.SemiparametricBN(["D1", "x", "y", "z"], [("D1", "y"), ("x", "y"), ("D1", "z"), ("y", "z")],
                                        [("D1", pbn.DiscreteFactorType()), ("y", pbn.CKDEType())])
    one, loop, took = fit_both(monkeypatch, modules, make, df)
    assert type(one.cpd("y")) is pbn.HCKDE and type(one.cpd("z")) is pbn.CLinearGaussianCPD
    assert took["calls"] == 1 and took["nodes_served"] == 1 and took["cells_fitted"] == 3 and took["discrete_nodes_fitted"] == 1
    assert compare_networks(pbn, one, loop) == 3      # z's configurations; y's slices are the loop's
    check_slogl(one, loop, df)


def test_a_nearly_collinear_configuration_is_refitted_by_the_loop(pbn, modules, monkeypatch):
    rng = np.random.default_rng(9)
    n = 3000
    d = rng.integers(0, 2, size=n)
    a, b = rng.normal(size=n), rng.normal(size=n)
    c = np.where(d == 1, a + 1e-7 * rng.normal(size=n), rng.normal(size=n))      # configuration 1: c is a copy of a up to 1e-7
    y = 1.0 + a - 0.5 * b + 0.25 * c + 0.3 * rng.normal(size=n)
    df = pd.DataFrame({"D": pd.Categorical.from_codes(d, ["p", "q"]), "a": a, "b": b, "c": c, "y": y})
    make = lambda: pbn.CLGNetwork(["D", "a", "b", "c", "y"], [("D", "y"), ("a", "y"), ("b", "y"), ("c", "y")], [("D", pbn.DiscreteFactorType())])
    one, loop, took = fit_both(monkeypatch, modules, make, df)
    assert took["nodes_served"] == 1 and took["cells_fitted"] == 1 and took["cells_refitted"] == 1
    assert equal_lg(one.cpd("y")._factors[1], loop.cpd("y")._factors[1]) and one.cpd("y")._factors[1] is not None
    assert compare_networks(pbn, one, loop) == 2


def test_nulls_in_a_continuous_column_keep_the_loop_for_that_node(pbn, modules, monkeypatch):
    df = sparse_frame(7)
    df.loc[::7, "x"] = np.nan       # x: a parent of y and z, not of w
    df.loc[3::11, "D2"] = None      # nulls in a discrete parent are served
    make = lambda: pbn.CLGNetwork(base.NODES + ["v"], base.ARCS + [("D2", "v"), ("w", "v")], base.discrete_types(pbn))
    df["v"] = 0.5 * df["w"] + np.where(df["D2"] == "v", 1.0, -1.0) + 0.2 * np.random.default_rng(1).normal(size=len(df))
    one, loop, took = fit_both(monkeypatch, modules, make, df)
    assert took["calls"] == 1 and took["nodes_served"] == 1 and took["cells_fitted"] == 2       # v | D2 alone
    assert compare_networks(pbn, one, loop, exact=("y", "z")) == 2


def test_a_python_subclass_fits_itself(pbn, modules, monkeypatch):
    from pybnesian_amd.factors import CLinearGaussianCPD

    calls = []

    class Mine(CLinearGaussianCPD):
        def fit(self, df):
            calls.append(self.variable())
            super().fit(df)

    df = sparse_frame(8)

    def make():
        # (y's type is given: a node whose type fit() resolves from the data loses the factor it had)
        net = pbn.CLGNetwork(base.NODES, base.ARCS, base.discrete_types(pbn) + [("y", pbn.LinearGaussianCPDType())])
        net._cpds = {"y": Mine("y", ["D1", "x"])}     # an unfitted factor of the user's: fit() keeps it and calls its fit
        return net

    one, loop, took = fit_both(monkeypatch, modules, make, df)
    assert calls == ["y", "y"] and type(one.cpd("y")) is Mine
    assert took["nodes_served"] == 1      # z
    assert compare_networks(pbn, one, loop, exact=("y",)) == 5


def test_an_integer_evidence_column_raises_the_loops_error(pbn, modules, monkeypatch):
    df = sparse_frame(9)
    df["x"] = (df["x"] * 10).astype("int64")
    messages = []
    for switch in (None, "0"):
        if switch is None:
            monkeypatch.delenv("PBN_CLG_FIT", raising=False)
        else:
            monkeypatch.setenv("PBN_CLG_FIT", switch)
        net = pbn.ConditionalCLGNetwork(["y", "z"], ["D1", "x"], [("D1", "y"), ("x", "y"), ("D1", "z")])
        with pytest.raises(ValueError) as err:
            net.fit(df)
        messages.append(str(err.value))
        assert not net.fitted()
    # _DiscreteAdaptator._split's message, from the loop, both times (z | D1 was served the first time: the decision is per node)
    assert messages[0] == messages[1] and "Non valid data type for variable x" in messages[0]
