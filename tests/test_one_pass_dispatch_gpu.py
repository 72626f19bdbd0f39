"""GPU tier: which one-pass evaluation a network takes (network_pass.one_pass behind BayesianNetwork.logl / slogl).  Three tiny fitted
networks - all-DiscreteFactor, all-LinearGaussianCPD and CLG - over 1 025 rows, one full 1 024-row tile and a one-row tail: with
every switch on only the network's own module's counters move; with its own switch off no module's move - an all-discrete or
all-Gaussian network does not fall into the CLG pass - and the per-factor loop gives the same rows.  The sums are the same for the
discrete and the Gaussian network; the CLG network's are held to test_clg_model_gpu's bound (two summation orders of the same terms).
The discrete network is evaluated on its 600 fitted rows, repeated up to 1 025: every configuration evaluated was seen in the fit, so
every CPT cell met is finite and the sum is a finite number on both paths - on an independent table of this generator the sum is
-inf on both, and the equality would say nothing.

The data, the fitting and that bound are those of test_discrete_model_gpu, test_gaussian_model_gpu and test_clg_model_gpu."""
import numpy as np
import pandas as pd
import pytest
from test_clg_model_gpu import discrete_types, sum_bound
from test_clg_model_gpu import make_frame as clg_frame
from test_discrete_model_gpu import frame as discrete_frame
from test_gaussian_model_gpu import make_frame as gaussian_frame

pytestmark = pytest.mark.gpu

ROWS = 1025
SWITCH = {"discrete": "PBN_DISCRETE_MODEL", "gaussian": "PBN_GAUSSIAN_MODEL", "clg": "PBN_CLG_MODEL"}


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def modules(pbn):
    from pybnesian_amd import clg_model, discrete_model, gaussian_model

    return {"discrete": discrete_model, "gaussian": gaussian_model, "clg": clg_model}


@pytest.fixture(scope="module")
def networks(pbn):
    """kind -> (the fitted network, the table it is evaluated on)"""
    discrete = pbn.DiscreteBN(["a", "b", "c", "d"], [("a", "b"), ("a", "c"), ("b", "c"), ("c", "d")])
    fitted_rows = discrete_frame(600, 11, False)
    discrete.fit(fitted_rows)
    discrete_rows = pd.concat([fitted_rows, fitted_rows.iloc[:ROWS - 600]], ignore_index=True)
    gaussian = pbn.GaussianNetwork(["d", "b", "a", "c"], [("a", "b"), ("a", "c"), ("b", "d"), ("c", "d")])
    gaussian.fit(gaussian_frame(600, 1))
    clg = pbn.CLGNetwork(["y", "D2", "x", "D1"], [("D1", "D2"), ("D1", "y"), ("x", "y")], discrete_types(pbn))
    clg.fit(clg_frame(600, 1))
    return {"discrete": (discrete, discrete_rows), "gaussian": (gaussian, gaussian_frame(ROWS, 2)), "clg": (clg, clg_frame(ROWS, 3))}


def snapshot(modules):
    return {k: dict(m.counters) for k, m in modules.items()}


@pytest.mark.parametrize("kind", ["discrete", "gaussian", "clg"])
def test_a_network_takes_its_own_pass_and_no_other(pbn, modules, networks, monkeypatch, kind):
    model, df = networks[kind]
    for name in SWITCH.values():
        monkeypatch.delenv(name, raising=False)
    before = snapshot(modules)
    on = model.logl(df), model.slogl(df)
    after = snapshot(modules)
    for k in modules:
        if k != kind:
            assert after[k] == before[k], k                      # the other two passes created nothing and launched nothing
    created = {"discrete": "dnet_created", "gaussian": "gnet_created", "clg": "clgnet_created"}[kind]
    assert after[kind][created] == before[kind][created] + 2   # one handle for logl, one for slogl
    assert after[kind]["rows_evaluated"] > before[kind]["rows_evaluated"]

    monkeypatch.setenv(SWITCH[kind], "0")                        # its own switch off, the other two on
    off = model.logl(df), model.slogl(df)
    assert snapshot(modules) == after                            # the per-factor loop: no pass took it instead
    assert on[0].shape == (ROWS,) and on[0].dtype == np.float64
    assert np.array_equal(on[0], off[0], equal_nan=True)
    print(f"{kind}: slogl one pass {on[1]!r} loop {off[1]!r} |difference| {abs(on[1] - off[1]):.3e}")
    if kind == "clg":
        bound = sum_bound([model.cpd(n).logl(df) for n in model.nodes()])
        print(f"clg: bound {bound:.3e}")
        assert abs(on[1] - off[1]) <= bound
    else:
        assert np.isfinite(off[1])
        # Exact, as for the Gaussian network.  For the discrete network this holds for THIS table, not by construction: the pass sums
        # count x logprob over the cells, the loop sums per row ("Not pinned"), and on other tables of this size the
        # two were seen one ulp apart.  A failure here by an ulp is that, not a wrong dispatch; a wrong dispatch moves the counters above.
        assert on[1] == off[1]
