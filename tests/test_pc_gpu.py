"""GPU tier: PC end to end on device tables.  The batched search over the device batch of LinearCorrelation must return what the serial
search over the scalar host routine returns from the SAME handle - graph, separating sets with their p-values, serial test count - and
must really have run on the device."""
import numpy as np
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import _lib
from pybnesian_amd.constraint import pc_estimate_indices
from test_pc_cpu import linear_gaussian_table

pytestmark = pytest.mark.gpu


def same(a, b):
    assert a["arcs"] == b["arcs"] and a["edges"] == b["edges"]
    assert a["sepsets"] == b["sepsets"]            # sets AND p-values: the recorded value is the scalar routine's
    assert a["serial_tests"] == b["serial_tests"]


def test_pc_over_256_variables():
    """256 variables x 5 000 rows, about two parents per node, alpha 0.05, default options.

    Counted on the CPU with the host routine alone (np.cov of the same table, every p-value the batched search asks its batch function
    for): 2 820 271 p-values (2 296 419 tests in the serial search, separating sets up to size 4), of which NONE lies within
    PC_BAND * alpha of alpha - the nearest is 9.8e-6 * alpha away, 30 000 band widths.  So the cap below (band re-evaluations + eigenvalue
    redos <= 1e-3 of the device tests) has nothing to absorb on this input; it guards against the two mechanisms firing wholesale."""
    df = linear_gaussian_table(256, 5000, 2, 2.0)
    test = pbn.LinearCorrelation(df)
    names = test.variable_names()
    k_dev = _lib.load().pbn_lincor_batch_max_cond()
    serial = pc_estimate_indices(test, names, batched=False)
    assert serial["evaluated"] == serial["serial_tests"] and test.batch_stats() == (0, 0, 0)

    graph = pbn.PC().estimate(test)                 # the public path, default dispatch threshold
    dev, host, redone = test.batch_stats()
    assert dev > 0
    idx = {v: i for i, v in enumerate(names)}
    assert sorted((idx[a], idx[b]) for a, b in graph.arcs()) == serial["arcs"]
    assert sorted(tuple(sorted((idx[a], idx[b]))) for a, b in graph.edges()) == serial["edges"]
    default = pc_estimate_indices(test, names)
    same(default, serial)
    assert default["evaluated"] >= default["serial_tests"]

    # threshold 0, through a recording wrapper around the native batch function: every requested test with at most K_DEV conditioning
    # variables is the kernel's, the deeper ones loop on the host inside the same call
    test.set_batch_threshold(0)
    lib = _lib.load()
    seen = {"tests": 0, "deep": 0, "calls": 0}

    def forward(user, n, v1, v2, off, cond, out):
        k = np.diff(np.ctypeslib.as_array(off, shape=(n + 1,)))
        seen["tests"] += n
        seen["deep"] += int((k > k_dev).sum())
        seen["calls"] += 1
        lib.pbn_lincor_pvalue_batch(user, n, v1, v2, off, cond, out)

    before = test.batch_stats()
    forced = pc_estimate_indices(test, names, batched=_lib.CI_BATCH_FN(forward))
    same(forced, serial)
    dev, host, redone = (a - b for a, b in zip(test.batch_stats(), before))
    print(f"serial tests {serial['serial_tests']}, evaluated {forced['evaluated']} in {seen['calls']} batches; device {dev}, host loop {host}, "
          f"eigenvalue redos {redone}, band re-evaluations {forced['band_redone']}; largest separating set "
          f"{max(len(s) for s, _ in serial['sepsets'].values())}")
    assert host == seen["deep"] and dev == seen["tests"] - seen["deep"] and dev > 0
    assert forced["band_redone"] + redone <= 1e-3 * dev


def test_defaults_and_sepsets_share_the_skeleton():
    df = linear_gaussian_table(64, 5000, 1, 2.0)
    test = pbn.LinearCorrelation(df)
    a = pbn.PC().estimate(test)
    b = pbn.PC().estimate(test, use_sepsets=True)
    skeleton = lambda g: {frozenset(p) for p in g.arcs() + g.edges()}
    assert skeleton(a) == skeleton(b) and len(skeleton(a)) > 60


def hybrid_table(rows, seed):
    import pandas as pd

    rng = np.random.default_rng(seed)
    a = rng.integers(0, 3, rows)
    b = (a + rng.integers(0, 2, rows)) % 3
    c = rng.integers(0, 2, rows)
    x = rng.normal(size=rows) + 0.8 * a
    y = 0.7 * x + rng.normal(size=rows) + 0.5 * c
    z = rng.normal(size=rows)
    cat = lambda v, k: pd.Categorical.from_codes(v, [f"l{i}" for i in range(k)])
    return pd.DataFrame({"a": cat(a, 3), "b": cat(b, 3), "c": cat(c, 2), "x": x, "y": y, "z": z})


def graphs_equal(test, names):
    serial = pc_estimate_indices(test, names, batched=False)
    batched = pc_estimate_indices(test, names)
    same(batched, serial)
    return serial


def test_mutual_information_and_chi_square():
    df = hybrid_table(4000, 0)
    mi = pbn.MutualInformation(df)
    res = graphs_equal(mi, mi.variable_names())
    assert res["arcs"] or res["edges"]
    chi = pbn.ChiSquare(df)
    res = graphs_equal(chi, ["a", "b", "c"])
    assert (0, 1) in res["edges"] + res["arcs"] or (1, 0) in res["arcs"]
    assert isinstance(pbn.PC().estimate(chi, nodes=["a", "b", "c"]), pbn.PartiallyDirectedGraph)


def test_rcot():
    df = linear_gaussian_table(6, 1500, 4, 1.5)
    t = pbn.RCoT(df, 3, 10, seed=3)
    graphs_equal(t, t.variable_names())


def test_dynamic_adaptor():
    df = linear_gaussian_table(4, 2000, 6, 1.0)
    dyn = pbn.DynamicLinearCorrelation(pbn.DynamicDataFrame(df, 1))
    g = pbn.PC().estimate(dyn.static_tests())
    assert isinstance(g, pbn.PartiallyDirectedGraph) and g.num_nodes() == len(dyn.static_tests().variable_names())
    g = pbn.PC().estimate(dyn.transition_tests())
    assert isinstance(g, pbn.PartiallyDirectedGraph)


CHAIN_COLLIDER = [(0, 1), (1, 2), (2, 3), (2, 4), (5, 4), (5, 6), (6, 7), (8, 7), (7, 9)]
RECOVERY_SEED = 0


def chain_collider_table(rows, seed):
    """0 -> 1 -> 2 -> 3, 2 -> 4 <- 5 -> 6 -> 7 <- 8, 7 -> 9 with weights 0.8 and unit noise."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    X = rng.normal(size=(rows, 10))
    for j in range(10):
        for s, t in CHAIN_COLLIDER:
            if t == j:
                X[:, j] += 0.8 * X[:, s]
    return pd.DataFrame(X, columns=[f"n{i}" for i in range(10)])


def test_recovery_of_a_chain_and_collider_design():
    """20 000 rows, alpha 0.01.  RECOVERY_SEED was chosen on the CPU so that the serial host search over the sample covariance returns the
    generating CPDAG exactly (a level-alpha test rejects a true independence now and then: exact recovery is a property of the input).
    The device run must return that same CPDAG, and a consistent extension of it fits as a Gaussian network."""
    df = chain_collider_table(20000, RECOVERY_SEED)
    names = list(df.columns)
    truth = pbn.Dag(names, [(names[s], names[t]) for s, t in CHAIN_COLLIDER]).to_pdag()
    assert truth.num_edges() == 4 and truth.num_arcs() == 5
    host = pbn.LinearCorrelation.from_covariance(names, np.cov(df.to_numpy(), rowvar=False), len(df))
    assert pbn.PC().estimate(host, alpha=0.01) == truth
    test = pbn.LinearCorrelation(df)
    test.set_batch_threshold(0)
    got = pbn.PC().estimate(test, alpha=0.01)
    assert test.batch_stats()[0] > 0
    assert got == truth
    dag = got.to_dag()
    bn = pbn.GaussianNetwork(dag.nodes(), dag.arcs())
    bn.fit(df)
    assert np.isfinite(bn.slogl(df))
