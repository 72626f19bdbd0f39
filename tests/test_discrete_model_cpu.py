"""CPU tier: the restatement the device path of discrete networks is tested against (tests/discrete_model_restatement.py) on a
table computed by hand, and the pure-Python plan builder (pybnesian_amd/discrete_model.py build_plan) that turns a model into
the arrays of pbn_dtable_family_counts / pbn_dnet_create.

Reference routines: factors/discrete/discrete_indices.cpp:134-150, learning/parameters/mle_DiscreteFactor.cpp:5-41,
factors/discrete/DiscreteFactor.cpp:91-171, models/BayesianNetwork.hpp:960-994."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import discrete_model_restatement as R  # noqa: E402

# six rows, columns a (2 categories), b (3), c (2); row 3 has a null in b
A = np.array([0, 1, 1, 0, 1, 0], dtype=np.int32)
B = np.array([0, 2, 2, -1, 1, 0], dtype=np.int32)
C_ = np.array([1, 1, 0, 0, 1, 1], dtype=np.int32)
CODES, CARDS = [A, B, C_], [2, 3, 2]


def test_restatement_on_a_hand_computed_table():
    # P(a | b): rows 0, 5 -> (a0, b0); 4 -> (a1, b1); 1, 2 -> (a1, b2); row 3 dropped (null in b).  Cell = a + 2 b.
    counts = R.joint_counts(CODES, CARDS, (0, [1]))
    assert counts.tolist() == [2, 0, 0, 1, 0, 2]
    assert R.joint_counts_fast(CODES, CARDS, (0, [1])).tolist() == counts.tolist()
    # a alone keeps row 3: the null is in another family's variable
    assert R.joint_counts(CODES, CARDS, (0, [])).tolist() == [3, 3]
    # P(b | a, c) with the parents as given (a fastest after b): cell = b + 3 a + 6 c
    assert R.joint_counts(CODES, CARDS, (1, [0, 2])).tolist() == [0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 1, 1]
    # ... and given the other way round: cell = b + 3 c + 6 a
    assert R.joint_counts(CODES, CARDS, (1, [2, 0])).tolist() == [0, 0, 0, 2, 0, 0, 0, 0, 1, 0, 1, 1]
    lp = R.logprob(counts, 2)
    assert lp.tolist() == [0.0, -math.inf, -math.inf, 0.0, -math.inf, 0.0]
    # an unseen parent configuration is uniform
    lp_c = R.logprob(R.joint_counts(CODES, CARDS, (2, [1])), 2)   # c | b: b0 -> c1 twice; b1 -> c1; b2 -> c1, c0
    assert lp_c.tolist() == [-math.inf, 0.0, -math.inf, 0.0, -math.log(2.0), -math.log(2.0)]
    unseen = R.logprob(np.array([0, 0, 0, 3, 1, 2]), 3)
    assert unseen[:3].tolist() == [math.log(1.0 / 3)] * 3 and unseen[3:].tolist() == [math.log(3.0) - math.log(6.0), math.log(1.0) - math.log(6.0),
                                                                                       math.log(2.0) - math.log(6.0)]
    # the per-row gather: NaN on the row with the null, the cell's value elsewhere
    table = np.array([-0.25, -1.5, -0.75, -0.5, -2.0, -0.125])
    ll = R.row_logl(CODES, CARDS, (0, [1]), table)
    assert np.array_equal(ll, np.array([-0.25, -0.125, -0.125, np.nan, -0.5, -0.25]), equal_nan=True)
    # node-order sum: a | b then a alone
    both = R.network_logl(CODES, CARDS, [(0, [1]), (0, [])], [table, np.array([-1.0, -3.0])])
    assert np.array_equal(both, np.array([-1.25, -3.125, -3.125, np.nan, -3.5, -1.25]), equal_nan=True)
    exact, magnitude, cells = R.slogl_exact(CODES, CARDS, (0, [1]), table)
    assert (exact, magnitude, cells) == (-1.25, 1.25, 6)
    assert R.slogl_exact(CODES, CARDS, (0, [1]), np.array([0.0, -math.inf, 0.0, 0.0, 0.0, 0.0]))[0] == 0.0   # no row on the -inf cell
    assert R.slogl_exact(CODES, CARDS, (0, [1]), np.array([-math.inf, 0.0, 0.0, 0.0, 0.0, 0.0]))[0] == -math.inf


def test_plan_of_a_discrete_bn():
    import pybnesian_amd as pbn
    from pybnesian_amd import discrete_model as dm

    model = pbn.DiscreteBN(["a", "b", "c"], [("a", "b"), ("c", "b"), ("a", "c")])
    families = [(n, model.parents(n)) for n in model.nodes()]
    plan = dm.build_plan(families, {"a": 2, "b": 3, "c": 4})
    assert plan.within_caps
    assert plan.columns == ["a", "b", "c"] and plan.cardinality == [2, 3, 4]
    assert plan.var == [0, 1, 2]
    by_node = {n: [plan.columns[p] for p in plan.parents[plan.par_off[i]: plan.par_off[i + 1]]] for i, n in enumerate(model.nodes())}
    assert by_node == {"a": [], "b": model.parents("b"), "c": ["a"]}
    assert sorted(by_node["b"]) == ["a", "c"]
    assert plan.par_off == [0, 0, 2, 3] and plan.cpt_off == [0, 2, 2 + 24, 2 + 24 + 8]
    # the evidence order of a factor is the layout of its CPT: it is kept, not sorted
    plan = dm.build_plan([("b", ["c", "a"])], {"a": 2, "b": 3, "c": 4})
    assert plan.columns == ["b", "c", "a"] and plan.var == [0] and plan.parents == [1, 2] and plan.cardinality == [3, 4, 2]


def test_plan_of_a_conditional_discrete_bn():
    import pybnesian_amd as pbn
    from pybnesian_amd import discrete_model as dm

    model = pbn.ConditionalDiscreteBN(["x", "y"], ["i1", "i2"], [("i1", "x"), ("x", "y"), ("i2", "y")])
    families = [(n, model.parents(n)) for n in model.nodes()]
    plan = dm.build_plan(families, {"x": 2, "y": 5, "i1": 3, "i2": 4})
    assert plan.within_caps
    # the interface columns are columns of the table without a node
    assert len(plan.var) == 2 and sorted(plan.columns) == ["i1", "i2", "x", "y"]
    assert [plan.columns[v] for v in plan.var] == ["x", "y"]
    assert {plan.columns[p] for p in plan.parents} == {"i1", "i2", "x"}
    assert plan.cpt_off == [0, 6, 6 + 5 * 2 * 4]


def test_a_nine_variable_family_keeps_the_per_factor_loop():
    import pybnesian_amd as pbn
    from pybnesian_amd import discrete_model as dm

    nodes = [f"v{i}" for i in range(9)]
    model = pbn.DiscreteBN(nodes, [(p, "v8") for p in nodes[:8]])
    families = [(n, model.parents(n)) for n in model.nodes()]
    cards = {n: 2 for n in nodes}
    assert not dm.build_plan(families, cards).within_caps
    assert dm.build_plan(families[:8], cards).within_caps                       # the parentless nodes alone
    assert dm.build_plan([("v8", nodes[:7])], cards).within_caps                # eight variables: at the cap
    assert not dm.build_plan([("v0", ["v1"])], {"v0": 65536, "v1": 32768}).within_caps   # 2^31 cells
    assert dm.build_plan([("v0", ["v1"])], {"v0": 65536, "v1": 32767}).within_caps
    assert not dm.build_plan([("v0", [])], {"v0": 0}).within_caps               # a column without categories


def test_the_knob_is_read_per_call(monkeypatch):
    from pybnesian_amd import discrete_model as dm

    monkeypatch.delenv("PBN_DISCRETE_MODEL", raising=False)
    assert dm.enabled()
    monkeypatch.setenv("PBN_DISCRETE_MODEL", "0")
    assert not dm.enabled()
    monkeypatch.setenv("PBN_DISCRETE_MODEL", "1")
    assert dm.enabled()
