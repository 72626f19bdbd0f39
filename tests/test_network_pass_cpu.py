"""CPU tier: what the three one-pass network evaluations share (pybnesian_amd/network_pass.py) - the numbering of columns, the
float-type check of the arrow side, the scatter of the kept rows' values, and the dispatcher with the three passes replaced by
recording stubs.  No device and no library."""
import numpy as np
import pyarrow as pa
import pytest

from pybnesian_amd import clg_model as cm
from pybnesian_amd import discrete_model as dm
from pybnesian_amd import gaussian_model as gm
from pybnesian_amd import network_pass as npass


def test_columns_are_numbered_in_order_of_first_use():
    index = npass.FirstUse()
    assert [index[n] for n in ["b", "a", "z", "a", "c", "b"]] == [0, 1, 2, 1, 3, 0]
    assert list(index) == ["b", "a", "z", "c"]
    # a transition network: the interface columns (x_t_1, y_t_1, y_t_2) are numbered where they are first met and have no node
    index = npass.FirstUse()
    families = [("x_t_0", ["x_t_1", "y_t_1"]), ("y_t_0", ["x_t_0", "y_t_2"])]
    ids = [[index[n] for n in [v] + ev] for v, ev in families]
    columns = list(index)
    assert columns == ["x_t_0", "x_t_1", "y_t_1", "y_t_0", "y_t_2"]
    assert ids == [[0, 1, 2], [3, 0, 4]]
    # the three plans number their columns with it
    assert gm.build_plan(families).columns == columns
    assert dm.build_plan(families, {c: 2 for c in columns}).columns == columns
    plan = cm.build_plan([("x_t_0", ["D_t_1"], ["x_t_1"]), ("D_t_0", ["D_t_1", "E_t_2"], None)], {"D_t_0": 2, "D_t_1": 2, "E_t_2": 5})
    assert plan.dcolumns == ["D_t_1", "D_t_0", "E_t_2"] and plan.ccolumns == ["x_t_0", "x_t_1"]


def test_float_type_of_the_columns():
    f64, f32 = pa.array([0.5, 1.5]), pa.array([0.5, 1.5], type=pa.float32())
    rb = pa.RecordBatch.from_arrays([f64, f64, f32, f32, pa.array([1, 2])], names=["a", "b", "s", "t", "i"])
    assert npass.float_type(rb, ["a", "b"]) == pa.float64()
    assert npass.float_type(rb, ["t", "s"]) == pa.float32()
    assert npass.float_type(rb, ["a", "missing"]) is None      # a column that is not there
    assert npass.float_type(rb, ["a", "s"]) is None            # float64 beside float32
    assert npass.float_type(rb, ["i"]) is None                 # an integer column
    assert npass.float_type(rb, ["a", "i"]) is None


def test_has_nulls_looks_at_the_named_columns_only():
    rb = pa.RecordBatch.from_arrays([pa.array([0.5, None]), pa.array([0.5, 1.5])], names=["a", "b"])
    assert npass.has_nulls(rb, ["b", "a"]) and not npass.has_nulls(rb, ["b"])


def test_scatter_puts_the_kept_rows_back_and_nan_elsewhere():
    mask = np.array([True, False, True, True, False])
    got = npass.scatter_rows(np.array([1.5, -2.0, 3.25]), mask, 5)
    assert np.array_equal(got, np.array([1.5, np.nan, -2.0, 3.25, np.nan]), equal_nan=True)
    vals = np.array([1.0, 2.0])
    assert npass.scatter_rows(vals, None, 2) is vals             # no row was dropped: the values themselves


# ---- the dispatcher --------------------------------------------------------------------------------------------------------------------

MODULES = {"discrete": dm, "gaussian": gm, "clg": cm}
PREDICATE = {"discrete": "all_discrete_factors", "gaussian": "all_lg_factors", "clg": "clg_factors"}
SUMS = {"discrete": "network_slogl", "gaussian": "network_node_slogl", "clg": "network_node_slogl"}


@pytest.fixture
def stubs(monkeypatch):
    """Every pass switched on, its predicate true and its calls answering None, each recording that it was asked: `asked` lists
    (pass, call) in order.  A test sets state["off"], state["unfit"] (predicate false) and state["answers"][pass]."""
    state = {"asked": [], "off": set(), "unfit": set(), "answers": {}}
    for key, module in MODULES.items():
        def call(model, rb, key=key, which=None):
            state["asked"].append((key, which))
            return state["answers"].get(key)

        monkeypatch.setattr(module, "enabled", lambda key=key: key not in state["off"])
        monkeypatch.setattr(module, PREDICATE[key], lambda model, key=key: key not in state["unfit"])
        monkeypatch.setattr(module, "network_logl", lambda model, rb, call=call: call(model, rb, which="logl"))
        monkeypatch.setattr(module, SUMS[key], lambda model, rb, call=call: call(model, rb, which="sums"))
    return state


RB = pa.RecordBatch.from_arrays([pa.array([0.5])], names=["a"])


def test_the_passes_are_asked_in_order_and_none_falls_through_to_the_loop(stubs):
    assert npass.one_pass(object(), RB, "logl") is None                        # None: the caller runs the per-factor loop
    assert stubs["asked"] == [("discrete", "logl"), ("gaussian", "logl"), ("clg", "logl")]
    stubs["asked"].clear()
    assert npass.one_pass(object(), RB, "slogl") is None
    assert stubs["asked"] == [("discrete", "sums"), ("gaussian", "sums"), ("clg", "sums")]


def test_the_first_answer_is_taken(stubs):
    stubs["answers"] = {"gaussian": "from gaussian", "clg": "from clg"}
    assert npass.one_pass(object(), RB, "logl") == (npass.GAUSSIAN, "from gaussian", False)
    assert stubs["asked"] == [("discrete", "logl"), ("gaussian", "logl")]     # discrete answered None, clg was not reached
    stubs["answers"] = {"discrete": 0.0}                                        # an answer that is falsy is still an answer
    assert npass.one_pass(object(), RB, "slogl") == (npass.DISCRETE, 0.0, True)     # the discrete sums' call gives the total ...
    assert npass.one_pass(object(), RB, "logl") == (npass.DISCRETE, 0.0, False)     # ... its per-row call does not
    stubs["answers"] = {"clg": "nodes' sums"}
    assert npass.one_pass(object(), RB, "slogl") == (npass.CLG, "nodes' sums", False)


def test_a_pass_that_is_switched_off_or_does_not_fit_is_not_asked(stubs):
    stubs["off"] = {"discrete"}
    stubs["unfit"] = {"gaussian"}
    stubs["answers"] = {"discrete": "d", "gaussian": "g", "clg": "c"}
    assert npass.one_pass(object(), RB, "logl") == (npass.CLG, "c", False)
    assert stubs["asked"] == [("clg", "logl")]
    stubs["off"] = {"discrete", "gaussian", "clg"}
    stubs["asked"].clear()
    assert npass.one_pass(object(), RB, "logl") is None and stubs["asked"] == []


def test_a_dynamic_network_never_asks_the_discrete_pass(stubs):
    from pybnesian_amd.dynamic import DynamicBayesianNetwork, temporal_name

    class Transition:
        _nodes = [temporal_name("a", 0), temporal_name("b", 0)]

    dbn = DynamicBayesianNetwork.__new__(DynamicBayesianNetwork)
    dbn._variables, dbn._transition = ["a", "b"], Transition()
    stubs["answers"] = {"discrete": "d"}
    assert dbn._transition_in_one_pass(RB, "logl") is None
    assert dbn._transition_in_one_pass(RB, "slogl") is None
    assert stubs["asked"] == [("gaussian", "logl"), ("clg", "logl"), ("gaussian", "sums"), ("clg", "sums")]
    stubs["answers"] = {"discrete": "d", "clg": "c"}
    assert dbn._transition_in_one_pass(RB, "logl") == "c"
    # a transition network whose node order is not the variables' is not asked at all
    stubs["asked"].clear()
    dbn._variables = ["b", "a"]
    assert dbn._transition_in_one_pass(RB, "logl") is None and stubs["asked"] == []
