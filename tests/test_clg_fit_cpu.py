"""CPU tier: the host side of the one-pass fit of conditional linear Gaussian nodes (pybnesian_amd/clg_fit.py) - the plan of hand-made
families (strides, offsets, caps), which nodes a call would serve, and the switch - without a device and without the library."""
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest


@pytest.fixture(scope="module")
def cf():
    from pybnesian_amd import clg_fit

    return clg_fit


def test_plan_of_hand_made_families(cf):
    """Fails without the module."""
    cards = {"A": 3, "B": 2, "C": 4}
    families = [("y", ["A", "B"], ["x"]),       # 6 configurations, D = 2
                ("A", ["B"], None),             # a discrete node: 6 cells
                ("z", ["C"], []),               # 4 configurations, D = 1
                ("x", ["B", "C", "A"], ["z", "y", "w"])]   # 24 configurations, D = 4; x is a parent above and the variable here
    p = cf.build_plan(families, cards)
    assert p.served == [True, True, True, True]
    assert p.dcolumns == ["A", "B", "C"] and p.cardinality == [3, 2, 4]      # numbered in order of first use
    assert p.ccolumns == ["y", "x", "z", "w"]
    assert p.nodes == [0, 2, 3] and p.var == [0, 2, 1]
    assert p.dpar_off == [0, 2, 3, 6] and p.dparents == [0, 1, 2, 1, 2, 0]
    assert p.cpar_off == [0, 1, 1, 4] and p.cparents == [1, 2, 0, 3]
    assert p.strides == [[1, 3], [1], [1, 2, 8]] and p.configs == [6, 4, 24]  # the first parent fastest
    assert p.cell_off == [0, 6, 10, 34]
    assert p.param_off == [0, 6 * 3, 6 * 3 + 4 * 2, 6 * 3 + 4 * 2 + 24 * 5]   # p + 2 doubles a cell
    d = p.discrete
    assert d.nodes == [1] and d.var == [0] and d.par_off == [0, 1] and d.parents == [1] and d.cpt_off == [0, 6]


def test_caps_are_per_family(cf):
    cards = {f"D{i}": 2 for i in range(9)}
    cards.update(W=256, V=257, Z=0)
    cont = [f"x{i}" for i in range(8)]
    ok = lambda fam: cf.within_caps(fam, cards)
    assert cf.MAX_CONFIGS == 256 and cf.MAX_FAMILY == 8 and cf.MAX_DISCRETE_PARENTS == 7
    assert ok(("y", ["D0"], cont[:7])) and not ok(("y", ["D0"], cont))                         # D <= 8
    assert ok(("y", [f"D{i}" for i in range(7)], [])) and not ok(("y", [f"D{i}" for i in range(8)], []))
    assert not ok(("y", [], ["x0"]))                                                            # no discrete parent: the loop's single factor
    assert ok(("y", ["W"], [])) and not ok(("y", ["V"], [])) and not ok(("y", ["W", "D0"], []))   # configurations up to the cap
    assert not ok(("y", ["D0", "D0"], [])) and not ok(("y", ["Z"], []))
    assert ok(("D0", [f"D{i}" for i in range(1, 8)], None)) and not ok(("D0", [f"D{i}" for i in range(1, 9)], None))
    # a family beyond the caps takes no part in the plan, the others are numbered without it
    p = cf.build_plan([("y", ["V"], ["x0"]), ("z", ["D1"], ["x1"]), ("D2", ["D1"], None)], cards)
    assert p.served == [False, True, True]
    assert p.dcolumns == ["D1", "D2"] and p.ccolumns == ["z", "x1"] and p.nodes == [1] and p.discrete.nodes == [2]
    assert p.cell_off == [0, 2] and p.param_off == [0, 6]


def frame(rows=40, seed=0):
    rng = np.random.default_rng(seed)
    df = pd.DataFrame({"A": pd.Categorical.from_codes(rng.integers(0, 3, rows), ["a", "b", "c"]),
                       "B": pd.Categorical.from_codes(rng.integers(0, 2, rows), ["u", "v"]),
                       "x": rng.normal(size=rows), "y": rng.normal(size=rows), "z": rng.normal(size=rows),
                       "f": rng.normal(size=rows).astype(np.float32), "k": rng.integers(0, 5, rows)})
    df.loc[3, "z"] = np.nan
    return pa.RecordBatch.from_pandas(df, preserve_index=False)


def model_of(factors):
    return SimpleNamespace(_cpds={f.variable(): f for f in factors}, _nodes=[f.variable() for f in factors])


def served(cf, factors, rb):
    model = model_of(factors)
    planned = cf.plan_nodes(model, rb, list(model._nodes))
    if planned is None:
        return None
    plan, families, names = planned
    return sorted(n for n, s in zip(names, plan.served) if s)


def test_which_nodes_a_call_serves(cf):
    from pybnesian_amd.factors import HCKDE, CLinearGaussianCPD, DiscreteFactor, LinearGaussianCPD

    class Mine(CLinearGaussianCPD):
        pass

    rb = frame()
    clg = CLinearGaussianCPD
    assert served(cf, [clg("y", ["A", "x"]), DiscreteFactor("B", ["A"]), LinearGaussianCPD("x", [])], rb) == ["B", "y"]
    # nothing to serve without a CLinearGaussianCPD that qualifies: the discrete nodes alone do not make a pass
    assert served(cf, [DiscreteFactor("B", ["A"]), LinearGaussianCPD("x", [])], rb) is None
    assert served(cf, [Mine("y", ["A", "x"]), HCKDE("x", ["A"]), clg("f", [])], rb) is None            # a subclass, an HCKDE, no discrete parent
    assert served(cf, [clg("y", ["A", "z"])], rb) is None                                              # nulls in a continuous parent
    assert served(cf, [clg("z", ["A"])], rb) is None                                                   # ... in the variable
    assert served(cf, [clg("y", ["A", "f"])], rb) is None                                              # float64 and float32 in one family
    assert served(cf, [clg("y", ["A", "k"])], rb) is None                                              # an integer column: the loop raises
    assert served(cf, [clg("y", ["A", "missing"])], rb) is None and served(cf, [clg("missing", ["A"])], rb) is None
    # per node: the one that qualifies is served beside those that do not
    assert served(cf, [clg("y", ["A", "z"]), clg("x", ["B", "A", "y"]), Mine("f", ["A"])], rb) == ["x"]
    # one float type a call: the first served node's
    assert served(cf, [clg("y", ["A", "x"]), clg("f", ["B"])], rb) == ["y"]
    # a discrete node whose column is not categorical stays with the loop (which raises)
    assert served(cf, [clg("y", ["A"]), DiscreteFactor("B", ["k"])], rb) == ["y"]
    plan = cf.plan_nodes(model_of([clg("x", ["B", "A", "y"])]), rb, ["x"])[0]
    assert plan.dcolumns == ["B", "A"] and plan.ccolumns == ["x", "y"] and plan.strides == [[1, 2]] and plan.configs == [6]


def test_a_first_row_that_is_not_finite_keeps_the_loop(cf):
    """the first row of a column is the pass's pilot shift: a non-null NaN or inf there would reach every configuration"""
    from pybnesian_amd.factors import CLinearGaussianCPD as clg

    for bad in (np.nan, np.inf):
        rb = frame()
        cols = {name: rb.column(i) for i, name in enumerate(rb.schema.names)}
        x = cols["x"].to_numpy().copy()
        x[0] = bad
        cols["x"] = pa.array(x)                      # non-null: arrow counts no null for a NaN given as a value
        assert cols["x"].null_count == 0
        rb = pa.RecordBatch.from_arrays(list(cols.values()), names=list(cols))
        assert served(cf, [clg("y", ["A", "x"])], rb) is None and served(cf, [clg("x", ["B"])], rb) is None
        assert served(cf, [clg("y", ["A"]), clg("x", ["B"])], rb) == ["y"]
    x = frame().column(2).to_numpy().copy()
    x[5] = np.nan                                    # elsewhere: the rows of one configuration, as in the loop
    rb = frame()
    rb = rb.set_column(2, "x", pa.array(x))
    assert served(cf, [clg("y", ["A", "x"])], rb) == ["y"]


def test_the_chunk_records_of_a_call_are_bounded(cf, monkeypatch):
    """pbn_clg_fit takes chunks x cells x S1 doubles of device memory; nodes beyond MAX_RECORD_BYTES in one call keep the loop"""
    from pybnesian_amd.factors import CLinearGaussianCPD as clg

    assert cf.MAX_CHUNKS == 512 and cf.TILE_ROWS == 1024
    assert cf.record_bytes(6, 2, 0) == 0 and cf.record_bytes(6, 2, 1) == 8 * 6 * 6 and cf.record_bytes(6, 2, 1024) == 8 * 6 * 6
    assert cf.record_bytes(1, 1, 1025) == 8 * 2 * 3 and cf.record_bytes(1, 1, 512 * 1024) == 8 * 512 * 3
    assert cf.record_bytes(1, 1, 512 * 1024 + 1) == 8 * 257 * 3         # 513 tiles, 2 a chunk: 257 chunks
    assert cf.record_bytes(137, 4, 10 ** 6) == 8 * 489 * 137 * 15       # 977 tiles, 2 a chunk: 489 chunks
    assert cf.record_bytes(256, 8, 10 ** 9) == 8 * 512 * 256 * 45 < cf.MAX_RECORD_BYTES   # one node at the caps always fits
    rb = frame()
    nodes = [clg("y", ["A", "x"]), clg("x", ["B", "A"]), clg("z2", ["B"])]
    rb = rb.append_column("z2", rb.column(3))
    assert served(cf, nodes, rb) == ["x", "y", "z2"]
    monkeypatch.setattr(cf, "MAX_RECORD_BYTES", cf.record_bytes(3, 2, 40) + cf.record_bytes(2, 1, 40))
    assert served(cf, nodes, rb) == ["y", "z2"]      # x (6 cells, D = 1) would pass the bound; the node after it still fits


def test_the_switch(cf, monkeypatch):
    from pybnesian_amd.factors import CLinearGaussianCPD, LinearGaussianCPD

    rb = frame()
    monkeypatch.delenv("PBN_CLG_FIT", raising=False)
    assert cf.enabled()
    monkeypatch.setenv("PBN_CLG_FIT", "1")
    assert cf.enabled()
    monkeypatch.setenv("PBN_CLG_FIT", "0")
    assert not cf.enabled()
    before = dict(cf.counters)
    model = model_of([CLinearGaussianCPD("y", ["A", "x"])])
    assert cf.fit_nodes(model, rb, ["y"]) == [] and not model._cpds["y"].fitted()      # off: nothing is touched, no device is asked for
    monkeypatch.delenv("PBN_CLG_FIT")
    model = model_of([LinearGaussianCPD("y", ["x"])])
    assert cf.fit_nodes(model, rb, ["y"]) == [] and cf.fit_nodes(model, rb, []) == []  # on, nothing to serve: no device either
    assert dict(cf.counters) == before
    assert set(cf.counters) == {"calls", "launches", "nodes_served", "cells_fitted", "cells_refitted", "discrete_nodes_fitted"}
