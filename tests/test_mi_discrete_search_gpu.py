"""GPU tier: PC, MMPC and MMHC over MutualInformation reach the device counts of pbn_mi_pvalue_batch (csrc/mi.hip) through
the batched callback, and learn what they learn with PBN_MI_DISCRETE_BATCH=0: the same graph, the same sepsets and p-values, the same
candidate sets, the same number of tests."""
import os

import numpy as np
import pandas as pd
import pytest

import pybnesian_amd as pbn
from pybnesian_amd.constraint import pc_estimate_indices
from pybnesian_amd.independences import mmpc_cpcs

from test_mi_discrete_batch_gpu import DEVICE, CACHED, Capture

pytestmark = pytest.mark.gpu


def discrete_frame(n, rows, seed, nulls):
    """n categorical columns of 2 ... 4 categories, each with up to two earlier parents; with `nulls`, 5 % null cells in three columns."""
    rng = np.random.default_rng(seed)
    cards = rng.integers(2, 5, n)
    cols = []
    for v in range(n):
        k = min(v, int(rng.integers(0, 3)))
        pa = sorted(rng.choice(v, k, replace=False)) if k else []
        cfg = np.zeros(rows, dtype=np.int64); m = 1
        for p in pa:
            cfg += cols[p] * m; m *= cards[p]
        cpt = rng.dirichlet(np.full(cards[v], 0.35), size=m)
        u = rng.random(rows)
        cols.append((u[:, None] > np.cumsum(cpt[cfg], axis=1)).sum(1).clip(0, cards[v] - 1))
    out = [c.copy() for c in cols]
    if nulls:
        for v in (1, 4, 7):
            out[v][rng.random(rows) < 0.05] = -1
    return pd.DataFrame({f"v{i}": pd.Categorical.from_codes(out[i], [f"l{j}" for j in range(int(cards[i]))]) for i in range(n)})


class switched_off:
    def __enter__(self):
        os.environ["PBN_MI_DISCRETE_BATCH"] = "0"

    def __exit__(self, *exc):
        del os.environ["PBN_MI_DISCRETE_BATCH"]


@pytest.fixture(scope="module")
def cap():
    with Capture() as c:
        yield c


@pytest.mark.parametrize("nulls", [False, True])
def test_pc_and_mmpc_on_a_discrete_table(cap, nulls):
    df = discrete_frame(12, 5000, 2, nulls)
    on = pbn.MutualInformation(df)
    on.set_batch_threshold(0)                       # every eligible test to the kernel, however few a call holds
    names = on.variable_names()
    cap.take()
    pc_on = pc_estimate_indices(on, names)
    calls = cap.take()
    dev, cached, grouped = on.batch_stats()
    assert dev > 0 and grouped == 0
    for call in calls:                              # every batched test is count-only here: none of them builds a grouping
        assert call["groups_after"] == call["groups_before"]
        assert all(r["where"] in (DEVICE, CACHED) for r in call["tests"])
    with switched_off():
        off = pbn.MutualInformation(df)
        pc_off = pc_estimate_indices(off, names)
        assert off.batch_stats()[0] == 0
    cap.take()                                      # (the capture is the library's, not a handle's: drop the calls of `off`)
    assert pc_on["arcs"] or pc_on["edges"]          # columns with parents: a skeleton that is not empty
    assert pc_on["arcs"] == pc_off["arcs"] and pc_on["edges"] == pc_off["edges"]
    assert pc_on["sepsets"] == pc_off["sepsets"]    # sets AND p-values
    assert pc_on["serial_tests"] == pc_off["serial_tests"]

    on = pbn.MutualInformation(df)
    on.set_batch_threshold(0)
    cpc_on = mmpc_cpcs(on, names, 0.05)
    calls = cap.take()
    assert on.batch_stats()[0] > 0 and on.batch_stats()[2] == 0
    assert all(call["groups_after"] == call["groups_before"] for call in calls)
    with switched_off():
        off = pbn.MutualInformation(df)
        cpc_off = mmpc_cpcs(off, names, 0.05)
        assert off.batch_stats()[0] == 0
    assert cpc_on == cpc_off and any(cpc_on[0])     # the sets of every node and the number of tests


def test_mmhc_on_a_hybrid_table():
    rows = 4000
    rng = np.random.default_rng(6)
    d1 = rng.integers(0, 3, rows)
    d2 = (d1 + rng.integers(0, 2, rows) * (rng.random(rows) < 0.6)) % 2
    d3 = rng.integers(0, 4, rows)
    d4 = (d3 + (rng.random(rows) < 0.3)) % 2
    c1 = rng.normal(size=rows) + 0.8 * d1
    c2 = 0.7 * c1 + rng.normal(scale=0.6, size=rows) - 0.5 * d2
    c3 = rng.normal(size=rows) * (1 + 0.3 * d3)
    df = pd.DataFrame({"c1": c1, "c2": c2, "c3": c3})
    for name, codes, k in (("d1", d1, 3), ("d2", d2, 2), ("d3", d3, 4), ("d4", d4, 2)):
        df[name] = pd.Categorical.from_codes(codes, [f"{name}_{i}" for i in range(k)])

    def learn():
        test = pbn.MutualInformation(df)
        test.set_batch_threshold(0)
        model = pbn.MMHC().estimate(test, pbn.ArcOperatorSet(), pbn.BIC(df), bn_type=pbn.CLGNetworkType(), alpha=0.05)
        return sorted(model.arcs()), test.batch_stats()

    arcs_on, stats_on = learn()
    with switched_off():
        arcs_off, stats_off = learn()
    assert stats_on[0] > 0 and stats_off[0] == 0
    assert arcs_on == arcs_off and arcs_on           # c2 is a linear function of c1 plus noise: at least that arc
