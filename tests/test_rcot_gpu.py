"""RCoT on the device (csrc/rcot.hip): parity with the numpy restatement given the drawn W and b, determinism of the seeded
draws and of the batch path, behaviour on non-linear dependence, integration with MMHC / DMMHC, errors."""
import itertools

import numpy as np
import pandas as pd
import pytest

from rcot_restatement import check_parity as _check_parity
from rcot_restatement import sigma_window

pytestmark = pytest.mark.gpu


def _table(n, k, seed, nonlinear=True):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(n, k))
    s = z.sum(axis=1) if k else np.zeros(n)
    x = np.sin(s) + 0.5 * rng.normal(size=n) if nonlinear else rng.normal(size=n)
    y = np.cos(s) + 0.3 * x ** 2 + 0.5 * rng.normal(size=n)
    d = {"x": x, "y": y}
    for i in range(k):
        d[f"z{i}"] = z[:, i]
    return pd.DataFrame(d)


@pytest.mark.parametrize("n,k", [(50, 0), (50, 1), (2000, 0), (20000, 0), (20000, 1), (20000, 2), (20000, 4)])
def test_parity(n, k):
    df = _table(n, k, n + k)
    det = _check_parity(df, [f"z{i}" for i in range(k)] or None)
    assert det["n_valid"] == n


def test_parity_large_three_z():
    _check_parity(_table(1_000_000, 3, 5), ["z0", "z1", "z2"])


def test_parity_float32_and_counts():
    df = _table(20000, 2, 7).astype("float32")
    _check_parity(df, ["z0", "z1"])
    _check_parity(_table(20000, 2, 8), ["z0", "z1"], nxy=3, nz=20)
    det = _check_parity(_table(5000, 1, 9), "z0", nxy=5, nz=1)   # random_fourier_z = 1: HBE forced
    assert det["method"] == "HBE"


def test_parity_nulls():
    df = _table(20000, 2, 10)
    rng = np.random.default_rng(1)
    for c in df.columns:
        df.loc[rng.random(len(df)) < 0.05, c] = np.nan
    det = _check_parity(df, ["z0", "z1"])
    assert det["n_valid"] < 20000
    _check_parity(df, None)


def test_sigma_median_zero_becomes_one():
    import pybnesian_amd as pbn

    df = _table(2000, 0, 15)
    df.loc[:399, "x"] = 0.75   # 400 equal values among the first 500 rows: most pairwise distances are 0
    t = pbn.RCoT(df, seed=2)
    det = t.detail("x", "y")
    table = {c: df[c].to_numpy(dtype=np.float64) for c in df.columns}
    assert det["sigma"][0] == 1.0 == sigma_window(table, ["x"])
    assert det["sigma"][1] == pytest.approx(sigma_window(table, ["y"]), rel=1e-12)


def test_constant_columns():
    import pybnesian_amd as pbn

    df = _table(3000, 2, 12)
    df["c"] = 2.5
    t = pbn.RCoT(df, seed=3)
    assert t.pvalue("c", "y") == 1.0
    assert t.pvalue("x", "c", ["z0"]) == 1.0
    assert t.detail("c", "y")["trivial"]
    assert t.pvalue("x", "y", "c") == t.pvalue("x", "y")
    assert t.pvalue("x", "y", ["c", "z1"]) == t.pvalue("x", "y", "z1")
    assert t.detail("x", "y", ["z0", "c"])["z"] == ["z0"]


def test_determinism_and_symmetry():
    import pybnesian_amd as pbn

    df = _table(4000, 3, 13)
    t1, t2 = pbn.RCoT(df, seed=42), pbn.RCoT(df, seed=42)
    z = ["z0", "z1", "z2"]
    p = t1.pvalue("x", "y", z)
    assert p == t2.pvalue("x", "y", z)
    for perm in itertools.permutations(z):
        assert t1.pvalue("x", "y", list(perm)) == p
        assert t1.pvalue("y", "x", list(perm)) == p
    assert pbn.RCoT(df, seed=43).pvalue("x", "y", z) != p


def test_batch_matches_single_calls():
    import ctypes as C

    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    df = _table(5000, 3, 14)
    t = pbn.RCoT(df, seed=5)
    names = list(df.columns)
    tests = [("x", "y", []), ("x", "y", ["z0"]), ("y", "z2", ["x", "z0"]), ("z0", "z1", []), ("x", "z1", ["z0", "z2", "y"]),
             ("z2", "x", ["y"])]
    single = [t.pvalue(a, b, z or None) for a, b, z in tests]
    lib = _lib.load()
    _lib.check(lib.pbn_rcot_set_order(t._handle, 0, None))

    def batch(items):
        v1 = _lib.int_array([names.index(a) for a, _, _ in items])
        v2 = _lib.int_array([names.index(b) for _, b, _ in items])
        off = np.cumsum([0] + [len(z) for _, _, z in items]).tolist()
        cond = _lib.int_array([names.index(c) for _, _, z in items for c in z] or [0])
        out = np.zeros(len(items))
        lib.pbn_rcot_pvalue_batch(t._handle, len(items), v1, v2, _lib.int_array(off), cond, _lib.dptr(out))
        return out

    assert batch(tests).tolist() == single
    order = np.random.default_rng(0).permutation(len(tests))
    shuffled = batch([tests[i] for i in order])
    assert shuffled.tolist() == [single[i] for i in order]
    assert batch(tests[:2]).tolist() + batch(tests[2:]).tolist() == single


def test_nonlinear_dependence_detected():
    import pybnesian_amd as pbn

    rng = np.random.default_rng(21)
    # an even link on a symmetric x: no linear correlation to find (an odd one such as sin(3x) on a finite range keeps some)
    x = rng.uniform(-3, 3, 2000)
    df = pd.DataFrame({"x": x, "y": np.cos(x) + 0.2 * rng.normal(size=2000)})
    assert pbn.RCoT(df, seed=1).pvalue("x", "y") < 1e-3
    assert pbn.LinearCorrelation(df).pvalue("x", "y") > 0.05


def test_chain_conditional_independence():
    import pybnesian_amd as pbn

    rng = np.random.default_rng(22)
    n = 3000
    x = rng.normal(size=n)
    z = np.tanh(1.5 * x) + 0.2 * rng.normal(size=n)
    y = z ** 3 + 0.2 * rng.normal(size=n)
    t = pbn.RCoT(pd.DataFrame({"x": x, "y": y, "z": z}), seed=2)
    assert t.pvalue("x", "y") < 1e-3
    assert t.pvalue("x", "y", "z") > 0.01


def test_null_pvalues_uniform():
    import pybnesian_amd as pbn

    ps = []
    for s in range(200):   # a fresh independent table and RCoT seed each time: p-values of one table are not independent draws
        rng = np.random.default_rng(1000 + s)
        df = pd.DataFrame({"x": rng.normal(size=2000), "y": rng.normal(size=2000)})
        ps.append(pbn.RCoT(df, seed=s).pvalue("x", "y"))
    from scipy import stats

    assert stats.kstest(ps, "uniform").pvalue > 1e-3


def _nonlinear_gaussian(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=n)
    b = np.sin(2 * a) + 0.4 * rng.normal(size=n)
    c = 0.8 * a + 0.5 * rng.normal(size=n)
    d = b * c + 0.4 * rng.normal(size=n)
    return pd.DataFrame({"a": a, "b": b, "c": c, "d": d})


def test_mmhc_batched_equals_unbatched():
    import pybnesian_amd as pbn

    df = _nonlinear_gaussian(1500, 31)
    t = pbn.RCoT(df, seed=9)

    class Forward(pbn.IndependenceTest):
        def pvalue(self, x, y, z=None):
            return t.pvalue(x, y, z)

        def variable_names(self):
            return t.variable_names()

    m1 = pbn.MMHC()
    m1.estimate(t, pbn.ArcOperatorSet(), pbn.BIC(df))
    m2 = pbn.MMHC()
    m2.estimate(Forward(), pbn.ArcOperatorSet(), pbn.BIC(df))
    c1, c2 = m1.last_cpcs, m2.last_cpcs
    assert [sorted(c) for c in c1] == [sorted(c) for c in c2]


def test_dynamic_rcot_and_dmmhc():
    import pybnesian_amd as pbn

    df = _nonlinear_gaussian(800, 32)
    ddf = pbn.DynamicDataFrame(df, 2)
    dt = pbn.DynamicRCoT(ddf, seed=4)
    st, tr = dt.static_tests(), dt.transition_tests()
    assert 0 <= st.pvalue("a_t_1", "b_t_1") <= 1
    assert 0 <= tr.pvalue("a_t_0", "b_t_1", ["a_t_1"]) <= 1
    res = pbn.DMMHC().estimate(dt, pbn.ArcOperatorSet(), pbn.DynamicBIC(ddf))
    assert res is not None


def test_errors():
    import pybnesian_amd as pbn

    df = _table(200, 1, 40)
    df["cat"] = pd.Categorical(["a", "b"] * 100)
    t = pbn.RCoT(df, seed=1)
    with pytest.raises(ValueError, match="Column are not continuous."):
        t.pvalue("x", "cat")
    with pytest.raises(ValueError):
        t.pvalue("x", "nope")
    with pytest.raises(ValueError, match="DataFrame does not contain enough continuous columns."):
        pbn.RCoT(pd.DataFrame({"x": np.arange(5.0), "c": pd.Categorical(list("abcab"))}))
    with pytest.raises(ValueError, match="random_fourier_xy"):
        pbn.RCoT(df, random_fourier_xy=9)
    with pytest.raises(ValueError, match="random_fourier_z"):
        pbn.RCoT(df, random_fourier_xy=5, random_fourier_z=250)
