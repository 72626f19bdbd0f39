"""GPU tier: HCKDE and CLinearGaussianCPD fit / logl / slogl on one device partition of the rows (pybnesian_amd/adaptator_group.py,
csrc/row_groups.hip) through the public interface, stand-alone and inside a SemiparametricBN.

Comparator: the same call under PBN_ADAPTATOR_GROUP=0 - _DiscreteAdaptator's per-configuration loop (factors/discrete/
DiscreteAdaptator.hpp:201-348).  Everything is demanded EQUAL: the same configurations without a factor; per configuration
num_instances, the bandwidth and both normalisation constants (CKDE) or the coefficients and the variance (LinearGaussianCPD); logl
array_equal with NaN in the same rows; slogl ==.  The reason: a configuration's gathered table is byte for byte the table the loop's upload
of the slice gives, and the base factor enters through the same code.  A network's slogl adds the nodes' sums, so it stays within
test_clg_model_gpu.sum_bound of them - and is in fact the same order of additions, hence also equal."""
import ctypes as C

import numpy as np
import pyarrow as pa
import pytest

import test_clg_model_gpu as base

pytestmark = pytest.mark.gpu

KINDS = ["HCKDE", "CLinearGaussianCPD"]
DTYPES = ["float64", "float32"]
EVIDENCE = ["D1", "y", "D2", "z"]     # discrete and continuous interleaved: _disc = [D1, D2], _cont = [y, z]


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def ag(pbn):
    from pybnesian_amd import adaptator_group

    return adaptator_group


def make_batch(dtype, rows=3000, seed=1, null_discrete=False, null_continuous=False, categories=("a", "b", "c")):
    """About `rows` rows: D1 and D2 of three categories each (configuration = D1 + 3 D2), x given y, z.  Configuration 8 (c, c) is absent,
    configuration 5 (c, b) keeps two rows - too few for either base factor: a dropped fit - and in configuration 4 (b, b) x = 2 y exactly:
    a singular covariance for the KDE, a variance of zero for the regression."""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 3, size=rows)
    d2 = rng.integers(0, 3, size=rows)
    keep = ~((d1 == 2) & (d2 == 2))
    rare = np.nonzero((d1 == 2) & (d2 == 1))[0]
    keep[rare[2:]] = False
    d1, d2 = d1[keep], d2[keep]
    n = d1.size
    y = rng.normal(size=n) + 0.5 * d1
    z = rng.normal(size=n) - 0.3 * y
    x = (1.0 + d2) * y - 0.5 * z + np.array([0.5, 1.0, 1.5])[d1] * rng.normal(size=n)
    flat = (d1 == 1) & (d2 == 1)
    x[flat] = 2.0 * y[flat]
    x, y, z = (v.astype(dtype) for v in (x, y, z))
    x[flat] = (2.0 * y[flat]).astype(dtype)   # exact in the frame's own type
    masks = {}
    if null_discrete:
        masks["D1"] = rng.random(n) < 0.05
        masks["D2"] = rng.random(n) < 0.05
    if null_continuous:
        masks["x"] = rng.random(n) < 0.05
        masks["z"] = rng.random(n) < 0.05
    cats2 = ["u", "v", "w"]
    cols = {"D1": pa.DictionaryArray.from_arrays(pa.array(d1.astype(np.int8), mask=masks.get("D1")), pa.array(list(categories))),
            "D2": pa.DictionaryArray.from_arrays(pa.array(d2.astype(np.int8), mask=masks.get("D2")), pa.array(cats2))}
    for name, v in (("x", x), ("y", y), ("z", z)):
        cols[name] = pa.array(v, mask=masks.get(name))
    return pa.RecordBatch.from_pydict(cols)


def lognorms(ckde):
    from pybnesian_amd import _lib

    lib = _lib.load()
    return float(lib.pbn_kde_lognorm(ckde._handle, 0)), float(lib.pbn_kde_lognorm(ckde._handle, 1))


def assert_equal_factors(pbn, f, g):
    """f: through the device partition, g: through the loop"""
    assert type(f) is type(g) and f.fitted() and g.fitted()
    assert f._disc == g._disc and f._cont == g._cont and f._categories == g._categories and len(f._factors) == len(g._factors)
    assert [s is None for s in f._factors] == [s is None for s in g._factors]
    for s, t in zip(f._factors, g._factors):
        if s is None:
            continue
        assert type(s) is type(t) and s.variable() == t.variable() and s.evidence() == t.evidence()
        if isinstance(s, pbn.CKDE):
            assert s.num_instances() == t.num_instances() and s.data_type() == t.data_type()
            assert np.array_equal(s.bandwidth, t.bandwidth)
            assert lognorms(s) == lognorms(t)
        else:
            assert np.array_equal(s.beta, t.beta) and s.variance == t.variance


def delta(ag, before):
    return {k: ag.counters[k] - before[k] for k in before}


def run_both(monkeypatch, ag, call, expect_partitions=1):
    """(call() with the switch on, call() with it off); the counters: one partition a call and no fallback - nothing with the switch off"""
    monkeypatch.delenv("PBN_ADAPTATOR_GROUP", raising=False)
    before = dict(ag.counters)
    on = call()
    took = delta(ag, before)
    assert took["partitions"] == expect_partitions and took["loop_fallbacks"] == 0, took
    monkeypatch.setenv("PBN_ADAPTATOR_GROUP", "0")
    before = dict(ag.counters)
    off = call()
    assert ag.counters == before
    monkeypatch.delenv("PBN_ADAPTATOR_GROUP")
    return on, off, took


def fitted(pbn, kind, rb):
    f = getattr(pbn, kind)("x", EVIDENCE)
    f.fit(rb)
    return f


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_stand_alone_factor_equals_the_loop(pbn, ag, monkeypatch, kind, dtype):
    """Fails without the route: the counters do not move (the module is missing)."""
    train = make_batch(dtype)
    assert 2300 < train.num_rows < 3000
    f, g, took = run_both(monkeypatch, ag, lambda: fitted(pbn, kind, train))
    assert f._disc == ["D1", "D2"] and f._cont == ["y", "z"]
    assert [s is None for s in f._factors] == [False, False, False, False, True, True, False, False, True]   # singular, two rows, absent
    assert took["rows_grouped"] == train.num_rows and took["tables_gathered"] == 8 and took["code_tables"] == 1
    assert_equal_factors(pbn, f, g)
    assert f.conditional_factor(pbn.Assignment({"D1": "c", "D2": "w"})) is None
    test = make_batch(dtype, rows=2100, seed=2)
    # the four combinations: a factor fitted either way, evaluated either way
    for factor in (f, g):
        on, off, took = run_both(monkeypatch, ag, lambda: factor.logl(test))
        assert took["rows_grouped"] == test.num_rows and took["tables_gathered"] == 6
        assert on.shape == (test.num_rows,) and on.dtype == np.float64
        assert np.array_equal(on, off, equal_nan=True)
        assert 0 < np.isnan(on).sum() < test.num_rows / 4            # the rows of configurations 4 and 5
        on, off, _ = run_both(monkeypatch, ag, lambda: factor.slogl(test))
        assert on == off and np.isfinite(on)
    assert np.array_equal(f.logl(test), g.logl(test), equal_nan=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["discrete", "continuous", "both"])
def test_nulls(pbn, ag, monkeypatch, kind, dtype, where):
    """Nulls in a discrete parent and in continuous columns of the family: the same slices in fit, NaN in the same rows of logl, the same
    rows in slogl."""
    nd, nc = where in ("discrete", "both"), where in ("continuous", "both")
    train = make_batch(dtype, seed=3, null_discrete=nd, null_continuous=nc)
    f, g, took = run_both(monkeypatch, ag, lambda: fitted(pbn, kind, train))
    assert took["rows_grouped"] < train.num_rows
    assert_equal_factors(pbn, f, g)
    if kind == "HCKDE":
        sizes = [s.num_instances() for s in f._factors if s is not None]
        assert sum(sizes) < took["rows_grouped"]          # (the groups of the configurations without a factor are not in the sum)
    test = make_batch(dtype, rows=2100, seed=4, null_discrete=nd, null_continuous=nc)
    on, off, _ = run_both(monkeypatch, ag, lambda: f.logl(test))
    assert np.array_equal(on, off, equal_nan=True)
    null_row = np.zeros(test.num_rows, dtype=bool)
    for name in ["x"] + EVIDENCE:
        null_row |= ~np.asarray(test.column(test.schema.get_field_index(name)).is_valid().to_numpy(zero_copy_only=False), dtype=bool)
    assert null_row.sum() > 50 and np.isnan(on[null_row]).all()
    on, off, _ = run_both(monkeypatch, ag, lambda: f.slogl(test))
    assert on == off and np.isfinite(on)


@pytest.mark.parametrize("kind", KINDS)
def test_other_categories_still_raise(pbn, ag, monkeypatch, kind):
    monkeypatch.delenv("PBN_ADAPTATOR_GROUP", raising=False)
    f = fitted(pbn, kind, make_batch("float64"))
    other = make_batch("float64", rows=500, seed=5, categories=("a", "b", "other"))
    before = dict(ag.counters)
    for call in (f.logl, f.slogl):
        with pytest.raises(ValueError, match="does not contain the same categories"):
            call(other)
    took = delta(ag, before)
    assert took["partitions"] == 0 and took["loop_fallbacks"] == 2       # decided before anything is grouped; the loop raises


def test_what_keeps_the_loop(pbn, ag, monkeypatch):
    """A subclass and a factor without discrete evidence are counted as fallbacks and give the loop's results."""
    monkeypatch.delenv("PBN_ADAPTATOR_GROUP", raising=False)

    class Mine(pbn.CLinearGaussianCPD):
        pass

    train = make_batch("float64")
    before = dict(ag.counters)
    a = Mine("x", EVIDENCE)
    a.fit(train)
    b = pbn.CLinearGaussianCPD("x", ["y", "z"])
    b.fit(train)
    vals = a.logl(train)
    took = delta(ag, before)
    assert took["partitions"] == 0 and took["loop_fallbacks"] == 3
    ref = fitted(pbn, "CLinearGaussianCPD", train)
    assert np.array_equal(vals, ref.logl(train), equal_nan=True)


# ---- inside a network --------------------------------------------------------------------------------------------------------------------

NODES = ["x", "D2", "w", "y", "D1", "z"]
ARCS = [("D1", "D2"), ("D1", "x"), ("D2", "x"), ("y", "x"), ("D1", "w"), ("y", "w"), ("y", "z")]
# x | D1, D2, y: HCKDE; w | D1, y: CLinearGaussianCPD; z | y: CKDE; y: LinearGaussianCPD; D1, D2 | D1: DiscreteFactor


def make_network(pbn):
    types = [("D1", pbn.DiscreteFactorType()), ("D2", pbn.DiscreteFactorType()), ("x", pbn.CKDEType()), ("z", pbn.CKDEType()),
             ("w", pbn.LinearGaussianCPDType()), ("y", pbn.LinearGaussianCPDType())]
    return pbn.SemiparametricBN(NODES, ARCS, types)


def network_batch(dtype, rows, seed):
    rb = make_batch(dtype, rows=rows, seed=seed)
    rng = np.random.default_rng(seed + 100)
    y = rb.column(rb.schema.get_field_index("y")).to_numpy()
    d1 = rb.column(rb.schema.get_field_index("D1")).indices.to_numpy()
    w = (0.5 - 0.4 * y.astype(np.float64) * (1 + d1) + 0.3 * rng.normal(size=rb.num_rows)).astype(dtype)
    return pa.RecordBatch.from_arrays(list(rb.columns) + [pa.array(w)], names=list(rb.schema.names) + ["w"])


@pytest.mark.parametrize("dtype", DTYPES)
def test_network(pbn, ag, monkeypatch, dtype):
    from pybnesian_amd import clg_fit, clg_model

    train = network_batch(dtype, 3000, 1)
    test = network_batch(dtype, 2100, 2)

    def fit():
        net = make_network(pbn)
        net.fit(train)
        return net

    before_fit = dict(clg_fit.counters)
    # fit: w is clg_fit's (one pass, as before), x takes this route - one partition, one code table for the call
    one, loop, took = run_both(monkeypatch, ag, fit)
    assert took["code_tables"] == 1 and took["tables_gathered"] == 8
    moved = {k: clg_fit.counters[k] - before_fit[k] for k in before_fit}
    assert moved["calls"] == 2 and moved["nodes_served"] == 2 and moved["discrete_nodes_fitted"] == 4    # the same in both fits
    kinds = {n: type(one.cpd(n)).__name__ for n in NODES}
    assert kinds == {"x": "HCKDE", "D2": "DiscreteFactor", "w": "CLinearGaussianCPD", "y": "LinearGaussianCPD", "D1": "DiscreteFactor", "z": "CKDE"}
    for n in NODES:
        f, g = one.cpd(n), loop.cpd(n)
        assert type(f) is type(g)
        if isinstance(f, (pbn.HCKDE, pbn.CLinearGaussianCPD)):
            assert_equal_factors(pbn, f, g)
        elif isinstance(f, pbn.DiscreteFactor):
            assert np.array_equal(f._logprob, g._logprob)
        elif isinstance(f, pbn.CKDE):
            assert f.num_instances() == g.num_instances() and np.array_equal(f.bandwidth, g.bandwidth)
        else:
            assert np.array_equal(f.beta, g.beta) and f.variance == g.variance
    # logl and slogl: x and w both take the route - two partitions on ONE code table a model call; the one-pass evaluators do not
    # serve a network with a KDE node, with the switch on or off
    before_model = dict(clg_model.counters)
    on, off, took = run_both(monkeypatch, ag, lambda: one.logl(test), expect_partitions=2)
    assert took["code_tables"] == 1
    assert np.array_equal(on, off, equal_nan=True) and np.isnan(on).any() and not np.isnan(on).all()
    assert np.array_equal(on, loop.logl(test), equal_nan=True)
    s_on, s_off, took = run_both(monkeypatch, ag, lambda: one.slogl(test), expect_partitions=2)
    assert took["code_tables"] == 1
    assert clg_model.counters == before_model
    per_node = [one.cpd(n).logl(test) for n in NODES]
    bound = base.sum_bound(per_node)
    print(f"slogl on {s_on!r} off {s_off!r} bound {bound:.3e}")
    assert np.isfinite(s_on) and abs(s_on - s_off) <= bound
    assert s_on == s_off


def test_a_clg_network_keeps_its_one_pass_evaluation(pbn, ag, monkeypatch):
    """PBN_CLG_FIT and PBN_CLG_MODEL serve what they served: a CLGNetwork's calls never reach this route."""
    from pybnesian_amd import clg_fit, clg_model

    monkeypatch.delenv("PBN_ADAPTATOR_GROUP", raising=False)
    df = base.make_frame(3000, 1)
    before = dict(ag.counters), dict(clg_fit.counters), dict(clg_model.counters)
    net = pbn.CLGNetwork(base.NODES, base.ARCS, base.discrete_types(pbn))
    net.fit(df)
    net.logl(df)
    net.slogl(df)
    assert ag.counters == before[0]
    assert clg_fit.counters["calls"] == before[1]["calls"] + 1 and clg_fit.counters["nodes_served"] == before[1]["nodes_served"] + 2
    assert clg_model.counters["launches"] == before[2]["launches"] + 2
