"""CPU tier: the PC engine (csrc/pc.hip behind pbn_pc_estimate / pbn_pdag_orient) against the Python restatement of the reference's
pc.cpp / constraint.hpp (tests/pc_restatement.py), both driven by the SAME deterministic p-value function through the Python-derived
IndependenceTest path, as tests/test_mmpc_cpu.py does for MMPC.  P-values are rounded so that exact ties, exact zeros and values equal
to alpha are common.  Arcs, edges, separating sets with their p-values and the serial test count must all match.

Then batched = serial: the same engine with and without a batch function, with a batch function that perturbs every p-value inside
the re-evaluation band (outputs must not move), and with the band switched off on an input built to sit inside it (outputs must move:
the band is what protects the decision)."""
import ctypes as C

import numpy as np
import pytest

import pc_restatement as pr
import pybnesian_amd as pbn
from oracle import mmpc_oracle
from pybnesian_amd import _lib
from pybnesian_amd.constraint import pc_estimate_indices, pdag_orient_indices, skeleton_from_cpcs
from pybnesian_amd.independences import validate_restrictions


def linear_gaussian_design(n, seed, parents=2.0):
    """A random linear-Gaussian DAG over n variables in topological order with about `parents` parents per node: (weights B with
    x = B^T x + e, noise variances)."""
    rng = np.random.default_rng(seed)
    B = np.zeros((n, n))
    for j in range(1, n):
        k = min(j, rng.poisson(parents))
        for i in rng.choice(j, size=k, replace=False):
            B[i, j] = rng.uniform(0.4, 1.2) * rng.choice([-1.0, 1.0])
    return B, rng.uniform(0.5, 1.5, n)


def linear_gaussian_covariance(n, seed, parents=2.0):
    B, var = linear_gaussian_design(n, seed, parents)
    A = np.linalg.inv(np.eye(n) - B)
    return A.T @ np.diag(var) @ A


def linear_gaussian_table(n, rows, seed, parents=2.0, dtype=np.float64):
    """`rows` samples of the design above as a DataFrame with columns v0 ... (the GPU tier's generator as well)."""
    import pandas as pd

    B, var = linear_gaussian_design(n, seed, parents)
    rng = np.random.default_rng(seed + 1000003)
    X = np.zeros((rows, n))
    for j in range(n):
        X[:, j] = X @ B[:, j] + rng.normal(0.0, np.sqrt(var[j]), rows)
    return pd.DataFrame(X.astype(dtype), columns=[f"v{i}" for i in range(n)])


class TableTest(pbn.IndependenceTest):
    """p-value of x _||_ y | z from partial correlations of a fixed covariance, rounded to create ties."""

    def __init__(self, cov, rows=300, decimals=3):
        self.cov, self.rows, self.decimals = np.asarray(cov), rows, decimals
        n = self.cov.shape[0]
        self.names = [f"v{i}" for i in range(n)]
        self.idx = {v: i for i, v in enumerate(self.names)}
        self.calls = 0

    def by_index(self, a, b, cond):
        self.calls += 1
        p = mmpc_oracle.lincor_pvalue(self.cov, self.rows, a, b, list(cond))
        return float(np.round(p, self.decimals)) if self.decimals is not None else float(p)

    def pvalue(self, x, y, z=None):
        cond = [] if z is None else ([z] if isinstance(z, str) else list(z))
        return self.by_index(self.idx[x], self.idx[y], [self.idx[c] for c in cond])

    def variable_names(self):
        return list(self.names)


def dense_cov(n, seed):
    """The covariance of tests/test_mmpc_cpu.py's TableTest: about a third of all pairs are arcs."""
    rng = np.random.default_rng(seed)
    B = np.triu(rng.uniform(-1, 1, (n, n)) * (rng.random((n, n)) < 0.35), 1)
    A = np.linalg.inv(np.eye(n) - B)
    return A.T @ np.diag(rng.uniform(0.5, 1.5, n)) @ A


def same(got, want, serial=True):
    assert got["arcs"] == want["arcs"]
    assert got["edges"] == want["edges"]
    assert got["sepsets"] == want["sepsets"]
    if serial:
        assert got["serial_tests"] == want["serial_tests"]


OPTIONS = [(u, b, t) for u in (False, True) for b in (False, True) for t in (0.0, 0.5)]


@pytest.mark.parametrize("use_sepsets,allow_bidirected,threshold", OPTIONS)
@pytest.mark.parametrize("n,seed,rows", [(6, 0, 300), (9, 1, 300), (12, 2, 2000), (10, 7, 60), (11, 4, 100000)])
def test_engine_matches_restatement(ensure_built, n, seed, rows, use_sepsets, allow_bidirected, threshold):
    t1, t2 = TableTest(dense_cov(n, seed), rows), TableTest(dense_cov(n, seed), rows)
    got = pc_estimate_indices(t1, t1.names, 0, 0.05, use_sepsets=use_sepsets, ambiguous_threshold=threshold, allow_bidirected=allow_bidirected,
                              batched=False)
    want = pr.estimate(t2.by_index, t2.names, 0, 0.05, use_sepsets=use_sepsets, ambiguous_threshold=threshold, allow_bidirected=allow_bidirected)
    same(got, want)
    assert got["evaluated"] == got["serial_tests"] == t1.calls   # no batch function: the engine IS the serial search


def test_separating_sets_of_three_and_more(ensure_built):
    """A dense 14-variable covariance with 100 000 rows: some edges fall only to separating sets of three to five variables."""
    cov = dense_cov(14, 5)
    t1, t2 = TableTest(cov, 100000), TableTest(cov, 100000)
    got = pc_estimate_indices(t1, t1.names, batched=False)
    want = pr.estimate(t2.by_index, t2.names)
    same(got, want)
    assert max(len(s) for s, _ in got["sepsets"].values()) >= 3


def test_forty_eight_nodes(ensure_built):
    """48 variables, about 1.5 parents each, 2 000 rows: 11 487 tests in the serial search (3 s through the engine's Python callback, 4 s
    through the restatement with its ctypes sets; nearly all of it is the scipy p-value both sides share)."""
    cov = linear_gaussian_covariance(48, 11, 1.5)
    t1, t2 = TableTest(cov, 2000), TableTest(cov, 2000)
    got = pc_estimate_indices(t1, t1.names, batched=False)
    want = pr.estimate(t2.by_index, t2.names)
    same(got, want)
    print("serial tests:", got["serial_tests"])
    assert got["serial_tests"] > 10000


@pytest.mark.parametrize("allow_bidirected", [False, True])
def test_restrictions(ensure_built, allow_bidirected):
    n = 9
    cov = dense_cov(n, 3)
    names = [f"v{i}" for i in range(n)]
    cases = [
        dict(arc_blacklist=[("v0", "v1"), ("v2", "v3"), ("v5", "v4")]),
        dict(arc_whitelist=[("v6", "v2"), ("v1", "v2"), ("v0", "v8")]),
        dict(edge_blacklist=[("v4", "v5"), ("v0", "v1"), ("v2", "v7")]),
        dict(edge_whitelist=[("v0", "v7"), ("v3", "v4")]),
        dict(arc_whitelist=[("v6", "v2"), ("v5", "v2"), ("v7", "v2"), ("v2", "v8")]),
        dict(arc_blacklist=[("v0", "v1"), ("v1", "v0"), ("v2", "v3")], arc_whitelist=[("v6", "v2"), ("v2", "v8")],
             edge_blacklist=[("v4", "v5")], edge_whitelist=[("v0", "v7"), ("v3", "v1")]),
    ]
    # more than two whitelisted arcs make the reference ask for a consistent extension of the STARTING graph (pc.cpp:288-297), and Dor
    # and Tarsi's leaf rule finds none in a complete graph with two missing edges: every leaf has two non-adjacent neighbours
    refused = dict(arc_whitelist=[("v6", "v2"), ("v5", "v2"), ("v7", "v2")], edge_blacklist=[("v4", "v5"), ("v0", "v1")])
    a_bl, a_wl, e_bl, e_wl = validate_restrictions(names, **refused)
    for run in (lambda: pr.estimate(TableTest(cov, 400).by_index, names, 0, 0.05, a_bl, a_wl, e_bl, e_wl),
                lambda: pc_estimate_indices(TableTest(cov, 400), names, 0, 0.05, a_bl, a_wl, e_bl, e_wl, batched=False)):
        with pytest.raises(ValueError, match="does not allow an acyclic graph"):
            run()
    raised = 0
    for kw in cases:
        a_bl, a_wl, e_bl, e_wl = validate_restrictions(names, **kw)
        for use_sepsets in (False, True):
            t1, t2 = TableTest(cov, 400), TableTest(cov, 400)
            args = (0, 0.05, a_bl, a_wl, e_bl, e_wl)
            try:
                want = pr.estimate(t2.by_index, names, *args, use_sepsets=use_sepsets, allow_bidirected=allow_bidirected)
            except IndexError as ex:
                # the reference looks a pair that only the edge blacklist separated up in its separating sets and throws
                # std::out_of_range (constraint.hpp:26-33); so does the engine
                assert use_sepsets and e_bl
                with pytest.raises(IndexError, match="not found in sepset") as info:
                    pc_estimate_indices(t1, names, *args, use_sepsets=use_sepsets, allow_bidirected=allow_bidirected, batched=False)
                assert str(info.value) == str(ex) or sorted(str(info.value)) == sorted(str(ex))   # (the pair may be named in either order)
                raised += 1
                continue
            got = pc_estimate_indices(t1, names, *args, use_sepsets=use_sepsets, allow_bidirected=allow_bidirected, batched=False)
            same(got, want)
            for a, b in a_wl:
                assert (a, b) in got["arcs"]
            for a, b in e_bl:
                assert (a, b) not in got["edges"] and (a, b) not in got["arcs"] and (b, a) not in got["arcs"]
            for a, b in e_wl:
                assert (a, b) in got["edges"] or (a, b) in got["arcs"] or (b, a) in got["arcs"]
    assert raised >= 1


def test_whitelist_cycle_is_refused(ensure_built):
    t = TableTest(dense_cov(6, 0), 300)
    cycle = [("v0", "v1"), ("v1", "v2"), ("v2", "v0")]
    with pytest.raises(ValueError, match="does not allow an acyclic graph"):
        pbn.PC().estimate(t, arc_whitelist=cycle)
    a_bl, a_wl, e_bl, e_wl = validate_restrictions(t.names, arc_whitelist=cycle)
    with pytest.raises(ValueError, match="does not allow an acyclic graph"):
        pr.estimate(t.by_index, t.names, arc_whitelist=a_wl)
    # (two arcs cannot close a cycle, and the reference does not look: pc.cpp:288)
    assert pbn.PC().estimate(t, arc_whitelist=cycle[:2]).has_arc("v0", "v1")


@pytest.mark.parametrize("use_sepsets,allow_bidirected,threshold", OPTIONS)
@pytest.mark.parametrize("n,ni,seed", [(6, 2, 0), (8, 4, 3), (9, 1, 5)])
def test_conditional_graphs(ensure_built, n, ni, seed, use_sepsets, allow_bidirected, threshold):
    cov = dense_cov(n + ni, seed)
    t1, t2 = TableTest(cov, 400), TableTest(cov, 400)
    names = t1.names
    kw = dict(arc_blacklist=[(names[n], names[0])]) if seed == 3 else {}
    a_bl, a_wl, e_bl, e_wl = validate_restrictions(names, **kw)
    got = pc_estimate_indices(t1, names, ni, 0.05, a_bl, a_wl, e_bl, e_wl, use_sepsets=use_sepsets, ambiguous_threshold=threshold,
                              allow_bidirected=allow_bidirected, batched=False)
    want = pr.estimate(t2.by_index, names, ni, 0.05, a_bl, a_wl, e_bl, e_wl, use_sepsets=use_sepsets, ambiguous_threshold=threshold,
                       allow_bidirected=allow_bidirected)
    same(got, want)
    assert all(a < n and b < n for a, b in got["edges"])          # interface edges end as arcs out of the interface node
    assert all(b < n for a, b in got["arcs"])
    g = pbn.PC().estimate_conditional(t1, names[:n], names[n:], use_sepsets=use_sepsets, ambiguous_threshold=threshold, allow_bidirected=allow_bidirected,
                                      **kw)
    assert isinstance(g, pbn.ConditionalPartiallyDirectedGraph) and g.interface_nodes() == names[n:]
    assert sorted(g.arcs()) == sorted((names[a], names[b]) for a, b in got["arcs"])


def test_argument_checks(ensure_built):
    t = TableTest(dense_cov(5, 0), 300)
    pc = pbn.PC()
    with pytest.raises(ValueError, match="alpha must be a number between 0 and 1"):
        pc.estimate(t, alpha=1.0)
    with pytest.raises(ValueError, match="ambiguous_threshold must be a number between 0 and 1"):
        pc.estimate(t, ambiguous_threshold=1.5)
    with pytest.raises(ValueError, match="do not contain all the variables in nodes list"):
        pc.estimate(t, nodes=["v0", "zz"])
    with pytest.raises(ValueError, match="Node list cannot be empty"):
        pc.estimate_conditional(t, [], ["v0"])
    with pytest.raises(ValueError, match="nodes/interface_nodes lists"):
        pc.estimate_conditional(t, ["v0", "v1"], ["zz"])
    g = pc.estimate_conditional(t, ["v0", "v1", "v2"])
    assert isinstance(g, pbn.ConditionalPartiallyDirectedGraph) and g.interface_nodes() == []
    sub = pc.estimate(t, nodes=["v3", "v1", "v0"])
    assert sub.nodes() == ["v3", "v1", "v0"]

    class Broken(pbn.IndependenceTest):
        def variable_names(self):
            return ["a", "b", "c"]

        def pvalue(self, x, y, z=None):
            raise KeyError("no data")

    with pytest.raises(KeyError, match="no data"):
        pc.estimate(Broken())


# ---- batched = serial ------------------------------------------------------------------------------------------------------------------
CASES = [(14, 5, 100000, None), (24, 5, 1000, 1.5), (48, 11, 2000, 1.5)]


def _cov(n, seed, parents):
    return dense_cov(n, seed) if parents is None else linear_gaussian_covariance(n, seed, parents)


@pytest.mark.parametrize("use_sepsets,allow_bidirected,threshold", OPTIONS)
@pytest.mark.parametrize("n,seed,rows,parents", CASES)
def test_batched_equals_serial_over_linear_correlation(ensure_built, n, seed, rows, parents, use_sepsets, allow_bidirected, threshold):
    """A host-only LinearCorrelation: its batch function is a loop over the scalar routine, so this exercises the engine's rounds."""
    names = [f"v{i}" for i in range(n)]
    test = pbn.LinearCorrelation.from_covariance(names, _cov(n, seed, parents), rows)
    kw = dict(use_sepsets=use_sepsets, ambiguous_threshold=threshold, allow_bidirected=allow_bidirected)
    serial = pc_estimate_indices(test, names, batched=False, **kw)
    before = test.batch_stats()
    batched = pc_estimate_indices(test, names, **kw)
    same(batched, serial)
    assert batched["evaluated"] >= batched["serial_tests"] == serial["evaluated"]
    dev, host, redone = (a - b for a, b in zip(test.batch_stats(), before))
    assert dev == 0 and redone == 0 and 0 < host <= batched["evaluated"]      # the batch function was used, and on the host


def perturbing_batch(test, band, first_sign):
    """A pbn_ci_pvalue_batch_fn that multiplies the p-values of test.by_index by 1 +- band / 4, the sign alternating from call to call."""
    state = {"sign": first_sign}

    def fn(_user, n_tests, v1, v2, off, cond, out):
        for i in range(n_tests):
            p = test.by_index(v1[i], v2[i], [cond[j] for j in range(off[i], off[i + 1])])
            out[i] = p * (1.0 + state["sign"] * band / 4)
            state["sign"] = -state["sign"]

    return _lib.CI_BATCH_FN(fn)


@pytest.mark.parametrize("decimals", [3, None])
@pytest.mark.parametrize("n,seed,rows,parents", CASES[:2])
def test_perturbation_inside_the_band_changes_nothing(ensure_built, n, seed, rows, parents, decimals):
    band = _lib.load().pbn_pc_band()
    assert 0 < band < 1e-3
    test = TableTest(_cov(n, seed, parents), rows, decimals)
    for kw in (dict(), dict(use_sepsets=True, allow_bidirected=False)):
        serial = pc_estimate_indices(test, test.names, batched=False, **kw)
        for first in (1.0, -1.0):
            same(pc_estimate_indices(test, test.names, batched=perturbing_batch(test, band, first), **kw), serial)


def test_without_the_band_the_same_perturbation_decides(ensure_built):
    """alpha is put just above a marginal p-value p0 of an edge the search keeps: p0 < alpha = p0 (1 + BAND / 16) < p0 (1 + BAND / 4).  A batch
    function that rounds p0 up by BAND / 4 removes the edge at level 0 unless the band sends the test back to the scalar function."""
    band = _lib.load().pbn_pc_band()
    test = TableTest(dense_cov(10, 7), 60, decimals=4)
    first = pc_estimate_indices(test, test.names, batched=False)
    kept = sorted((test.by_index(a, b, []), a, b) for a, b in first["edges"] + first["arcs"])
    kept = [k for k in kept if 0 < k[0] < 0.05]
    assert kept
    p0, a, b = kept[-1]
    alpha = p0 * (1 + band / 16)
    assert p0 < alpha and abs(p0 - alpha) <= band / 8 * alpha
    serial = pc_estimate_indices(test, test.names, alpha=alpha, batched=False)
    key = (min(a, b), max(a, b))
    assert serial["sepsets"].get(key, (None, None))[0] != []
    moved = 0
    for sign in (1.0, -1.0):
        same(pc_estimate_indices(test, test.names, alpha=alpha, batched=perturbing_batch(test, band, sign)), serial)
        off = pc_estimate_indices(test, test.names, alpha=alpha, batched=perturbing_batch(test, band, sign), band=0.0)
        moved += off["sepsets"] != serial["sepsets"]
        if off["sepsets"] != serial["sepsets"]:
            assert off["sepsets"][key][0] == []     # the edge fell to the marginal test
    assert moved >= 1                               # (the phase of the alternation that rounds this test up)


# ---- MMPC ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("allow_bidirected", [False, True])
@pytest.mark.parametrize("n,ni,seed,rows", [(6, 0, 0, 300), (9, 0, 1, 300), (12, 0, 2, 2000), (8, 3, 3, 400)])
def test_mmpc_estimate(ensure_built, n, ni, seed, rows, allow_bidirected):
    cov = dense_cov(n + ni, seed)
    t1, t2 = TableTest(cov, rows), TableTest(cov, rows)
    names = t1.names
    cpcs, _ = mmpc_oracle.mmpc_all_variables(t2.by_index, n + ni, 0.05, symmetric=False, n_interface=ni)
    arcs, edges = skeleton_from_cpcs(cpcs, n, [])
    want = pr.orient(t2.by_index, names, ni, 0.05, arcs, edges, allow_bidirected=allow_bidirected)
    if ni:
        g = pbn.MMPC().estimate_conditional(t1, names[:n], names[n:], allow_bidirected=allow_bidirected, ambiguous_threshold=0.9)
    else:
        g = pbn.MMPC().estimate(t1, allow_bidirected=allow_bidirected, ambiguous_threshold=0.9)
    idx = t1.idx
    assert sorted((idx[a], idx[b]) for a, b in g.arcs()) == want["arcs"]
    assert sorted((min(idx[a], idx[b]), max(idx[a], idx[b])) for a, b in g.edges()) == want["edges"]
    got = pdag_orient_indices(t1, names, ni, 0.05, arcs, edges, allow_bidirected=allow_bidirected, batched=False)
    assert got["serial_tests"] == want["serial_tests"] == got["evaluated"]
    assert g.num_edges() + g.num_arcs() > 0


def test_mmpc_restrictions_and_checks(ensure_built):
    t = TableTest(dense_cov(8, 3), 400)
    g = pbn.MMPC().estimate(t, arc_whitelist=[("v6", "v2")], edge_blacklist=[("v4", "v5")], arc_blacklist=[("v0", "v1")])
    assert g.has_arc("v6", "v2") and not g.has_connection("v4", "v5") and not g.has_arc("v0", "v1")
    with pytest.raises(ValueError, match="alpha must be"):
        pbn.MMPC().estimate(t, alpha=0.0)
    with pytest.raises(ValueError, match="ambiguous_threshold must be"):
        pbn.MMPC().estimate(t, ambiguous_threshold=-0.1)


def test_public_names(ensure_built):
    for name in ("PC", "MMPC", "MeekRules", "PartiallyDirectedGraph", "ConditionalPartiallyDirectedGraph"):
        assert hasattr(pbn, name) and name in pbn.__all__
    assert isinstance(C.cast(_lib.load().pbn_lincor_pvalue_batch, C.c_void_p).value, int)
