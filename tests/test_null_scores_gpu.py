"""GPU tier: BIC / BGe / BDe on tables with nulls, through the public classes.  Every null case of pbn_score_batch is served by device passes
over the batch: null codes (-1) in the family-count pass, the masked moment pass (csrc/masked_moments.hip) for Gaussian and CLG candidates.

Reference: learning/scores/bic.cpp:12-96 (valid_rows of the candidate's columns; bic_clg; bic_discrete), learning/scores/bde.cpp:5-47,
factors/discrete/discrete_indices.cpp:134-204 (rows that are null in the family's own columns are dropped), bge.hpp:154-234.
Nulls are injected as test_scores_gpu.py::test_scores_with_nulls injects them: np.random.seed(0), 100 random rows per column."""
import math

import numpy as np
import pandas as pd
import pytest
from scipy.special import gammaln

from discrete_model_restatement import joint_counts_fast
from helpers import RTOL_F64

pytestmark = pytest.mark.gpu

NODES = list("abcdefgh")
CARD = {"a": 3, "b": 3, "c": 2, "d": 4, "e": 2, "f": 3, "g": 3, "h": 2}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def discrete_codes(n, seed=0):
    """The DAG of test_discrete_scores_gpu.py: a -> b -> c, (a, c) -> d weakly, e -> f -> g, h alone."""
    rng = np.random.default_rng(seed)
    code = {}

    def child(parent, card, keep=0.8):
        return np.where(rng.random(n) < keep, parent % card, rng.integers(0, card, size=n))

    code["a"] = rng.integers(0, 3, size=n)
    code["b"] = child(code["a"], 3)
    code["c"] = child(code["b"], 2)
    code["d"] = child(code["a"] + code["c"], 4, keep=0.3)
    code["e"] = rng.integers(0, 2, size=n)
    code["f"] = child(code["e"], 3)
    code["g"] = child(code["f"], 3)
    code["h"] = rng.integers(0, 2, size=n)
    return {v: code[v].astype(np.int64) for v in NODES}


def categorical(codes, name, card):
    return pd.Categorical.from_codes(codes, [f"{name}{i}" for i in range(card)])   # code -1 = null


def discrete_table(n=5000, seed=0):
    """(frame, codes with -1 under the nulls)."""
    codes = discrete_codes(n, seed)
    np.random.seed(0)
    for v in NODES:
        codes[v][np.random.randint(0, n, size=100)] = -1
    return pd.DataFrame({v: categorical(codes[v], v, CARD[v]) for v in NODES}), codes


def gaussian_table(n=4000, cols=10, seed=0, dtype="float64"):
    """(frame, float64 array with NaN under the nulls)."""
    rng = np.random.default_rng(seed)
    mix = np.triu(rng.uniform(-0.8, 0.8, size=(cols, cols)), 1) + np.eye(cols)
    x = (rng.normal(size=(n, cols)) @ mix + rng.uniform(-3, 3, size=cols)).astype(dtype).astype(np.float64)
    np.random.seed(0)
    for j in range(cols):
        x[np.random.randint(0, n, size=100), j] = np.nan
    names = [f"g{j}" for j in range(cols)]
    return pd.DataFrame(x, columns=names).astype(dtype), x, names


def hybrid_table(n=6000, seed=0, dtype="float64"):
    """Discrete A (2), B (3); continuous x | A, y | x, B, z | x, y; nulls in every column."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 2, size=n)
    B = (rng.random(n) < np.where(A == 0, 0.3, 0.6)).astype(int) + (rng.random(n) < 0.2)
    x = rng.normal(loc=np.where(A == 0, -1.0, 2.0), scale=1.0)
    y = 0.7 * x + np.array([0.0, 3.0, -2.0])[B] + rng.normal(scale=0.5, size=n)
    z = np.tanh(x) - 0.4 * y + rng.normal(scale=0.3, size=n)
    cont = np.stack([x, y, z], axis=1).astype(dtype).astype(np.float64)
    codes = {"A": A.astype(np.int64), "B": B.astype(np.int64)}
    np.random.seed(0)
    for j in range(3):
        cont[np.random.randint(0, n, size=100), j] = np.nan
    for v in ("A", "B"):
        codes[v][np.random.randint(0, n, size=100)] = -1
    df = pd.DataFrame(cont, columns=list("xyz")).astype(dtype)
    df["A"] = categorical(codes["A"], "a", 2)
    df["B"] = categorical(codes["B"], "b", 3)
    return df, cont, codes


def random_families(names, count, max_parents, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        cols = rng.choice(len(names), size=int(rng.integers(1, max_parents + 2)), replace=False)
        out.append((names[cols[0]], [names[c] for c in cols[1:]]))
    return out


# ---- transcriptions over null-aware counts -----------------------------------------------------------------------------------------
def family_counts(codes, variable, parents):
    cols = [variable] + list(parents)
    table = [codes[c] for c in cols]
    return joint_counts_fast(table, [CARD[c] for c in cols], (0, list(range(1, len(cols))))).astype(np.float64)


def bde_transcribed(codes, variable, parents, iss):
    """bde.cpp:5-47: (score, sum of |terms|, number of terms)."""
    counts = family_counts(codes, variable, parents)
    card0, total = CARD[variable], len(counts)
    alpha = iss / total
    terms = [-total * gammaln(alpha)]
    if not parents:
        terms += [gammaln(m + alpha) for m in counts]
        terms += [gammaln(iss), -gammaln(iss + counts.sum())]
    else:
        for k in range(total // card0):
            block = counts[k * card0: (k + 1) * card0]
            terms += [gammaln(m + alpha) for m in block]
            terms += [gammaln(alpha * card0), -gammaln(alpha * card0 + block.sum())]
    terms = np.asarray(terms, dtype=np.float64)
    return math.fsum(terms), math.fsum(np.abs(terms)), len(terms)


def bic_discrete_transcribed(codes, variable, parents):
    """bic.cpp:66-96: (score, sum of |terms|, number of terms)."""
    counts = family_counts(codes, variable, parents)
    card0 = CARD[variable]
    configs = len(counts) // card0
    terms = []
    for k in range(configs):
        block = counts[k * card0: (k + 1) * card0]
        if block.sum() > 0:
            inv = 1.0 / block.sum()
            terms += [c * math.log(c * inv) for c in block if c > 0]
    terms.append(-math.log(counts.sum()) * 0.5 * (card0 - 1) * configs)
    return math.fsum(terms), math.fsum(np.abs(terms)), len(terms)


def numpy_bge(data, total_nodes, iss_mu=1.0):
    """bge.hpp:154-234 (bge_no_parents / bge_parents), nu = the sample means."""
    data = np.asarray(data, dtype=np.float64)
    N, d = data.shape
    p = d - 1
    iss_w = total_nodes + 2
    c = data - data.mean(axis=0)
    t = iss_mu * (iss_w - total_nodes - 1) / (iss_mu + 1)
    lp = 0.5 * (math.log(iss_mu) - math.log(N + iss_mu))
    lp += gammaln(0.5 * (N + iss_w - total_nodes + p + 1)) - gammaln(0.5 * (iss_w - total_nodes + p + 1))
    lp -= 0.5 * N * math.log(math.pi)
    R = c.T @ c + t * np.eye(d)
    if p == 0:
        lp += 0.5 * (iss_w - total_nodes + 1) * math.log(t)
        return lp - 0.5 * (N + iss_w - total_nodes + 1) * math.log(R[0, 0])
    lp += 0.5 * (iss_w - total_nodes + 2 * p + 1) * math.log(t)
    lp -= 0.5 * (N + iss_w - total_nodes + p + 1) * np.linalg.slogdet(R)[1]
    lp += 0.5 * (N + iss_w - total_nodes + p) * np.linalg.slogdet(R[1:, 1:])[1]
    return lp


def numpy_bic_lg(data):
    """bic.cpp:12-27 over mle_LinearGaussianCPD.hpp: least squares, unbiased variance."""
    data = np.asarray(data, dtype=np.float64)
    N, d = data.shape
    p = d - 1
    X = np.column_stack([np.ones(N), data[:, 1:]])
    beta = np.linalg.lstsq(X, data[:, 0], rcond=None)[0]
    r = data[:, 0] - X @ beta
    var = float(r @ r) / (N - p - 1)
    return 0.5 * (1 + p - N) - 0.5 * N * math.log(2 * math.pi) - N * 0.5 * math.log(var) - math.log(N) * 0.5 * (p + 2)


# ---- discrete tables: BIC and BDe --------------------------------------------------------------------------------------------------
def make_discrete_score(pbn, name, df):
    return pbn.BIC(df) if name == "bic" else pbn.BDe(df, iss=1.5)


def test_bic_accepts_a_dictionary_column_with_nulls(pbn):
    """Before null codes reached the engine, BIC raised "Discrete columns with nulls are not supported by the device score engine." here."""
    df, codes = discrete_table()
    assert all((codes[v] < 0).sum() > 0 for v in NODES)
    bic = pbn.BIC(df)
    model = pbn.DiscreteBN(NODES)
    assert np.isfinite(bic.local_score(model, "b", ["a"]))
    assert bic.discrete_stats()[0] > 0


@pytest.mark.parametrize("name", ["bic", "bde"])
def test_discrete_scores_equal_the_filtered_frame(pbn, name):
    """The local score of a family = the engine's score of the same family on the frame filtered to the rows valid in that family, bit for
    bit: the same integer counts through the same function."""
    df, codes = discrete_table()
    model = pbn.DiscreteBN(NODES)
    score = make_discrete_score(pbn, name, df)
    for v, ev in [(n, []) for n in NODES[:3]] + random_families(NODES, 20, 4, seed=1):
        keep = np.ones(len(df), dtype=bool)
        for c in [v] + ev:
            keep &= codes[c] >= 0
        assert 0 < keep.sum() < len(df)
        filtered = make_discrete_score(pbn, name, df[keep].reset_index(drop=True))
        got = score.local_score_node_type(model, pbn.DiscreteFactorType(), v, ev)
        assert got == filtered.local_score_node_type(model, pbn.DiscreteFactorType(), v, ev), (v, ev)


@pytest.mark.parametrize("name", ["bic", "bde"])
def test_discrete_scores_against_the_transcribed_reference(pbn, name, monkeypatch):
    """|score - transcription| <= (T + 2) 2^-53 sum |term| over the T terms; device units are counted; the host loop gives the same doubles."""
    df, codes = discrete_table()
    model = pbn.DiscreteBN(NODES)
    cands = [(v, []) for v in NODES] + [("b", ["a"]), ("d", ["a", "c", "b", "f"])] + random_families(NODES, 40, 5, seed=11)
    values = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PBN_DISCRETE_COUNTS", knob)
        score = make_discrete_score(pbn, name, df)
        values[knob] = [score.local_score_node_type(model, pbn.DiscreteFactorType(), v, ev) for v, ev in cands]
        stats = score.discrete_stats()
        assert (stats[0] > 0 and stats[1] == 0) if knob == "1" else (stats[0] == 0 and stats[1] > 0), (knob, stats)
    assert values["1"] == values["0"]
    for (v, ev), got in zip(cands, values["1"]):
        # the engine orders the parents by column: the transcription's table in the same order (the terms are the same set in any order)
        want, magnitude, terms = bde_transcribed(codes, v, sorted(ev), 1.5) if name == "bde" else bic_discrete_transcribed(codes, v, sorted(ev))
        bound = (terms + 2) * U * magnitude
        print(name, v, ev, got, want, abs(got - want) / bound)
        assert abs(got - want) <= bound, (v, ev, got, want, abs(got - want) / bound)


# ---- Gaussian tables: BIC and BGe --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bic", "bge"])
def test_gaussian_scores_over_the_valid_rows(pbn, oracle, name):
    """200 random candidates of 0 ... 7 parents in one batch against the oracle / numpy on the filtered rows; the same doubles whether a
    candidate is asked alone or inside the batch."""
    df, x, names = gaussian_table()
    model = pbn.GaussianNetwork(names)
    score = pbn.BIC(df) if name == "bic" else pbn.BGe(df)
    cands = random_families(names, 200, 7, seed=3)
    assert {len(ev) for _, ev in cands} == set(range(8))
    batch = score._batch(model, [(v, pbn.LinearGaussianCPDType(), ev) for v, ev in cands], score._kind)
    for (v, ev), got in zip(cands, batch):
        sub = x[:, [names.index(c) for c in [v] + ev]]
        sub = sub[~np.isnan(sub).any(axis=1)]
        if name == "bic":
            want = oracle.bic_lg(sub)
            assert abs(got - want) <= RTOL_F64 * abs(want), (v, ev, got, want)
        else:
            want = numpy_bge(sub, len(names))
            assert abs(got - want) <= 1e-9 * abs(want), (v, ev, got, want)
        assert got == score.local_score(model, v, ev), (v, ev)


def test_masked_knob_and_tables_without_nulls(pbn, oracle, golden, monkeypatch):
    """PBN_NULL_MOMENTS=0 keeps the per-candidate path (the same rows, another summation order: RTOL_F64); a table without nulls gives the
    same doubles and the same counters with the knob on and off."""
    from helpers import CKDE_SETS, COLS, frame

    df, x, names = gaussian_table(3000, 5)
    model = pbn.GaussianNetwork(names)
    cands = random_families(names, 30, 4, seed=4)
    values = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PBN_NULL_MOMENTS", knob)
        score = pbn.BIC(df)
        values[knob] = [score.local_score(model, v, ev) for v, ev in cands]
    for a, b in zip(values["1"], values["0"]):
        assert abs(a - b) <= RTOL_F64 * abs(b)
    clean = frame(golden["train10k"][:3000])
    gbn = pbn.GaussianNetwork(COLS)
    out = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PBN_NULL_MOMENTS", knob)
        bic, bge = pbn.BIC(clean), pbn.BGe(clean)
        out[knob] = ([bic.local_score(gbn, v, ev) for v, ev in CKDE_SETS], [bge.local_score(gbn, v, ev) for v, ev in CKDE_SETS], bic.discrete_stats())
    assert out["1"] == out["0"]
    for (v, ev), got in zip(CKDE_SETS, out["1"][0]):
        want = oracle.bic_lg(golden["train10k"][:3000][:, [COLS.index(c) for c in [v] + ev]])
        assert abs(got - want) <= RTOL_F64 * abs(want)


# ---- CLG candidates under BIC ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_bic_clg_over_the_valid_rows(pbn, oracle, dtype):
    """Nulls in the child, in a continuous parent and in a discrete parent: bic_clg on the rows valid in all of the candidate's columns.
    (Before the masked cell moments this case failed for both element types: the cells' N came from the grouping and the moments from the
    zero-filled values.)"""
    df, cont, codes = hybrid_table(dtype=dtype)
    cards = {"A": 2, "B": 3}
    net = pbn.CLGNetwork(list(df.columns), [], [("A", pbn.DiscreteFactorType()), ("B", pbn.DiscreteFactorType())])
    bic = pbn.BIC(df)
    pos = {"x": 0, "y": 1, "z": 2}
    rtol = RTOL_F64   # (fp32 tables too: the oracle sees the rounded data, and the moments are accumulated in fp64)
    for var, dpar, cpar in [("x", ["A"], []), ("y", ["B"], ["x"]), ("z", ["A", "B"], ["x", "y"]), ("y", ["B", "A"], []), ("z", ["B"], ["y"]),
                            ("x", ["A", "B"], ["z", "y"])]:
        sub = cont[:, [pos[c] for c in [var] + cpar]]
        keep = ~np.isnan(sub).any(axis=1)
        for d in dpar:
            keep &= codes[d] >= 0
        assert keep.sum() < len(df) - 100
        cfg = sum(codes[d][keep] * s for d, s in zip(dpar, np.cumprod([1] + [cards[d] for d in dpar[:-1]])))
        assert len(np.unique(cfg)) == int(np.prod([cards[d] for d in dpar]))   # no configuration is empty of valid rows
        want = oracle.bic_clg(sub[keep], [codes[d][keep].astype(np.int32) for d in dpar], [cards[d] for d in dpar])
        got = bic.local_score(net, var, dpar + cpar)
        print(dtype, var, dpar, cpar, got, want, abs(got - want) / abs(want))
        assert abs(got - want) <= rtol * abs(want), (var, dpar, cpar, got, want)
        assert abs(bic.local_score(net, var, cpar + dpar) - want) <= rtol * abs(want)


# ---- hill-climbs: the engine path against a Python Score over the restatement ----------------------------------------------------------
def climb(pbn, score, start):
    trace = []

    class Record(pbn.Callback):
        def call(self, model, operator, score, iteration):
            if operator is not None:
                trace.append((repr(operator).split(";")[0], operator.delta()))   # "AddArc(a -> b", without the delta

    learned = pbn.GreedyHillClimbing().estimate(pbn.ArcOperatorSet(), score, start, callback=Record())
    return learned, trace


def restated(pbn, local, names):
    """A plain Score whose local_score is `local(variable, sorted parents)`, memoised."""
    memo = {}

    class Restated(pbn.Score):
        def local_score(self, model, variable, evidence=None):
            evidence = model.parents(variable) if evidence is None else list(evidence)
            key = (variable, tuple(sorted(evidence)))
            if key not in memo:
                memo[key] = local(variable, list(key[1]))
            return memo[key]

        def local_score_node_type(self, model, variable_type, variable, evidence):
            return self.local_score(model, variable, evidence)

        def has_variables(self, variables):
            variables = [variables] if isinstance(variables, str) else list(variables)
            return all(v in names for v in variables)

        def compatible_bn(self, model):
            return True

    return Restated()


def reaches(arcs, src, dst):
    stack, seen = [src], set()
    while stack:
        u = stack.pop()
        if u == dst:
            return True
        if u not in seen:
            seen.add(u)
            stack.extend(b for a, b in arcs if a == u)
    return False


def assert_no_near_tie(names, local, trace):
    """Replays the trace on the restatement alone: at every step the applied operator is the best one, and the best and the second-best
    delta differ by more than 1e-6 relative."""
    arcs = set()
    memo = {}

    def ls(v, pa):
        key = (v, tuple(sorted(pa)))
        if key not in memo:
            memo[key] = local(v, list(key[1]))
        return memo[key]

    def parents(v):
        return [a for a, b in arcs if b == v]

    for op, _ in trace:
        deltas = {}
        for i in names:
            for j in names:
                if i == j:
                    continue
                if (i, j) in arcs:
                    rem = ls(j, [p for p in parents(j) if p != i]) - ls(j, parents(j))
                    deltas[("RemoveArc", i, j)] = rem
                    if not reaches(arcs - {(i, j)}, i, j):
                        deltas[("FlipArc", i, j)] = rem + ls(i, parents(i) + [j]) - ls(i, parents(i))
                elif (j, i) not in arcs and not reaches(arcs, j, i):
                    deltas[("AddArc", i, j)] = ls(j, parents(j) + [i]) - ls(j, parents(j))
        ranked = sorted(deltas.items(), key=lambda kv: -kv[1])
        (kind, i, j), best = ranked[0]
        second = ranked[1][1]
        assert best - second > 1e-6 * abs(best), (op, ranked[:3])
        assert op == f"{kind}({i} -> {j}", (op, ranked[0])
        if kind == "AddArc":
            arcs.add((i, j))
        elif kind == "RemoveArc":
            arcs.discard((i, j))
        else:
            arcs.discard((i, j))
            arcs.add((j, i))


GAUSSIAN_HC_SEED = 0
DISCRETE_HC_SEED = 0


def test_bic_hill_climb_on_a_gaussian_table_with_nulls(pbn):
    df, x, names = gaussian_table(3000, 6, seed=GAUSSIAN_HC_SEED)

    def local(v, pa):
        sub = x[:, [names.index(c) for c in [v] + pa]]
        return numpy_bic_lg(sub[~np.isnan(sub).any(axis=1)])

    learned_r, trace_r = climb(pbn, restated(pbn, local, names), pbn.GaussianNetwork(names))
    assert len(trace_r) >= 4
    assert_no_near_tie(names, local, trace_r)
    learned, trace = climb(pbn, pbn.BIC(df), pbn.GaussianNetwork(names))
    assert [op for op, _ in trace] == [op for op, _ in trace_r]
    assert sorted(learned.arcs()) == sorted(learned_r.arcs())
    for (_, d), (_, dr) in zip(trace, trace_r):
        assert abs(d - dr) <= RTOL_F64 * abs(dr)


def test_bde_hill_climb_on_a_discrete_table_with_nulls(pbn):
    df, codes = discrete_table(5000, seed=DISCRETE_HC_SEED)

    def local(v, pa):
        return bde_transcribed(codes, v, pa, 1.0)[0]

    learned_r, trace_r = climb(pbn, restated(pbn, local, NODES), pbn.DiscreteBN(NODES))
    assert len(trace_r) >= 4
    assert_no_near_tie(NODES, local, trace_r)
    engine = pbn.BDe(df)
    learned, trace = climb(pbn, engine, pbn.DiscreteBN(NODES))
    assert [op for op, _ in trace] == [op for op, _ in trace_r]
    assert sorted(learned.arcs()) == sorted(learned_r.arcs())
    stats = engine.discrete_stats()
    assert stats[0] > 0 and stats[1] == 0   # the batched engine protocol: every family counted on the device
