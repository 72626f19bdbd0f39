"""GPU tier: discrete networks in the score engine - all-discrete tables under BIC / CVLikelihood / HoldoutLikelihood / ValidatedLikelihood,
the batched family counts against the host loop (PBN_DISCRETE_COUNTS), BDe as a device score, and the hill-climb of a DiscreteBN.

Reference: learning/scores/bic.cpp:66-96 (bic_discrete), cv_likelihood.cpp:5-25 and holdout_likelihood.cpp:8-23 over
learning/parameters/mle_DiscreteFactor.cpp:5-41, learning/scores/bde.cpp:5-47."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

NODES = list("abcdefgh")
CARD = {"a": 3, "b": 3, "c": 2, "d": 4, "e": 2, "f": 3, "g": 3, "h": 2}
STRONG = [("a", "b"), ("b", "c"), ("e", "f"), ("f", "g")]


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


def sample(n, seed=0, nodes=NODES):
    """A fixed DAG: a -> b -> c, (a, c) -> d weakly, e -> f -> g, h alone.  A strong arc copies its parent (mod the cardinality) with
    probability 0.8."""
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
    df = pd.DataFrame({v: pd.Categorical.from_codes(code[v], [f"{v}{i}" for i in range(CARD[v])]) for v in nodes})
    return df, {v: code[v].astype(np.int64) for v in nodes}


def random_candidates(names, count, max_parents, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        cols = rng.choice(len(names), size=int(rng.integers(1, min(max_parents, len(names) - 1) + 2)), replace=False)
        out.append((names[cols[0]], [names[c] for c in cols[1:]]))
    return out


def make_scores(pbn, df):
    return {"bic": pbn.BIC(df), "cv": pbn.CVLikelihood(df, k=5, seed=0), "holdout": pbn.HoldoutLikelihood(df, 0.2, seed=0),
            "validated": pbn.ValidatedLikelihood(df, 0.2, 5, seed=0)}


def local(pbn, score, model, variable, parents, validation=False):
    fn = score.vlocal_score_node_type if validation else score.local_score_node_type
    return fn(model, pbn.DiscreteFactorType(), variable, parents)


def test_all_discrete_tables_score_as_inside_a_hybrid_table(pbn):
    """A table without continuous columns builds discrete-only score data; each local score equals, bit for bit, the score of the same
    columns inside a table that also carries one continuous column (same rows, same seed, same folds)."""
    nodes = NODES[:6]
    df, _ = sample(5000, nodes=nodes)
    hybrid = df.copy()
    hybrid["x"] = np.random.default_rng(1).normal(size=len(df))
    model = pbn.DiscreteBN(nodes)
    cands = [(v, []) for v in nodes] + random_candidates(nodes, 40, 3, seed=2)
    alone, inside = make_scores(pbn, df), make_scores(pbn, hybrid)
    for name in alone:
        assert alone[name].has_variables(nodes) and alone[name].compatible_bn(model)
        for v, ev in cands:
            assert local(pbn, alone[name], model, v, ev) == local(pbn, inside[name], model, v, ev), (name, v, ev)
        assert alone[name].discrete_stats()[0] > 0
    for v, ev in cands[:12]:
        assert local(pbn, alone["validated"], model, v, ev, True) == local(pbn, inside["validated"], model, v, ev, True)
    assert alone["bic"].local_score(model, "b", ["a"]) == local(pbn, alone["bic"], model, "b", ["a"])
    assert alone["cv"].score(model) == pytest.approx(sum(alone["cv"].local_score(model, v) for v in nodes), rel=1e-12)
    perm, limits = alone["cv"].fold_layout()
    assert sorted(perm.tolist()) == list(range(5000)) and len(limits) == 6
    assert len(alone["holdout"].training_data()) + len(alone["holdout"].test_data()) == 5000


def make_c5(n, seed=0, dtype=np.float32):
    """C5's shape in small (the generator of test_c5_gpu.py): discrete A (2), B (3); continuous x | A, y | x, B, z | x, y, w | z."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 2, size=n)
    B = (rng.random(n) < np.where(A == 0, 0.3, 0.6)).astype(int) + (rng.random(n) < 0.2)
    x = rng.normal(loc=np.where(A == 0, -1.0, 2.0), scale=1.0)
    y = 0.7 * x + np.array([0.0, 3.0, -2.0])[B] + rng.normal(scale=0.5, size=n)
    z = np.tanh(x) * 2.0 - 0.4 * y + rng.normal(scale=0.3, size=n)
    w = 0.5 * z + rng.normal(scale=0.7, size=n)
    df = pd.DataFrame({"x": x, "y": y, "z": z, "w": w}).astype(dtype)
    df["A"] = pd.Categorical.from_codes(A, ["a0", "a1"])
    df["B"] = pd.Categorical.from_codes(B, ["b0", "b1", "b2"])
    return df


@pytest.mark.parametrize("table", ["discrete", "c5"])
def test_device_counts_equal_the_host_loop(pbn, table, monkeypatch):
    """PBN_DISCRETE_COUNTS on against off, every score kind: equal doubles (the counts are integers, the arithmetic is one function)."""
    if table == "discrete":
        df, _ = sample(5000)
        names = NODES
        cands = random_candidates(names, 200, 4, seed=5)
    else:
        df = make_c5(6000, seed=3)
        names = ["A", "B"]
        cands = [("A", []), ("B", []), ("A", ["B"]), ("B", ["A"])]
    model = pbn.DiscreteBN(names)
    values, stats = {}, {}
    for knob in ("1", "0"):
        monkeypatch.setenv("PBN_DISCRETE_COUNTS", knob)
        scores = make_scores(pbn, df)   # fresh score data: nothing remembered from the other setting
        if table == "discrete":
            scores["bde"] = pbn.BDe(df, iss=1.5)
        values[knob] = {name: [local(pbn, s, model, v, ev) for v, ev in cands] for name, s in scores.items()}
        values[knob]["vlocal"] = [local(pbn, scores["validated"], model, v, ev, True) for v, ev in cands]
        stats[knob] = {name: s.discrete_stats() for name, s in scores.items()}
    for name in values["1"]:
        assert values["1"][name] == values["0"][name], name
        assert not any(np.isnan(values["1"][name]))   # (-inf is a value here: a test row in a cell its training rows never visit)
    for name in stats["1"]:
        assert stats["1"][name][0] > 0 and stats["1"][name][1] == 0, (name, stats["1"][name])
        assert stats["0"][name][0] == 0 and stats["0"][name][2] == 0 and stats["0"][name][1] > 0, (name, stats["0"][name])


def bde_transcribed(codes, cards, variable, parents, iss):
    """bde.cpp:5-47 with numpy.bincount counts and scipy's gammaln: (score, sum of |terms|, number of lgamma terms)."""
    from scipy.special import gammaln

    cols = [variable] + list(parents)
    key, stride = np.zeros(len(codes[variable]), dtype=np.int64), 1
    for c in cols:
        key += codes[c] * stride
        stride *= cards[c]
    counts = np.bincount(key, minlength=stride).astype(np.float64)
    card0, total = cards[variable], stride
    alpha = iss / total
    terms = [-total * gammaln(alpha)]
    if not parents:   # bde.cpp:5-21
        terms += [gammaln(m + alpha) for m in counts]
        terms += [gammaln(iss), -gammaln(iss + counts.sum())]
    else:             # bde.cpp:23-47
        for k in range(total // card0):
            block = counts[k * card0: (k + 1) * card0]
            terms += [gammaln(m + alpha) for m in block]
            terms += [gammaln(alpha * card0), -gammaln(alpha * card0 + block.sum())]
    terms = np.asarray(terms, dtype=np.float64)
    return float(np.sum(terms)), float(np.sum(np.abs(terms))), len(terms)


@pytest.mark.parametrize("iss", [1.0, 2.5])
def test_bde_against_the_transcribed_reference(pbn, iss):
    """|BDe - transcription| <= (T + 2) 2^-53 sum |term_i| over the T lgamma terms: the forward error of any summation order plus the
    libraries' ulp errors.  `u` never takes its third category next to `a`'s first: unseen configurations."""
    df, codes = sample(5000)
    u = np.where(codes["a"] == 0, codes["h"], np.random.default_rng(9).integers(0, 3, size=len(df)))
    df["u"] = pd.Categorical.from_codes(u, ["u0", "u1", "u2"])
    codes["u"] = u.astype(np.int64)
    cards = dict(CARD, u=3)
    nodes = NODES + ["u"]
    bde = pbn.BDe(df, iss=iss)
    model = pbn.DiscreteBN(nodes)
    assert str(bde) == "BDe" and bde.compatible_bn(model) and not bde.compatible_bn(pbn.GaussianNetwork(nodes)) and bde.data() is not None
    cands = [(v, []) for v in nodes] + [("b", ["a", "u"]), ("u", ["a"]), ("d", ["a", "c", "u", "b", "f"])] + random_candidates(nodes, 40, 5, seed=11)
    for v, ev in cands:
        got = bde.local_score(model, v, ev)
        want, magnitude, terms = bde_transcribed(codes, cards, v, ev, iss)
        bound = (terms + 2) * 2.0 ** -53 * magnitude
        assert abs(got - want) <= bound, (v, ev, got, want, abs(got - want) / bound)
        assert got == bde.local_score(model, v, ev[::-1]) == bde.local_score_node_type(model, pbn.DiscreteFactorType(), v, sorted(ev))
    model.add_arc("a", "b")
    assert bde.local_score(model, "b") == bde.local_score(model, "b", ["a"])
    assert bde.score(model) == pytest.approx(sum(bde.local_score(model, v) for v in nodes), rel=1e-12)
    assert bde.discrete_stats()[0] > 0


def test_bde_error_messages(pbn):
    df, _ = sample(500)
    df["x"] = np.random.default_rng(0).normal(size=len(df))
    bde = pbn.BDe(df)
    model = pbn.DiscreteBN(NODES)
    assert bde.has_variables(["a", "x"])
    with pytest.raises(ValueError, match="not valid for score BDe"):
        bde.local_score_node_type(model, pbn.LinearGaussianCPDType(), "a", [])
    with pytest.raises(ValueError, match="not valid for score BDe"):
        bde.local_score(pbn.GaussianNetwork(NODES), "a", [])
    with pytest.raises(ValueError, match="Variable x is not categorical"):
        bde.local_score_node_type(model, pbn.DiscreteFactorType(), "x", [])
    with pytest.raises(ValueError, match="Variable x is not categorical"):
        bde.local_score_node_type(model, pbn.DiscreteFactorType(), "a", ["x"])
    assert np.isfinite(bde.local_score(model, "a", ["b"]))


def climb(pbn, score, start, **kw):
    """(learned model, [(operator, delta)] in the order applied, [candidates of every batch])."""
    trace, batches = [], []

    class Record(pbn.Callback):
        def call(self, model, operator, score, iteration):
            if operator is not None:
                trace.append((repr(operator), operator.delta()))

    learned = pbn.GreedyHillClimbing().estimate(pbn.ArcOperatorSet(), score, start, callback=Record(), batch_hook=batches.append, **kw)
    return learned, trace, batches


def skeleton(model):
    return {frozenset(a) for a in model.arcs()}


def test_bde_hill_climb_engine_path_against_the_trampoline(pbn):
    """The hill-climb hands BDe whole batches; hidden behind a plain Score subclass the same object is called candidate by candidate.  Both
    end in the same engine arithmetic: same arcs, same operator deltas to the last bit."""
    df, _ = sample(5000)

    class Hidden(pbn.Score):
        def __init__(self, inner):
            self.inner = inner

        def local_score(self, model, variable, evidence=None):
            return self.inner.local_score(model, variable, evidence)

        def local_score_node_type(self, model, variable_type, variable, evidence):
            return self.inner.local_score_node_type(model, variable_type, variable, evidence)

        def has_variables(self, variables):
            return self.inner.has_variables(variables)

        def compatible_bn(self, model):
            return self.inner.compatible_bn(model)

    engine = pbn.BDe(df)
    learned, trace, batches = climb(pbn, engine, pbn.DiscreteBN(NODES))
    hidden = pbn.BDe(df)
    learned_t, trace_t, batches_t = climb(pbn, Hidden(hidden), pbn.DiscreteBN(NODES))
    assert type(learned) is pbn.DiscreteBN and sorted(learned.arcs()) == sorted(learned_t.arcs())
    assert trace == trace_t and len(trace) >= 4 and all(d > 0 for _, d in trace)
    assert batches == batches_t
    # one batch per step (plus the start caches), each counted by at most one launch; the trampoline: one engine call per candidate
    assert len(batches) <= len(trace) + 3
    assert 0 < engine.discrete_stats()[2] <= len(batches)
    assert hidden.discrete_stats()[2] == sum(batches)
    assert all(frozenset(e) in skeleton(learned) for e in STRONG)
    assert not any("h" in e for e in skeleton(learned))
    assert engine.score(learned) == pytest.approx(sum(engine.local_score(learned, v) for v in NODES), rel=1e-12)


@pytest.mark.parametrize("name", ["bic", "validated"])
def test_hill_climb_of_an_all_discrete_table(pbn, name):
    df, _ = sample(5000)
    score = pbn.BIC(df) if name == "bic" else pbn.ValidatedLikelihood(df, 0.2, 5, seed=0)
    learned, trace, batches = climb(pbn, score, pbn.DiscreteBN(NODES))
    assert 0 < score.discrete_stats()[2] <= len(batches)   # at most one launch per batch
    assert type(learned) is pbn.DiscreteBN and len(trace) >= 4
    assert all(frozenset(e) in skeleton(learned) for e in STRONG)
    assert score.score(learned) == pytest.approx(sum(score.local_score(learned, v) for v in NODES), rel=1e-12)


def test_discrete_only_handle_refuses_what_needs_a_table(pbn):
    from pybnesian_amd import _lib

    lib = _lib.load()
    df, _ = sample(3000)
    score = pbn.CVLikelihood(df, k=3, seed=1)
    h, i32 = score._handle, _lib.int_array
    out = np.zeros(1)

    def batch(kind, node_type):
        return lib.pbn_score_batch(h, kind, 1, i32([0]), i32([node_type]), i32([0, 1]), i32([1]), None, 0, _lib.dptr(out))

    def refused(rc, word):
        assert rc == _lib.PBN_ERR_INVALID
        msg = lib.pbn_last_error().decode()
        assert word in msg, msg

    refused(batch(_lib.PBN_SCORE_BGE, _lib.PBN_NODE_DISCRETE), "BGe")
    refused(batch(_lib.PBN_SCORE_CVLIK, _lib.PBN_NODE_LG), "continuous node type")
    refused(batch(_lib.PBN_SCORE_CVLIK, _lib.PBN_NODE_CKDE), "continuous node type")
    refused(lib.pbn_score_batch(h, _lib.PBN_SCORE_CVLIK, 1, i32([8]), i32([_lib.PBN_NODE_LG]), i32([0, 0]), i32([0]), None, 0, _lib.dptr(out)), "out of range")
    length = C.c_int64(0)
    refused(lib.pbn_scoredata_moments(h, None, C.byref(length), 0), "no table")
    cb = _lib.ALLGATHER_FN(lambda user, send, count, recv: 0)
    comm = _lib.Comm(0, 1, cb, None)
    refused(lib.pbn_scoredata_set_comm(h, C.byref(comm)), "discrete-only")
    beta, var = np.zeros(2), C.c_double(0)
    refused(lib.pbn_lg_fit(h, 0, i32([1]), 1, _lib.dptr(beta), C.byref(var)), "discrete-only")
    with pytest.raises(ValueError, match="at least one continuous column"):
        pbn.BGe(df)
    # the handle is usable afterwards
    assert batch(_lib.PBN_SCORE_CVLIK, _lib.PBN_NODE_DISCRETE) == _lib.PBN_OK and np.isfinite(out[0]) and out[0] < 0
    assert out[0] == score.local_score(pbn.DiscreteBN(NODES), "a", ["b"])
