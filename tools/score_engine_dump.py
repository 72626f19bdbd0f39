"""Values and counters of the score engine on every path of pbn_score_batch, for bit-exact comparison of two builds.

    python tools/score_engine_dump.py            -> "BLOCK <name> <json>" lines as it goes, then one "RESULT <json>" line

Python floats are printed with repr (json.dumps), so two runs compare with ==.  Through the Python layer only (scores.py), so the same
file runs against any revision of the library.  Seeded inputs at the smallest sizes that reach each path; after every block the
handle's counters: kde_cache_stats = (entries, sweeps) and discrete_stats.  (memo hits, precise redos and cache resets have no accessor
in the ABI: they show as sweeps that do not move, one extra sweep per redo, and entries that fall.)

Blocks that need a switch read once per process (PBN_NULL_MOMENTS=0, PBN_SCORE_CACHE_ENTRIES=8) run in a child process:
    python tools/score_engine_dump.py --child <block>
"""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pybnesian_amd as pbn  # noqa: E402
from pybnesian_amd import _lib  # noqa: E402

OUT = {}


def counters(*scores):
    c = []
    for s in scores:
        c.append({"kde_cache": list(s.kde_cache_stats()) if hasattr(s, "kde_cache_stats") else None, "discrete": list(s.discrete_stats())})
    return c


def emit(name, values, *scores):
    OUT[name] = {"values": values, "counters": counters(*scores)}
    print(f"BLOCK {name} " + json.dumps(OUT[name]), flush=True)


def floats(xs):
    return [float(x) for x in xs]


def gaussian_table(n, cols, seed, shift=3.0):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, cols)) @ (np.eye(cols) + 0.4 * np.tril(rng.normal(size=(cols, cols)), -1)).T + shift
    return pd.DataFrame(x, columns=[f"x{i}" for i in range(cols)])


def nonlinear_table(n, cols, seed, dtype="float64"):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, cols))
    x[:, 1] += 0.8 * x[:, 0]
    x[:, 2] += 0.5 * x[:, 0] * x[:, 1]
    x[:, 3] += np.sin(x[:, 2])
    for j in range(4, cols):
        x[:, j] += 0.6 * np.tanh(x[:, j - 2]) - 0.3 * x[:, j - 4]
    return pd.DataFrame(x.astype(dtype), columns=[f"v{i}" for i in range(cols)])


def hybrid_table(n, seed, dtype="float64"):
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 3, size=n)
    d2 = (d1 + rng.integers(0, 2, size=n)) % 2
    c1 = rng.normal(size=n) + 0.7 * d1
    c2 = 0.5 * c1 + rng.normal(size=n) * (1 + 0.3 * d2)
    c3 = np.sin(c2) + 0.4 * rng.normal(size=n) - 0.5 * d1
    df = pd.DataFrame({"c1": c1, "c2": c2, "c3": c3}).astype(dtype)
    df["d1"] = pd.Categorical.from_codes(d1, ["a", "b", "c"])
    df["d2"] = pd.Categorical.from_codes(d2, ["u", "v"])
    return df


GAUSS_CANDS = [("x0", []), ("x1", ["x0"]), ("x2", ["x0", "x1"]), ("x3", ["x2", "x0", "x1"]), ("x5", ["x4", "x3", "x2", "x1", "x0"]), ("x0", ["x5"])]


def gaussian_scores(df, cands):
    names = list(df.columns)
    gbn = pbn.GaussianNetwork(names)
    bic, bge = pbn.BIC(df), pbn.BGe(df)
    lg = pbn.LinearGaussianCPDType()
    vals = {"bic": floats(bic._batch(gbn, [(v, lg, p) for v, p in cands], bic._kind)), "bic_single": [bic.local_score(gbn, v, p) for v, p in cands],
            "bge": floats(bge._batch(gbn, [(v, lg, p) for v, p in cands], bge._kind))}
    return vals, (bic, bge)


def with_nulls(df, cols, seed):
    rng = np.random.default_rng(seed)
    df = df.copy()
    for i, c in enumerate(cols):
        df.loc[df.index[rng.choice(len(df), size=len(df) // (11 + 3 * i), replace=False)], c] = np.nan
    return df


def block_gaussian():
    df = gaussian_table(5000, 6, 1)
    vals, scores = gaussian_scores(df, GAUSS_CANDS)
    emit("gaussian_plain", vals, *scores)


def block_gaussian_nulls_masked():
    df = with_nulls(gaussian_table(5000, 6, 1), ["x1", "x4"], 2)
    vals, scores = gaussian_scores(df, GAUSS_CANDS)
    emit("gaussian_nulls_masked", vals, *scores)


def block_gaussian_nulls_gather():
    df = with_nulls(gaussian_table(4000, 11, 3), ["x2", "x9"], 4)
    ten = ("x10", [f"x{i}" for i in range(9)])          # 10 columns: beyond the masked pass
    vals, scores = gaussian_scores(df, [ten, ("x0", ["x1"]), ("x2", ["x9", "x0"])])
    emit("gaussian_nulls_gather", vals, *scores)


def near_collinear_table(p, kappa):
    # the inputs of tests/test_scores_gpu.py::test_near_collinear_parents_vs_pivoted_qr
    rng = np.random.default_rng(int(p * 1000 + np.log10(kappa)))
    n = 20000
    X = rng.normal(size=(n, p)) @ (np.eye(p) + 0.3 * np.tril(rng.normal(size=(p, p)), -1)).T + 5.0
    X[:, p - 1] = X[:, 0] + rng.normal(size=n) / kappa
    y = X @ rng.uniform(0.5, 1.5, size=p) + rng.normal(scale=0.5, size=n)
    names = ["y"] + [f"x{i}" for i in range(p)]
    return pd.DataFrame(np.column_stack([y, X]), columns=names), names


def block_near_collinear():
    vals = {}
    scores = []
    for p, kappa in ((4, 1e6), (6, 1e8)):
        df, names = near_collinear_table(p, kappa)
        gbn = pbn.GaussianNetwork(names)
        for tag, frame in (("plain", df), ("nulls", with_nulls(df, ["y", "x1"], 5))):
            bic = pbn.BIC(frame)
            vals[f"bic_p{p}_{tag}"] = bic.local_score(gbn, "y", names[1:])
            scores.append(bic)
        cv = pbn.CVLikelihood(df, 4, 3)
        ho = pbn.HoldoutLikelihood(df, 0.2, 3)
        vals[f"cv_p{p}"] = cv.local_score(gbn, "y", names[1:])
        vals[f"holdout_p{p}"] = ho.local_score(gbn, "y", names[1:])
        scores += [cv, ho]
    emit("near_collinear", vals, *scores)


def block_lg_likelihood():
    df = gaussian_table(5000, 6, 1)
    gbn = pbn.GaussianNetwork(list(df.columns))
    lg = pbn.LinearGaussianCPDType()
    cv, ho = pbn.CVLikelihood(df, 4, 7), pbn.HoldoutLikelihood(df, 0.25, 7)
    vals = {"cv": floats(cv._batch(gbn, [(v, lg, p) for v, p in GAUSS_CANDS], cv._kind)),
            "holdout": floats(ho._batch(gbn, [(v, lg, p) for v, p in GAUSS_CANDS], ho._kind))}
    emit("lg_likelihood", vals, cv, ho)


def ckde_cands(names, big):
    ck = pbn.CKDEType()
    cands = [(a, ck, [b]) for a, b in itertools.permutations(names, 2)]      # all ordered pairs
    cands += [(names[0], ck, []), (names[2], ck, [names[0], names[1]]), (names[3], ck, [names[2], names[0], names[1]]), (names[1], ck, [names[3], names[2]])]
    if big:
        cands.append((names[4], ck, [names[3], names[2], names[1], names[0]]))   # a 5-variable term: a chain of its own
        cands.append((names[5], ck, [names[0], names[2], names[4]]))
    return cands


def block_ckde(tag, n, cols, dtype, k, ratio, big):
    df = nonlinear_table(n, cols, 12, dtype)
    names = list(df.columns)
    net = pbn.SemiparametricBN(names)
    cands = ckde_cands(names, big)
    vals = {}
    for kind_tag, score in (("cv", pbn.CVLikelihood(df, k, 3)), ("holdout", pbn.HoldoutLikelihood(df, ratio, 3))):
        vals[f"{kind_tag}_batch"] = floats(score._batch(net, cands, score._kind))
        vals[f"{kind_tag}_stats_first"] = list(score.kde_cache_stats())
        vals[f"{kind_tag}_again"] = floats(score._batch(net, cands, score._kind))                 # from the cache
        vals[f"{kind_tag}_stats_again"] = list(score.kde_cache_stats())
        vals[f"{kind_tag}_single"] = [score.local_score_node_type(net, t, v, p) for v, t, p in cands[-3:]]
        emit(f"ckde_{tag}_{kind_tag}", {k2: v for k2, v in vals.items() if k2.startswith(kind_tag)}, score)


def block_terms():
    """pbn_score_terms / _term_regions / _terms_put / _terms_missing, then a batch assembled from installed totals."""
    for tag, n, k in (("small", 2500, 3), ("large", 60000, 4)):
        df = nonlinear_table(n, 4, 21)
        names = list(df.columns)
        net = pbn.SemiparametricBN(names)
        ck = pbn.CKDEType()
        terms = [(2, 0, 1), (2, 1), (1, 0), (3, 2, 0, 1), (3, 0, 1), (2, 0), (4, 3, 1, 2)]     # (m, columns...): joint m = columns, marginal one more
        vals = {}
        for kind_tag, a, b in (("cv", pbn.CVLikelihood(df, k, 5), pbn.CVLikelihood(df, k, 5)), ("holdout", pbn.HoldoutLikelihood(df, 0.2, 5), pbn.HoldoutLikelihood(df, 0.2, 5))):
            kind = a._kind
            regions = a._term_regions(kind)
            vals[f"{kind_tag}_missing_before"] = a._terms("missing", kind, terms)
            totals = a._terms("eval", kind, terms)
            vals[f"{kind_tag}_totals"] = floats(totals)
            items = [(t, r) for t in terms for r in range(regions)]
            vals[f"{kind_tag}_regions"] = floats(a._terms("eval_regions", kind, [t for t, _ in items], regions=[r for _, r in items]))
            # the second handle knows nothing: the totals are installed, and its candidates are assembled from them
            b._terms("put", kind, terms, values=totals)
            vals[f"{kind_tag}_missing_after"] = b._terms("missing", kind, terms + [(2, 2, 3)])
            cands = [(names[0], ck, [names[1]]), (names[1], ck, [names[0]]), (names[2], ck, [names[0], names[1]]), (names[0], ck, []), (names[3], ck, [names[2]])]
            vals[f"{kind_tag}_from_totals"] = floats(b._batch(net, cands, kind))
            vals[f"{kind_tag}_own"] = floats(a._batch(net, cands, kind))
            emit(f"terms_{tag}_{kind_tag}", {k2: v for k2, v in vals.items() if k2.startswith(kind_tag)}, a, b)


def hybrid_cands():
    ck, lg, df_ = pbn.CKDEType(), pbn.LinearGaussianCPDType(), pbn.DiscreteFactorType()
    return [("c2", ck, ["c1", "d1"]), ("c3", ck, ["d2", "c2", "d1"]), ("c3", lg, ["d1", "c1"]), ("c1", ck, ["d1"]), ("d2", df_, ["d1"]),
            ("c1", ck, ["c2", "d1"]), ("c2", ck, ["d1", "c1"]), ("c2", lg, ["d1", "d2", "c1", "c3"])]


def block_hybrid():
    for dtype in ("float64", "float32"):
        df = hybrid_table(9000, 31, dtype)
        net = pbn.SemiparametricBN(list(df.columns), [], [("d1", pbn.DiscreteFactorType()), ("d2", pbn.DiscreteFactorType())])
        cands = hybrid_cands()
        vals = {}
        scores = []
        for kind_tag, s in (("cv", pbn.CVLikelihood(df, 3, 1)), ("holdout", pbn.HoldoutLikelihood(df, 0.2, 1))):
            vals[f"{kind_tag}_batch"] = floats(s._batch(net, cands, s._kind))
            vals[f"{kind_tag}_stats_first"] = list(s.kde_cache_stats())
            vals[f"{kind_tag}_memo"] = floats(s._batch(net, cands, s._kind))       # the memo: no new sweeps
            vals[f"{kind_tag}_stats_memo"] = list(s.kde_cache_stats())
            ckc = [(v, t, p) for v, t, p in cands if t == pbn.CKDEType()]
            var, ntype, off, par = s._encode(ckc)
            for part, n_parts in ((0, 1), (0, 2), (1, 2)):
                vals[f"{kind_tag}_parts_{part}_{n_parts}"] = floats(s._batch_parts(net, var, ntype, off, par, s._kind, part, n_parts).ravel())
            scores.append(s)
        bic = pbn.BIC(df)
        vals["bic"] = [bic.local_score_node_type(net, t, v, p) for v, t, p in cands if t != pbn.CKDEType()]
        scores.append(bic)
        emit(f"hybrid_{dtype}", vals, *scores)
    ddf = hybrid_table(9000, 31)[["d1", "d2"]]
    bde = pbn.BDe(ddf, 2.0)
    dnet = pbn.DiscreteBN(["d1", "d2"])
    emit("bde", [bde.local_score(dnet, "d1", []), bde.local_score(dnet, "d2", ["d1"]), bde.local_score(dnet, "d1", ["d2"])], bde)


def block_validated():
    df = nonlinear_table(3000, 4, 41)
    names = list(df.columns)
    net = pbn.SemiparametricBN(names)
    ck = pbn.CKDEType()
    s = pbn.ValidatedLikelihood(df, 0.2, 3, 9)
    vals = []
    for v, p in (("v1", ["v0"]), ("v0", ["v1"]), ("v2", ["v0", "v1"]), ("v3", [])):
        vals += [s.local_score_node_type(net, ck, v, p), s.vlocal_score_node_type(net, ck, v, p)]
    emit("validated", vals, s)


def block_precise():
    df = nonlinear_table(2500, 4, 12)
    names = list(df.columns)
    net = pbn.SemiparametricBN(names)
    cands = ckde_cands(names, False)[:8]
    s = pbn.CVLikelihood(df, 3, 3)
    vals = {"off": floats(s._batch(net, cands, s._kind)), "stats_off": list(s.kde_cache_stats())}
    _lib.check(_lib.load().pbn_scoredata_set_precise(s._handle, 1))
    vals["on"] = floats(s._batch(net, cands, s._kind))
    vals["stats_on"] = list(s.kde_cache_stats())
    _lib.check(_lib.load().pbn_scoredata_set_precise(s._handle, 0))
    vals["off_again"] = floats(s._batch(net, cands, s._kind))
    emit("precise_switch", vals, s)


def block_f32_widen():
    # the inputs of tests/test_c5_gpu.py::test_fp32_engine_redoes_far_out_sets_on_fp64_fragments
    rng = np.random.default_rng(123)
    n, far = 60_000, 60
    a = rng.normal(size=n)
    b = np.tanh(a) + 0.5 * rng.normal(size=n)
    idx = rng.choice(n, size=far, replace=False)
    a[idx] = 400.0 + 0.3 * rng.normal(size=far)
    b[idx] = -250.0 + 0.3 * rng.normal(size=far)
    D = rng.integers(0, 2, size=n)
    df = pd.DataFrame({"a": a, "b": b}).astype(np.float32)
    df["D"] = pd.Categorical.from_codes(D, ["d0", "d1"])
    net = pbn.SemiparametricBN(list(df.columns), [], [("D", pbn.DiscreteFactorType())])
    cv = pbn.CVLikelihood(df, 3, 2)
    ho = pbn.HoldoutLikelihood(df, 0.2, 2)
    vals = [cv.local_score_node_type(net, pbn.CKDEType(), "b", ["a"]), ho.local_score_node_type(net, pbn.CKDEType(), "b", ["a", "D"]),
            cv.local_score_node_type(net, pbn.CKDEType(), "a", ["b"])]
    emit("f32_widen_redo", vals, cv, ho)


def block_near_zero():
    """fp64 terms whose sum cancels to ~0 (a Gaussian of sigma = 1 / sqrt(2 pi e) has mean log-density 0): evaluated twice."""
    rng = np.random.default_rng(77)
    n = 2500
    a = rng.normal(size=n) / np.sqrt(2 * np.pi * np.e)
    b = 0.5 * a + rng.normal(size=n)
    c = rng.normal(size=n) * 3.0
    df = pd.DataFrame({"a": a, "b": b, "c": c})
    net = pbn.SemiparametricBN(list(df.columns))
    ck = pbn.CKDEType()
    cands = [("a", ck, []), ("b", ck, ["a"]), ("c", ck, []), ("c", ck, ["a"])]
    vals = {}
    scores = []
    for tag, s in (("cv", pbn.CVLikelihood(df, 3, 4)), ("holdout", pbn.HoldoutLikelihood(df, 0.3, 4))):
        vals[tag] = floats(s._batch(net, cands, s._kind))
        vals[f"{tag}_stats"] = list(s.kde_cache_stats())     # sweeps = evaluations + precise redos
        scores.append(s)
    emit("near_zero_redo", vals, *scores)


def block_cache8():
    """PBN_SCORE_CACHE_ENTRIES=8: the caches start over between the batches."""
    df = nonlinear_table(2500, 4, 12)
    names = list(df.columns)
    net = pbn.SemiparametricBN(names)
    cands = ckde_cands(names, False)
    s = pbn.CVLikelihood(df, 3, 3)
    vals = {}
    for i in range(3):
        vals[f"round{i}"] = floats(s._batch(net, cands[4 * i:4 * i + 8], s._kind))
        vals[f"stats{i}"] = list(s.kde_cache_stats())
    hdf = hybrid_table(6000, 31)
    hnet = pbn.SemiparametricBN(list(hdf.columns), [], [("d1", pbn.DiscreteFactorType()), ("d2", pbn.DiscreteFactorType())])
    h = pbn.CVLikelihood(hdf, 3, 1)
    for i in range(3):
        vals[f"hybrid{i}"] = floats(h._batch(hnet, hybrid_cands(), h._kind))
        vals[f"hstats{i}"] = list(h.kde_cache_stats())
    a = pbn.CVLikelihood(df, 3, 3)
    for i in range(3):   # term_total is trimmed in terms_put
        terms = [(2, i, j) for j in range(4) if j != i] + [(2, j) for j in range(4)] + [(1, j) for j in range(4)]
        a._terms("put", a._kind, terms, values=np.arange(len(terms), dtype=np.float64) + i)
        vals[f"missing{i}"] = a._terms("missing", a._kind, [(2, 0, 1), (2, 1, 2), (2, 2, 3), (1, 0)])
    emit("cache_entries_8", vals, s, h, a)


def block_null_moments_off():
    """PBN_NULL_MOMENTS=0: every BIC / BGe candidate with nulls through the gather path."""
    df = with_nulls(gaussian_table(5000, 6, 1), ["x1", "x4"], 2)
    vals, scores = gaussian_scores(df, GAUSS_CANDS)
    df2, names = near_collinear_table(4, 1e6)
    bic = pbn.BIC(with_nulls(df2, ["y", "x1"], 5))
    vals["near_collinear_nulls"] = bic.local_score(pbn.GaussianNetwork(names), "y", names[1:])
    emit("null_moments_off", vals, *scores, bic)


CHILDREN = {"null_moments_off": (block_null_moments_off, {"PBN_NULL_MOMENTS": "0"}), "cache_entries_8": (block_cache8, {"PBN_SCORE_CACHE_ENTRIES": "8"})}


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        CHILDREN[sys.argv[2]][0]()
        return
    blocks = [block_gaussian, block_gaussian_nulls_masked, block_gaussian_nulls_gather, block_near_collinear, block_lg_likelihood,
              lambda: block_ckde("small", 2500, 4, "float64", 3, 0.2, False),         # single chains
              lambda: block_ckde("large_f64", 60000, 6, "float64", 4, 0.2, True),     # grouped pools up to 4 variables, the 5-variable term on its own chain
              lambda: block_ckde("large_f32", 60000, 6, "float32", 4, 0.2, True),
              block_terms, block_hybrid, block_validated, block_precise, block_f32_widen, block_near_zero]
    for i, block in enumerate(blocks):
        try:
            block()
        except (ValueError, TypeError, AttributeError, KeyError, pbn.SingularCovarianceData) as ex:   # an input the library refuses: part of the record (a device error ends the run)
            emit(f"refused_{i}", f"{type(ex).__name__}: {ex}")
    for name, (_, env) in CHILDREN.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        sys.stderr.write(r.stderr)
        if r.returncode != 0:
            raise SystemExit(f"child {name} failed with status {r.returncode}")
        for line in r.stdout.splitlines():
            if line.startswith("BLOCK "):
                print(line, flush=True)
                _, key, payload = line.split(" ", 2)
                OUT[key] = json.loads(payload)
    print("RESULT " + json.dumps(OUT), flush=True)


if __name__ == "__main__":
    main()
