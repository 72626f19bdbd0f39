"""GPU tier: the grouped KDE evaluation (csrc/kde_group.hip, kde_group_run) stage by stage.  The test aid pbn_debug_group_stages (codes at its
definition) copies every chunk back behind its reduce: the completed pool and unit tables and what the eleven kernels left - sorted order,
regions, whitened rows, positions, boxes, bounds, tile moments, split partials, sums.  Each stage is held against the plain numpy
restatement of tests/group_restatement.py or against brute force over all training rows, unit by unit, query by query.  The path is reached
through the public scores (CVLikelihood / HoldoutLikelihood local scores of CKDE terms) with PBN_PRUNE_MIN_ROWS=256.

Stages 3 to 6 take the CAPTURED zs / zq as their input, so the whitening tolerance does not leak into them.

Tolerances that are derived (never tuned):
  whitening, fp64 chunks   |z - W (x - mu)| <= (2 d + 3) 2^-53 sum_j |W_ij| |x_j - mu_j|: the kernel rounds x - mu and each of its <= d fmas
                           (d + 1 roundings of magnitudes below the absolute sum), numpy rounds the difference, the products' sum (d + 2).
  whitening, f16x2 chunks  zs holds the REPRESENTED value a1 + a2 of split2: a1 = f16(z) leaves r with |r| <= 2^-11 |z| (11-bit significand),
                           a2 = f16(64 r) / 64 leaves 2^-11 |r|, or all of r where |64 r| < 2^-14 is flushed (h_piece: never subnormal):
                           |zr - z| <= 2^-22 (1 + 2^-9) |z| + 2^-20, on top of the fp64 bound above.  (Below 2^-14 a1 is 0 and r = z.)
  bounds below the truth   group_restatement.bound_slack: (d + 3) ulps of the exponent's magnitude and log2(1 + N 2^-53) per side.
  centroids                6 x 2^-53 x mean |z|: a 16-lane tree sum (4 roundings), the division, numpy's own rounding.
  radii                    true rho^2 <= rad2 <= true rho^2 (1 + 2e-6) + 2e-30.
  per-query log-density    fp64: 3.3e-7 absolute (the sum-only budget, kde_model.hpp); fp32 tables: atol 5e-4, rtol 1e-4 (test_kde_gpu.py).
  unit sum                 1e-12 relative to the sum of the merged values.

Tolerances that were MEASURED on an MI355X with this file (printed before they are asserted; the test asserts measured <= constant / 8;
the run is kept in profiles/group_stages/tests.txt):
  BOUND_TOL  |qlb, qthr (kernel) - restatement| / max(1, |restatement|), over the finite ones (the infinite ones must coincide)
             measured 6.66e-16 (cv3-767-f64; 1.8e-16 to 4.7e-16 in the other eleven cases)                  -> BOUND_TOL = 6e-15
  COEF_TOL   |C_alpha (kernel) - longdouble formula about the kernel's centroid| / sum_t |term| (the same sum over absolute values)
             measured 9.34e-15 (holdout-16401-f64-mom; 1.6e-15 to 2.0e-15 in the other three)            -> COEF_TOL = 8e-14
The per-query log-densities came within 7.4e-8 of brute force on float64 (budget 3.3e-7) and within 6.8e-4 at |logl| ~ 10 on float32.

Data: four clusters, a block of identical rows (a tile of radius 0), a tenth of the rows copied from other rows (test rows equal to
training rows of other folds), one row at +40 and one at -40 standard deviations (the key cells saturate).  The float32 tables carry those
two rows at +-10 standard deviations instead: still beyond the key range, but inside what the f16x2 fragments hold - at 40 the engine flags
the unit (kde_wants_widening) and evaluates it again on fp64 fragments, and the grouped chunk's own partials are not what the score uses."""
import ctypes as C
import functools
import os

import numpy as np
import pandas as pd
import pytest

import group_restatement as gr

pytestmark = pytest.mark.gpu

BOUND_TOL = 6e-15
COEF_TOL = 8e-14
EPS = 2.0 ** -53


# ---- the aid ------------------------------------------------------------------------------------------------------------------------------
class Aid:
    def __init__(self):
        from pybnesian_amd import _lib

        self.fn = _lib.load().pbn_debug_group_stages
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]

    def arm(self):
        self.fn(-1, 0, 0, None, 0, 0)
        self.fn(-1, 0, 0, None, 0, 1)

    def clear(self):
        self.fn(-1, 0, 0, None, 0, 0)

    def chunks(self):
        return int(self.fn(-1, 0, 0, None, 0, 1))

    def get(self, chunk, what, index, dtype):
        n = self.fn(chunk, what, index, None, 0, 1)
        assert n >= 0, (chunk, what, index)
        out = np.zeros(max(int(n), 1), dtype=dtype)
        assert self.fn(chunk, what, index, out.ctypes.data, n, 1) == n
        return out[:n]


def read_chunk(aid, c):
    head = aid.get(c, 0, 0, np.int64)
    ch = dict(zip(("np", "nu", "f16", "KS", "fold", "moments", "bboxes", "window", "tile_window", "use_sum_bound", "d", "dtype"), map(int, head)))
    ch["pools"], ch["units"] = [], []
    for p in range(ch["np"]):
        i = aid.get(c, 10, p, np.int64)
        P = dict(zip(("n", "R", "d", "kd", "nblk", "row_base", "nunits", "unit0"), map(int, i[:8])))
        P["cols"], P["rb"], P["test_unit"] = i[8:16], i[16:81], i[81:145]
        f = aid.get(c, 11, p, np.float64)
        P["Wg"], P["mug"] = f[:64], f[64:]
        P["rows"] = aid.get(c, 12, p, np.float64).reshape(P["n"], P["d"])
        P["vals"] = aid.get(c, 13, p, np.uint32).astype(np.int64)
        P["reg"] = aid.get(c, 14, p, np.uint8).astype(np.int64)
        P["rowid"] = aid.get(c, 15, p, np.int64)
        ch["pools"].append(P)
    for u in range(ch["nu"]):
        i = aid.get(c, 20, u, np.int64)
        U = dict(zip(("pool", "test_region", "train_mask", "N", "nq", "ntiles", "nqtiles", "tps", "nsplit", "nsplit_fin", "sum_slot", "mstride",
                      "has_bbox", "has_mom"), map(int, i)))
        U["train_mask"] &= (1 << 64) - 1
        f = aid.get(c, 21, u, np.float64)
        U["lognorm"], U["margin"], U["sum"], U["W"], U["mu"] = float(f[0]), float(f[1]), float(f[2]), f[3:67], f[67:]
        P = ch["pools"][U["pool"]]
        d, kd = P["d"], P["kd"]
        U["zs"] = aid.get(c, 22, u, np.float64).reshape(U["N"], d)
        U["zq"] = aid.get(c, 23, u, np.float64).reshape(U["nq"], d)
        U["qpos"] = aid.get(c, 24, u, np.int32).astype(np.int64)
        U["box"] = aid.get(c, 25, u, np.float64).reshape(U["ntiles"], 2 * kd)
        U["bbox"] = aid.get(c, 26, u, np.float64).reshape(-1, 2 * kd)
        U["qbox"] = aid.get(c, 27, u, np.float64).reshape(U["nqtiles"], 2 * kd)
        U["qthr"] = aid.get(c, 28, u, np.float64)
        U["qlb"] = aid.get(c, 29, u, np.float64)
        U["rad2"] = aid.get(c, 30, u, np.float32).astype(np.float64)
        U["mom"] = aid.get(c, 31, u, np.float64).reshape(-1, U["mstride"]) if U["has_mom"] else None
        U["part"] = aid.get(c, 32, u, np.float64).reshape(U["nsplit_fin"], U["nqtiles"] * 16, 2)
        ch["units"].append(U)
    return ch


# ---- data and cases -----------------------------------------------------------------------------------------------------------------------
def table(n, dtype, seed, configs=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(4, 4)) * 4.0
    x = centres[rng.integers(0, 4, n)] + rng.normal(size=(n, 4)) * np.array([0.5, 0.4, 0.6, 0.3])
    x[:, 1] += np.tanh(x[:, 0])
    x[:, 3] += 0.3 * x[:, 2]
    x = x.astype(dtype)
    src = rng.integers(0, n, n // 10)
    x[rng.choice(n, n // 10, replace=False)] = x[src]                 # rows equal to rows of other folds
    x[rng.choice(n, max(60, n // 8), replace=False)] = x[0]           # identical rows: tiles of radius 0
    far = 40.0 if dtype == "float64" else 10.0
    sd, mean = x.std(0), x.mean(0)
    x[n // 3], x[2 * n // 3] = mean + far * sd, mean - far * sd
    df = pd.DataFrame(x, columns=list("abcd"))
    codes = None
    if configs is not None:
        codes = rng.choice(len(configs), size=n, p=configs).astype(np.int32)
        df["A"] = pd.Categorical.from_codes(codes, [f"a{i}" for i in range(len(configs))])
    return df, codes


# name: (score, n, k or ratio, dtype, terms, env, configurations of a discrete parent)
CASES = {
    "cv3-767-f64": ("cv", 767, 3, "float64", [("a", ["b"]), ("a", ["b", "c", "d"])], {}, None),
    "cv3-768-f64-mom-split16": ("cv", 768, 3, "float64", [("a", ["b"])], {"PBN_MOMENT_MIN_ROWS": "0", "PBN_GROUP_SPLIT_TILES": "16"}, None),
    "cv3-769-f64-split16": ("cv", 769, 3, "float64", [("a", ["b", "c"])], {"PBN_GROUP_SPLIT_TILES": "16"}, None),
    "cv3-1920-f64-split80": ("cv", 1920, 3, "float64", [("a", ["b"])], {"PBN_GROUP_SPLIT_TILES": "80"}, None),
    "cv10-2559-f64-mom-split80": ("cv", 2559, 10, "float64", [("a", ["b"])], {"PBN_MOMENT_MIN_ROWS": "0", "PBN_GROUP_SPLIT_TILES": "80"}, None),
    "cv10-2561-f64-split80": ("cv", 2561, 10, "float64", [("a", ["b", "c", "d"])], {"PBN_GROUP_SPLIT_TILES": "80"}, None),
    "cv64-1023-f64-mom": ("cv", 1023, 64, "float64", [("a", ["b"])], {"PBN_MOMENT_MIN_ROWS": "0"}, None),
    "cv64-1023-f32": ("cv", 1023, 64, "float32", [("a", ["b"])], {}, None),
    "cv3-769-f32-split80": ("cv", 769, 3, "float32", [("a", ["b"]), ("a", ["b", "c", "d"])], {"PBN_GROUP_SPLIT_TILES": "80"}, None),
    "holdout-16401-f64-mom": ("holdout", 16401, 0.2, "float64", [("a", ["b"])], {"PBN_MOMENT_MIN_ROWS": "0"}, None),
    "holdout-16401-f64": ("holdout", 16401, 0.2, "float64", [("b", ["a"])], {"PBN_GROUP_SPLIT_TILES": "80"}, None),
    "hybrid-cv3-4000-f64": ("cv", 4000, 3, "float64", [("b", ["a", "A"])], {"PBN_GROUP_SPLIT_TILES": "16"}, [0.45, 0.30, 0.23, 0.02]),
}
SEED = 2


@functools.lru_cache(maxsize=None)
def captured(name):
    """Runs the case's scores with the aid armed -> (chunks, [(score, oracle value, tolerance)], table, codes)."""
    import pybnesian_amd as pbn
    from oracle import oracle

    kind, n, kr, dtype, terms, env, configs = CASES[name]
    df, codes = table(n, dtype, 100 + n, configs)
    env = dict(env, PBN_PRUNE_MIN_ROWS="256")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    aid = Aid()
    aid.arm()
    try:
        disc = [("A", pbn.DiscreteFactorType())] if configs else []
        net = pbn.SemiparametricBN(list(df.columns), [], disc)
        score = pbn.CVLikelihood(df, kr, SEED) if kind == "cv" else pbn.HoldoutLikelihood(df, kr, SEED)
        got = [score.local_score_node_type(net, pbn.CKDEType(), v, ps) for v, ps in terms]
        chunks = [read_chunk(aid, c) for c in range(aid.chunks())]
    finally:
        aid.clear()
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    scores = []
    for (v, ps), g in zip(terms, got):
        cont = df[[v] + [p for p in ps if p != "A"]].to_numpy().astype(np.float64)
        if configs:
            folds = oracle.cv_folds(n, kr, SEED)
            want = sum(oracle.adaptator_fit_slogl(cont, [codes], [len(configs)], tr, te, "ckde") for tr, te in folds)
            tol = 1e-6     # helpers.RTOL_F64, the hybrid tests' tolerance
        else:
            want = oracle.cv_likelihood(cont, "ckde", kr, SEED) if kind == "cv" else oracle.holdout_likelihood(cont, "ckde", kr, SEED)
            tol = 1e-8 if dtype == "float64" else 1e-4     # test_moment_pass_gpu.py / test_w32_gpu.py
        scores.append((g, want, tol))
    return chunks, scores, df, codes


def expected_chunks(name):
    kind, n, kr, dtype, terms, env, configs = CASES[name]
    out = set()
    for v, ps in terms:
        p = len([q for q in ps if q != "A"])
        for d in ((p + 1, p) if p else (1,)):
            f16 = dtype == "float32"
            out.add((d, int(f16), int(not f16 and d <= 2 and env.get("PBN_MOMENT_MIN_ROWS") == "0"), int(not f16)))
    return out


def units_of(name):
    """Every captured (chunk, pool, unit) of the case, after the two checks without which nothing below proves anything."""
    chunks, scores, df, codes = captured(name)
    assert len(chunks) > 0, "no chunk was captured: the grouped path did not run"
    # (fp32 chunks hold the pools of one fragment shape, which several d share: the pools' own d count)
    seen = {(P["d"], ch["f16"], ch["moments"], ch["bboxes"]) for ch in chunks for P in ch["pools"]}
    assert seen == expected_chunks(name), (seen, expected_chunks(name))
    for ch in chunks:
        assert ch["window"] == 8 and ch["tile_window"] == 256 and ch["use_sum_bound"] == 1 and ch["np"] == len(ch["pools"]) > 0
        assert ch["KS"] >= 1 and ch["fold"] == int(ch["d"] % 4 != 0)
    return [(ch, ch["pools"][U["pool"]], U) for ch in chunks for U in ch["units"]]


@functools.lru_cache(maxsize=None)
def truth(name, ui):
    """Brute force over all training rows of unit ui from its captured zs / zq: (largest exponent, log2 sum) per query."""
    ch, P, U = units_of(name)[ui]
    return gr.true_max_exponent(U["zs"], U["zq"]), gr.true_log2_sums(U["zs"], U["zq"])


MEASURED = {"bound": 0.0, "coef": 0.0}
ALL = sorted(CASES)


# ---- 1. sort and compaction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_sort_and_compaction(name):
    chunks, scores, df, codes = captured(name)
    kind, n, kr, dtype, terms, env, configs = CASES[name]
    units = units_of(name)
    for ch in chunks:
        for P in ch["pools"]:
            assert np.array_equal(np.sort(P["vals"]), np.arange(P["n"])), "a pool's sorted order is no permutation of its positions"
            assert np.array_equal(P["reg"], gr.region_of(P["rb"], P["R"], P["vals"]))
            assert P["nblk"] == (P["n"] + 255) // 256 and P["rb"][0] == 0 and P["rb"][P["R"]] == P["n"]
            assert P["R"] == (2 if kind == "holdout" else kr)
            # the pool's rows are rows of the table: the same multiset of values per column as the frame's rows the aid names
            assert P["rows"].shape == (P["n"], P["d"]) and len(np.unique(P["rowid"])) == P["n"]
    if configs:
        counts = np.bincount(codes, minlength=len(configs))
        small = int(counts.argmin())
        for ch in chunks:
            assert ch["np"] == len(configs) - 1 and ch["np"] > 2                    # three pools: two pool bits above the Morton bits
            assert sorted(P["n"] for P in ch["pools"]) == sorted(int(c) for i, c in enumerate(counts) if i != small)
            assert counts[small] < 256
    else:
        assert all(P["n"] == n for ch in chunks for P in ch["pools"])
    if name.startswith("holdout"):
        assert any(P["nblk"] > 64 for ch in chunks for P in ch["pools"])            # group_scan_kernel carries into a second round
    mods = set()
    for ch, P, U in units:
        R, rb = P["R"], P["rb"]
        tr, qu, qpos, reg = gr.orders(P["vals"], rb, R, U["train_mask"], U["test_region"])
        assert U["N"] == len(tr) == sum(int(rb[r + 1] - rb[r]) for r in range(R) if (U["train_mask"] >> r) & 1)
        assert U["nq"] == len(qu) == int(rb[U["test_region"] + 1] - rb[U["test_region"]])
        assert U["ntiles"] == (U["N"] + 15) // 16 and U["nqtiles"] == (U["nq"] + 15) // 16
        assert np.array_equal(U["qpos"][:U["nq"]], qpos), np.flatnonzero(U["qpos"][:U["nq"]] != qpos)[:5]
        mods.add((U["N"] % 16, U["nq"] % 16))
    if name in ("cv3-767-f64", "cv10-2559-f64-mom-split80"):
        assert {(0, 15), (15, 0)} <= mods, mods
    if name in ("cv3-769-f64-split16", "cv10-2561-f64-split80"):
        assert {(0, 1), (1, 0)} <= mods, mods
    if name.startswith("cv64"):
        assert any(U["nq"] < 16 for _, _, U in units) and all(P["R"] == 64 for _, P, _ in units)


# ---- 2. whitening -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_whitening(name):
    for ch, P, U in units_of(name):
        d = P["d"]
        tr, qu, _, _ = gr.orders(P["vals"], P["rb"], P["R"], U["train_mask"], U["test_region"])
        for got, idx in ((U["zs"], tr), (U["zq"], qu)):
            want = gr.whiten(P["rows"][idx], U["W"], U["mu"], d)
            tol = (2 * d + 3) * EPS * gr.whiten_scale(P["rows"][idx], U["W"], U["mu"], d)
            if ch["f16"]:
                tol = tol + 2.0 ** -22 * (1.0 + 2.0 ** -9) * np.abs(want) + 2.0 ** -20
            bad = np.abs(got - want) > tol
            assert not bad.any(), (name, d, np.argwhere(bad)[:3], np.max(np.abs(got - want) - tol))


# ---- 3. boxes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_boxes(name):
    ragged = short = False
    for ch, P, U in units_of(name):
        kd = P["kd"]
        box = gr.tile_boxes(U["zs"], kd)
        assert np.array_equal(U["box"], box), np.argwhere(U["box"] != box)[:3]
        assert np.array_equal(U["qbox"], gr.query_boxes(U["zq"], kd))
        if ch["bboxes"]:
            assert U["has_bbox"]
            bb = gr.batch_boxes(box, kd, U["tps"])
            assert U["bbox"].shape == bb.shape == (U["nsplit"] * ((U["tps"] + 63) // 64), 2 * kd)
            assert np.array_equal(U["bbox"], bb), np.argwhere(U["bbox"] != bb)[:3]
            ragged = ragged or (U["tps"] > 64 and U["tps"] % 64 != 0)
            short = short or U["ntiles"] % U["tps"] != 0
        else:
            assert not U["has_bbox"]
        assert U["nsplit"] == (U["ntiles"] + U["tps"] - 1) // U["tps"]
        env = CASES[name][5]
        if env.get("PBN_GROUP_SPLIT_TILES") == "16":
            assert U["tps"] <= 16 and U["nsplit"] > 1
        if "PBN_GROUP_SPLIT_TILES" not in env:
            assert U["nsplit"] == 1
    if name == "holdout-16401-f64":
        assert ragged and short       # 821 tiles in eleven splits of 75: batches of 64 + 11, the last split shorter
    if name == "cv3-1920-f64-split80":
        assert all(U["tps"] == 80 and U["ntiles"] == 80 and U["bbox"].shape[0] == 2 for _, _, U in units_of(name))   # batches of 64 + 16


# ---- 4. bounds ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_bounds(name):
    worst = 0.0
    for ui, (ch, P, U) in enumerate(units_of(name)):
        d, kd, N, nq = P["d"], P["kd"], U["N"], U["nq"]
        tmax, tsum = truth(name, ui)
        qlb, qthr = U["qlb"], U["qthr"]
        assert len(qlb) == U["nqtiles"] * 16 and np.all(np.isneginf(qlb[nq:]))
        over = qlb[:nq] - tmax - gr.bound_slack(N, d, tmax)
        assert np.all(over <= 0), (name, d, "qlb above the largest exponent", int(over.argmax()), float(over.max()))
        tile_min = np.array([tsum[t * 16:(t + 1) * 16].min() for t in range(U["nqtiles"])])
        over = qthr - tile_min - gr.bound_slack(N, d, tile_min)
        assert np.all(over <= 0), (name, d, "qthr above a query's log2 sum", int(over.argmax()), float(over.max()))
        # ... and equal to the definition (a uselessly low bound would pass the two above)
        rl, rt = gr.bounds(U["zs"], U["zq"], U["qpos"][:nq], kd, ch["window"], ch["tile_window"], bool(ch["use_sum_bound"]), U["box"])
        for got, want in ((qlb[:nq], rl[:nq]), (qthr, rt)):
            assert np.array_equal(np.isfinite(got), np.isfinite(want))
            f = np.isfinite(want)
            if f.any():
                worst = max(worst, float(np.max(np.abs(got[f] - want[f]) / np.maximum(1.0, np.abs(want[f])))))
    MEASURED["bound"] = max(MEASURED["bound"], worst)
    print(f"\n[{name}] bounds against the restatement: measured {worst:.3e} (BOUND_TOL {BOUND_TOL:.1e})")
    assert worst <= BOUND_TOL / 8


# ---- 5. tile moments ----------------------------------------------------------------------------------------------------------------------
MOMENT_CASES = [n for n in ALL if CASES[n][5].get("PBN_MOMENT_MIN_ROWS") == "0"]


@pytest.mark.parametrize("name", MOMENT_CASES)
def test_tile_moments(name):
    worst, zero_radius, padded, ran = 0.0, False, False, 0
    for ch, P, U in units_of(name):
        if not ch["moments"]:
            assert U["mom"] is None and U["nsplit_fin"] == U["nsplit"]
            continue
        d = P["d"]
        ran += 1
        assert d in (1, 2) and U["nsplit_fin"] == 2 * U["nsplit"] and U["mstride"] == (U["ntiles"] + 63) // 64 * 64
        assert U["mom"].shape == (d + (9 if d == 1 else 45), U["mstride"])
        nt = U["ntiles"]
        cen_dev = U["mom"][:d, :nt].T
        cen, rho2, _, _ = gr.tile_moments(U["zs"])
        absmean = np.array([np.abs(U["zs"][t * 16:(t + 1) * 16]).mean(0) for t in range(nt)])
        assert np.all(np.abs(cen_dev - cen) <= 6 * EPS * absmean), np.max(np.abs(cen_dev - cen) - 6 * EPS * absmean)
        rad2 = U["rad2"]
        assert np.all(rho2 <= rad2) and np.all(rad2 <= rho2 * (1 + 2e-6) + 2e-30), (name, d, np.max(rad2 - rho2 * (1 + 2e-6)))
        _, _, coef, scale = gr.tile_moments(U["zs"], centroids=cen_dev)
        got = U["mom"][d:, :nt].T.astype(np.longdouble)
        err = np.abs(got - coef)
        nz = scale > 0
        assert np.all(err[~nz] == 0)
        worst = max(worst, float(np.max(err[nz] / scale[nz])))
        zero_radius = zero_radius or bool(np.any(rho2 == 0.0))
        padded = padded or U["N"] % 16 != 0
        assert U["mstride"] != nt or nt % 64 == 0
    # (the folds of 768 rows train on 512: the one moment case without a padded last tile)
    assert ran > 0 and zero_radius and (padded or name == "cv3-768-f64-mom-split16"), (ran, zero_radius, padded)
    MEASURED["coef"] = max(MEASURED["coef"], worst)
    print(f"\n[{name}] moment coefficients against longdouble: measured {worst:.3e} of the absolute sum (COEF_TOL {COEF_TOL:.1e})")
    assert worst <= COEF_TOL / 8


# ---- 6. partials, finish, sums, score -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_partials_and_finish(name):
    chunks, scores, df, codes = captured(name)
    worst = 0.0
    for ui, (ch, P, U) in enumerate(units_of(name)):
        nq = U["nq"]
        merged = gr.merge_partials(U["part"], U["lognorm"])[:nq]
        _, tsum = truth(name, ui)
        want = U["lognorm"] + gr.LN2 * tsum
        assert np.all(np.isfinite(merged))
        worst = max(worst, float(np.max(np.abs(merged - want))))
        if ch["f16"]:
            assert np.allclose(merged, want, atol=5e-4, rtol=1e-4), (name, P["d"], int(np.argmax(np.abs(merged - want))), np.max(np.abs(merged - want)))
        else:
            assert np.all(np.abs(merged - want) <= 3.3e-7), (name, P["d"], int(np.argmax(np.abs(merged - want))), np.max(np.abs(merged - want)))
        total = float(np.sum(merged))
        assert abs(U["sum"] - total) <= 1e-12 * abs(total), (U["sum"], total)
        assert 8.0 <= U["margin"] <= 52.0, U["margin"]      # prune_margin: the base less log2(1e6 / N), at least 8
    print(f"\n[{name}] per-query log-density against brute force: largest difference {worst:.3e}")
    for got, want, tol in scores:
        assert abs(got - want) <= tol * abs(want), (name, got, want)
