"""GPU tier: the pruning prepass of the fitted KDE / ProductKDE / CKDE handles (csrc/kde_prepass.hip, driven by kde_pack_train and
kde_eval_enqueue in csrc/kde_model.hip) stage by stage.  The test aid pbn_debug_prune_stages (codes at its definition) copies back what every
kernel of the chain left for a pruned fit and a pruned evaluation; each stage is held against the numpy restatement of
tests/prune_restatement.py applied to the CAPTURED output of the stage before it, so that one stage's tolerance does not leak into the next,
or against brute force over all training rows.  The path is reached through the public classes (fit, logl, slogl) with
PBN_PRUNE_MIN_ROWS=256; the edge queries of a case are built from the fitted model's own whitening matrix, read through the aid.

Cases (prune_restatement.CASES): fp64 KDE at d = 1 ... 6 (one Morton key axis, the 2-D Hilbert walk, the n-dimensional curve at 3 and 4 axes,
d > pdims with and without a subsample; FOLD and WMUL sweeps), ProductKDE, CKDE as two plain sweeps (2, 3 variables) and fused (5: which = 2,
no tile-window bound), float32 tables at d = 2 and 5 (f16x2 fragments, margin 36), a float32 table whose pinned bandwidth widens it
(prune_keys_kernel<double, float>), rotated fp64 models at d = 7 and 8 (up to query_prepass_kernel only: full W, four key axes under seven /
eight box axes, the generic loops at 7, the unrolled zd == 8 and pd == PBN_PRUNE_PD branches at 8 - the restatement has ONE order of
operations, the generic one, and the d = 8 case is held to the same BOUND_TOL against it).
Training rows 257 (one partial tile behind 16 full ones), 1 023 (nsub = 0 at d = 5), 1 100 (nsub = 16, stride 68), 4 133 (259 tiles: with four
splits of 65 a split's last batch holds one tile and the last split is clipped).  Queries 1, 15, 16, 17, 33, 255, 257, 600.

Tolerances that are derived (never tuned):
  whitening            |z - W (x - mu)| <= (2 d + 3) 2^-53 sum_j |W_ij| |x_j - mu_j| (test_group_stages_gpu.py), + 2^-24 |z| where the fragment
                       type is float (zrow holds the value rounded to float).
  keys, sort, boxes    equality: integers, permutations, bit-for-bit doubles.
  bounds below truth   group_restatement.bound_slack.
  subsample sums       the sweep's per-term budget: fp64 2.3e-9 (the 2^x polynomial) + the Gram form's rounding (below), as natural
                       logarithms; float32 tables atol 5e-4, rtol 1e-4.
  merged partials      per-row logl: 2.3e-9 + N 2^-52 (polynomial + what pruning may drop: DESIGN.md 3.1 / 4); sum-only: 3.3e-7 (kde_model.hpp);
                       both + ln 2 (d + 3) 2^-53 (|z_q|^2 + max_t |z_t|^2): the sweep forms an exponent as norm + norm + dot product, each of
                       magnitude up to (|z_q|^2 + |z_t|^2) / 2, in d + 3 rounded operations - what matters for the edge queries, which sit
                       1 500 units out.  float32 tables: atol 5e-4, rtol 1e-4.
  visits               certain <= visited <= certain + borderline with the slack 8 2^-53 max(|d2 / 2|, |thr|) of numpy's unfused sum of squares
                       against the kernel's fma; borderline <= 0.1 % of certain is a condition on the data (checked on the CPU, too).

Tolerance that was MEASURED on an MI355X with this file (printed before it is asserted; the test asserts measured <= constant / 8; the run is
kept in profiles/prune_stages/tests.txt):
  BOUND_TOL  |qlb, qthr (kernel) - restatement| / max(1, |restatement|), over the finite ones (the infinite ones must coincide)
             measured 8.882e-16 (ckde-d5; 7.8e-16 rot-d8, 6.7e-16 rot-d7, 6.1e-16 f32-d5, 0 to 4.4e-16 in the other twelve) -> BOUND_TOL = 7.2e-15
The merged partials came within 2.3e-9 (per-row logl) and 6.8e-8 (sum-only) of brute force on float64 and within 3.4e-2 at |logl| ~ 10^6
(3.7e-4 at |logl| ~ 10^4) on float32; the subsample sums within 2.2e-9 / 2.8e-4; no case had a borderline (tile, group) pair.

What this file found when it first ran: at ckde-d5 qthr of one tile lay 3.2e-9 units above the true log2 sum of its edge query, whose one
relevant training row is a row of the subsample - the subsample sweep's sum, polynomial error and all, was taken as a lower bound as it stood.
query_prepass_kernel now takes the sweep's error budget off first (prune_subsample_slack, restated in prune_restatement.subsample_slack).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pandas as pd
import pytest

import prune_restatement as pr

pytestmark = pytest.mark.gpu

BOUND_TOL = 7.2e-15
EPS = 2.0 ** -53
LN2 = math.log(2.0)
LD = np.longdouble
PINNED_BANDWIDTH = 2.5e-5      # f32-widen-d2: h = 0.005 on columns of spread ~ 5 - |z| in the thousands, beyond the fp32 Gram form and the key range

ALL = sorted(pr.CASES)
SWEPT = [c for c in ALL if not c.startswith("rot")]           # the rotated models are checked up to query_prepass_kernel only
FIT_HEAD = ("N", "d", "dm", "zdims", "pdims", "kdims", "nsub", "ntiles", "wfull", "cond", "fdtype", "src_f32", "bits", "hilbert")
EVAL_HEAD = ("n", "nqtiles", "nsplit", "tps", "nbps", "sum_only", "bboxes", "use_qlb", "window", "sub", "P", "which", "N", "d", "cond", "fdtype",
             "rows", "qg", "num_cus", "tile_bytes", "KS")


# ---- the aid ------------------------------------------------------------------------------------------------------------------------------
class Aid:
    def __init__(self):
        from pybnesian_amd import _lib

        L = _lib.load()
        self.fn = L.pbn_debug_prune_stages
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
        self.visits = L.pbn_debug_sweep_visits
        self.visits.restype = None
        self.visits.argtypes = [C.c_void_p, C.c_void_p, C.c_int]

    def arm(self):
        self.fn(0, 0, -1, None, 0, 0)
        self.fn(0, 0, -1, None, 0, 1)

    def clear(self):
        self.fn(0, 0, -1, None, 0, 0)

    def count(self, side):
        return int(self.fn(side, 0, -1, None, 0, -1))

    def get(self, side, back, what, dtype):
        n = self.fn(side, back, what, None, 0, -1)                    # (capture < 0: a read, the aid stays as it is)
        assert n >= 0, (side, back, what)
        out = np.zeros(max(int(n), 1), dtype=dtype)
        assert self.fn(side, back, what, out.ctypes.data, n, -1) == n
        return out[:n]

    def fit(self, back):
        f = dict(zip(FIT_HEAD, map(int, self.get(0, back, 0, np.int64))))
        d, zd, pd_, N = f["d"], f["zdims"], f["pdims"], f["N"]
        f["cell"] = float(self.get(0, back, 1, np.float64)[0])
        f["W"] = self.get(0, back, 2, np.float64).reshape(d, d)
        f["mu"] = self.get(0, back, 3, np.float64)
        f["zrow"] = self.get(0, back, 4, np.float64).reshape(N, zd)
        f["keys_unsorted"] = self.get(0, back, 5, np.uint32)
        f["keys"] = self.get(0, back, 6, np.uint32)
        f["perm"] = self.get(0, back, 7, np.int32).astype(np.int64)
        f["zsorted"] = self.get(0, back, 8, np.float64).reshape(N, zd)
        f["box"] = self.get(0, back, 9, np.float64).reshape(f["ntiles"], 2 * pd_)
        return f

    def evaluation(self, back, zd, pd_):
        e = dict(zip(EVAL_HEAD, map(int, self.get(1, back, 0, np.int64))))
        e["margin"], e["log2_nsub"] = map(float, self.get(1, back, 1, np.float64))
        n, nqt, P = e["n"], e["nqtiles"], e["P"]
        e["zrow"] = self.get(1, back, 4, np.float64).reshape(n, zd)
        e["keys_unsorted"] = self.get(1, back, 5, np.uint32)
        e["keys"] = self.get(1, back, 6, np.uint32)
        e["qperm"] = self.get(1, back, 7, np.int32).astype(np.int64)
        e["subpart"] = self.get(1, back, 8, np.float64).reshape(-1, P)
        e["qbox"] = self.get(1, back, 9, np.float64).reshape(nqt, 2 * pd_)
        e["qthr"] = self.get(1, back, 10, np.float64)
        e["qlb"] = self.get(1, back, 11, np.float64)
        e["qtpos"] = self.get(1, back, 12, np.int64)
        e["bbox"] = self.get(1, back, 13, np.float64).reshape(-1, 2 * pd_)
        e["part"] = self.get(1, back, 14, np.float64).reshape(e["rows"], nqt * 16, P)
        return e

    def sweep_visits(self, reset):
        v, t = C.c_ulonglong(0), C.c_ulonglong(0)
        self.visits(C.byref(v), C.byref(t), int(reset))
        return int(v.value), int(t.value)


@pytest.fixture(autouse=True)
def pruned_at_256_rows(monkeypatch):
    """Every test of this file runs the handles with the pruned path from 256 training rows on and with the sweep's visit counters on (they
    change no result); a case is captured by the first test that asks for it."""
    monkeypatch.setenv("PBN_PRUNE_MIN_ROWS", "256")
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def model_of(pbn, name):
    cls, d, dtype, N, n = pr.CASES[name]
    cols = [f"c{j}" for j in range(d)]
    if cls == "CKDE":
        return pbn.CKDE(cols[0], cols[1:]), cols
    return getattr(pbn, cls)(cols), cols


def fit_model(pbn, name, train_df):
    k, cols = model_of(pbn, name)
    k.fit(train_df)
    if name == "f32-widen-d2":
        k.bandwidth = np.full(len(cols), PINNED_BANDWIDTH)
    return k


def model_columns(name, f):
    """The table's columns in the order of the captured model's W: a fused conditional model takes the evidence first and the variable
    last; the marginal model of a split CKDE leaves the variable out."""
    cls, d, dtype, N, n = pr.CASES[name]
    if f["cond"]:
        return list(range(1, d)) + [0]
    if cls == "CKDE" and f["d"] == d - 1:
        return list(range(1, d))
    return list(range(d))


@functools.lru_cache(maxsize=None)
def captured(name):
    """Fits the case's model and evaluates logl and slogl with the aid armed -> dict(train, query, logl, slogl, recs): recs = one
    (fit, logl evaluation or None, slogl evaluation, columns) per captured model - two for a CKDE evaluated as two plain sweeps."""
    import pybnesian_amd as pbn

    cls, d, dtype, N, n = pr.CASES[name]
    cols = [f"c{j}" for j in range(d)]
    x = pr.case_training(name)
    train_df = pd.DataFrame(x.astype(dtype), columns=cols)
    assert os.environ.get("PBN_PRUNE_MIN_ROWS") == "256"
    aid = Aid()
    aid.arm()
    try:
        k = fit_model(pbn, name, train_df)
        nfit = aid.count(0)
        assert nfit > 0, "no pruned fit was captured"
        want_fits = 2 if name in ("ckde-d2", "ckde-d3") else 1
        fits = [aid.fit(b) for b in range(want_fits)][::-1]          # in the order they were made: a split CKDE's joint model first
        # the queries: built in the columns' order of the first (for a split CKDE: the joint) model, from its own W and mu
        f0 = fits[0]
        mc = model_columns(name, f0)
        xq_m = pr.query_rows(x[:, mc], n, pr.QUERY_SEED + n, f0["W"], f0["mu"], f0["kdims"], f0["perm"], full_w=bool(f0["wfull"]))
        xq = np.empty_like(xq_m)
        xq[:, mc] = xq_m
        query_df = pd.DataFrame(xq.astype(dtype), columns=cols)
        out = dict(train=train_df.to_numpy().astype(np.float64), query=query_df.to_numpy().astype(np.float64), logl=None, visits=None)
        evals = {}
        for kind in ("logl", "slogl"):
            if kind == "logl" and name.startswith("rot"):
                continue                                              # per-row logl of a rotated model takes the plain sweep
            aid.clear()
            aid.arm()
            aid.sweep_visits(True)
            out[kind] = getattr(k, kind)(query_df)
            if kind == "logl":
                out["visits"] = aid.sweep_visits(False)
            got = []
            for b in reversed(range(aid.count(1))):                   # in the order they ran
                fit = next(f for f in fits if f["d"] == int(aid.get(1, b, 0, np.int64)[13]))
                got.append(aid.evaluation(b, fit["zdims"], fit["pdims"]))
            assert got, f"no pruned evaluation was captured by {kind}"
            evals[kind] = {e["d"]: e for e in got}                   # (the last one per model: a sum too close to 0 is evaluated twice)
        out["recs"] = [(f, evals.get("logl", {}).get(f["d"]), evals["slogl"][f["d"]], model_columns(name, f)) for f in fits]
        return out
    finally:
        aid.clear()


def evaluations(rec):
    f, el, es, mc = rec
    return [e for e in (el, es) if e is not None]


@functools.lru_cache(maxsize=None)
def truth(name, ri, which):
    """Brute force over all training rows of record ri from its captured rows, queries in their sorted order: (largest exponent, log2 sum)."""
    c = captured(name)
    f, el, es, mc = c["recs"][ri]
    e = el if which == "logl" else es
    zq = e["zrow"][e["qperm"]]
    return pr.true_max_exponent(f["zsorted"], zq), pr.log2_sum_over(f["zsorted"], zq)


MEASURED = {"bound": 0.0}


# ---- 0. every case reached its branch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_case_reaches_its_branch(name):
    from pybnesian_amd import _lib

    cls, d, dtype, N, n = pr.CASES[name]
    c = captured(name)
    recs = c["recs"]
    assert len(recs) == (2 if name in ("ckde-d2", "ckde-d3") else 1)
    for ri, (f, el, es, mc) in enumerate(recs):
        dd = d - ri                                                    # the marginal model of a split CKDE
        rot = name.startswith("rot")
        fused = name == "ckde-d5"
        dm = dd - 1 if fused else dd
        pdims = dd if rot else min(dm, 4)
        kdims = 4 if rot else pdims
        want = dict(N=N, d=dd, dm=dm, zdims=dd, pdims=pdims, kdims=kdims, nsub=pr.nsub_of(N, dd, pdims), ntiles=pr.ceil_div(N, 16), wfull=int(rot),
                    cond=int(fused), fdtype=_lib.PBN_F32 if (dtype == "float32" and name != "f32-widen-d2") else _lib.PBN_F64,
                    src_f32=int(name == "f32-widen-d2"), bits=pr.key_bits(kdims), hilbert=1)
        assert {k: f[k] for k in want} == want
        assert f["cell"] == pr.key_cell(kdims)
        assert N % 16 != 0                                             # a partial last tile in every case
        if not f["wfull"]:
            assert np.all(np.triu(f["W"], 1) == 0)
        for e in evaluations((f, el, es, mc)):
            assert (e["n"], e["nqtiles"], e["N"], e["d"], e["cond"], e["fdtype"]) == (n, pr.ceil_div(n, 16), N, dd, int(fused), f["fdtype"])
            assert (e["nsplit"], e["tps"], e["nbps"]) == pr.split_rule(f["ntiles"], e["nqtiles"], e["num_cus"], e["qg"], e["tile_bytes"])
            base = 36.0 if f["fdtype"] == _lib.PBN_F32 else (43.0 if e["sum_only"] else 52.0)
            assert abs(e["margin"] - pr.prune_margin(N, base)) <= 1e-12
            assert e["sub"] == int(f["nsub"] > 0) and e["which"] == (2 if fused else 0) and e["P"] == (4 if fused else 2)
            assert e["bboxes"] == int(f["fdtype"] == _lib.PBN_F64 and not fused) and e["use_qlb"] == 1
            assert (e["window"] > 0) == (rot and f["d"] in (7, 8) and e["KS"] == 2)
            assert e["rows"] in (e["nsplit"], 2 * e["nsplit"])
            if f["nsub"]:
                assert e["log2_nsub"] == math.log2(f["nsub"]) and e["subpart"].shape == (e["nqtiles"] * 16, e["P"])
            if N == 4133 and e["nsplit"] > 1:
                # what the captured split implies: a last batch of one tile where tps = 64 k + 1, a clipped last split where tps does not divide
                if e["tps"] % 64 == 1:
                    assert e["nbps"] == e["tps"] // 64 + 1
                assert (f["ntiles"] % e["tps"] != 0) == (e["nsplit"] * e["tps"] > f["ntiles"])
            if e["num_cus"] == 256 and N == 4133:
                assert (e["nsplit"], e["tps"], e["nbps"]) == (4, 65, 2)
        if el is not None:
            assert el["sum_only"] == 0
    assert recs[0][2]["n"] == n
    # clamped key cells and the ends of the curve, from the captured rows
    f, el, es, mc = recs[0]
    kd = f["kdims"]
    if n >= 15:
        e = es
        assert pr.clamped(e["zrow"], kd).sum() >= 2
        pos = set(pr.lower_bound(f["keys"], e["keys"]).tolist())
        # (the pinned bandwidth of f32-widen-d2 puts training rows into the curve's last cell, too: the end query then meets them)
        assert N in pos or (name == "f32-widen-d2" and f["keys"][-1] == e["keys"].max()), sorted(pos)[-4:]
        assert 0 in pos and any(0 < p < 32 for p in pos) and any(N - 32 <= p < N for p in pos), sorted(pos)[:4] + sorted(pos)[-4:]
    if name in ("kde-d4", "kde-d6", "f32-widen-d2"):
        assert pr.clamped(f["zrow"], kd).sum() >= 1                    # training rows beyond the key range, too
    assert any(np.array_equal(b[:f["pdims"]], b[f["pdims"]:]) for b in f["box"]), "no tile of zero extent"


# ---- 1. whitening -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_whitening(name):
    from pybnesian_amd import _lib

    c = captured(name)
    for f, el, es, mc in c["recs"]:
        d = f["d"]
        W = f["W"] if f["wfull"] else np.tril(f["W"])
        sides = [(f["zrow"], c["train"][:, mc])] + [(e["zrow"], c["query"][:, mc]) for e in evaluations((f, el, es, mc))]
        for got, x in sides:
            xc = x.astype(LD) - f["mu"].astype(LD)
            want = (xc @ W.astype(LD).T).astype(np.float64)
            scale = (np.abs(xc) @ np.abs(W).astype(LD).T).astype(np.float64)
            tol = (2 * d + 3) * EPS * scale
            if f["fdtype"] == _lib.PBN_F32:
                tol = tol + 2.0 ** -24 * np.abs(want)
            bad = np.abs(got - want) > tol
            assert not bad.any(), (name, d, np.argwhere(bad)[:3], float(np.max(np.abs(got - want) - tol)))


# ---- 2. keys ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_keys(name):
    c = captured(name)
    for f, el, es, mc in c["recs"]:
        kd = f["kdims"]
        assert pr.curve_kind(kd, bool(f["hilbert"])) == ("morton" if kd == 1 else "hilbert")
        for side in [f] + evaluations((f, el, es, mc)):
            want = pr.keys(side["zrow"], kd, bool(f["hilbert"]))
            assert np.array_equal(side["keys_unsorted"], want), (name, kd, np.flatnonzero(side["keys_unsorted"] != want)[:5])


# ---- 3. sort ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_sort(name):
    c = captured(name)
    for f, el, es, mc in c["recs"]:
        for side, perm in [(f, f["perm"])] + [(e, e["qperm"]) for e in evaluations((f, el, es, mc))]:
            n = len(perm)
            assert np.array_equal(np.sort(perm), np.arange(n)), "not a permutation"
            assert np.array_equal(side["keys"], side["keys_unsorted"][perm])
            assert np.all(np.diff(side["keys"].astype(np.int64)) >= 0)
            assert np.array_equal(perm, pr.stable_order(side["keys_unsorted"])), "the sort is not stable"
        assert np.array_equal(f["zsorted"].view(np.uint64), f["zrow"][f["perm"]].view(np.uint64))


# ---- 4. boxes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_boxes(name):
    c = captured(name)
    for f, el, es, mc in c["recs"]:
        pd_ = f["pdims"]
        box = pr.tile_boxes(f["zsorted"], pd_)
        assert np.array_equal(f["box"], box), np.argwhere(f["box"] != box)[:3]
        assert np.all(np.isfinite(f["box"]))
        for e in evaluations((f, el, es, mc)):
            qbox = pr.tile_boxes(e["zrow"][e["qperm"]], pd_)
            assert np.array_equal(e["qbox"], qbox), np.argwhere(e["qbox"] != qbox)[:3]
            assert np.all(np.isfinite(e["qbox"]))
            if e["bboxes"]:
                bb = pr.batch_boxes(f["box"], pd_, e["tps"])
                assert e["bbox"].shape == bb.shape == (e["nsplit"] * e["nbps"], 2 * pd_)
                assert np.array_equal(e["bbox"], bb), np.argwhere(e["bbox"] != bb)[:3]
                for s in range(e["nsplit"]):
                    t1 = min((s + 1) * e["tps"], f["ntiles"])
                    for k in range(e["nbps"]):
                        if s * e["tps"] + 64 * k < t1:
                            assert np.all(np.isfinite(e["bbox"][s * e["nbps"] + k])), (s, k)
            else:
                assert e["bbox"].size == 0


# ---- 5. subsample -------------------------------------------------------------------------------------------------------------------------
SUB_CASES = [c for c in ALL if pr.CASES[c][1] in (5, 6)]


def rounding_term(f, zq):
    """ln 2 (d + 3) 2^-53 (|z_q|^2 + max_t |z_t|^2) per query: see the header."""
    return LN2 * (f["d"] + 3) * EPS * ((zq ** 2).sum(1) + (f["zsorted"] ** 2).sum(1).max())


def subsample_log2_sums(e):
    sp = e["subpart"][:e["n"], e["which"]:e["which"] + 2]
    return sp[:, 0] + np.log2(sp[:, 1])


@pytest.mark.parametrize("name", SUB_CASES)
def test_subsample(name):
    from pybnesian_amd import _lib

    c = captured(name)
    for ri, (f, el, es, mc) in enumerate(c["recs"]):
        N, nsub = f["N"], f["nsub"]
        if name == "kde-d5-nosub":
            assert nsub == 0 and all(e["subpart"].size == 0 for e in evaluations((f, el, es, mc)))
            continue
        assert nsub == pr.nsub_of(N, f["d"], f["pdims"]) > 0
        rows = pr.subsample_rows(N, nsub)
        if N == 1100:
            assert nsub == 16 and rows[1] == 68
        for which, e in (("logl", el), ("slogl", es)):
            zq = e["zrow"][e["qperm"]]
            want = pr.log2_sum_over(f["zsorted"][rows], zq)
            got = subsample_log2_sums(e)
            if f["fdtype"] == _lib.PBN_F32:
                tol = 5e-4 + 1e-4 * np.abs(LN2 * want)
            else:
                tol = 2.3e-9 + rounding_term(f, zq)
            err = np.abs(LN2 * (got - want))
            print(f"\n[{name}/{which}] subsample sums against longdouble over the restated rows: largest error {err.max():.3e} (ln units)")
            assert np.all(err <= tol), (name, int(np.argmax(err - tol)), float(err.max()))
            tmax, _ = truth(name, ri, which)
            over = (got - math.log2(nsub)) - tmax - pr.bound_slack(N, f["d"], tmax)
            assert np.all(over <= 0), (name, "the subsample bound lies above the largest exponent", int(over.argmax()), float(over.max()))


# ---- 6. prepass bounds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_prepass_bounds(name):
    from pybnesian_amd import _lib

    c = captured(name)
    worst = 0.0
    for ri, (f, el, es, mc) in enumerate(c["recs"]):
        N, d, pd_ = f["N"], f["d"], f["pdims"]
        for which, e in (("logl", el), ("slogl", es)):
            if e is None:
                continue
            n, nqt = e["n"], e["nqtiles"]
            zq = e["zrow"][e["qperm"]]
            qpos = pr.lower_bound(f["keys"], e["keys"])
            assert np.array_equal(e["qtpos"], qpos[::16]), (name, np.flatnonzero(e["qtpos"] != qpos[::16])[:5])
            qlb, qthr = e["qlb"], e["qthr"]
            assert len(qlb) == nqt * 16 and len(qthr) == nqt
            assert np.all(np.isneginf(qlb[n:])) and not np.any(np.isneginf(qlb[:n]))
            # validity, against brute force over all N training rows
            tmax, tsum = truth(name, ri, which)
            over = qlb[:n] - tmax - pr.bound_slack(N, d, tmax)
            assert np.all(over <= 0), (name, which, "qlb above the largest exponent", int(over.argmax()), float(over.max()))
            tile_min = np.array([tsum[t * 16:(t + 1) * 16].min() for t in range(nqt)])
            over = qthr - tile_min - pr.bound_slack(N, d, tile_min)
            assert np.all(over <= 0), (name, which, "qthr above a query's log2 sum", int(over.argmax()), float(over.max()))
            # ... and equal to the definition (a uselessly low bound would pass the two above)
            ls = subsample_log2_sums(e) if f["nsub"] else None
            rl, rt = pr.prepass_bounds(f["zsorted"], zq, qpos, pd_, f["box"], ls, f["nsub"], tile_box_bound=not f["cond"],
                                       f16x2=f["fdtype"] == _lib.PBN_F32)
            for got, want in ((qlb[:n], rl[:n]), (qthr, rt)):
                assert np.array_equal(np.isfinite(got), np.isfinite(want))
                fin = np.isfinite(want)
                if fin.any():
                    worst = max(worst, float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))))
    MEASURED["bound"] = max(MEASURED["bound"], worst)
    print(f"\n[{name}] bounds against the restatement: measured {worst:.3e} (BOUND_TOL {BOUND_TOL:.1e})")
    assert worst <= BOUND_TOL / 8


# ---- 7. visits ----------------------------------------------------------------------------------------------------------------------------
VISIT_CASES = pr.VISIT_CASES + ["pkde-d3"]


@pytest.mark.parametrize("name", VISIT_CASES)
def test_visits(name):
    from pybnesian_amd import _lib

    c = captured(name)
    f, el, es, mc = c["recs"][0]
    assert f["fdtype"] == _lib.PBN_F64 and not f["cond"] and el["bboxes"] and el["window"] == 0
    pd_, qg = f["pdims"], el["qg"]
    thr = el["qthr"] - el["margin"]
    certain, borderline, offered = pr.visit_counts(f["box"], el["bbox"], el["qbox"], thr, pd_, el["tps"], qg)
    visited, tiles = c["visits"]
    print(f"\n[{name}] (tile, group) pairs: certain {certain}, borderline {borderline}, visited {visited}, offered {offered}")
    assert tiles == offered == pr.ceil_div(el["nqtiles"], qg) * f["ntiles"] * qg
    assert borderline <= 1e-3 * certain, (certain, borderline)
    assert certain <= visited <= certain + borderline, (certain, visited, borderline)


# ---- 8. result ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEPT)
def test_result(name):
    from pybnesian_amd import _lib

    c = captured(name)
    cls, d, dtype, N, n = pr.CASES[name]
    logl, mag = np.zeros(n), np.zeros(n)
    for ri, (f, el, es, mc) in enumerate(c["recs"]):
        sign = 1.0 if ri == 0 else -1.0                                # a split CKDE: joint - marginal
        for which, e in (("logl", el), ("slogl", es)):
            zq = e["zrow"][e["qperm"]]
            # fused: the marginal pair first, then the joint pair (kde_finish_kernel: logl = joint - marginal)
            slots = [(2, f["d"], 1.0), (0, f["dm"], -1.0)] if f["cond"] else [(0, f["d"], 1.0)]
            for slot, dims, ssign in slots:
                merged = pr.merge_partials(e["part"], slot)[:n]
                want = pr.log2_sum_over(f["zsorted"][:, :dims], zq[:, :dims])
                assert np.all(np.isfinite(merged)), (name, which, np.flatnonzero(~np.isfinite(merged))[:5])
                err = np.abs(LN2 * (merged - want))
                if f["fdtype"] == _lib.PBN_F32:
                    tol = 5e-4 + 1e-4 * np.abs(LN2 * want)
                else:
                    tol = (3.3e-7 if e["sum_only"] else 2.3e-9 + N * 2.0 ** -52) + rounding_term(f, zq)
                print(f"\n[{name}/{which}/slot {slot}] merged partials against longdouble brute force: largest error {err.max():.3e}")
                assert np.all(err <= tol), (name, which, slot, int(np.argmax(err - tol)), float(err.max()))
                if which == "logl":
                    part = np.empty(n)
                    part[e["qperm"]] = LN2 * merged                    # the caller's row order
                    logl += sign * ssign * part
                    mag += np.abs(part)
    # logl in the caller's row order: what the finish kernel adds to ln 2 x merged is one constant per case (the models' log-normalisers)
    got = c["logl"]
    assert got.shape == (n,) and np.all(np.isfinite(got)), "a far query's logl is not finite"
    off = got - logl
    spread = np.abs(off - np.median(off))
    assert np.all(spread <= 16 * EPS * (mag + np.abs(np.median(off)) + 1.0)), (name, int(spread.argmax()), float(spread.max()))
    assert np.isfinite(c["slogl"])


# ---- the aid is inert ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kde-d3", "f32-d5"])
def test_aid_is_inert(name):
    import pybnesian_amd as pbn

    cls, d, dtype, N, n = pr.CASES[name]
    c = captured(name)
    cols = [f"c{j}" for j in range(d)]
    train_df = pd.DataFrame(c["train"].astype(dtype), columns=cols)
    query_df = pd.DataFrame(c["query"].astype(dtype), columns=cols)
    aid = Aid()
    aid.clear()
    k0 = fit_model(pbn, name, train_df)
    plain = (k0.logl(query_df), k0.slogl(query_df))
    assert np.all(np.isfinite(plain[0]))
    assert aid.count(0) == 0 and aid.count(1) == 0                     # nothing is kept while the aid is not armed
    aid.arm()
    try:
        k1 = fit_model(pbn, name, train_df)
        armed = (k1.logl(query_df), k1.slogl(query_df))
        assert aid.count(0) >= 1 and aid.count(1) >= 2
    finally:
        aid.clear()
    after = (k1.logl(query_df), k1.slogl(query_df))
    for got in (armed, after, (c["logl"], c["slogl"])):
        assert np.array_equal(got[0].view(np.uint64), plain[0].view(np.uint64))
        assert np.float64(got[1]).view(np.uint64) == np.float64(plain[1]).view(np.uint64)
