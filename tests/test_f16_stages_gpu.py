"""GPU tier: the fp32 KDE path on the 16-bit matrix cores ("f16x2": csrc/kde_sweep_f16.inc, helpers in csrc/kde_kernels.hpp) stage by stage.
The test aid pbn_debug_f16_stages (csrc/kde_model.hip, codes at its definition) copies back, for every f16x2 evaluation of kde_eval_enqueue,
the training and query fragments as pack_rows_f16_kernel left them, the partial sums behind the sweep and again behind kde_far_fix_kernel.
Each stage is held against tests/f16_restatement.py applied to the CAPTURED output of the stage before it:
  A  pack: (a) exact designs (W the identity - for the full bandwidth rule to the one rounding the host's chol and inverse leave, see pin_unit_bandwidth -,
     mu = 0; both asserted on what the aid read): every slot, norm, flag and padding row
     EQUALS the restatement bit for bit; (b) general designs: the decoded z^ lies within the split bound of W (x - mu) in longdouble, every
     other slot follows exactly from the row's own decoded pieces, the norm pieces are split3s(float(-1/2 sum z^^2)) exactly.
  B  sweep: per (split, query) m + log2 s of the pre-fix partials against log2 sum_t 2^e(t, q) with e from the decoded operands in float64.
  C  far fix: flagged queries' partials against fp64 over the decoded training rows and the unclamped W (x - mu); unflagged ones untouched.
  D  logl / slogl of the class = lognorm + ln 2 x (merge of the captured post-fix partials), to fp64 rounding.
The path is reached through KDE, ProductKDE and CKDE on float32 frames.  The grouped launches of the score engine are not covered here.

Kernel forms (CASES; each asserted through the header's kernel code and pbn_debug_w32_launches): kde_sweep_f16_kernel unpruned at NB = 1, 2
(PBN_F32_W32=0), at NB = 3 (d = 21) and where W32 does not apply (d = 9, 20); kde_sweep_f16_w32_kernel<1> (d = 5, 8) and <2> (d = 10, 19); the
fused CKDE sweep at NB = 1 and 2; with PBN_PRUNE_MIN_ROWS=256 kde_sweep_f16_w32p_kernel<1> (d = 2, 6), the pruned 16x16 form (PBN_F32_W32=0)
and the pruned fused CKDE.  Training rows 17, 257, 1 023, 1 040 (65 tiles: one over a 64-tile blind chunk), 2 064 and 4 133 (nsplit > 1 where
the card's CU count gives it - read from the header, never assumed; a split that ends inside a chunk; an odd number of tiles for the paired
forms; a clipped last split); queries 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 600.

Tolerances that are derived (never tuned), in base-2 exponent units unless said otherwise:
  split         |z - z^| <= max(2^-22 |z|, 2^-20) (f16_restatement's docstring has the proof) + (2 d + 3) 2^-53 sum_j |W_ij| |x_j - mu_j|.
  exponent      f32 accumulation in the matrix cores in any order: per pair (nonzero terms + 1) 2^-24 sum |terms|, the query offset counted among
                the terms (16x16: the C operand float(ny - m), one term; W32 forms: its three split3s pieces + the split3s residual
                max(2^-33 |ny - m|, 2^-20); fused CKDE joint: the six slots of the extra block, the three pieces of xn + (m - mj) with their
                residual, and the two float operations that form it).  Taken at the pairs that carry the sum - the largest over the terms within
                2^-24 of it - plus the weighted bounds of the others.
  fp64 sum      of the reference itself: K 2^-53 sum |terms| per pair.
  additions     fp32 additions of positive terms on a term's path before the fp64 sum, count x 2^-24 relative (ADDS below):
                  16x16 unpruned  2 in the tile sum (e0 + e1) + (e2 + e3), then fs += ts once per tile of a blind chunk of PBN_F16_BLIND_CHUNK =
                                  64 tiles (kde_sweep_f16_body: FSUM, run_range): 66; the checked form (PAIRSUM) has 3.
                  16x16 pruned    the same inside a 64-tile batch (run_batch): 66.          fused CKDE: sum += (double)ts per tile: 2.
                  W32             expsum: 2 in a quad, 3 over the quads, then fs += once per super-group and tile pair: 32 pairs per chunk + the
                                  pipeline's first (empty) one: 5 + 33 = 38.
                  W32P            the whole split is one blind region: 5 + ceil(tps / 2) + 1, tps from the header.
  pruning       a pruned sweep may drop tiles: N 2^-margin of the query's whole sum, margin from the aid.
  far fix       (d + 3) 2^-53 (|z_q|^2 + max_t |z^_t|^2) (as tests/test_prune_stages_gpu.py) + what the whitening slack of z_q (the split line's second
                term, s_k per coordinate) moves an exponent by: 2 max_t sum_k |z^_tk - z_qk| s_k.  Nothing else.
  end to end    64 2^-53 (|lognorm| + ln 2 (|m| + |log2 s|) + 1): kde_finish_kernel is fp64 (library exp2 / log2: a few ulp).

Tolerance that is MEASURED on an MI355X with this file (printed before it is asserted; the test asserts measured <= constant / 8; the run is
kept in profiles/f16_stages/tests.txt):
  EXP_TOL   what remains of |m + log2 s - reference| after the derived parts, over the unpruned plain cases - the error of Tr<float>::ex2
            (v_exp_f32), which nothing at hand states.  Measured against the restatement on captured fragments, never against another run.
            Measured 0 in all ten plain cases (the largest error is 0.030 of its derived bound, at w32-d5; 0.038 at ckde-nb1 - the f32 accumulation bound of
            the exponent dwarfs a 2^-23 exponential) -> EXP_TOL = 0: the derived parts are the whole tolerance, for the fused CKDE and the
            pruned forms as well.

What the first runs found: the compiled split2 rounds double -> half ONCE where the source reads double -> float -> half (KDE-5 / KDE-10 of the
exact designs, at grid values on an f16 midpoint under W = (1 - 2^-53) I; the restatement follows the device, both orders keep the bounds);
no bandwidth makes the full rule's W an exact power of two (pin_unit_bandwidth); a pack mutation is invisible to stage B by construction (its
reference starts from the captured fragments) and is stage A's to find.  No kernel was wrong.

Conditions on the data (checked here from the restatement): a (split, query) is left out of stage B only when every one of its terms lies
below 2^-126 of 2^m (the float sum underflows whatever the kernel does); at most 0.1 % of a case's pairs - counted with the kernel's m and, from
the reference alone, with m = the split's largest exponent for the query; an unpruned kernel's m may not lie above that exponent by more than
the pair's own bound, so a wrong offset cannot widen the set.  No row is left out in A, C, D.
"""
import contextlib
import ctypes as C
import functools
import math
import os

import numpy as np
import pandas as pd
import pytest

import f16_restatement as fr

pytestmark = pytest.mark.gpu

EXP_TOL_MEASURED = 0.0           # profiles/f16_stages/tests.txt: nothing remains - the derived parts cover every partial of every plain case
EXP_TOL = None if EXP_TOL_MEASURED is None else 8.0 * EXP_TOL_MEASURED
EPS = 2.0 ** -53
F32 = 2.0 ** -24
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
LD = np.longdouble
HEAD = ("n", "N", "d", "dm", "cond", "NB", "spd", "ntiles", "nqtiles", "nsplit", "tps", "P", "w32", "prune", "sum_only", "qg", "kernel", "num_cus", "sub")
K16, KW32, K16P, KW32P = 0, 1, 2, 3
ALL_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 600)
FEW_N = (1, 17, 33, 65, 600)

# name: (class, d, training rows, query counts, environment, kernel, NB)
CASES = {
    "plain16-nb1": ("KDE", 5, 1040, ALL_N, {"PBN_F32_W32": "0"}, K16, 1),
    "plain16-nb2": ("KDE", 10, 2064, FEW_N, {"PBN_F32_W32": "0"}, K16, 2),
    "plain16-nb3": ("KDE", 21, 257, FEW_N, {}, K16, 3),
    "plain16-d9": ("KDE", 9, 1023, FEW_N, {}, K16, 1),
    "plain16-d20": ("ProductKDE", 20, 257, FEW_N, {}, K16, 2),
    "w32-d5": ("KDE", 5, 4133, ALL_N, {}, KW32, 1),
    "w32-d8": ("KDE", 8, 1040, ALL_N, {}, KW32, 1),
    "w32-d8-small": ("ProductKDE", 8, 17, FEW_N, {}, KW32, 1),
    "w32-d10": ("KDE", 10, 2064, FEW_N, {}, KW32, 2),
    "w32-d19": ("KDE", 19, 1023, FEW_N, {}, KW32, 2),
    "ckde-nb1": ("CKDE", 4, 4133, ALL_N, {}, K16, 1),
    "ckde-nb2": ("CKDE", 11, 1040, FEW_N, {}, K16, 2),
    "w32p-d2": ("KDE", 2, 4133, ALL_N, {"PBN_PRUNE_MIN_ROWS": "256"}, KW32P, 1),
    "w32p-d6": ("KDE", 6, 2064, FEW_N, {"PBN_PRUNE_MIN_ROWS": "256"}, KW32P, 1),
    "prune16-d2": ("ProductKDE", 2, 4133, FEW_N, {"PBN_PRUNE_MIN_ROWS": "256", "PBN_F32_W32": "0"}, K16P, 1),
    "pckde-d5": ("CKDE", 5, 4133, FEW_N, {"PBN_PRUNE_MIN_ROWS": "256"}, K16P, 1),
    "prune16-257": ("KDE", 3, 257, FEW_N, {"PBN_PRUNE_MIN_ROWS": "256", "PBN_F32_W32": "0"}, K16P, 1),
}
PLAIN = [c for c in CASES if CASES[c][5] in (K16, KW32) and CASES[c][0] != "CKDE"]
NAMES = sorted(CASES)


def adds(rec):
    """fp32 additions on a term's path before the fp64 sum (module docstring)."""
    if rec["cond"]:
        return 2
    if rec["kernel"] in (K16, K16P):
        return 66
    if rec["kernel"] == KW32:
        return 38
    return 5 + fr.ceil_div(rec["tps"], 2) + 1


# ---- the aid ------------------------------------------------------------------------------------------------------------------------------
class Aid:
    def __init__(self):
        from pybnesian_amd import _lib

        L = _lib.load()
        self.fn = L.pbn_debug_f16_stages
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
        self.prune = L.pbn_debug_prune_stages
        self.prune.restype = C.c_int64
        self.prune.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
        self.w32 = L.pbn_debug_w32_launches
        self.w32.restype = None
        self.w32.argtypes = [C.c_void_p, C.c_int]

    def arm(self):
        self.fn(0, -1, None, 0, 0)
        self.fn(0, -1, None, 0, 1)

    def clear(self):
        self.fn(0, -1, None, 0, 0)

    def count(self):
        return int(self.fn(0, -1, None, 0, -1))

    def fit_perm(self, arm):
        """arm: pbn_debug_prune_stages on (a pruned fit keeps its order); else the last pruned fit's perm (sorted position -> row), the aid off again."""
        if arm:
            self.prune(0, 0, -1, None, 0, 0)
            self.prune(0, 0, -1, None, 0, 1)
            return None
        n = self.prune(0, 0, 7, None, 0, -1)
        out = np.zeros(max(int(n), 1), dtype=np.int32)
        if n > 0:
            assert self.prune(0, 0, 7, out.ctypes.data, n, -1) == n
        self.prune(0, 0, -1, None, 0, 0)
        return out[: max(int(n), 0)].astype(np.int64)

    def w32_launches(self, reset):
        c = C.c_ulonglong(0)
        self.w32(C.byref(c), int(reset))
        return int(c.value)

    def get(self, back, what, dtype):
        n = self.fn(back, what, None, 0, -1)
        assert n >= 0, (back, what)
        out = np.zeros(max(int(n), 1), dtype=dtype)
        assert self.fn(back, what, out.ctypes.data, n, -1) == n
        return out[:n]

    def record(self, back=0):
        r = dict(zip(HEAD, map(int, self.get(back, 0, np.int64))))
        r["margin"], r["lognorm"], r["lognorm_marg"] = map(float, self.get(back, 1, np.float64))
        d, nt, nqt, NB, P = r["d"], r["ntiles"], r["nqtiles"], r["NB"], r["P"]
        r["W"] = self.get(back, 2, np.float64).reshape(d, d)
        r["mu"] = self.get(back, 3, np.float64)
        r["cols"] = self.get(back, 4, np.int32).astype(np.int64)
        r["A"] = fr.decode_main(self.get(back, 5, np.uint16), nt, NB)
        r["B"] = fr.decode_main(self.get(back, 7, np.uint16), nqt, NB)
        r["ny"] = self.get(back, 8, np.float32)
        if r["cond"]:
            r["AX"] = fr.decode_extra(self.get(back, 6, np.uint16), nt)
            r["BX"] = fr.decode_extra(self.get(back, 9, np.uint16), nqt)
            r["xn"] = self.get(back, 10, np.float32)
        else:
            assert self.get(back, 6, np.uint16).size == 0 and self.get(back, 9, np.uint16).size == 0 and self.get(back, 10, np.float32).size == 0
        r["far"] = self.get(back, 11, np.uint8)
        r["qperm"] = self.get(back, 12, np.int32).astype(np.int64)
        r["part0"] = self.get(back, 13, np.float64).reshape(r["nsplit"], nqt * 16, P)
        r["part1"] = self.get(back, 14, np.float64).reshape(r["nsplit"], nqt * 16, P)
        assert r["ny"].size == nqt * 16 and r["far"].size == nqt * 16 and r["qperm"].size == (r["n"] if r["prune"] else 0)
        return r


@contextlib.contextmanager
def environment(env):
    keys = ("PBN_F32_W32", "PBN_PRUNE_MIN_ROWS", "PBN_F32_WIDEN_AT")
    old = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def make_model(pbn, cls, cols):
    if cls == "CKDE":
        return pbn.CKDE(cols[0], cols[1:])
    return getattr(pbn, cls)(cols)


def correlated(rng, rows, d):
    """Correlated normal columns of different scales and offsets, as float32."""
    mix = np.eye(d) + 0.35 * np.tril(rng.normal(size=(d, d)), -1)
    scale = 10.0 ** rng.uniform(-1, 1, size=d)
    return ((rng.normal(size=(rows, d)) @ mix.T) * scale + rng.normal(size=d) * 3 * scale).astype(np.float32)


def evaluate(k, aid, df, kind="logl"):
    """One armed evaluation -> (the class's result, the LAST record it left, W32 launches it made)."""
    aid.clear()
    aid.arm()
    aid.w32_launches(True)
    try:
        out = getattr(k, kind)(df)
        launches = aid.w32_launches(False)
        assert aid.count() >= 1, "no f16x2 evaluation was captured"
        return out, aid.record(0), launches
    finally:
        aid.clear()


@functools.lru_cache(maxsize=None)
def captured(name):
    """Fits the case's model and evaluates logl for every query count and slogl for the largest, with the aid armed."""
    import pybnesian_amd as pbn

    cls, d, N, ns, env, kernel, NB = CASES[name]
    cols = [f"c{j}" for j in range(d)]
    rng = np.random.default_rng(sum(map(ord, name)))
    data = correlated(rng, N + max(ns), d)
    train, pool = data[:N], data[N:]
    aid = Aid()
    with environment(env):
        k = make_model(pbn, cls, cols)
        aid.fit_perm(True)
        k.fit(pd.DataFrame(train, columns=cols))
        perm = aid.fit_perm(False)
        evals = {}
        for n in ns:
            q = pool[:n].copy()
            got, rec, launches = evaluate(k, aid, pd.DataFrame(q, columns=cols))
            evals[n] = dict(query=q, logl=got, rec=rec, launches=launches)
        q = pool[: max(ns)]
        got, rec, launches = evaluate(k, aid, pd.DataFrame(q, columns=cols), "slogl")
    return dict(train=train, perm=perm, evals=evals, slogl=dict(query=q, slogl=got, rec=rec, launches=launches))


def records(name):
    c = captured(name)
    return [(n, e) for n, e in sorted(c["evals"].items())] + [(len(c["slogl"]["query"]), c["slogl"])]


# ---- 0. every case reached its kernel -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_kernel(name):
    cls, d, N, ns, env, kernel, NB = CASES[name]
    cond = cls == "CKDE"
    dm = d - 1 if cond else d
    for n, e in records(name):
        r = e["rec"]
        want = dict(n=n, N=N, d=d, dm=dm, cond=int(cond), NB=NB, spd=fr.spd(dm), ntiles=fr.ceil_div(N, 16), nqtiles=fr.ceil_div(n, 16), P=4 if cond else 2,
                    kernel=kernel, prune=int(kernel in (K16P, KW32P)), w32=int(kernel in (KW32, KW32P)))
        assert {k: r[k] for k in want} == want
        assert NB == fr.blocks(dm)
        assert e["launches"] == (1 if kernel in (KW32, KW32P) else 0), "pbn_debug_w32_launches"
        assert r["nsplit"] == fr.ceil_div(r["ntiles"], r["tps"]) and 1 <= r["nsplit"] <= max(1, r["ntiles"] // 64)
        assert r["sum_only"] == int("slogl" in e)
        if kernel == KW32:
            assert fr.w32_applies(dm, NB)
        if kernel == K16 and not cond and "PBN_F32_W32" not in env:
            assert not fr.w32_applies(dm, NB)
        if N == 4133 and r["num_cus"] == 256:
            assert r["nsplit"] == 4 and r["tps"] == 65, "a clipped last split, a split that ends one tile into a blind chunk"
        if N == 2064 and r["num_cus"] == 256:
            assert r["nsplit"] == 2 and r["tps"] == 65


# ---- A (b). the pack on general designs ---------------------------------------------------------------------------------------------------
def whitened(rec, x):
    """W (x - mu) in longdouble for table rows x (columns in the table's order), and the fp64 slack of the kernel's fma chain."""
    xc = x[:, rec["cols"]].astype(LD) - rec["mu"].astype(LD)
    W = np.tril(rec["W"])
    z = (xc @ W.astype(LD).T).astype(np.float64)
    slack = (2 * rec["d"] + 3) * EPS * (np.abs(xc) @ np.abs(W).astype(LD).T).astype(np.float64)
    return z, slack


def check_side(rec, slots, xslots, x, query, order=None):
    """Stage A (b) for one side: x the table's rows in the order the fragments hold them."""
    dm, NB, cond = rec["dm"], rec["NB"], rec["cond"]
    rows = x.shape[0]
    smap = fr.slot_map(dm, NB, query)
    hi, lo, norm = fr.decoded_pieces(slots, smap)
    zr = fr.represented(hi, lo)
    z, slack = whitened(rec, x)
    assert np.all(np.abs(z) <= fr.H_MAX)
    err = np.abs(zr[:rows] - z[:, :dm])
    bound = fr.split_error_bound(z[:, :dm]) + slack[:, :dm]
    assert np.all(err <= bound), ("split", float((err / bound).max()))
    assert np.array_equal(fr.bits(fr.consistent_slots(slots, smap)), fr.bits(slots)), "a slot that does not follow from the row's own pieces"
    nv = fr.half_norm(zr[:rows])
    if query:
        assert np.array_equal(rec["ny"][:rows].view(np.uint32), nv.view(np.uint32)) and np.all(rec["ny"][rows:] == 0)
        assert np.all(slots[rows:].astype(np.float32)[:, : fr.spd(dm) * dm] == 0), "padding queries"
    else:
        want = fr.split3s(np.concatenate([nv, np.full(slots.shape[0] - rows, fr.PAD_NORM, dtype=np.float32)]))
        for t in range(3):
            assert np.array_equal(fr.bits(norm[t]), fr.bits(want[t])), ("norm piece", t)
    if cond:
        xmap = fr.extra_map(query)
        xhi, xlo, xnorm = fr.decoded_pieces(xslots, xmap)
        xr = fr.represented(xhi, xlo)[:, 0]
        errx = np.abs(xr[:rows] - z[:, dm])
        assert np.all(errx <= fr.split_error_bound(z[:, dm]) + slack[:, dm])
        assert np.array_equal(fr.bits(fr.consistent_slots(xslots, xmap)), fr.bits(xslots))
        hn = (-0.5 * xr * xr).astype(np.float32)
        want = fr.split3s(hn)
        for t in range(3):
            assert np.array_equal(fr.bits(xnorm[t]), fr.bits(want[t])), ("extra norm piece", t)
        if query:
            assert np.array_equal(rec["xn"].view(np.uint32), hn.view(np.uint32))
    if query:
        assert not rec["far"].any()


@pytest.mark.parametrize("name", NAMES)
def test_stage_a_pack_general(name):
    c = captured(name)
    for n, e in records(name):
        r = e["rec"]
        q = e["query"].astype(np.float64)
        check_side(r, r["B"], r.get("BX"), q[r["qperm"]] if r["prune"] else q, True)
    n, e = records(name)[0]
    r = e["rec"]
    if not r["prune"]:
        check_side(r, r["A"], r.get("AX"), c["train"].astype(np.float64), False)
    else:
        # a pruned model packs its training rows in the order of its space-filling curve (the fit's perm, through pbn_debug_prune_stages)
        assert sorted(c["perm"].tolist()) == list(range(r["N"]))
        check_side(r, r["A"], r.get("AX"), c["train"].astype(np.float64)[c["perm"]], False)


# ---- B. sweep partials --------------------------------------------------------------------------------------------------------------------
def stage_b(rec):
    """-> (worst remainder after the derived parts over the compared (split, query) pairs, pairs compared, pairs left out, the largest error /
    derived bound (unpruned forms), pairs the reference alone would leave out)."""
    N, n, NB, dm, cond = rec["N"], rec["n"], rec["NB"], rec["dm"], rec["cond"]
    K = 32 * NB
    w32 = rec["kernel"] in (KW32, KW32P)
    A, B = rec["A"][:N], rec["B"][:n]
    ny = rec["ny"][:n].astype(np.float64)
    assert np.all(fr.join3(*fr.decoded_pieces(rec["A"], fr.slot_map(dm, NB, False))[2])[N:] == -float(fr.X_MAX)), "padding rows' norm"
    main = fr.Pairs(A, B, ny)
    halves = [(main.e, main.mag, main.nnz, 0)]
    if cond:
        AX, BX = rec["AX"][:N, :6].astype(np.float64), rec["BX"][:n, :6].astype(np.float64)
        xn = rec["xn"][:n].astype(np.float64)
        assert np.all(rec["AX"][N:, :3].astype(np.float32) == 0)
        halves.append((main.e + AX @ BX.T + xn[None, :], main.mag + np.abs(AX) @ np.abs(BX).T + np.abs(xn)[None, :],
                       main.nnz + (AX != 0).astype(np.float64) @ (BX != 0).astype(np.float64).T, 2))
    worst, compared, skipped, ratio, ref_skipped = 0.0, 0, 0, 0.0, 0
    n_adds = adds(rec)
    for e, mag, nnz, o in halves:
        total = fr.log2_sum(e)
        for sp, (r0, r1) in enumerate(fr.split_ranges(rec["ntiles"], rec["tps"], N)):
            m, s = rec["part0"][sp, :n, o], rec["part0"][sp, :n, o + 1]
            assert np.all(np.isfinite(m)) and np.all(np.isfinite(s)) and np.all(s >= 0)
            es, mg, nz = e[r0:r1], mag[r0:r1], nnz[r0:r1]
            ref = fr.log2_sum(es)
            # the offset among the terms: one term (C operand) or three pieces + their residual; the fused joint: + xn + (m - mj), two float operations
            moff = np.abs(ny) + np.abs(m) if o == 0 else np.abs(ny) + np.abs(rec["part0"][sp, :n, 0]) + np.abs(m) + np.abs(rec["xn"][:n].astype(np.float64))
            k_off = (3 if w32 else 1) if o == 0 else 1 + 3 + 2
            per_pair = (nz + k_off + 1) * F32 * (mg + moff[None, :]) + K * EPS * (mg + moff[None, :])
            if w32 or o == 2:
                per_pair = per_pair + fr.norm_error_bound(moff)[None, :]
            w = np.exp2(es - ref[None, :])
            carries = w >= F32
            bound = np.where(carries, per_pair, 0.0).max(axis=0) + np.where(carries, 0.0, w * per_pair).sum(axis=0)
            lost = np.where(es - m[None, :] < -125.0, w, 0.0).sum(axis=0)            # terms the float exponential flushes
            dead = np.all(es - m[None, :] < -126.0, axis=0)
            # the same condition from the reference alone, m = the split's largest exponent for the query: what the DATA leaves out
            ref_skipped += int(np.all(es - es.max(axis=0)[None, :] < -126.0, axis=0).sum())
            if not rec["prune"]:
                # an unpruned kernel's offset is an exponent of this split (probe tiles, first tile, a rescued tile) as the matrix cores summed
                # it: never above the split's largest by more than that pair's own bound - a wrong offset cannot widen the set left out
                assert np.all(m <= es.max(axis=0) + per_pair.max(axis=0)), ("offset above the split's largest exponent", sp, o, float((m - es.max(axis=0)).max()))
            rel = ((1 + F32) ** n_adds - 1) + lost
            if rec["prune"]:
                # tiles may be dropped: up to N 2^-margin of the query's WHOLE sum; compared on the scale of that sum
                got = s * np.exp2(m - total)
                want = np.exp2(ref - total)
                tol = want * (np.exp2(bound) - 1 + rel + (0.0 if EXP_TOL is None else np.exp2(EXP_TOL) - 1)) + N * 2.0 ** -rec["margin"] + 2.0 ** -64
                rem = np.abs(got - want) - tol
                assert np.all(rem <= 0), ("pruned partial", sp, o, float(rem.max()))
                dead[:] = False                                       # (on the scale of the whole sum nothing needs leaving out)
            else:
                assert np.all(s[~dead] > 0)
                with np.errstate(divide="ignore"):
                    diff = np.abs(m + np.log2(s) - ref)
                rem = diff - bound - rel / LN2 * (1 + rel)
                ok = ~dead
                if ok.any():
                    worst = max(worst, float(rem[ok].max()))
                    ratio = max(ratio, float((diff[ok] / (bound + rel / LN2 * (1 + rel))[ok]).max()))
            compared += int((~dead).sum())
            skipped += int(dead.sum())
    return worst, compared, skipped, ratio, ref_skipped


MEASURED = {}


@pytest.mark.parametrize("name", NAMES)
def test_stage_b_sweep_partials(name):
    worst = ratio = 0.0
    compared = skipped = ref_skipped = 0
    for n, e in records(name):
        w, c, s, r, rs = stage_b(e["rec"])
        worst, compared, skipped, ratio, ref_skipped = max(worst, w), compared + c, skipped + s, max(ratio, r), ref_skipped + rs
    assert ref_skipped <= 0.001 * (compared + skipped), ("the data alone leaves out too much", ref_skipped, compared)
    assert skipped <= 0.001 * (compared + skipped), (skipped, compared)
    remainder = max(worst, 0.0)
    MEASURED[name] = remainder
    shown = "-: asserted on the scale of the whole sum" if CASES[name][5] in (K16P, KW32P) else f"{ratio:.3f}"
    print(f"\n[f16 stages] {name}: {compared} (split, query) partials, {skipped} left out, |m + log2 s - reference| beyond the derived parts: {remainder:.3e} (largest error / derived bound in this case {shown})")
    if CASES[name][5] in (K16P, KW32P):
        return                                                       # (asserted inside stage_b, on the scale of the whole sum)
    assert EXP_TOL is not None, "EXP_TOL has not been measured yet"
    if name in PLAIN:
        assert remainder <= EXP_TOL / 8, "the measured constant no longer covers its own measurement"
    assert remainder <= EXP_TOL


def test_exp_tol_measurement():
    """Prints the measured constant: the worst remainder over the unpruned plain cases."""
    for name in PLAIN:
        if name not in MEASURED:
            MEASURED[name] = max(0.0, max(stage_b(e["rec"])[0] for n, e in records(name)))
    worst = max(MEASURED[c] for c in PLAIN)
    print(f"\n[f16 stages] EXP_TOL measured {worst:.3e} over {len(PLAIN)} plain cases (worst: {max(PLAIN, key=lambda c: MEASURED[c])}) -> EXP_TOL = {8 * worst:.3e}")
    assert EXP_TOL is not None and worst <= EXP_TOL / 8


# ---- D. end to end ------------------------------------------------------------------------------------------------------------------------
def finish(rec):
    """What kde_finish_kernel makes of the captured post-fix partials: per (sorted) query logl, and the magnitude its rounding scales with."""
    n, P = rec["n"], rec["P"]
    part = rec["part1"][:, :n, :]
    marg = fr.merge_partials(part[:, :, 0:2])
    mag = np.abs(part[:, :, 0]).max(axis=0) + np.abs(marg)
    if not rec["cond"]:
        return rec["lognorm"] + LN2 * marg, abs(rec["lognorm"]) + LN2 * mag + 1
    joint = fr.merge_partials(part[:, :, 2:4])
    magj = np.abs(part[:, :, 2]).max(axis=0) + np.abs(joint)
    return (rec["lognorm"] + LN2 * joint) - (rec["lognorm_marg"] + LN2 * marg), abs(rec["lognorm"]) + abs(rec["lognorm_marg"]) + LN2 * (mag + magj) + 1


@pytest.mark.parametrize("name", NAMES)
def test_stage_d_end_to_end(name):
    c = captured(name)
    for n, e in sorted(c["evals"].items()):
        r = e["rec"]
        want, mag = finish(r)
        got = e["logl"][r["qperm"]] if r["prune"] else e["logl"]
        assert got.shape == (n,) and np.all(np.isfinite(got))
        assert np.all(np.abs(got - want) <= 64 * EPS * mag), float((np.abs(got - want) / mag).max())
    e = c["slogl"]
    want, mag = finish(e["rec"])
    assert abs(e["slogl"] - want.sum()) <= 64 * EPS * mag.sum() + len(want) * EPS * np.abs(want).sum()


# ---- A (a). the pack on exact designs -----------------------------------------------------------------------------------------------------
def exact_values(rng, count):
    """float32 coordinates at the edges of the split: 22 significant bits, below 2^-14 (a1 flushed), a flushed low piece, exact f16 values,
    +-65504, zeros of both signs; the rest 22-bit values over many binades."""
    special = np.array([1 + 2.0 ** -21, -(1 + 2.0 ** -21 + 2.0 ** -11), 2.0 ** -15 * (1 + 2.0 ** -21), -(2.0 ** -15) * 1.5, 2.0 ** -14, 2.0 ** -21, -(2.0 ** -22), 1.5, 1000.0,
                        -0.375, 65504.0, -65504.0, 0.0, -0.0, 3.0 + 2.0 ** -20, 2047.0 + 2.0 ** -11, 2.0 ** -14 * (1 - 2.0 ** -12), 65503.99609375, 4.0 - 2.0 ** -21])
    v = rng.normal(size=count) * 10.0 ** rng.uniform(-6, 4.5, size=count)
    v = np.clip(v, -fr.H_MAX, fr.H_MAX).astype(np.float32)
    v = (v.view(np.uint32) & np.uint32(0xFFFFFFFC)).view(np.float32)                # 22 significant bits
    idx = rng.permutation(count)[: 4 * len(special)]
    v[idx] = np.tile(special, 4).astype(np.float32)
    return v


def pin_unit_bandwidth(k, cls, d):
    """The product rule whitens with W_ii = sqrt(log2 e) / sqrt(h) = 1 exactly at h = log2 e.  The full rule goes through chol(H) and its inverse on
    the host, W_ii = sqrt(log2 e) (1 / sqrt(h)): at h = log2 e that is 1 - 2^-53, and no h within 200 ulps of log2 e, 4 log2 e, 16 log2 e or their
    inverses' images gives a power of two (1 / sqrt(h) steps over the one double that would) - for KDE the design is exact all the same: W is w I,
    and the kernel's fma(w, x, +-0) is the one rounding of w x that numpy's product makes."""
    k.bandwidth = np.full(d, LOG2E) if cls == "ProductKDE" else np.eye(d) * LOG2E


@pytest.mark.parametrize("cls,d", [("ProductKDE", 3), ("KDE", 5), ("ProductKDE", 9), ("KDE", 10)])
def test_stage_a_pack_exact(cls, d):
    import pybnesian_amd as pbn

    N, n = 4133, 257
    rng = np.random.default_rng(40 + d)
    cols = [f"c{j}" for j in range(d)]
    train = np.empty((N, d), dtype=np.float32)
    grid = (rng.integers(-2 ** 16, 2 ** 16, size=(512, d)) * 2.0 ** -10).astype(np.float32)   # +- rows on a grid: the centre (mean of the first 1 024 rows) is exactly 0
    train[0:1024:2], train[1:1024:2] = grid, -grid
    train[1024:] = exact_values(rng, (N - 1024) * d).reshape(N - 1024, d)
    train[1024] = 65504.0                                                           # |z|^2 beyond the norm's clamp
    query = exact_values(rng, n * d).reshape(n, d)
    query[3, 0], query[16, d - 1], query[200, 1], query[256, 0] = 65504.00390625, -65504.00390625, 1e6, -3e38   # just beyond the range, and far beyond
    flagged = np.zeros(n, dtype=bool)
    flagged[[3, 16, 200, 256]] = True
    aid = Aid()
    with environment({"PBN_F32_WIDEN_AT": "inf"}):
        k = make_model(pbn, cls, cols)
        k.fit(pd.DataFrame(train, columns=cols))
        pin_unit_bandwidth(k, cls, d)
        got, r, _ = evaluate(k, aid, pd.DataFrame(query, columns=cols))
    assert r["kernel"] in (K16, KW32) and (r["N"], r["n"], r["d"], r["cond"]) == (N, n, d, 0), "f16x2 fragments (not widened)"
    W, mu = r["W"], r["mu"]
    w = W[0, 0]
    assert np.array_equal(W, np.eye(d) * w), W
    assert w == 1.0 if cls == "ProductKDE" else abs(w - 1.0) <= 2.0 ** -52, ("W is the identity (the full rule: to one rounding of the host's chol and inverse)", w)
    assert np.all(mu == 0.0), mu
    assert not np.isnan(train).any() and not np.isnan(query).any()
    NB = r["NB"]
    T = fr.pack_rows(train.astype(np.float64)[:, r["cols"]] * w, N, d, NB, False, False)
    Q = fr.pack_rows(query.astype(np.float64)[:, r["cols"]] * w, n, d, NB, True, False)
    for side, want, have in (("training", T["slots"], r["A"]), ("query", Q["slots"], r["B"])):
        bad = np.argwhere(fr.bits(want) != fr.bits(have))
        assert bad.size == 0, (side, bad[:5], [(float(want[i, j]), float(have[i, j])) for i, j in bad[:5]])
    assert np.array_equal(Q["npack"].view(np.uint32), r["ny"].view(np.uint32))
    assert np.array_equal(Q["far"], r["far"]) and np.array_equal(r["far"][:n].astype(bool), flagged)
    assert r["far"][:n].sum() >= 4
    # and the rows behind the last valid one
    assert np.all(r["B"][n:, : fr.spd(d) * d].astype(np.float32) == 0) and np.all(r["ny"][n:] == 0) and not r["far"][n:].any()
    _, _, norm = fr.decoded_pieces(r["A"], fr.slot_map(d, NB, False))
    assert np.all(fr.join3(*norm)[N:] == -float(fr.X_MAX)) and np.all(fr.join3(*norm)[1024] == -float(fr.X_MAX))


# ---- C. the far fix -----------------------------------------------------------------------------------------------------------------------
FAR_ROWS = (0, 15, 19, 25, 37)          # tile positions 0 and 15, two in one tile, one in the last, partial tile (40 queries)


@pytest.mark.parametrize("cls,d,N", [("KDE", 3, 4133), ("ProductKDE", 2, 1040), ("CKDE", 3, 2064), ("KDE", 10, 2064)])
def test_stage_c_far_fix(cls, d, N):
    import pybnesian_amd as pbn

    n = 40
    rng = np.random.default_rng(90 + d + N)
    cols = [f"c{j}" for j in range(d)]
    data = correlated(rng, N + n, d)
    train, query = data[:N], data[N:].copy()
    sd = train.std(axis=0)
    for i, row in enumerate(FAR_ROWS):
        j = 0 if (cls == "CKDE" and i == 1) else (i % d)             # (a CKDE's variable is its extra coordinate: flagged through the CKDE block)
        query[row, j] = np.float32((-1) ** i * 2e5 * sd[j] * (1 + i))
    aid = Aid()
    with environment({}):
        k = make_model(pbn, cls, cols)
        k.fit(pd.DataFrame(train, columns=cols))
        got, r, _ = evaluate(k, aid, pd.DataFrame(query, columns=cols))
    cond, dm, NB, P = r["cond"], r["dm"], r["NB"], r["P"]
    assert (r["n"], r["N"], r["prune"]) == (n, N, 0)
    if N >= 2048 and r["num_cus"] >= 64:
        assert r["nsplit"] > 1
    z, slack = whitened(r, query.astype(np.float64))
    flagged = np.zeros(r["nqtiles"] * 16, dtype=bool)
    flagged[list(FAR_ROWS)] = True
    assert np.array_equal(r["far"].astype(bool), flagged)
    assert np.all(np.abs(z[list(FAR_ROWS)]).max(axis=1) > fr.H_MAX) and np.all(np.abs(z[~flagged[:n]]).max(axis=1) < 1000)
    # unflagged queries: untouched
    keep = ~flagged
    assert np.array_equal(r["part0"][:, keep, :].view(np.uint64), r["part1"][:, keep, :].view(np.uint64))
    hi, lo, _ = fr.decoded_pieces(r["A"], fr.slot_map(dm, NB, False))
    zt = fr.represented(hi, lo)[:N]
    if cond:
        xhi, xlo, _ = fr.decoded_pieces(r["AX"], fr.extra_map(False))
        zt = np.concatenate([zt, fr.represented(xhi, xlo)[:N]], axis=1)
    for row in FAR_ROWS:
        zq = z[row]
        for o, dims in ((0, dm),) + (((2, dm + 1),) if cond else ()):
            e = -0.5 * ((zt[:, :dims].astype(LD) - zq[:dims].astype(LD)) ** 2).sum(axis=1)
            top = e.max()
            want = float(top + np.log2(np.exp2(e - top).sum()))
            tol = (d + 3) * EPS * ((zq ** 2).sum() + (zt ** 2).sum(axis=1).max()) + 2 * float(np.abs(-(zt[:, :dims] - zq[:dims]) * slack[row, :dims]).sum(axis=1).max())
            m, s = r["part1"][:, row, o], r["part1"][:, row, o + 1]
            assert s[0] > 0 and np.isfinite(m[0])
            assert abs(m[0] + math.log2(s[0]) - want) <= tol, (row, o, m[0] + math.log2(s[0]) - want, tol)
            assert np.all(m[1:] == m[0]) and np.all(s[1:] == 0)
    # D for these rows too: what the class returns is the merge of the captured post-fix partials
    want, mag = finish(r)
    assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= 64 * EPS * mag)
