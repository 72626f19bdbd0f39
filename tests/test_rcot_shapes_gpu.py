"""RCoT's two device passes (csrc/rcot.hip) at every kernel shape, against fp64 numpy references.

K1 (rcot_gram_kernel<PPW>) is the Gram of A = [sqrt(2) cos(v W + b) - shift, 1] over a test's valid rows; K2 (rcot_prod_kernel) is the
Gram of the residual products rx_i ry_j, R = A P.  The test aid pbn_debug_rcot captures W, b, the pilot shift, P and both unpacked Grams
of every test, and logs every launch (the PPW instantiation or the product tiles, the tests, the dynamic LDS).  The references are
built from the captured parameters and the table itself, and each Gram entry is held to a forward-error bound (gram_bound).  The grid
covers every K1 tile count, every PPW instantiation, every K2 tile count, conditioning sets up to the cap and the row partition's
edges; then nulls at those edges, end-to-end parity on some of the shapes, batches (mixed tile counts in one launch, several memory
chunks) against single calls, the trivial cases, and the rows of a test whose every Z column is dropped."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from rcot_restatement import check_parity, normalize

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
U = EPS / 2            # unit roundoff
REF_BLOCK = 1024       # rows per block of the reference Grams


def rows_per_block(n):
    """run_plans' row partition (rows_per_block in rcot.hip)."""
    return max(1024, (-(-n // 512) + 15) // 16 * 16)


def gamma(n):
    return n * U / (1 - n * U)


# ---- the capture hook ----------------------------------------------------------------------------------------------------------
class Capture:
    def __init__(self):
        from pybnesian_amd import _lib

        self.fn = _lib.load().pbn_debug_rcot
        self.fn.restype = C.c_int64
        self.fn.argtypes = [C.c_int, C.c_void_p, C.c_int64]

    def arm(self):
        self.fn(1, None, 0)

    def disarm(self):
        self.fn(0, None, 0)

    def launches(self):
        """[pass (1 = K1, 2 = K2), PPW (K1) or ntq (K2), tests, dynamic LDS bytes, blocks] per launch since arm()."""
        n = self.fn(3, None, 0)
        out = np.zeros(n, dtype=np.int64)
        self.fn(3, out.ctypes.data, n)
        return out.reshape(-1, 5)

    def records(self):
        n = self.fn(2, None, 0)
        buf = np.zeros(n)
        self.fn(2, buf.ctypes.data, n)
        recs, i = [], 0
        while i < n:
            F, nxy, k, nz, n_valid, nc = (int(v) for v in buf[i:i + 6])
            i += 6
            r = {"F": F, "nxy": nxy, "k": k, "nz": nz, "n_valid": n_valid, "cols": buf[i:i + nc].astype(int)}
            i += nc
            for name, size in (("W", 2 * nxy + k * nz), ("b", F), ("shift", F), ("G1", (F + 1) ** 2), ("P", (F + 1) * 2 * nxy),
                               ("G2", nxy ** 4)):
                r[name] = buf[i:i + size]
                i += size
            r["G1"] = r["G1"].reshape(F + 1, F + 1)
            r["P"] = r["P"].reshape(F + 1, 2 * nxy)
            r["G2"] = r["G2"].reshape(nxy * nxy, nxy * nxy)
            recs.append(r)
        return recs


@pytest.fixture(scope="module")
def cap():
    import pybnesian_amd

    pybnesian_amd.load_library()
    c = Capture()
    yield c
    c.disarm()
    print(f"\nlargest err / bound: K1 {WORST['K1']:.3g}, K2 {WORST['K2']:.3g}")


# ---- the references --------------------------------------------------------------------------------------------------------------
def features(rec, v):
    """A = [sqrt(2) cos(v W + b) - shift, 1] of the rows v (columns x, y, Z used) and T, a bound of |v W| + |b| per entry."""
    F, nxy, k = rec["F"], rec["nxy"], rec["k"]
    W, b = rec["W"], rec["b"]
    arg = np.empty((len(v), F))
    T = np.empty((len(v), F))
    arg[:, :nxy] = v[:, :1] * W[:nxy] + b[:nxy]
    arg[:, nxy:2 * nxy] = v[:, 1:2] * W[nxy:2 * nxy] + b[nxy:2 * nxy]
    T[:, :nxy] = np.abs(v[:, :1] * W[:nxy]) + np.abs(b[:nxy])
    T[:, nxy:2 * nxy] = np.abs(v[:, 1:2] * W[nxy:2 * nxy]) + np.abs(b[nxy:2 * nxy])
    if k:
        Wz = W[2 * nxy:].reshape(rec["nz"], k).T
        arg[:, 2 * nxy:] = v[:, 2:2 + k] @ Wz + b[2 * nxy:]
        T[:, 2 * nxy:] = np.abs(v[:, 2:2 + k]) @ np.abs(Wz) + np.abs(b[2 * nxy:])
    A = np.ones((len(v), F + 1))
    A[:, :F] = np.sqrt(2.0) * np.cos(arg) - rec["shift"]
    return A, T


def gram_bound(rec, table_cols, n_rows):
    """The references of both Grams of one captured test and their forward-error bounds.

    Units: eps = 2^-52, u = eps / 2, gamma(n) = n u / (1 - n u).  The inputs are the device's own bits (normalize repeats the host's
    arithmetic); W, b, shift and P are captured.

    Features.  The argument t = v W + b is k' + 1 roundings (k' = max(1, k)) away from exact on either side, so within
    gamma(k' + 1) T of it, T = |v| |W| + |b|.  cos is within 2 ulp (<= eps) on either side, and sqrt(2) * and - shift round once
    each.  Hence |A_dev - A_ref| <= E = (sqrt(2) (2 gamma(k' + 1) T + 3 eps) + eps |A|) / (1 - eps), 0 in the ones column, and
    Abar = |A| + E bounds both sides' |A|.

    K1.  Any order of summation of n terms is within gamma(n - 1) of the sum of their magnitudes.  The device sums a block's rows on the
    MFMA and the blocks in order, a chain of L_dev = rows per block + blocks + 1 (the product's rounding); the reference sums
    REF_BLOCK-row blocks in BLAS and the blocks in order, L_ref = REF_BLOCK + blocks + 1.  So
        |G1 - G1_ref| <= E^T Abar + Abar^T E + (gamma(L_dev) + gamma(L_ref)) Abar^T Abar,
    i.e. c eps M with M = |A|^T |A| and c = (L_dev + L_ref) / 2, plus the features' term, which grows with |v W + b|.  The count
    G1[F, F] is an integer sum: exact.

    K2.  R = A P is a sum of F + 1 products on either side (the device splits it over four waves: four more additions), so
    |R_dev - R_ref| <= ER = E |P| + (gamma(F + 6) + gamma(F + 2)) Abar |P|, and Rbar = |R_ref| + ER bounds both.  A product
    q = rx ry rounds once: |q_dev - q_ref| <= EQ = ERx Rbar_y + Rbar_x ERy + eps Qbar, Qbar = Rbar_x Rbar_y (1 + u).  Then as K1:
        |G2 - G2_ref| <= EQ^T Qbar + Qbar^T EQ + (gamma(L_dev) + gamma(L_ref)) Qbar^T Qbar.
    P is large where Czz is nearly singular; the bound carries it through |P|, not through its constant."""
    F, nxy, k = rec["F"], rec["nxy"], rec["k"]
    nq = nxy * nxy
    kp = max(1, k)
    P, Pa = rec["P"], np.abs(rec["P"])
    acc = {key: 0.0 for key in ("G1", "M1", "E1", "G2", "M2", "E2")}
    for r0 in range(0, len(table_cols), REF_BLOCK):
        v = table_cols[r0:r0 + REF_BLOCK]
        A, T = features(rec, v)
        E = np.zeros_like(A)
        E[:, :F] = (np.sqrt(2.0) * (2 * gamma(kp + 1) * T + 3 * EPS) + EPS * np.abs(A[:, :F])) / (1 - EPS)
        Abar = np.abs(A) + E
        acc["G1"] = acc["G1"] + A.T @ A
        acc["M1"] = acc["M1"] + Abar.T @ Abar
        acc["E1"] = acc["E1"] + E.T @ Abar
        R = A @ P
        ER = E @ Pa + (gamma(F + 6) + gamma(F + 2)) * (Abar @ Pa)
        Rbar = np.abs(R) + ER
        Q = (R[:, :nxy, None] * R[:, None, nxy:]).reshape(-1, nq)
        Qbar = (Rbar[:, :nxy, None] * Rbar[:, None, nxy:]).reshape(-1, nq) * (1 + U)
        EQ = (ER[:, :nxy, None] * Rbar[:, None, nxy:] + Rbar[:, :nxy, None] * ER[:, None, nxy:]).reshape(-1, nq) + EPS * Qbar
        acc["G2"] = acc["G2"] + Q.T @ Q
        acc["M2"] = acc["M2"] + Qbar.T @ Qbar
        acc["E2"] = acc["E2"] + EQ.T @ Qbar
    rpb = min(rows_per_block(n_rows), n_rows)
    nb_dev = -(-n_rows // rows_per_block(n_rows))
    nb_ref = -(-len(table_cols) // REF_BLOCK)
    chain = gamma(rpb + nb_dev + 1) + gamma(REF_BLOCK + nb_ref + 1)
    b1 = acc["E1"] + acc["E1"].T + chain * acc["M1"]
    b2 = acc["E2"] + acc["E2"].T + chain * acc["M2"]
    return acc["G1"], b1, acc["G2"], b2


WORST = {"K1": 0.0, "K2": 0.0}


def ratio(err, bound):
    """|err| / bound, where a zero bound (a residual whose coefficients are all zero) admits only a zero error."""
    return np.where(bound > 0, np.abs(err) / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))


def check_record(rec, table, names, n_rows):
    """K1 and K2 of one captured test against the references over the rows valid in every column the test read."""
    cols = [names[c] for c in rec["cols"]]
    v = np.column_stack([normalize(table[c]) for c in cols])
    v = v[~np.isnan(v).any(axis=1)]
    F = rec["F"]
    assert rec["G1"][F, F] == float(len(v)) and rec["n_valid"] == len(v), (rec["G1"][F, F], rec["n_valid"], len(v))
    g1, b1, g2, b2 = gram_bound(rec, v[:, :2 + rec["k"]], n_rows)
    r1, r2 = ratio(rec["G1"] - g1, b1), ratio(rec["G2"] - g2, b2)
    WORST["K1"] = max(WORST["K1"], float(r1.max()))
    WORST["K2"] = max(WORST["K2"], float(r2.max()))
    assert r1.max() <= 1, ("K1", np.unravel_index(r1.argmax(), r1.shape), float(r1.max()))
    assert r2.max() <= 1, ("K2", np.unravel_index(r2.argmax(), r2.shape), float(r2.max()))


def make_table(n, k, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(n, k))
    s = z.sum(axis=1) / np.sqrt(max(k, 1)) if k else np.zeros(n)
    x = np.sin(s) + 0.5 * rng.normal(size=n)
    y = np.cos(s) + 0.3 * x ** 2 + 0.5 * rng.normal(size=n)
    d = {"x": x, "y": y}
    for i in range(k):
        d[f"z{i}"] = z[:, i]
    return pd.DataFrame(d)


def run_one(cap, df, nxy, nz, z, seed=3):
    """One test x, y | z with the capture armed: its record and the launches it made."""
    import pybnesian_amd as pbn
    from pybnesian_amd import _lib

    t = pbn.RCoT(df, nxy, nz, seed=seed)
    a = t._args("x", "y", z)
    cap.arm()
    try:
        _lib.check(_lib.load().pbn_rcot_set_order(t._handle, 0, None))
        p = _lib.load().pbn_rcot_pvalue(t._handle, *a)
        recs, log = cap.records(), cap.launches()
    finally:
        cap.disarm()
    return t, p, recs, log


# ---- the shape grid --------------------------------------------------------------------------------------------------------------
# (nxy, nz, k, N): F + 1 = 2 nxy + (nz if k else 0) + 1, nt = ceil((F + 1) / 16), PPW = ceil(nt (nt + 1) / 8) rounded up to the
# instantiations 1, 2, 4, 8, 16, 34; ntq = ceil(nxy^2 / 16).
SHAPES = [
    (1, 4, 0, 2),            # F + 1 = 3: nt 1, PPW 1
    (2, 4, 0, 3),            # 5: nt 1
    (8, 4, 0, 15),           # 17: nt 2 (no Z), ntq 4
    (4, 7, 1, 16),           # 16: nt 1, a full 16-column tile; a full product tile (16 products)
    (5, 6, 2, 17),           # 17: nt 2
    (6, 20, 7, 1023),        # 33: nt 3, PPW 2; ntq 3
    (7, 40, 2, 1024),        # 55: nt 4, PPW 4
    (2, 70, 16, 1025),       # 75: nt 5, PPW 4
    (5, 80, 1, 20_000),      # 91: nt 6, PPW 8
    (5, 100, 7, 20_000),     # 111: nt 7, PPW 8 (the defaults)
    (8, 110, 2, 1025),       # 127: nt 8, PPW 16
    (1, 140, 62, 1024),      # 143: nt 9, 62 Z columns (the cap)
    (4, 150, 16, 1023),      # 159: nt 10, PPW 16
    (6, 160, 1, 1025),       # 173: nt 11, PPW 34
    (7, 175, 7, 20_000),     # 190: nt 12
    (2, 200, 2, 1025),       # 205: nt 13
    (8, 200, 62, 1024),      # 217: nt 14
    (5, 225, 1, 1023),       # 236: nt 15
    (4, 231, 7, 1025),       # 240: nt 15, full
    (5, 230, 16, 1024),      # 241: nt 16
    (8, 239, 62, 20_000),    # 256: nt 16 (the cap); K2 LDS 75 776 B
    (4, 10, 1, 600_001),     # 19: nt 2; blocks of 1 184 rows, a short last block
    (1, 3, 2, 3),            # 6: nt 1; three rows, a rank-deficient Czz
]


def ppw_of(nt):
    need = (nt * (nt + 1) // 2 + 3) // 4   # tile pairs per wave
    return next(p for p in (1, 2, 4, 8, 16, 34) if p >= need)


def nt_of(nxy, nz, k):
    return -(-(2 * nxy + (nz if k else 0) + 1) // 16)


def test_grid_covers_every_axis():
    fp1 = {2 * nxy + (nz if k else 0) + 1 for nxy, nz, k, _ in SHAPES}
    assert {nt_of(nxy, nz, k) for nxy, nz, k, _ in SHAPES} == set(range(1, 17))
    assert {16, 17, 240, 241, 256} <= fp1
    assert {ppw_of(nt_of(nxy, nz, k)) for nxy, nz, k, _ in SHAPES} == {1, 2, 4, 8, 16, 34}
    assert {nxy for nxy, _, _, _ in SHAPES} >= {1, 2, 4, 5, 6, 7, 8}
    assert {k for _, _, k, _ in SHAPES} >= {0, 1, 2, 7, 16, 62}
    assert {n for _, _, _, n in SHAPES} >= {2, 3, 15, 16, 17, 1023, 1024, 1025, 20_000, 600_001}


@pytest.mark.parametrize("nxy,nz,k,n", SHAPES, ids=[f"nxy{a}-nz{b}-k{c}-N{d}" for a, b, c, d in SHAPES])
def test_kernels_against_reference(cap, nxy, nz, k, n):
    df = make_table(n, k, 1000 + n + 7 * k + nxy)
    z = [f"z{i}" for i in range(k)] or None
    t, p, recs, log = run_one(cap, df, nxy, nz, z)
    assert len(recs) == 1 and len(log) == 2, (len(recs), log)
    rec = recs[0]
    nt = nt_of(nxy, nz, k)
    assert rec["F"] + 1 == 2 * nxy + (nz if k else 0) + 1 and rec["k"] == k
    assert log[0, 0] == 1 and log[0, 1] == ppw_of(nt) and log[1, 0] == 2 and log[1, 1] == -(-nxy * nxy // 16)
    table = {c: df[c].to_numpy(dtype=np.float64) for c in df.columns}
    check_record(rec, table, t._names, n)
    assert 0 <= p <= 1, p
    print(f"nxy {nxy} nz {nz} k {k} N {n}: nt {nt} PPW {log[0, 1]} ntq {log[1, 1]} LDS {log[0, 3]} / {log[1, 3]} B; "
          f"worst err/bound so far K1 {WORST['K1']:.3g} K2 {WORST['K2']:.3g}")


def test_nulls_at_partition_edges(cap):
    """Nulls at rows 0, 15, 16, 1023, 1024 and N - 1, a whole null 16-row chunk and a whole null 1024-row block (N = 4100: blocks
    of 1024 rows and a 4-row last block)."""
    n = 4100
    df = make_table(n, 2, 77)
    for c, r in (("x", 0), ("y", 15), ("z0", 16), ("z1", 1023), ("x", 1024), ("y", n - 1), ("z0", 4096)):
        df.loc[r, c] = np.nan
    df.loc[32:47, "z1"] = np.nan              # the chunk of rows 32 .. 47
    df.loc[2048:3071, "y"] = np.nan           # the third block
    table = {c: df[c].to_numpy(dtype=np.float64) for c in df.columns}
    for nxy, nz, z in ((5, 30, ["z0", "z1"]), (7, 100, ["z1"]), (4, 20, None)):
        t, p, recs, log = run_one(cap, df, nxy, nz, z)
        assert len(recs) == 1, len(recs)
        valid = ~np.isnan(np.column_stack([table[c] for c in ["x", "y"] + (z or [])])).any(axis=1)
        assert recs[0]["n_valid"] == int(valid.sum())
        check_record(recs[0], table, t._names, n)
        assert 0 <= p <= 1


def test_coverage_from_launch_log(cap):
    """A compact list whose launch log must show every PPW instantiation, K2 at every product tile count and a K2 launch above the
    default 64 KiB of dynamic LDS."""
    import pybnesian_amd as pbn

    df = make_table(300, 16, 5)
    z16 = [f"z{i}" for i in range(16)]
    runs = [(4, 4, None), (5, 22, ["z0"]), (6, 40, ["z0", "z1"]), (7, 70, ["z2"]), (5, 120, z16[:3]), (8, 160, ["z3"]),
            (5, 245, z16)]
    cap.arm()
    try:
        for nxy, nz, z in runs:
            t = pbn.RCoT(df, nxy, nz, seed=1)
            assert 0 <= t.pvalue("x", "y", z) <= 1
        log = cap.launches()
    finally:
        cap.disarm()
    seen = sorted(set(map(tuple, log[:, :2].tolist())))
    print("launches (pass, PPW | ntq):", seen, "K2 LDS:", log[log[:, 0] == 2, 3].tolist())
    assert {int(v) for v in log[log[:, 0] == 1, 1]} == {1, 2, 4, 8, 16, 34}
    assert {int(v) for v in log[log[:, 0] == 2, 1]} == {1, 2, 3, 4}
    assert (log[log[:, 0] == 2, 3] > 65536).any()


def _batch(t, items):
    from pybnesian_amd import _lib

    lib = _lib.load()
    _lib.check(lib.pbn_rcot_set_order(t._handle, 0, None))
    names = t._names
    v1 = _lib.int_array([names.index(a) for a, _, _ in items])
    v2 = _lib.int_array([names.index(b) for _, b, _ in items])
    off = np.cumsum([0] + [len(z) for _, _, z in items]).tolist()
    cond = _lib.int_array([names.index(c) for _, _, z in items for c in z] or [0])
    out = np.zeros(len(items))
    lib.pbn_rcot_pvalue_batch(t._handle, len(items), v1, v2, _lib.int_array(off), cond, _lib.dptr(out))
    return out


def test_batch_mixes_one_and_sixteen_tiles(cap):
    """A 1-tile test (no Z) runs in rcot_gram_kernel<34> with LDS sized for the 16-tile test beside it: the same bits as alone."""
    import pybnesian_amd as pbn

    df = make_table(3000, 2, 21)
    t = pbn.RCoT(df, 5, 245, seed=8)
    items = [("x", "y", []), ("x", "y", ["z0", "z1"])]
    cap.arm()
    try:
        single = [t.pvalue(a, b, z or None) for a, b, z in items]
        alone = cap.records()
        cap.arm()
        got = _batch(t, items)
        log, together = cap.launches(), cap.records()
    finally:
        cap.disarm()
    assert got.tolist() == single
    assert log[0].tolist()[:3] == [1, 34, 2] and log[1].tolist()[:3] == [2, 2, 2]
    for r1, r2 in zip(alone, together):
        assert np.array_equal(r1["G1"], r2["G1"]) and np.array_equal(r1["G2"], r2["G2"])
    table = {c: df[c].to_numpy(dtype=np.float64) for c in df.columns}
    for rec in together:
        check_record(rec, table, t._names, len(df))


def test_batch_over_three_memory_chunks(cap):
    """Five 16-tile tests at N = 600 001: 136 tile pairs x 507 blocks x 256 doubles each, two to a 48 Mi-double chunk."""
    import pybnesian_amd as pbn

    df = make_table(600_001, 4, 22)
    t = pbn.RCoT(df, 5, 245, seed=9)
    items = [("x", "y", ["z0"]), ("x", "y", ["z1"]), ("x", "z0", ["z2"]), ("y", "z2", ["z3"]), ("z1", "z3", ["x"])]
    single = [t.pvalue(a, b, z) for a, b, z in items]
    cap.arm()
    try:
        got = _batch(t, items)
        log = cap.launches()
    finally:
        cap.disarm()
    k1 = log[log[:, 0] == 1]
    assert len(k1) >= 3 and k1[:, 2].sum() == len(items), log
    assert got.tolist() == single


def test_trivial_cases(cap):
    import pybnesian_amd as pbn

    one = pd.DataFrame({"x": [0.5], "y": [1.5]})
    df = make_table(500, 1, 23)
    df.loc[1:, "x"] = np.nan                  # every row but the first null in x
    cap.arm()
    try:
        assert pbn.RCoT(one, seed=1).pvalue("x", "y") == 1.0
        t = pbn.RCoT(df, seed=1)
        assert t.pvalue("x", "y") == 1.0
        assert t.pvalue("x", "y", "z0") == 1.0
        assert len(cap.launches()) == 0 and cap.records() == []
    finally:
        cap.disarm()


def test_constant_z_with_nulls_uses_rows_valid_in_z():
    """Every Z column constant on the rows valid in x, y and Z, and null on rows where x and y are valid: the reference runs RIT on
    the rows valid in x, y and Z (RCoT.cpp, pvalue with one Z and with several)."""
    df = make_table(3000, 0, 24)
    rng = np.random.default_rng(3)
    df.loc[rng.random(3000) < 0.03, "x"] = np.nan
    df["c"] = 2.5
    df.loc[rng.random(3000) < 0.2, "c"] = np.nan
    df["d"] = -1.0
    df.loc[rng.random(3000) < 0.1, "d"] = np.nan
    table = {c: df[c].to_numpy(dtype=np.float64) for c in df.columns}
    ok = lambda cs: ~np.isnan(np.column_stack([table[c] for c in cs])).any(axis=1)
    for z in ("c", ["c", "d"]):
        zs = [z] if isinstance(z, str) else z
        rows = ok(["x", "y"] + zs)
        assert rows.sum() < ok(["x", "y"]).sum()
        det = check_parity(df, z, rows=rows)
        assert det["z"] == [] and det["n_valid"] == int(rows.sum())
    # a Z column without nulls still leaves the bits of the no-Z test alone
    import pybnesian_amd as pbn

    df["e"] = 4.0
    t = pbn.RCoT(df, seed=11)
    assert t.pvalue("x", "y", "e") == t.pvalue("x", "y")


def test_parity_on_new_shapes():
    """End-to-end parity: one weight (HBE), four weights (the LPB4 edge), nxy = 8, 16 tiles with 62 Z columns, 16 Z columns."""
    for nxy, nz, k, n in ((1, 10, 0, 20_000), (2, 20, 2, 20_000), (8, 239, 62, 20_000), (5, 100, 16, 20_000)):
        df = make_table(n, k, 3000 + nxy + k)
        det = check_parity(df, [f"z{i}" for i in range(k)] or None, nxy=nxy, nz=nz, seed=12)
        assert det["n_valid"] == n
        if nxy == 1:
            assert det["method"] == "HBE"
