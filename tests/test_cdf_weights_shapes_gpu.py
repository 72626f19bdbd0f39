"""GPU tier: the weight kernels behind CKDE.cdf and CKDE.sample (csrc/kde_cdf.hip: kde_cdf_kernel, kde_cdf_finish_kernel;
csrc/sampling.hip: pick_locate_kernel, pick_scan_kernel) at every launch shape, against a log-domain restatement in numpy fp64.

The reference's exp(logl) form (oracle.ckde_cdf / oracle.ckde_sample restate it) underflows exactly where the device's offset
machinery starts to work, so the truth here is

    lw[t, q] = -1/2 |L^-1 (e_q - e_t)|^2,   L L^T = H[1:, 1:]
    cdf_q    = exp(logsumexp_t(lw + log Phi((x_q - x_t - b.(e_q - e_t)) / sigma_c)) - logsumexp_t(lw))

with b = H22^-1 H21 and sigma_c^2 = H11 - H12 b; the oracle is a second reference wherever no weight underflows, which every test
checks on the CPU.  Bandwidths are pinned (a selector that returns H; one test pins through kde_joint().bandwidth and must agree bit
for bit), so that the test knows H, b and sigma_c.

Launch shapes follow from the callers' rules alone, never from the device: pbn_ckde_cdf takes
nsplit = min(ceil(16 CUs / qblocks), ntiles / 16) training splits, qblocks = ceil(query tiles / 8) - hence one split up to 496 rows
on any device, and ntiles / 16 of them whenever ceil(16 / qblocks) >= ntiles / 16 (true on one CU already: `cdf_splits` asserts it);
pbn_ckde_sample always splits at 64 tiles (1 024 rows).  A block serves 4 waves x 2 query tiles; the training rows come in tiles of 16.

Reach conditions (rescale thresholds, split counts, the 2^-80 isolation of forced picks, oracle validity) are asserted from CPU
arithmetic in every test: a case that stops reaching its branch fails."""
import functools
import os

import numpy as np
import pandas as pd
import pytest
from scipy.linalg import solve_triangular
from scipy.special import logsumexp
from scipy.stats import norm

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
DTYPES = ["float64", "float32"]
P_BOTH = [1, 4, 5, 16]          # KS = 1, 1, 2, 4 fragments per tile
P_CDF = [(dt, p) for dt in DTYPES for p in P_BOTH] + [("float64", 17)]      # 17: the runtime-sized fp64 kernel
P_SAMPLE = [(dt, p) for dt in DTYPES for p in (1, 5, 16)] + [("float64", 17)]
QUERY_COUNTS = [1, 15, 16, 17, 112, 113, 127, 128, 129, 257]
TRAIN_COUNTS = [1, 2, 15, 16, 17, 31, 33, 496, 512, 513, 1237]
SAMPLE_COUNTS = TRAIN_COUNTS + [1024, 1025, 1040, 2049]
# fp64: the project's numbers (test_ckde_gpu.py); fp32: the reference tests' absolute 5e-4 against the fp64 truth
TOL = {"float64": dict(rtol=1e-8, atol=1e-13), "float32": dict(rtol=0.0, atol=5e-4)}
# below these, exp(lw + lognorm) in the oracle's arithmetic has lost its leading weights (fp64: the issue's -700; fp32: expf
# leaves the normal range at -87.3)
ORACLE_FLOOR = {"float64": -700.0, "float32": -80.0}
# kde_cdf_kernel rescales when a lane's four weights reach big() = 2^900 (fp64) / 2^100 (fp32) against the running offset: a rise of the
# tile maximum beyond HI certainly does, one below LO certainly does not
RESCALE_HI = {"float64": 950.0, "float32": 110.0}
RESCALE_LO = {"float64": 850.0, "float32": 90.0}


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def recorded():
    """results of the library before fp32 handles that KDE.logl widens got fp64 cdf / sample fragments: written by
    tests/golden/gen_cdf_weights_recorded.py with the library built from commit 8bfb9b6, the parent of that change"""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cdf_weights_recorded.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


def names(p):
    return ["y"] + [f"e{i}" for i in range(p)]


def frame(arr, dtype):
    return pd.DataFrame(np.asarray(arr), columns=names(arr.shape[1] - 1)).astype(dtype)


def rounded(arr, dtype):
    """the table as the device sees it, in fp64 (the truth is computed on the rounded values)"""
    return np.asarray(arr).astype(dtype).astype(np.float64)


def fitted(pbn, train, H, dtype):
    """CKDE on `train` (column 0 = variable) with the joint bandwidth pinned at H: a selector that returns H hands it to pbn_ckde_fit
    like `kde_joint().bandwidth = H` does, and lets fit accept fewer rows than variables"""

    class Pinned(pbn.BandwidthSelector):
        def bandwidth(self, df, variables):
            return np.array(H)

    cpd = pbn.CKDE("y", names(train.shape[1] - 1)[1:], Pinned())
    cpd.fit(frame(train, dtype))
    assert np.array_equal(cpd.bandwidth, H) and cpd.num_instances() == train.shape[0]
    return cpd


def cond(H):
    """(L, b, sigma_c, lognorm of the evidence KDE without its 1/N)"""
    H = np.asarray(H, dtype=np.float64)
    L = np.linalg.cholesky(H[1:, 1:])
    b = np.linalg.solve(H[1:, 1:], H[1:, 0])
    p = H.shape[0] - 1
    return L, b, np.sqrt(H[0, 0] - H[0, 1:] @ b), -np.log(np.diag(L)).sum() - 0.5 * p * np.log(2 * np.pi)


def log_weights(train, H, ev):
    """lw[t, q] from the differences, in fp64"""
    L = cond(H)[0]
    p = L.shape[0]
    diff = ev[None, :, :] - train[:, None, 1:]
    z = solve_triangular(L, diff.reshape(-1, p).T, lower=True, check_finite=False)
    return (-0.5 * (z * z).sum(axis=0)).reshape(train.shape[0], ev.shape[0])


def true_cdf(train, H, test, lw=None):
    _, b, sc, _ = cond(H)
    if lw is None:
        lw = log_weights(train, H, test[:, 1:])
    mu = train[:, None, 0] + (test[None, :, 1:] - train[:, None, 1:]) @ b
    lc = norm.logcdf((test[None, :, 0] - mu) / sc)
    return np.exp(logsumexp(lw + lc, axis=0) - logsumexp(lw, axis=0))


def cdf_splits(N, n):
    """(nsplit, tiles per split) of pbn_ckde_cdf, and the proof that no device has another"""
    ntiles, qblocks = -(-N // 16), -(-(-(-n // 16)) // 8)
    cap = max(1, ntiles // 16)
    assert -(-16 // qblocks) >= cap, "the split count would depend on the device's CU count"
    tps = -(-ntiles // cap)
    return -(-ntiles // tps), tps


def random_table(seed, rows, p):
    rng = np.random.default_rng(seed)
    ev = rng.normal(size=(rows, p)) @ (np.tril(rng.uniform(-0.4, 0.4, size=(p, p)), -1) + np.eye(p)).T
    y = 0.5 * ev.sum(axis=1) + rng.normal(scale=0.7, size=rows) + np.sin(ev[:, 0])
    return np.column_stack([y, ev])


def normal_reference(data, N):
    d = data.shape[1]
    return np.atleast_2d(np.cov(data.T)) * (4.0 / (d + 2)) ** (2.0 / (d + 4)) * N ** (-2.0 / (d + 4))


def check_cdf(oracle, dtype, train, H, test, got, lw=None):
    """device against the truth, the oracle against the truth where its exp form is valid; returns the worst device error"""
    lw = log_weights(train, H, test[:, 1:]) if lw is None else lw
    want = true_cdf(train, H, test, lw)
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all((got >= 0) & (got <= 1))
    assert np.allclose(got, want, **TOL[dtype]), (np.abs(got - want).max(), np.argmax(np.abs(got - want)))
    valid = lw.max(axis=0) + cond(H)[3] > ORACLE_FLOOR[dtype]
    if valid.any():
        np_t = np.dtype(dtype).type
        ref = oracle.ckde_cdf(train.astype(np_t), H, test[valid].astype(np_t))
        assert np.allclose(ref, want[valid], **TOL[dtype]), "the oracle's own arithmetic misses the tolerance on this input"
        if dtype == "float64":
            assert np.allclose(got[valid], ref, **TOL[dtype])
    return np.abs(got - want).max()


# ---- cdf: query and training counts ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_query_counts(pbn, oracle, dtype, p):
    """One table of 600 rows (38 tiles: two splits of 19 on any device) against 1 ... 257 queries: a lone tile whose wave clamps its
    second tile (n <= 16, and every odd tile count), waves that leave after the table barrier (n <= 112: fewer than 8 tiles in the
    last block), exactly one, two and three blocks (128, 129 ... 257).  The first n queries of the largest run are the same MFMA
    columns whatever else is in the launch: every shorter run must equal its prefix bit for bit."""
    N = 600
    data = random_table(100 + p, N + 257, p)
    data[N:N + 3, 0] += 25.0         # cdf -> 1
    data[N + 3:N + 6, 0] -= 25.0     # cdf -> 0
    data = rounded(data, dtype)
    train, test = data[:N], data[N:]
    H = normal_reference(data, N)
    cpd = fitted(pbn, train, H, dtype)
    lw = log_weights(train, H, test[:, 1:])
    full = cpd.cdf(frame(test, dtype))
    check_cdf(oracle, dtype, train, H, test, full, lw)
    assert np.all(full[:3] > 1 - 1e-6) and np.all(full[3:6] < 1e-6)
    for n in QUERY_COUNTS:
        assert cdf_splits(N, n) == (2, 19)
        got = cpd.cdf(frame(test[:n], dtype))
        assert got.shape == (n,)
        assert np.array_equal(got, full[:n]), (n, np.flatnonzero(got != full[:n])[:5])


@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_training_counts(pbn, oracle, dtype, p):
    """1 ... 1 237 training rows against 33 queries (three tiles: the second wave clamps): below one tile, the padded last tile with
    1, 15 and 16 valid rows (PBN_PAD_NORM rows must weigh nothing), one split up to 496 rows, two from 512 (513: the second split's
    last tile holds one row), four at 1 237."""
    n = 33
    data = rounded(random_table(200 + p, 1237 + n, p), dtype)
    test = data[1237:]
    H = normal_reference(data, 1237)
    want_splits = {496: 1, 512: 2, 513: 2, 1237: 4}
    for N in TRAIN_COUNTS:
        nsplit, _ = cdf_splits(N, n)
        assert nsplit == want_splits.get(N, 1)
        train = data[:N]
        cpd = fitted(pbn, train, H, dtype)
        check_cdf(oracle, dtype, train, H, test, cpd.cdf(frame(test, dtype)))


def test_cdf_pinned_through_kde_joint(pbn):
    """The reference's way of pinning - assigning kde_joint().bandwidth on a fitted factor - gives the same handle as the selector."""
    data = random_table(7, 400, 4)
    H = normal_reference(data, 300) * 0.7
    for dtype in DTYPES:
        cpd = pbn.CKDE("y", names(4)[1:])
        cpd.fit(frame(data[:300], dtype))
        assert not np.array_equal(cpd.bandwidth, H)
        cpd.kde_joint().bandwidth = H
        assert np.array_equal(cpd.bandwidth, H)
        test = frame(data[300:], dtype)
        assert np.array_equal(cpd.cdf(test), fitted(pbn, data[:300], H, dtype).cdf(test))


@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_nan_query_row(pbn, dtype, p):
    """A NaN row among finite ones: NaN there, every other row bit for bit what a run without the NaN gives (the null row never
    reaches the device, so the rows behind it move one MFMA column down: columns are independent)."""
    N, n = 513, 50
    data = rounded(random_table(300 + p, N + n, p), dtype)
    H = normal_reference(data, N)
    cpd = fitted(pbn, data[:N], H, dtype)
    clean = cpd.cdf(frame(data[N:], dtype))
    for row, col in ((0, 0), (16, 1), (49, p)):
        holed = data[N:].copy()
        holed[row, col] = np.nan
        got = cpd.cdf(frame(holed, dtype))
        keep = np.arange(n) != row
        assert np.isnan(got[row]) and np.array_equal(got[keep], clean[keep])


# ---- cdf: the online rescale and the merge of splits -----------------------------------------------------------------
LEVELS = {"float64": [4400.0, 3300.0, 2200.0, 1100.0, 0.0], "float32": [600.0, 450.0, 300.0, 150.0, 0.0]}   # log2 units below the nearest rows


def staircase(dtype, p, tile_levels, n, seed):
    """Training rows in tiles at the given levels: level k sits LEVELS[k] log2 units of weight below level 4 (the rows around the
    queries), along the first whitened axis.  Returns (train, test, H); rows are whitened coordinates mapped through a full L."""
    rng = np.random.default_rng(seed)
    A = np.tril(rng.uniform(-0.3, 0.3, size=(p, p)), -1) + np.diag(rng.uniform(0.8, 1.2, size=p))
    Hee = 0.04 * A @ A.T
    L = np.linalg.cholesky(Hee)
    c = Hee @ rng.uniform(0.1, 0.4, size=p) / np.sqrt(p)             # b = H22^-1 c, |b| ~ 0.25
    H = np.empty((p + 1, p + 1))
    H[1:, 1:], H[0, 1:], H[1:, 0] = Hee, c, c
    H[0, 0] = 0.09 + c @ np.linalg.solve(Hee, c)                      # sigma_c = 0.3
    lev = np.repeat(np.asarray(tile_levels), 16)
    radius = np.sqrt(2.0 * np.asarray(LEVELS[dtype])[lev] / LOG2E)
    near = lev == 4
    z = rng.uniform(-1.0, 1.0, size=(lev.size, p)) * np.where(near, 1.5, 0.1)[:, None]
    z[:, 0] += radius
    zq = rng.uniform(-1.0, 1.0, size=(n, p))
    e, eq = z @ L.T, zq @ L.T
    y = 0.4 * z.sum(axis=1) + rng.normal(scale=0.5, size=lev.size)
    yq = 0.4 * zq.sum(axis=1) + rng.normal(scale=0.6, size=n)
    return rounded(np.column_stack([y, e]), dtype), rounded(np.column_stack([yq, eq]), dtype), H


def tile_maxima(lw, rows_per_split):
    """[split][tile, query]: the largest exponent (log2 units) of every training tile, split by split"""
    N = lw.shape[0]
    out = []
    for r0 in range(0, N, rows_per_split):
        blk = lw[r0:min(N, r0 + rows_per_split)] * LOG2E
        out.append(np.stack([blk[t:t + 16].max(axis=0) for t in range(0, blk.shape[0], 16)]))
    return out


def certain_rises(T, dtype):
    """per query: tiles whose maximum exceeds everything before them in the split by more than the rescale threshold.  The kernel's
    offset never exceeds the running maximum, so each of them enters the branch with mx > 0."""
    run = np.maximum.accumulate(T, axis=0)
    return (T[1:] - run[:-1] > RESCALE_HI[dtype]).sum(axis=0)


def never_rises(T, dtype):
    """the offset starts at the first tile's maximum and only grows: no later tile comes near the threshold above it"""
    return bool(np.all(T[1:] - T[0] < RESCALE_LO[dtype]))


UP = [0] * 6 + [1] * 6 + [2] * 6 + [3] * 6 + [4] * 6          # 30 tiles = 480 rows: one split on any device
FOUR = ([0] * 16,                                              # 64 tiles = 1 024 rows, few queries: four splits of 16 tiles
        [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4,
        [4] * 4 + [3] * 4 + [1] * 4 + [0] * 4,
        [0] * 4 + [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3)


@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_rescale_single_split(pbn, oracle, dtype, p):
    """480 rows, farthest first, in five steps of 1 100 (fp64) / 150 (fp32) log2 units: the running offset rises four times by more
    than big() within the one split.  The sums collected before a rise must be scaled down by 2^-mx and the offset moved: either one
    missing leaves the far rows' mass on top of the near ones'."""
    train, test, H = staircase(dtype, p, UP, 40, 500 + p)
    assert cdf_splits(480, 40) == (1, 30)
    assert fragment_type(dtype, train, H) == dtype          # rises of 150 log2 units only enter the float kernel's branch
    lw = log_weights(train, H, test[:, 1:])
    (T,) = tile_maxima(lw, 480)
    assert certain_rises(T, dtype).min() >= 3
    cpd = fitted(pbn, train, H, dtype)
    check_cdf(oracle, dtype, train, H, test, cpd.cdf(frame(test, dtype)), lw)


@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_rescale_mirror(pbn, oracle, dtype, p):
    """The same rows, nearest first: the first tile's offset is already the largest and the branch must never fire; the far rows'
    weights underflow to zero against it."""
    train, test, H = staircase(dtype, p, UP[::-1], 40, 500 + p)
    assert fragment_type(dtype, train, H) == dtype          # rises of 150 log2 units only enter the float kernel's branch
    lw = log_weights(train, H, test[:, 1:])
    (T,) = tile_maxima(lw, 480)
    assert never_rises(T, dtype) and certain_rises(T, dtype).max() == 0
    cpd = fitted(pbn, train, H, dtype)
    check_cdf(oracle, dtype, train, H, test, cpd.cdf(frame(test, dtype)), lw)


@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_rescale_four_splits(pbn, oracle, dtype, p):
    """1 024 rows in four splits of 16 tiles: the first is flat at the farthest level (its whole mass underflows against the winner
    in kde_cdf_finish_kernel's 2^(m - M)), the second climbs three steps but stays 1 100 / 150 log2 units below the winner, the third
    starts at the nearest rows and never rescales, the fourth climbs all four steps.  Offsets of the four splits differ by hundreds
    to thousands of log2 units."""
    train, test, H = staircase(dtype, p, sum(FOUR, []), 40, 600 + p)
    assert cdf_splits(1024, 40) == (4, 16)
    assert fragment_type(dtype, train, H) == dtype          # rises of 150 log2 units only enter the float kernel's branch
    lw = log_weights(train, H, test[:, 1:])
    T = tile_maxima(lw, 256)
    assert never_rises(T[0], dtype) and never_rises(T[2], dtype)
    assert certain_rises(T[1], dtype).min() >= 3 and certain_rises(T[3], dtype).min() >= 4
    tops = np.stack([t.max(axis=0) for t in T])
    assert np.all(tops[2] - tops[0] > 4 * RESCALE_HI[dtype]) and np.all(np.abs(tops[2] - tops[1]) > RESCALE_HI[dtype])
    cpd = fitted(pbn, train, H, dtype)
    check_cdf(oracle, dtype, train, H, test, cpd.cdf(frame(test, dtype)), lw)


@pytest.mark.parametrize("N", [480, 1237])
@pytest.mark.parametrize("dtype,p", P_CDF)
def test_cdf_far_evidence(pbn, oracle, dtype, p, N):
    """Evidence far outside the cloud (one split and four): every weight underflows the exp form - 0/0 there, asserted on the oracle -
    while the offset form returns the cdf of the nearest kernels: finite and equal to the log-domain answer."""
    n = 24
    data = rounded(random_table(700 + p, N + n, p), dtype)
    train, test = data[:N], data[N:].copy()
    H = normal_reference(data, N)
    test[:, 1] += 30.0 if dtype == "float64" else 12.0
    test = rounded(test, dtype)
    assert fragment_type(dtype, train, H) == dtype
    lw = log_weights(train, H, test[:, 1:])
    # the variable around the conditional mean of each query's nearest kernel, so that the answers spread over (0, 1)
    _, b, sc, _ = cond(H)
    best = lw.argmax(axis=0)
    test[:, 0] = train[best, 0] + ((test[:, 1:] - train[best, 1:]) * b).sum(axis=1) + sc * np.linspace(-1.5, 1.5, n)
    test = rounded(test, dtype)
    assert cdf_splits(N, n)[0] == (1 if N == 480 else 4)
    assert np.all(lw.max(axis=0) + cond(H)[3] < (-760.0 if dtype == "float64" else -110.0))
    np_t = np.dtype(dtype).type
    with np.errstate(all="ignore"):
        assert not np.any(np.isfinite(oracle.ckde_cdf(train.astype(np_t), H, test.astype(np_t))))
    cpd = fitted(pbn, train, H, dtype)
    got = cpd.cdf(frame(test, dtype))
    want = true_cdf(train, H, test, lw)
    assert np.all(np.isfinite(got))
    assert np.allclose(got, want, **TOL[dtype]), np.abs(got - want).max()
    assert want.min() < 0.3 and want.max() > 0.7            # the answers are not all 0 or 1


@pytest.mark.parametrize("scale", [5e-4, 3e-5])
@pytest.mark.parametrize("p", [1, 4])
def test_cdf_small_bandwidth_f32(pbn, oracle, p, scale):
    """fp32, 480 rows, a user-set bandwidth of 5e-4 and 3e-5 times the normal reference rule, queries inside the cloud: the
    whitened evidence reaches |z|^2 of 10^5 ... 10^6 from the centre, past the point where KDE.logl gives up on fp32 fragments
    (2^-24 max|z|^2 > 5e-4).  The reference's differences-first float arithmetic keeps 5e-4 here (check_cdf asserts it on the oracle)."""
    N, n = 480, 64
    rng = np.random.default_rng(1000 + p)
    data = random_table(1000 + p, N, p)
    H = scale * normal_reference(data, N)
    L = cond(H)[0]
    test = data[rng.choice(N, n, replace=False)].copy()
    test[:, 1:] += rng.uniform(-0.7, 0.7, size=(n, p)) @ L.T
    test[:, 0] += rng.normal(scale=cond(H)[2], size=n)
    train, test = rounded(data, "float32"), rounded(test, "float32")
    z = solve_triangular(L, (train[:, 1:] - train[:, 1:].mean(axis=0)).T, lower=True)
    znorm2 = (z * z).sum(axis=0).max()
    assert 2.0 ** -24 * znorm2 > 5e-4
    lw = log_weights(train, H, test[:, 1:])
    assert np.all(lw.max(axis=0) + cond(H)[3] > ORACLE_FLOOR["float32"])
    want = true_cdf(train, H, test, lw)
    assert want.min() < 0.2 and want.max() > 0.8
    cpd = fitted(pbn, train, H, "float32")
    got = cpd.cdf(frame(test, "float32"))
    print(f"p={p} scale={scale} max|z|^2={znorm2:.3g} worst cdf error={np.abs(got - want).max():.3g}")
    check_cdf(oracle, "float32", train, H, test, got, lw)


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwidened_results_unchanged(pbn, recorded, dtype):
    """The widening of the cdf / sample fragments must leave every fp64 handle and every fp32 handle below the threshold alone:
    cdf at 1 237 x 77 rows and sample at 1 500 x 700 (the sizes of test_ckde_gpu.py / test_sampling_gpu.py), at the normal reference
    bandwidth, equal the values recorded before the change bit for bit."""
    for p in (3, 9):
        data = rounded(random_table(90 + p, 1237 + 77, p), dtype)
        cpd = fitted(pbn, data[:1237], normal_reference(random_table(90 + p, 1237 + 77, p), 1237), dtype)
        assert np.array_equal(cpd.cdf(frame(data[1237:], dtype)), recorded[f"cdf_{dtype}_{p}"])
    for p in (2, 5):
        data = rounded(random_table(30 + p, 1500 + 700, p), dtype)
        cpd = fitted(pbn, data[:1500], normal_reference(random_table(30 + p, 1500 + 700, p), 1500), dtype)
        got = cpd.sample(700, frame(data[1500:], dtype).iloc[:, 1:], 9).to_numpy().astype(np.float64)
        assert np.array_equal(got, recorded[f"sample_{dtype}_{p}"])


# ---- sample -----------------------------------------------------------------------------------------------------------
def sample_splits(N):
    return -(-(-(-N // 16)) // 64)


def widening_norm2(train, H):
    """max over the rows of log2(e) (x - mean)^T H^-1 (x - mean), all d columns: the |z|^2 that kde_wants_widening() looks at"""
    x = train - train.mean(axis=0)
    z = solve_triangular(np.linalg.cholesky(np.asarray(H, dtype=np.float64)), x.T, lower=True, check_finite=False)
    return LOG2E * (z * z).sum(axis=0).max()


def fragment_type(dtype, train, H):
    """The type of the cdf / sample fragments and kernels: the table's, except that an fp32 handle past the widening threshold
    (2^-24 |z|^2 > 5e-4 = 8 389 with four products per coordinate, 2^-22 |z|^2 > 1e-3 = 4 194 with three) runs the double kernels.
    A table between 4 000 and 9 000 would leave the kernel under test undecided and is refused."""
    if dtype == "float64":
        return "float64"
    norm2 = widening_norm2(train, H)
    assert norm2 < 4000.0 or norm2 > 9000.0, norm2
    return "float32" if norm2 < 4000.0 else "float64"


def std_uniforms(seed, n, dtype):
    """The first n draws of std::uniform_real_distribution<T>(0, 1) on std::mt19937{seed} as libstdc++ forms them: one 32-bit word
    per float (rounded, then divided by 2^32), two per double (low word first).  check_uniforms holds this against the oracle."""
    st = np.random.RandomState(seed).get_state()          # init_genrand(seed), the seeding of std::mt19937
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": st[1], "pos": st[2]}}
    if dtype == "float32":
        r = bg.random_raw(n).astype(np.float32) / np.float32(2.0 ** 32)
        return np.where(r >= 1, np.nextafter(np.float32(1), np.float32(0)), r).astype(np.float64)
    r = bg.random_raw(2 * n).astype(np.float64)
    return (r[0::2] + r[1::2] * 2.0 ** 32) / 2.0 ** 64


@functools.lru_cache(maxsize=None)
def check_uniforms(dtype, seed, n):
    """4 096 equally weighted rows: the oracle's pick is floor(u * 4096) - 1, up to one row of its float prefix sums"""
    from oracle import oracle

    np_t = np.dtype(dtype).type
    _, idx = oracle.ckde_sample(np.zeros((4096, 2), dtype=np_t), np.eye(2), np.zeros((n, 1), dtype=np_t), n, seed)
    pred = np.floor(std_uniforms(seed, n, dtype) * 4096).astype(int) - 1
    assert np.all((np.abs(pred - idx) <= 1) | (pred < 1)), "std_uniforms no longer restates the library's random stream"
    return True


def reference_picks(dtype, train, H, ev, rn):
    """CKDE::sample's instance selection in the log domain, fp64: prefix sums of exp(lw - max), j = the first row whose normalised
    prefix sum exceeds the draw, instance j - 1; for j < 2 the reference's rule on its un-normalised row 0 (c[0] <= u: instance 0, else
    the default N - 1).  Also returns, per query, whether the draw lies within 1e-9 of a prefix-sum boundary."""
    N = train.shape[0]
    lw = log_weights(train, H, ev)
    w = np.exp(lw - lw.max(axis=0))
    c = np.cumsum(w, axis=0) / w.sum(axis=0)
    j = np.minimum((c <= rn[None, :]).sum(axis=0), N - 1)
    with np.errstate(over="ignore"):
        c0 = np.dtype(dtype).type(1) * np.exp(lw[0] + cond(H)[3] - np.log(N)).astype(dtype)
    idx = np.where(j >= 2, j - 1, np.where(c0 <= rn, 0, N - 1))
    near = (np.abs(c - rn[None, :]).min(axis=0) < 1e-9) | ((j < 2) & (np.abs(c0 - rn) < 1e-9))
    return idx, near


def forced_table(dtype, p, N, designated, seed, wide):
    """N training rows whose evidence is a cloud except the designated rows, which sit alone on the first evidence axis.
    wide: cloud inside |e0| <= 3, rows at +-6, +-9, ..., H[1:, 1:] = 0.004 I - the nearest other row is 47 bandwidths away, 1 623 log2
    units of weight (enough for the double kernels' rescale); an fp32 table of this kind is far past the widening threshold.
    not wide (fp32 on float fragments): cloud inside |e0| <= 4, at most six rows at +-17, +-30, +-43, H[1:, 1:] = I - 13 bandwidths,
    122 log2 units, |z|^2 below 4 000."""
    rng = np.random.default_rng(seed)
    e = rng.normal(size=(N, p))
    clip, first, step, h = (3.0, 6.0, 3.0, 0.004) if wide else (4.0, 17.0, 13.0, 1.0)
    assert wide or len(designated) <= 6
    e[:, 0] = np.clip(e[:, 0], -clip, clip)
    for k, r in enumerate(designated):
        e[r] = 0.0
        e[r, 0] = (first + step * (k // 2)) * (1.0 if k % 2 == 0 else -1.0)
    y = rng.normal(size=N) + 3.0 * np.arange(N) / N               # neighbouring rows differ visibly in y
    H = np.zeros((p + 1, p + 1))
    H[1:, 1:] = h * np.eye(p)
    H[0, 1:] = H[1:, 0] = 0.25 * h / np.sqrt(p)
    H[0, 0] = 12.5 * h
    return rounded(np.column_stack([y, e]), dtype), H


def expected_samples(dtype, train, H, ev, idx, noise):
    """y_r + b.(e_q - e_r) + noise_i in the factor's type, term by term as CKDE::sample forms it"""
    np_t = np.dtype(dtype).type
    b = cond(H)[1].astype(np_t)
    tr, e = train.astype(np_t), ev.astype(np_t)
    cm = np.zeros(len(idx), dtype=np_t)
    for j in range(e.shape[1]):
        cm = cm + (e[:, j] - tr[idx, j + 1]) * b[j]
    return cm + (tr[idx, 0] + noise.astype(np_t))


def noise_stream(oracle, dtype, H, n, seed, stream_n=0):
    """The normal draws of CKDE::sample depend on (type, sigma_c, seed, n, stream_n) alone.  An all-zero table makes the oracle return
    them bare: every conditional mean is 0 whatever row is picked."""
    np_t = np.dtype(dtype).type
    d = H.shape[0]
    out, _ = oracle.ckde_sample(np.zeros((2, d), dtype=np_t), H, np.zeros((n, d - 1), dtype=np_t), n, seed, stream_n)
    return out


SAMPLE_TOL = {"float64": dict(rtol=1e-10, atol=1e-12), "float32": dict(rtol=1e-5, atol=1e-5)}


@pytest.mark.parametrize("N", SAMPLE_COUNTS)
@pytest.mark.parametrize("dtype,p", P_SAMPLE)
def test_sample_training_counts(pbn, oracle, dtype, p, N):
    """CKDE.sample at every edge of r1 = min(t1 * 16, N) and of the 64-tile splits: 1 024 (exactly one split), 1 025 (a second split of
    one tile with one valid row), 1 040 (a second split of one full tile), 2 049 (three).  n = 1, 17 and 700 queries, two seeds, and
    fewer samples than evidence rows.  The reference is the log-domain selection (reference_picks) with the library's own uniform
    draws (std_uniforms, held against the oracle) and normal draws (noise_stream); in fp64 the oracle's full restatement as well,
    at rtol 1e-10.  A sample is excluded from the exact comparison only if its draw lies within 1e-9 of a prefix-sum boundary of the
    fp64 reference: none in fp64, at most 1 % of a case in fp32; every other sample must be the reference's.  fp32 tables stay below
    the widening threshold (asserted): the float kernels run."""
    data = rounded(random_table(800 + p, 2049 + 700, p), dtype)
    train, ev = data[:N], data[2049:, 1:]
    H = normal_reference(random_table(800 + p, 2049 + 700, p)[:2049], 2049)
    assert sample_splits(N) == {1237: 2, 1024: 1, 1025: 2, 1040: 2, 2049: 3}.get(N, 1)
    assert fragment_type(dtype, train, H) == dtype
    lw = log_weights(train, H, ev)
    if dtype == "float64":
        assert np.all(lw.max(axis=0) + cond(H)[3] - np.log(N) > ORACLE_FLOOR[dtype])       # the oracle is valid on every query
    cpd = fitted(pbn, train, H, dtype)
    evq = frame(data[2049:], dtype).iloc[:, 1:]
    for n in (1, 17, 700):
        for seed in (0, 123):
            assert check_uniforms(dtype, seed, n)
            got = cpd.sample(n, evq.iloc[:n], seed).to_numpy()
            idx, near = reference_picks(dtype, train, H, ev[:n], std_uniforms(seed, n, dtype))
            want = expected_samples(dtype, train, H, ev[:n], idx, noise_stream(oracle, dtype, H, n, seed))
            differs = ~np.isclose(got, want, **SAMPLE_TOL[dtype])
            print(f"{dtype} p={p} N={N} n={n} seed={seed}: {differs.sum()} differ, {near.sum()} within 1e-9 of a boundary")
            assert not np.any(differs & ~near), (n, seed, np.flatnonzero(differs & ~near)[:5])
            excluded = (differs & near).sum()
            assert excluded <= (0 if dtype == "float64" else 0.01 * n), (n, seed, excluded)
            if dtype == "float64":
                ref, _ = oracle.ckde_sample(train, H, ev[:n], n, seed)
                assert (~np.isclose(got, ref, rtol=1e-10, atol=1e-12)).sum() == 0
    got = cpd.sample(10, evq, 5).to_numpy()                  # n < evidence rows: the first n are used
    idx, near = reference_picks(dtype, train, H, ev[:10], std_uniforms(5, 10, dtype))
    assert not near.any()
    assert np.allclose(got, expected_samples(dtype, train, H, ev[:10], idx, noise_stream(oracle, dtype, H, 10, 5)), **SAMPLE_TOL[dtype])


def check_isolated(lw, rows):
    """every query's designated row outweighs every other row by more than 2^80"""
    for q, r in enumerate(rows):
        others = np.delete(lw[:, q], r)
        assert (lw[r, q] - others.max()) * LOG2E > 80.0, (q, r)


# (type of the table, evidence variables, wide table): fp64, fp32 on float fragments, and one fp32 table past the widening threshold,
# whose handle takes fp64 fragments and the double kernels on the float columns
FORCED = [("float64", p, True) for p in (1, 5, 16, 17)] + [("float32", p, False) for p in (1, 5, 16)] + [("float32", 5, True)]
FORCED_ROWS = [(17, (0, 1, 2, 15, 16)), (33, (0, 1, 2, 15, 16)), (33, (32,)), (1025, (0, 1, 15, 1023, 1024)), (1040, (2, 16, 1023, 1024, 1039)),
               (2049, (0, 1, 2, 15, 16)), (2049, (1023, 1024, 2047, 2048))]


@pytest.mark.parametrize("N,designated", FORCED_ROWS)
@pytest.mark.parametrize("dtype,p,wide", FORCED)
def test_sample_forced_selection(pbn, oracle, dtype, p, wide, N, designated):
    """Every query's evidence sits on one designated training row and the bandwidth isolates it by more than 2^80, so pick_locate /
    pick_scan must find that row j whatever the uniform draw; the reference's bracket then returns instance j - 1 (c[r] <= u < c[r+1]
    with c the inclusive prefix sums), and for j < 2 - where row 0 of its prefix sums is left un-normalised - whatever the oracle
    returns.  Designated: rows 0, 1, 2, 15, 16 (tile edge), N - 1 (the last valid row of a padded tile, or of a full one at 1 040),
    1 023 / 1 024 (last row of one 64-tile split, first of the next), 2 047 - at most six per table, so that the fp32 tables stay
    below the widening threshold and pick_scan_kernel<float> / kde_cdf_kernel<float, KS, 2, 0> run (fragment_type asserts which
    kernels a table reaches; the rescale thresholds are those of that type)."""
    train, H = forced_table(dtype, p, N, designated, 900 + p, wide)
    ftype = fragment_type(dtype, train, H)
    assert ftype == ("float64" if wide else dtype)
    rows = np.repeat(designated, 3)
    n = rows.size
    ev = train[rows, 1:]
    lw = log_weights(train, H, ev)
    check_isolated(lw, rows)
    # designated rows beyond the first tile of their split enter the rescale of the weights-only kernel
    T = tile_maxima(lw, 1024)
    for q in [q for q, r in enumerate(rows) if r % 1024 >= 16]:
        assert certain_rises(T[rows[q] // 1024][:, [q]], ftype)[0] >= 1
    cpd = fitted(pbn, train, H, dtype)
    np_t = np.dtype(dtype).type
    for seed in (0, 123):
        got = cpd.sample(n, frame(np.column_stack([np.zeros(n), ev]), dtype).iloc[:, 1:], seed).to_numpy()
        ref, ref_idx = oracle.ckde_sample(train.astype(np_t), H, ev.astype(np_t), n, seed)
        idx = np.where(rows >= 2, rows - 1, ref_idx)
        assert np.array_equal(ref_idx[rows >= 2], rows[rows >= 2] - 1)            # the oracle agrees with the bracket rule
        want = expected_samples(dtype, train, H, ev, idx, noise_stream(oracle, dtype, H, n, seed))
        assert np.allclose(ref, want, **SAMPLE_TOL[dtype])                        # ... and with the expected values
        assert np.allclose(got, want, **SAMPLE_TOL[dtype]), (seed, np.flatnonzero(~np.isclose(got, want, **SAMPLE_TOL[dtype])))
        # a pick one row early or late would show: the y of the rows on both sides differ by far more than the tolerance
        assert np.all(np.abs(train[idx, 0] - train[np.maximum(idx - 1, 0), 0])[idx > 0] > 1e-3)
        assert np.all(np.abs(train[idx, 0] - train[np.minimum(idx + 1, N - 1), 0])[idx < N - 1] > 1e-3)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("dtype,p,wide", FORCED)
def test_sample_forced_selection_far_evidence(pbn, oracle, dtype, p, wide, where):
    """The queries lie 63 (wide tables) / 16 (fp32 on float fragments) bandwidths outside the one designated row: every weight
    underflows the exp form (asserted: the oracle falls back to instance N - 1), but that row is still more than 2^80 closer than any
    other and the device must find it - in the first, the second and the last (one-row) of three splits, whose offsets differ by
    hundreds to thousands of log2 units in pick_locate_kernel."""
    N = 2049
    j = {"first": 5, "middle": 1500, "last": 2048}[where]
    train, H = forced_table(dtype, p, N, [j], 950 + p, wide)
    assert fragment_type(dtype, train, H) == ("float64" if wide else dtype)
    n = 300
    rows = np.full(n, j)
    ev = np.repeat(train[[j], 1:], n, axis=0)
    ev[:, 0] += 4.0 if wide else 16.0
    ev = rounded(ev, dtype)
    lw = log_weights(train, H, ev)
    check_isolated(lw, rows)
    assert sample_splits(N) == 3
    assert np.all(lw.max(axis=0) + cond(H)[3] < (-760.0 if dtype == "float64" else -110.0))
    np_t = np.dtype(dtype).type
    cpd = fitted(pbn, train, H, dtype)
    evq = frame(np.column_stack([np.zeros(n), ev]), dtype).iloc[:, 1:]
    for seed in (0, 123):
        with np.errstate(all="ignore"):
            assert np.all(oracle.ckde_sample(train.astype(np_t), H, ev.astype(np_t), n, seed)[1] == N - 1)
        got = cpd.sample(n, evq, seed).to_numpy()
        want = expected_samples(dtype, train, H, ev, rows - 1, noise_stream(oracle, dtype, H, n, seed))
        assert np.allclose(got, want, **SAMPLE_TOL[dtype]), (seed, got[:4], want[:4])
    # stream_n: the uniform draws skipped before the normals move the noise, not the pick
    got = cpd.sample(n, evq, 7, _stream_n=50).to_numpy()
    assert np.allclose(got, expected_samples(dtype, train, H, ev, rows - 1, noise_stream(oracle, dtype, H, n, 7, 50)), **SAMPLE_TOL[dtype])


@pytest.mark.parametrize("N", [33, 1025, 2049])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_overflowing_evidence_returns_a_training_row(pbn, oracle, dtype, N):
    """Evidence so far out that |z|^2 overflows the fragments' type: every weight is 2^-inf, offsets and prefix sums are NaN, no row of
    the last split is ever 'the first whose prefix sum exceeds the target', and pick_scan_kernel falls back to the split's last row.
    That must be the last VALID row, r1 = min(t1 * 16, N) - the last tile here holds one valid row and fifteen padding rows - so the
    instance returned is N - 2 (the bracket below the last row) or N - 1 (the reference's default), never a padding row.  b = 0, so
    the sample is y_r + noise and names its row.  The table stays below the widening threshold (asserted), so that the fp32 fragments
    are floats and 1e30 overflows them.  The finite queries sharing the tile are not disturbed."""
    assert N % 16 == 1 and sample_splits(N) == {33: 1, 1025: 2, 2049: 3}[N]
    train, H = forced_table(dtype, 1, N, [], 990, True)
    H[0, 1] = H[1, 0] = 0.0
    assert fragment_type(dtype, train, H) == dtype
    n = 10
    ev = train[7:7 + n, 1:].copy()
    ev[:5, 0] = 1e200 if dtype == "float64" else 1e30
    np_t = np.dtype(dtype).type
    with np.errstate(over="ignore"):
        assert np.isinf((np_t(ev[0, 0]) / np_t(np.sqrt(H[1, 1]))) ** 2)
    cpd = fitted(pbn, train, H, dtype)
    for seed in (0, 123):
        got = cpd.sample(n, frame(np.column_stack([np.zeros(n), ev]), dtype).iloc[:, 1:], seed).to_numpy()
        noise = noise_stream(oracle, dtype, H, n, seed)
        last = [expected_samples(dtype, train, H, ev, np.full(n, r), noise) for r in (N - 2, N - 1)]
        assert abs(train[N - 2, 0] - train[N - 1, 0]) > 1e-3
        for q in range(5):
            assert any(np.isclose(got[q], w[q], **SAMPLE_TOL[dtype]) for w in last), (q, got[q], last[0][q], last[1][q])
        assert np.all(np.isfinite(got[5:]))
        if dtype == "float64":
            # b = 0: every finite query's sample is some training row's y plus its own noise
            assert np.all(np.abs((got[5:] - noise[5:])[:, None] - train[None, :, 0]).min(axis=1) < 1e-9)
