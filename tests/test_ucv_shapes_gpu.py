"""GPU tier: the UCV pair sums (csrc/ucv.hip -> kde_cdf_kernel<T, KS, 2, 2>, ucv_block_sums_kernel, reduce_final_kernel) at every
launch shape, against the oracle's all-pairs restatement in fp64 and against closed forms.

UcvScorer::score sweeps the N rows against themselves with the offset pinned at 0: N query columns in tiles of 16 (a block serves
4 waves x 2 tiles), N training rows in min(ceil(16 CUs / qblocks), ntiles / 16) splits - one split up to 496 rows on any device, two
from 512 (`ucv_splits` asserts that one CU already gives the cap) -, then ucv_block_sums_kernel adds the splits per query and reduces
256 queries per block.  Hence the sizes around 16, 256 and 496 / 512.  Dimensions d = 1 ... 16 take KS = 1 ... 4 fragments per tile
in the table's type, d > 16 the runtime-sized fp64 kernel.

Tolerances are the project's (test_ucv_gpu.py): rel 1e-9 / abs 1e-14 in fp64, rel 2e-4 in fp32 against the fp64 oracle on the rounded
table."""
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

SIZES = [2, 3, 15, 16, 17, 255, 256, 257, 496, 512, 513]
DIMS = [1, 4, 5, 8, 9, 12, 13, 16]
SCALES = [0.3, 1.0, 3.0]
F64 = dict(rel=1e-9, abs=1e-14)
F32_REL = 2e-4


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as o

    return o


def cols(d):
    return [f"v{i}" for i in range(d)]


def frame(x, dtype="float64"):
    return pd.DataFrame(np.asarray(x), columns=cols(x.shape[1])).astype(dtype)


def table(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d)) @ (np.eye(d) + np.tril(rng.uniform(-0.5, 0.5, (d, d)), -1)).T
    x[:, 0] = np.where(rng.random(n) < 0.4, x[:, 0] + 3.0, x[:, 0])
    return x


def normal_reference(cov, n):
    """the normal reference rule's matrix for n rows of covariance `cov` (which need not come from those rows: the smallest tables
    have fewer rows than columns)"""
    d = cov.shape[0]
    return np.atleast_2d(cov) * (4.0 / (d + 2)) ** (2.0 / (d + 4)) * n ** (-2.0 / (d + 4))


def ucv_splits(N):
    ntiles = -(-N // 16)
    qblocks = -(-ntiles // 8)
    cap = max(1, ntiles // 16)
    assert -(-16 // qblocks) >= cap, "the split count would depend on the device's CU count"
    tps = -(-ntiles // cap)
    return -(-ntiles // tps)


def bandwidths(cov, n):
    H = normal_reference(cov, n)
    return [s * H for s in SCALES] + [s * np.diag(H) for s in SCALES]


@pytest.mark.parametrize("d", DIMS + [17, 20])
def test_ucv_sizes_and_dimensions(pbn, oracle, d):
    """Every size x full and diagonal bandwidths at 0.3, 1 and 3 times the normal reference rule; fp64 against the oracle, fp32
    (d <= 16: the fragments in the table's type) against the same fp64 value: the rows are float-representable, so both types see
    the same table.  (The oracle's own float arithmetic keeps rel 2e-4 on every one of these inputs; checked when they were chosen.)"""
    x_all = table(513, d, 20 + d).astype(np.float32).astype(np.float64)
    cov = np.cov(x_all.T).reshape(d, d)
    ucv = pbn.UCV()
    want_splits = {512: 2, 513: 2}
    for N in SIZES:
        assert ucv_splits(N) == want_splits.get(N, 1)
        x = x_all[:N]
        df, df32 = frame(x), frame(x, "float32")
        for bw in bandwidths(cov, N):
            want = oracle.ucv_score(x, bw)
            got = ucv.score(df, cols(d), bw)
            assert got == pytest.approx(want, **F64), (N, bw.ndim, got, want)
            if d <= 16:
                got32 = ucv.score(df32, cols(d), bw)
                assert got32 == pytest.approx(want, rel=F32_REL), (N, bw.ndim, got32, want)


def closed_form_identical(N, d, H):
    """N identical rows: every pair has K_H = (2 pi)^(-d/2) |H|^(-1/2) =: k and K_2H = 2^(-d/2) k, so
    N UCV = K_2H + (2 / N) C(N, 2) K_2H - (4 / (N - 1)) C(N, 2) k = N K_2H - 2 N k"""
    k = (2 * np.pi) ** (-0.5 * d) / np.sqrt(np.linalg.det(H))
    return N * k * 2.0 ** (-0.5 * d) - 2.0 * N * k


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d", [1, 5, 16, 17])
def test_ucv_identical_rows(pbn, dtype, d):
    """All pair weights are exactly 1 (the centred rows are exactly 0), so the score follows from N, d and |H| alone - any query or
    training row counted twice or not at all, any padding row that weighs, any split added twice shows as a wrong integer."""
    rng = np.random.default_rng(d)
    row = rng.normal(size=d).astype(np.float32).astype(np.float64)
    A = np.tril(rng.uniform(-0.3, 0.3, size=(d, d)), -1) + np.eye(d)
    H = 0.5 * A @ A.T
    ucv = pbn.UCV()
    for N in SIZES:
        got = ucv.score(frame(np.tile(row, (N, 1)), dtype), cols(d), H)
        assert got == pytest.approx(closed_form_identical(N, d, H), rel=1e-12), (N, got)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("d,n", [(1, 16), (4, 100), (9, 171), (17, 40)])
def test_ucv_separated_clusters(pbn, dtype, d, n):
    """Copies of one cluster of n rows, 60 (fp64) / 24 (fp32) bandwidths apart along the last axis: every cross weight is exactly 0
    (below 2^-2000 / 2^-200, past the smallest subnormal), so the pair sums of k copies are k times the cluster's own, S_H and S_2H.
    With N UCV(k copies) = K_2H(0) + 2 S_2H / n - 4 k S_H / (k n - 1), the scores of one, two and three copies determine S_H twice:
        S_H = (s_1 - s_k) / (4 k / (k n - 1) - 4 / (n - 1)),  k = 2, 3
    Both values must agree with each other and with the direct sum of the cluster's pairs.  Rows and shift are multiples of 1/64, so
    the copies are exact translates in fp32 too.  The division by a coefficient of order 1 / n^2 costs accuracy: the slack below is
    about 12 n rel of S_H - 2e-6 at n = 171 in fp64, but 24 to 40 % at n = 100 and 171 in fp32, where this identity only catches
    gross errors (a split or a copy dropped); the fp32 leg therefore also holds each score to rel 2e-4 of the fp64 run on the same
    float-representable rows."""
    rng = np.random.default_rng(40 + d)
    x = np.round(np.clip(rng.normal(size=(n, d)), -3.5, 3.5) * 64.0) / 64.0
    H = normal_reference(np.eye(d), n) * (1.0 + d / 4.0)        # wider with d, so that the cluster's own pairs still overlap
    sep = 60.0 if dtype == "float64" else 24.0
    step = np.zeros(d)
    step[d - 1] = np.ceil((7.0 + sep * np.sqrt(H[d - 1, d - 1])) * 64.0) / 64.0       # 7: the cluster's extent along the axis
    two, three = np.vstack([x, x + step]), np.vstack([x, x + step, x + 2 * step])
    assert np.array_equal(three.astype(np.float32).astype(np.float64), three)
    # the closest cross pair, in log2 units of weight: H is a multiple of the identity
    gap = (step[d - 1] - 7.0) ** 2 / H[d - 1, d - 1] * 0.5 * 1.4426950408889634
    assert gap > (1100.0 if dtype == "float64" else 160.0)
    ucv = pbn.UCV()
    s1, s2, s3 = (ucv.score(frame(t, dtype), cols(d), H) for t in (x, two, three))
    if dtype == "float32":
        for got, t in ((s1, x), (s2, two), (s3, three)):
            assert got == pytest.approx(ucv.score(frame(t), cols(d), H), rel=F32_REL)
    L = np.linalg.cholesky(H)
    z = np.linalg.solve(L, x.T).T
    d2 = ((z[:, None, :] - z[None, :, :]) ** 2).sum(axis=2)[np.triu_indices(n, 1)]
    S_H = np.exp(-0.5 * d2).sum() * (2 * np.pi) ** (-0.5 * d) / np.sqrt(np.linalg.det(H))
    est2 = (s1 - s2) / (8.0 / (2 * n - 1) - 4.0 / (n - 1))
    est3 = (s1 - s3) / (12.0 / (3 * n - 1) - 4.0 / (n - 1))
    # each score carries rel 1e-9 (fp64) / 2e-4 (fp32); the coefficients are 4 (k - 1) / ((k n - 1)(n - 1)) >= 2 / n^2 in size, so a
    # difference of two scores divided by one is off by at most rel (|s_1| + |s_k|) n^2 / 2
    rel = 1e-9 if dtype == "float64" else F32_REL
    slack = rel * (abs(s1) + abs(s2) + abs(s3)) * n * n
    assert abs(est2 - est3) <= slack and abs(est2 - S_H) <= slack, (est2, est3, S_H, slack)


@pytest.mark.parametrize("d", [1, 4, 9, 16])
def test_ucv_common_offset(pbn, oracle, d):
    """10^6 on every column: the centring at the pilot means must take it out before the Gram form squares it.  fp32: the rows are
    rounded first (a grid of 1/16 at 10^6), truth is the fp64 oracle on the rounded rows."""
    N = 300
    x = table(N, d, 60 + d) + 1e6
    H = normal_reference(np.cov(x.T).reshape(d, d), N)
    ucv = pbn.UCV()
    for bw in (H, np.diag(H)):
        assert ucv.score(frame(x), cols(d), bw) == pytest.approx(oracle.ucv_score(x, bw), **F64)
    x32 = x.astype(np.float32)
    H32 = normal_reference(np.cov(x32.astype(np.float64).T).reshape(d, d), N)
    for bw in (H32, np.diag(H32)):
        want = oracle.ucv_score(x32.astype(np.float64), bw)
        assert ucv.score(frame(x32, "float32"), cols(d), bw) == pytest.approx(want, rel=F32_REL)


@pytest.mark.parametrize("scale", [0.01, 0.003])
@pytest.mark.parametrize("d", [1, 2, 4])
def test_ucv_small_bandwidth_f32(pbn, oracle, d, scale):
    """480 fp32 rows - five of them a tight group 30 standard deviations out - at 0.01 and 0.003 times the normal reference bandwidth,
    points a Nelder-Mead search visits.  The whitened rows reach |z|^2 of 10^4 ... 10^5 from the centre, past the point where KDE.logl
    gives up on fp32 fragments (2^-24 max|z|^2 > 5e-4).  The oracle's float arithmetic (differences first) passes rel 2e-4 here,
    asserted below, so the device must."""
    N = 480
    x = table(N, d, 80 + d)
    x[:5] = x[5] + 0.01 * x[:5]
    x[:5, 0] += 30.0
    x32 = x.astype(np.float32)
    x = x32.astype(np.float64)
    H = scale * normal_reference(np.cov(x.T).reshape(d, d), N)
    z = np.linalg.solve(np.linalg.cholesky(H), (x - x.mean(axis=0)).T)
    assert 2.0 ** -24 * (z * z).sum(axis=0).max() > 5e-4
    ucv = pbn.UCV()
    for bw in (H, np.diag(H)):
        want = oracle.ucv_score(x, bw)
        assert oracle.ucv_score(x32, bw) == pytest.approx(want, rel=F32_REL)
        got = ucv.score(frame(x32, "float32"), cols(d), bw)
        print(f"d={d} scale={scale} kind={bw.ndim} max|z|^2={(z * z).sum(axis=0).max():.3g} rel err={abs(got - want) / abs(want):.3g}")
        assert got == pytest.approx(want, rel=F32_REL), (got, want)


def test_ucv_f64_results_unchanged(pbn):
    """fp64 scores at four sizes of test_ucv_gpu.py equal the values recorded before fp32 tables got the widening rule and the exact
    self pairs, bit for bit (tests/golden/gen_cdf_weights_recorded.py, run with the library built from commit 8bfb9b6)."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cdf_weights_recorded.npz")) as f:
        recorded = {k: f[k] for k in f.files}
    ucv = pbn.UCV()
    for n, d in ((257, 1), (700, 2), (611, 16), (903, 17)):
        x = table(n, d, 3 + d)
        H = normal_reference(np.cov(x.T).reshape(d, d), n)
        got = np.array([ucv.score(frame(x), cols(d), H), ucv.score(frame(x), cols(d), 0.3 * np.diag(H))])
        assert np.array_equal(got, recorded[f"ucv_{n}_{d}"])
