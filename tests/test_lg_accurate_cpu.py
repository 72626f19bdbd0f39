"""CPU tier: the host solve of the double-double LinearGaussianCPD refit (csrc/lg_dd_solve.hpp: centring, pivoted Cholesky with its rank
decision, solves, RSS) against exact rational least squares (tests/lg_exact.py), without a GPU.

tests/c/lg_dd_check.cpp accumulates the raw moments row by row in double-double - the device kernel's arithmetic in another order - and
calls the header's solve; it is built once with hipcc (host code only) and run once on a file of all cases.

Full-rank cases must meet the bound 64 eps + 16 kappa^2 (1 + m^2) 2^-104 on beta (max-abs error relative to max |beta|) and on the
variance (relative); the fp64 normal equations miss it by six or more orders of magnitude on the same data.  With an EXACTLY dependent
parent (x_p = x_1 + x_2 or x_p = 2 x_1 on the integer grid) the solve must report rank p - 1 and give exactly one member of the dependent
set coefficient 0, whatever the columns' offset: before the rank decision looked at the centring noise it kept all p columns in one to
three of six seeds at every offset from 50 sigma on.  The tables keep their raw moments inside double-double (lg_exact.Table), so the
sums are exact in any order and the test measures the solve; one family fills all 52 bits instead, for the rank decision under the
accumulation's own roundoff."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lg_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL = [(d, kappa, offset) for d in (4, 8, 16) for kappa in (1e4, 1e7, 1e9) for offset in (5, 1000)]
DEPENDENT = [(kind, p, offset, seed) for kind in ("sum", "double") for p in (4, 9) for offset in (0, 50, 1000, 10000) for seed in range(6)]
FULL_WIDTH = [(kind, p, offset, seed) for kind in ("sum", "double") for p in (4, 9) for offset in (1000, 10000) for seed in range(6)]
N_FULL, N_DEP = 2000, 2000


def _tables():
    t = {}
    for d, kappa, offset in FULL:
        t["full", d, kappa, offset] = lg_exact.make_table(d * 100 + offset + int(np.log10(kappa)), N_FULL, d, kappa=kappa, offset=offset)
    t["near-exact"] = lg_exact.make_table(77, N_FULL, 8, offset=5, resp_noise=1e-5)
    for kind, p, offset, seed in DEPENDENT:
        t[kind, p, offset, seed] = lg_exact.make_table(1000 * seed + 10 * p + offset, N_DEP, p + 1, offset=offset, dependency=kind)
    for kind, p, offset, seed in FULL_WIDTH:
        t["wide", kind, p, offset, seed] = lg_exact.make_table(seed + p + offset, N_DEP, p + 1, offset=offset, dependency=kind, full_width=True)
    return t


@pytest.fixture(scope="module")
def solved(tmp_path_factory):
    """{case: (table, rank, variance, beta)} from ONE run of the host program over every case."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("lg_dd")
    exe = tmp / "lg_dd_check"
    subprocess.run([hipcc, "-O2", "-std=c++17", "--offload-arch=gfx950", "-o", str(exe), os.path.join(ROOT, "tests", "c", "lg_dd_check.cpp")],
                   check=True, capture_output=True, timeout=600)
    tables = _tables()
    with open(tmp / "cases.bin", "wb") as f:
        for t in tables.values():
            np.array(t.data.shape, dtype=np.int64).tofile(f)
            np.asfortranarray(t.data, dtype=np.float64).T.tofile(f)    # column-major
    out = subprocess.run([str(exe), str(tmp / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(tables)
    res = {}
    for (key, t), line in zip(tables.items(), lines):
        w = line.split()
        res[key] = (t, int(w[0]), float.fromhex(w[1]), np.array([float.fromhex(v) for v in w[2:]]))
    return res


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    for family, ratio in sorted(w.items()):
        print(f"\nlg_accurate cpu {family}: worst error / bound = {ratio:.3g}")


def test_exact_fit_against_float_least_squares():
    """The reference itself, where float64 lstsq is good: a well-conditioned table, all parents and a kept subset."""
    t = lg_exact.make_table(3, 300, 5, offset=2)
    x = t.data.astype(np.float64)
    for keep in (None, [1, 3]):
        cols = [1, 2, 3, 4] if keep is None else keep
        A = np.column_stack([np.ones(len(x)), x[:, cols]])
        sol, rss = np.linalg.lstsq(A, x[:, 0], rcond=None)[:2]
        beta, var = t.exact(keep=keep)
        assert np.allclose(beta[[0] + cols], sol, rtol=1e-11, atol=1e-12)
        assert all(beta[j] == 0.0 for j in range(1, 5) if j not in cols)
        assert np.isclose(var, rss[0] / (300 - 4 - 1), rtol=1e-11)
    assert t.exact(rows=np.arange(5))[1] == np.inf


@pytest.mark.parametrize("d,kappa,offset", FULL)
def test_full_rank_meets_the_double_double_bound(solved, worst, d, kappa, offset):
    lg_exact.check_full_rank(*solved["full", d, kappa, offset], worst, "full-rank")


def test_near_exact_fit(solved, worst):
    lg_exact.check_full_rank(*solved["near-exact"], worst, "near-exact")


@pytest.mark.parametrize("kind,p,offset,seed", DEPENDENT)
def test_exact_dependency_drops_one_column(solved, worst, kind, p, offset, seed):
    lg_exact.check_dependent(*solved[kind, p, offset, seed], worst, "dependent")


@pytest.mark.parametrize("kind,p,offset,seed", FULL_WIDTH)
def test_exact_dependency_with_rounded_raw_moments(solved, worst, kind, p, offset, seed):
    """Parents that fill all 52 bits: the raw moments no longer fit double-double and their accumulation rounds, which leaves noise of
    ~sqrt(n) 2^-106 (1 + m^2) of the centred entries that no exact centring can remove - the case the noise floor of the rank decision is
    for (without it: rank p in 8 of these 48)."""
    lg_exact.check_dependent(*solved["wide", kind, p, offset, seed], worst, "dependent, rounded moments", rounded_moments=True)
