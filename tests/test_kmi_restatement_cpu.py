"""CPU tier: the brute-force restatement the KMI shape tests hold the device kernels to (tests/kmi_restatement.py) is itself held to
the CPU checker of KMutualInformation on tie-free tables - two independent statements of the estimator, one in numpy on integer ranks,
one following the reference's routines in C++ - and its neighbour reference to a second formulation."""
import numpy as np
import pytest

import kmi_restatement as kr


def tie_free(n, dims, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, dims))
    v[:, 1] += 0.8 * v[:, 0]
    for d in range(2, dims):
        v[:, d] += 0.5 * v[:, d - 2]
    return v


def ordinal_ranks(v):
    """Without ties the ordinal ranks do not depend on the sorting routine."""
    r = np.empty(v.shape, np.int64)
    for d in range(v.shape[1]):
        assert len(np.unique(v[:, d])) == len(v)
        r[np.argsort(v[:, d]), d] = np.arange(len(v))
    return r


@pytest.mark.parametrize("n,k", [(65, 1), (65, 64), (257, 3), (700, 64), (1201, 10)])
@pytest.mark.parametrize("dims", [2, 3, 4, 6, 7, 11, 16])
def test_restatement_equals_the_cpu_checker_on_tie_free_tables(ensure_built, n, k, dims):
    from oracle import oracle

    v = tie_free(n, dims, 100 * dims + k)
    want, _ = oracle.kmi(v, k)
    got = kr.mi(ordinal_ranks(v), k)
    print(f"n {n} k {k} dims {dims}: restatement - checker = {got - want:.3g}")
    assert got == pytest.approx(want, rel=0, abs=1e-12)


def test_eps_and_counts_on_a_table_small_enough_to_read():
    """Five rows, x = y = z = the row number: the k-th neighbour of an interior row is ceil(k / 2) ranks away."""
    R = np.repeat(np.arange(5)[:, None], 3, axis=1)
    eps, cnt = kr.eps_counts(R, [2])[2]
    assert eps.tolist() == [2, 1, 1, 1, 2]
    assert cnt.tolist() == [[2, 1, 1, 1, 2]] * 3                # strictly inside eps: the row itself, and at the ends its one neighbour
    some = kr.eps_counts(R, [1, 2], rows=[4, 0])
    assert some[2][0].tolist() == [2, 2] and some[1][0].tolist() == [1, 1] and some[1][1].tolist() == [[1, 1]] * 3
    eps2, none = kr.eps_counts(R[:, :2], [4])[4]
    assert none is None and eps2.tolist() == [4, 3, 2, 3, 4]
    psi = kr.digamma_table(4)
    assert psi[1] == -kr.EULER and psi[4] == pytest.approx(1 + 0.5 + 1 / 3 - kr.EULER, abs=1e-15)


@pytest.mark.parametrize("nz,m,n", [(1, 1, 255), (2, 5, 256), (7, 64, 257), (14, 64, 600)])
def test_neighbour_reference_equals_a_full_sort(nz, m, n):
    z = np.random.default_rng(nz).normal(size=(n, nz))
    z[::7] = np.round(z[::7])                                    # tied distances too
    full = np.sort(np.abs(z[:, None, :] - z[None, :, :]).max(axis=2), axis=1)[:, :m]
    assert np.array_equal(kr.neighbor_distances(z, m), full)
    rows = np.array([n - 1, 0, 17])
    assert np.array_equal(kr.neighbor_distances(z, m, rows), full[rows])
    assert np.array_equal(kr.chebyshev(z, rows[:, None], np.arange(n)[None, :]), np.abs(z[rows, None, :] - z[None, :, :]).max(axis=2))
    assert (full[:, 0] == 0).all()


def test_row_sample_holds_the_edges():
    R = ordinal_ranks(tie_free(5000, 3, 1))
    s = kr.row_sample(R, 2, 0)
    assert len(s) == len(set(s)) and set(range(64)) <= set(s) and set(range(5000 - 64, 5000)) <= set(s)
    assert set(R[s, 2]) >= {0, 1, 2, 3, 4996, 4997, 4998, 4999}
