"""CPU tier: the weighted chi-square sums behind RCoT's p-values (pbn_rcot_chisq_sum_sf, host only) against the numpy
restatement, the exact equal-weight case and an Imhof numerical inversion."""
import ctypes as C

import numpy as np
import pytest
from scipy import integrate, stats

from rcot_restatement import chisq_sum_sf, hbe_sf, lpb4_sf

WEIGHTS = [
    [0.5, 0.3, 0.2, 0.1, 0.05],
    [1.0, 1.0, 1.0, 1.0],
    [3.0, 0.01, 0.01, 0.01, 0.01, 0.01],
    list(np.linspace(0.02, 0.4, 25)),
    list(np.random.default_rng(3).exponential(0.1, 25)),
    [0.7, 0.2],
    [0.9],
]


def _lib():
    from pybnesian_amd import _lib

    return _lib


def native(w, q, method):
    L = _lib()
    w = np.ascontiguousarray(w, dtype=np.float64)
    out = C.c_double(0)
    rc = L.load().pbn_rcot_chisq_sum_sf(L.dptr(w), len(w), C.c_double(q), int(method), C.byref(out))
    return rc, out.value


def imhof_sf(w, q):
    w = np.asarray(w, dtype=np.float64)

    def integrand(u):
        theta = 0.5 * np.sum(np.arctan(w * u)) - 0.5 * q * u
        rho = np.prod((1 + (w * u) ** 2) ** 0.25)
        return np.sin(theta) / (u * rho)

    val, _ = integrate.quad(integrand, 0, np.inf, limit=2000, epsabs=1e-12)
    return 0.5 + val / np.pi


@pytest.mark.parametrize("wi", range(len(WEIGHTS)))
@pytest.mark.parametrize("qf", [0.3, 1.0, 2.5])
def test_auto_rule_matches_restatement(ensure_built, wi, qf):
    w = WEIGHTS[wi]
    q = qf * sum(w)
    rc, got = native(w, q, 0)
    assert rc == 0
    want, _ = chisq_sum_sf(w, q, 0)
    assert abs(got - want) <= 1e-10, (w, q, got, want)


@pytest.mark.parametrize("wi", range(len(WEIGHTS)))
def test_hbe_matches_restatement(ensure_built, wi):
    w = WEIGHTS[wi]
    for q in (0.2 * sum(w), sum(w), 3 * sum(w)):
        rc, got = native(w, q, 1)
        assert rc == 0
        assert abs(got - hbe_sf(w, q)) <= 1e-10


def test_lpb4_failure_falls_back_to_hbe(ensure_built):
    # equal weights: the moments are those of a scaled chi-square, the LPB4 determinants vanish and the method breaks down
    w = [1.0, 1.0, 1.0, 1.0]
    q = 6.0
    with pytest.raises(ArithmeticError):
        lpb4_sf(w, q)
    rc, _ = native(w, q, 2)
    assert rc != 0
    rc, got = native(w, q, 0)
    assert rc == 0 and abs(got - hbe_sf(w, q)) <= 1e-12


def test_fewer_than_four_weights_use_hbe(ensure_built):
    for w in ([0.7, 0.2], [0.9], [0.5, 0.3, 0.1]):
        rc, got = native(w, 1.0, 0)
        assert rc == 0 and abs(got - hbe_sf(w, 1.0)) <= 1e-12
    rc, got = native([], 1.0, 0)   # no positive weight: p = 1
    assert rc == 0 and got == 1.0
    rc, got = native([-0.1, 0.0], 1.0, 0)
    assert rc == 0 and got == 1.0


@pytest.mark.parametrize("k", [1, 3, 7, 25])
@pytest.mark.parametrize("c", [0.05, 1.0, 4.0])
def test_hbe_exact_for_equal_weights(ensure_built, k, c):
    for q in (0.1 * c * k, c * k, 3 * c * k):
        rc, got = native([c] * k, q, 1)
        assert rc == 0
        assert abs(got - stats.chi2.sf(q / c, k)) <= 1e-12 * max(1.0, stats.chi2.sf(q / c, k)) + 1e-14


@pytest.mark.parametrize("wi", [0, 2, 3, 4])
def test_lpb4_against_imhof(ensure_built, wi):
    w = WEIGHTS[wi]
    for qf in (0.5, 1.0, 2.0, 3.0):
        q = qf * sum(w)
        exact = imhof_sf(w, q)
        if exact < 1e-4:
            continue
        rc, got = native(w, q, 2)
        assert rc == 0
        assert abs(got - exact) <= 5e-3, (w, q, got, exact)


def test_bad_method_is_rejected(ensure_built):
    rc, _ = native([1.0, 2.0], 1.0, 7)
    assert rc == _lib().PBN_ERR_INVALID
