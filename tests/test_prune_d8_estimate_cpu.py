"""tools/prune_d8_estimate.py (the d = 8 pruning estimator): its rotation and its kd order on a small table."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import prune_d8_estimate as E  # noqa: E402


def test_rotation_is_orthonormal_and_widest_first():
    rng = np.random.default_rng(0)
    z = E.bench_table(20_000, 0)
    R, spread = E.principal_rotation(z)
    assert np.allclose(R @ R.T, np.eye(E.D), atol=1e-12)
    assert np.all(np.diff(spread) <= 0)
    zr = z @ R.T
    # the same distances, decorrelated axes whose spreads are the principal ones
    a, b = rng.integers(0, len(z), 50), rng.integers(0, len(z), 50)
    assert np.allclose(((z[a] - z[b]) ** 2).sum(1), ((zr[a] - zr[b]) ** 2).sum(1), rtol=1e-12)
    c = np.cov(zr, rowvar=False)
    assert np.allclose(c - np.diag(np.diag(c)), 0.0, atol=1e-9 * c.max())
    assert np.allclose(np.sqrt(np.diag(c)), spread, rtol=1e-9)


def test_kd_order_tiles_and_descent():
    z = E.bench_table(16 * 300 + 5, 1)
    for axes in (None, 4):
        perm, axis, split, T = E.kd_order(z, axes)
        assert T == 301 and np.array_equal(np.sort(perm), np.arange(len(z)))
        if axes is not None:
            assert axis.max() < axes
        # every training row descends to its own tile (ties at a split value go right, as the partition puts them)
        leaf = E.kd_leaf(z[perm], axis, split, T)
        assert np.array_equal(leaf, np.arange(len(z)) // 16)
        # tighter 8-D tile boxes than an unsorted order
        lo, hi = E.tile_boxes(z[perm], E.D)
        lo0, hi0 = E.tile_boxes(z, E.D)
        assert np.median((hi - lo).sum(1)) < 0.8 * np.median((hi0 - lo0).sum(1))


def test_visited_fraction_bound_is_conservative():
    rng = np.random.default_rng(2)
    zt = rng.normal(size=(16 * 64, E.D)) * 3.0
    zq = zt[:16] + 0.01
    lo, hi = E.tile_boxes(zt, E.D)
    thr = np.array([E.log2_sums(zq, zt).min()])
    frac = E.visited_fraction(lo, hi, zq.min(0)[None], zq.max(0)[None], thr, 43.0)
    assert 0.0 < frac <= 1.0
    # a tile the bound skips holds no term within 2^-43 of the group's smallest sum
    g = np.maximum(np.maximum(lo - zq.max(0), zq.min(0) - hi), 0.0)
    skipped = np.nonzero(-0.5 * (g * g).sum(1) < thr[0] - 43.0)[0]
    for t in skipped:
        d2 = ((zq[:, None, :] - zt[16 * t:16 * t + 16][None]) ** 2).sum(2)
        assert (-0.5 * d2).max() < thr[0] - 43.0
