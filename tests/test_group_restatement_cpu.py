"""The restatement of the grouped KDE evaluation's prepass (tests/group_restatement.py) against brute force, without a device: on synthetic
pools (clustered, duplicated rows, rows at +-40 sigma, test rows equal to training rows of other regions) and ARBITRARY valid sorted orders
- a pool sorted along a curve, a random permutation, the identity - the restated bounds are lower bounds of the true largest exponent and
of the true log2 sum of every query, the orders are the stable compaction of the pool's order, the batch boxes are the unions of their
tiles' boxes, the moment coefficients reproduce a tile's sum, and the merge of split partials reproduces the whole sum.  This is what
tests/test_group_stages_gpu.py asks of the kernels: that the definitions are sound for these inputs, and that a correct kernel can meet them."""
import numpy as np
import pytest

import group_restatement as gr


def pool(n, d, R, seed, even=True):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(5, d)) * 3.0
    x = centres[rng.integers(0, 5, n)] + rng.normal(size=(n, d)) * 0.4      # clustered
    x[10:40] = x[3]                                                          # duplicated rows (a tile of identical rows)
    x[50], x[51] = 40.0 * x.std(0), -40.0 * x.std(0)                         # far rows on both sides
    if even:
        rb = np.array([r * n // R for r in range(R + 1)])
    else:
        rb = np.sort(np.concatenate([[0, n], rng.choice(np.arange(1, n), R - 1, replace=False)]))
    x[rb[1]:rb[1] + 20] = x[rb[0]:rb[0] + 20]                                # test rows equal to training rows of another region
    return x, rb


def sorted_orders(x, seed):
    n = len(x)
    rng = np.random.default_rng(seed)
    return {"curve": np.lexsort((x[:, -1], np.floor(x[:, 0] * 4.0))), "random": rng.permutation(n), "identity": np.arange(n)}


def whitening(x, d, n):
    L = np.linalg.cholesky(np.cov(x.T).reshape(d, d) * n ** (-2.0 / (d + 4)) + 1e-12 * np.eye(d))
    W = np.linalg.inv(L) * np.sqrt(1.0 / np.log(2.0))     # base-2 units
    return np.tril(W).ravel(), x.mean(0)


CASES = [(1, 2, 1000, 8, 256), (2, 3, 1203, 8, 256), (3, 10, 1519, 8, 2), (4, 64, 2100, 8, 256), (2, 3, 700, 1, 0), (1, 10, 1601, 64, 1)]


@pytest.mark.parametrize("d,R,n,window,tile_window", CASES)
@pytest.mark.parametrize("order", ["curve", "random", "identity"])
def test_restated_bounds_are_lower_bounds(d, R, n, window, tile_window, order):
    x, rb = pool(n, d, R, 10 * d + R, even=(R != 10))
    vals = sorted_orders(x, 3)[order]
    W, mu = whitening(x, d, n)
    for test_region in sorted({0, 1, R - 1}):
        mask = ((1 << R) - 1) & ~(1 << test_region) if R > 2 else 1
        if R == 2 and test_region != 1:
            continue
        r = gr.restate(x, rb, R, vals, mask, test_region, W, mu, d, min(d, 4), window, tile_window, tps=80)
        # orders: the stable compaction of the pool's order; qpos counts the training rows before a query
        reg = gr.region_of(rb, R, vals)
        assert np.array_equal(r["reg"], reg) and np.array_equal(np.sort(vals), np.arange(n))
        keep = np.array([(mask >> int(g)) & 1 for g in reg], dtype=bool)
        assert np.array_equal(r["train"], vals[keep]) and np.array_equal(r["query"], vals[reg == test_region])
        pos = {int(v): i for i, v in enumerate(vals)}
        for j in (0, len(r["query"]) // 2, len(r["query"]) - 1):
            assert r["qpos"][j] == sum(1 for v in r["train"] if pos[int(v)] < pos[int(r["query"][j])])
        zs, zq = r["zs"], r["zq"]
        N, nq = len(zs), len(zq)
        assert N == sum(rb[g + 1] - rb[g] for g in range(R) if (mask >> g) & 1) and nq == rb[test_region + 1] - rb[test_region]
        # the two lower-bound properties
        tmax, tsum = gr.true_max_exponent(zs, zq), gr.true_log2_sums(zs, zq)
        qlb, qthr = r["qlb"], r["qthr"]
        assert np.all(np.isneginf(qlb[nq:])) and len(qlb) == (nq + 15) // 16 * 16
        assert np.all(qlb[:nq] <= tmax + gr.bound_slack(N, d, tmax)), np.max(qlb[:nq] - tmax)
        tile_min = np.array([tsum[t * 16:(t + 1) * 16].min() for t in range(len(qthr))])
        assert np.all(qthr <= tile_min + gr.bound_slack(N, d, tile_min)), np.max(qthr - tile_min)
        # boxes: a batch box is the union of its tiles' boxes, every row inside its tile's box
        kd = min(d, 4)
        box, bbox = r["box"], r["bbox"]
        nbps = (80 + 63) // 64
        for s in range((len(box) + 79) // 80):
            for k in range(nbps):
                a, b = s * 80 + 64 * k, min(s * 80 + 64 * k + 64, s * 80 + 80, len(box))
                if a < b:
                    assert np.array_equal(bbox[s * nbps + k, :kd], box[a:b, :kd].min(0)) and np.array_equal(bbox[s * nbps + k, kd:], box[a:b, kd:].max(0))
                else:
                    assert np.all(np.isposinf(bbox[s * nbps + k, :kd]))
        assert np.all(zs[:, :kd] >= np.repeat(box[:, :kd], 16, 0)[:N]) and np.all(zs[:, :kd] <= np.repeat(box[:, kd:], 16, 0)[:N])


def test_tile_window_raises_the_threshold():
    """The tile-window bound is worth having on clustered data in curve order: it lifts the median threshold by bits, and stays below the truth."""
    x, rb = pool(3000, 2, 3, 5)
    vals = sorted_orders(x, 1)["curve"]
    W, mu = whitening(x, 2, 3000)
    off = gr.restate(x, rb, 3, vals, 0b110, 0, W, mu, 2, 2, 8, 0, 4096)
    on = gr.restate(x, rb, 3, vals, 0b110, 0, W, mu, 2, 2, 8, 256, 4096)
    assert np.all(on["qthr"] >= off["qthr"]) and np.median(on["qthr"] - off["qthr"]) > 1.0


@pytest.mark.parametrize("d", [1, 2])
def test_moment_coefficients_reproduce_a_tile(d):
    rng = np.random.default_rng(d)
    zs = np.concatenate([rng.normal(size=(16, d)) * 0.05 + 1.0, np.full((16, d), -2.0), rng.normal(size=(5, d)) * 0.05])   # full, identical rows, padded
    cen, rho2, coef, scale = gr.tile_moments(zs)
    assert rho2[1] == 0.0 and np.allclose(cen[1], -2.0) and coef.shape == (3, 9 if d == 1 else 45)
    alphas = [(i, 0) for i in range(8, -1, -1)] if d == 1 else [(i, j) for j in range(8, -1, -1) for i in range(8 - j, -1, -1)]
    for t in range(3):
        rows = zs[t * 16:(t + 1) * 16]
        for u in (np.full(d, 0.3), np.full(d, -0.2) * np.arange(1, d + 1)):
            direct = np.exp2(-0.5 * ((u + cen[t] - rows) ** 2).sum(1)).sum()
            series = 2.0 ** (-0.5 * (u ** 2).sum()) * sum(float(coef[t, k]) * u[0] ** i * (u[d - 1] ** j if d == 2 else 1.0) for k, (i, j) in enumerate(alphas))
            assert abs(series - direct) <= 1e-9 * direct, (t, series, direct)   # order-8 remainder: (a |u| rho)^9 / 9! ~ 1e-13 here


def test_merge_of_split_partials():
    rng = np.random.default_rng(0)
    e = -rng.uniform(0, 300, size=(7, 400))                  # exponents of 7 queries
    parts = []
    for sl in (slice(0, 100), slice(100, 101), slice(101, 400)):
        o = e[:, sl].max(1)
        parts.append(np.stack([o, np.exp2(e[:, sl] - o[:, None]).sum(1)], 1))
    got = gr.merge_partials(np.array(parts), -3.5)
    m = e.max(1)
    want = -3.5 + gr.LN2 * (m + np.log2(np.exp2(e - m[:, None]).sum(1)))
    assert np.allclose(got, want, rtol=0, atol=1e-12)
