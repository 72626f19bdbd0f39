"""The restatement of the fitted KDE handles' pruning prepass (tests/prune_restatement.py) against itself and against brute force, without a
device.  tests/test_prune_stages_gpu.py holds the kernels against this restatement; a restatement that was wrong in the same way as a kernel
would hide the kernel's fault, so what can be checked without a kernel is checked here:

  keys      the Hilbert keys are a bijection onto 0 .. cells - 1 and consecutive keys are neighbouring cells, on the grids and with the cell
            numbering of tests/c/hilbert_check.cpp (which holds the C++ function to the same two properties); the 2-D walk of the kernel and
            the n-dimensional form agree at n = 2; the curve starts in cell 0 and ends in the corner (top, 0, ..., 0); the Morton interleave
            against a bit-by-bit loop; the cell clamp.
  sort      lower_bound and the stable order on keys with ties.
  subsample nsub and the rows at the sizes the GPU tier uses (1 023: none at d = 5; 1 100: 16 rows, stride 68).
  bounds    qlb <= the true largest exponent and qthr <= the smallest true log2 sum of the tile, by brute force over all training rows, on
            every fp64 plain case of the GPU tier (rounding slack only: group_restatement.bound_slack).
  visits    on the same cases, from the restated keys, boxes and bounds alone: the borderline (tile, group) pairs are at most 0.1 % of the
            certain ones (the condition under which the GPU tier can bracket the sweep's visit counter), and no pair the rule skips for
            certain holds a term above 2^(true log2 sum - margin) for any query of the group.
  splits    the split rule at the sizes of the GPU tier: 259 tiles in splits whose last batch holds one tile, the last split clipped.
The whitening here is the same rule as the handles' (full normal-reference bandwidth) computed with numpy - not the same bits, which the GPU
tier does not need: it restates from the captured matrix."""
import functools

import numpy as np
import pytest

import prune_restatement as pr

NUM_CUS = 256          # an MI355X; the GPU tier reads the count the library used
QG = 2                 # PBN_QG_PRUNE


def grid(n, bits):
    """Cells in the numbering of hilbert_check.cpp: axis i = bits [i bits, (i + 1) bits) of the cell's number."""
    ids = np.arange(1 << (n * bits), dtype=np.uint64)
    return np.stack([(ids >> np.uint64(i * bits)) & np.uint64((1 << bits) - 1) for i in range(n)], axis=1)


@pytest.mark.parametrize("n,bits", [(2, 5), (3, 4), (4, 3), (3, 5), (4, 4)])
def test_hilbert_keys_are_a_bijection_of_neighbours(n, bits):
    g = grid(n, bits)
    k = pr.hilbert_nd(g, n, bits)
    assert np.array_equal(np.sort(k), np.arange(len(g), dtype=np.uint32))
    walk = g[np.argsort(k)].astype(np.int64)
    assert np.all(np.abs(np.diff(walk, axis=0)).sum(1) == 1)
    assert np.all(walk[0] == 0) and walk[-1, 0] == (1 << bits) - 1 and np.all(walk[-1, 1:] == 0)
    if n == 2:
        assert np.array_equal(pr.hilbert2(g, bits), k)


def test_hilbert2_at_the_kernel_width():
    rng = np.random.default_rng(0)
    c = rng.integers(0, 1 << 16, size=(4096, 2)).astype(np.uint32)
    c[:4] = [[0, 0], [65535, 0], [65535, 65535], [0, 65535]]
    k = pr.hilbert2(c, 16)
    assert np.array_equal(k, pr.hilbert_nd(c, 2, 16))
    assert k[0] == 0 and k[1] == 0xFFFFFFFF
    # a step along the curve from any of the cells is a step to a neighbour: the inverse is not restated, so walk a small block exhaustively
    g = grid(2, 6)
    kk = pr.hilbert2(g + np.uint64(1 << 15), 16).astype(np.int64)      # a 64 x 64 block of the 65 536 x 65 536 grid, aligned to 64
    walk = g[np.argsort(kk)].astype(np.int64)
    assert kk.max() - kk.min() == len(g) - 1 and np.all(np.abs(np.diff(walk, axis=0)).sum(1) == 1)


@pytest.mark.parametrize("kd", [1, 3, 4])
def test_morton_interleave(kd):
    bits = pr.key_bits(kd)
    rng = np.random.default_rng(kd)
    c = rng.integers(0, 1 << bits, size=(257, kd)).astype(np.uint32)
    want = [sum(((int(row[i]) >> b) & 1) << (b * kd + i) for i in range(kd) for b in range(bits)) for row in c]
    assert pr.morton(c, kd, bits).tolist() == want
    assert np.array_equal(pr.keys(np.zeros((1, kd)), kd, hilbert_3_4=False), pr.morton(np.full((1, kd), 1 << (bits - 1)), kd, bits))


@pytest.mark.parametrize("kd", [1, 2, 3, 4])
def test_key_cells_and_clamp(kd):
    bits, cell = pr.key_bits(kd), pr.key_cell(kd)
    assert (bits, cell) == {1: (16, 0.03125), 2: (16, 0.03125), 3: (10, 0.5), 4: (8, 0.5)}[kd]
    half, top = 1 << (bits - 1), (1 << bits) - 1
    z = np.array([[0.0], [-cell], [-cell * 0.5], [cell * (half - 1)], [cell * half], [-cell * half], [-cell * half - 1e-9], [1e300], [-1e300]])
    z = np.repeat(z, kd, axis=1)
    assert pr.key_cells(z, kd)[:, 0].tolist() == [half, half - 1, half - 1, top, top, 0, 0, top, 0]
    assert pr.clamped(z, kd).tolist() == [False, False, False, False, True, False, True, True, True]
    assert pr.far_units(kd) > cell * half


def test_sort_and_lower_bound():
    k = np.array([5, 1, 5, 0, 1, 5, 9], dtype=np.uint32)
    o = pr.stable_order(k)
    assert o.tolist() == [3, 1, 4, 0, 2, 5, 6]
    assert pr.lower_bound(k[o], np.array([0, 1, 2, 5, 9, 10], dtype=np.uint32)).tolist() == [0, 1, 3, 3, 6, 7]


def test_subsample_rule():
    assert pr.nsub_of(1023, 5, 4) == 0 and pr.nsub_of(1100, 5, 4) == 16 and pr.nsub_of(4133, 6, 4) == 64 and pr.nsub_of(4133, 4, 4) == 0
    assert pr.nsub_of(10 ** 6, 5, 4) == 4096
    rows = pr.subsample_rows(1100, 16)
    assert rows.tolist() == [68 * k for k in range(16)] and len(pr.subsample_rows(1023, 0)) == 0


def test_split_rule_at_the_tier_sizes():
    fp64_d4 = (64 + 16) * 8
    # 4 133 rows: 259 tiles in four splits of 65 - two batches, the second of one tile - and the last split clipped to 64 tiles
    assert pr.split_rule(259, 38, NUM_CUS, QG, fp64_d4) == (4, 65, 2)
    assert 3 * 65 + 64 == 259
    assert pr.split_rule(17, 2, NUM_CUS, QG, fp64_d4) == (1, 17, 1)
    assert pr.split_rule(69, 16, NUM_CUS, QG, fp64_d4) == (1, 69, 2)
    # a large model: 62 500 tiles, 6 250 query tiles: 782 query blocks -> 8 splits by the CUs, 62 by the tile cap -> 64
    assert pr.split_rule(62500, 6250, NUM_CUS, QG, fp64_d4) == (64, 977, 16)
    bb = pr.batch_boxes(np.zeros((259, 2)), 1, 65)
    assert bb.shape == (8, 2) and np.isinf(bb[7]).all() and not np.isinf(bb[:7]).any()


@functools.lru_cache(maxsize=None)
def chain(name):
    cls, d, dtype, N, n = pr.CASES[name]
    x = pr.case_training(name)
    W, mu = pr.cpu_whitening(x)
    pd = min(d, 4)
    r = pr.restate_chain(x, W, mu, n, pr.QUERY_SEED + n, pd, pd, NUM_CUS, QG, ((d + 3) // 4 * 64 + 16) * 8)
    r["tmax"], r["tsum"] = pr.true_max_exponent(r["zs"], r["zq"]), pr.true_log2_sums(r["zs"], r["zq"])
    return r


@pytest.mark.parametrize("name", pr.VISIT_CASES)
def test_case_reaches_its_edges(name):
    cls, d, dtype, N, n = pr.CASES[name]
    r = chain(name)
    pd = min(d, 4)
    assert pr.clamped(r["zq"], pd).sum() >= 2                       # the two edge queries
    if name in ("kde-d4", "kde-d6"):
        assert pr.clamped(r["zs"], pd).sum() >= 1                   # four key axes of 8 bits: the rows at +-40 sd leave the key range
    pos = set(r["qpos"].tolist())
    assert 0 in pos and N in pos and any(0 < p < 32 for p in pos) and any(N - 32 < p < N for p in pos), sorted(pos)
    assert r["nsub"] == {"kde-d5-nosub": 0, "kde-d5": 16, "kde-d6": 64}.get(name, 0)
    lens = [len(r["zs"][t * 16:(t + 1) * 16]) for t in range(len(r["box"]))]
    assert lens[-1] == N % 16 != 0
    zero = [t for t in range(len(r["box"])) if np.array_equal(r["box"][t, :pd], r["box"][t, pd:])]
    assert zero, "no tile of zero extent: the identical rows do not fill a tile"
    if N == 4133:
        assert (r["nsplit"], r["tps"], r["nbps"]) == (4, 65, 2)


@pytest.mark.parametrize("name", pr.VISIT_CASES)
def test_restated_bounds_are_below_the_truth(name):
    cls, d, dtype, N, n = pr.CASES[name]
    r = chain(name)
    over = r["qlb"][:n] - r["tmax"] - pr.bound_slack(N, d, r["tmax"])
    assert np.all(over <= 0), (name, int(over.argmax()), float(over.max()))
    tile_min = np.array([r["tsum"][t * 16:(t + 1) * 16].min() for t in range(len(r["qthr"]))])
    over = r["qthr"] - tile_min - pr.bound_slack(N, d, tile_min)
    assert np.all(over <= 0), (name, int(over.argmax()), float(over.max()))
    assert np.all(np.isneginf(r["qlb"][n:])) and np.all(np.isfinite(r["qlb"][:n])) and np.all(np.isfinite(r["qthr"]))
    if r["nsub"]:
        # the subsample's mean term is a bound of the LARGEST term, its sum a part of the whole sum
        lb, sb = pr.subsample_bounds(r["ls"], r["nsub"])
        assert np.all(lb <= r["tmax"] + pr.bound_slack(N, d, r["tmax"])) and np.all(sb <= r["tsum"] + pr.bound_slack(N, d, r["tsum"]))


@pytest.mark.parametrize("name", pr.VISIT_CASES)
def test_visit_rule_borderline_cap_and_safety(name):
    cls, d, dtype, N, n = pr.CASES[name]
    r = chain(name)
    pd = min(d, 4)
    margin = pr.prune_margin(N)
    thr = r["qthr"] - margin
    certain, borderline, offered = pr.visit_counts(r["box"], r["bbox"], r["qbox"], thr, pd, r["tps"], QG)
    assert offered == pr.ceil_div(len(r["qbox"]), QG) * len(r["box"]) * QG
    assert 0 < certain <= offered
    assert borderline <= 1e-3 * certain, (name, certain, borderline)
    # safety: a pair skipped for certain holds no term above 2^(true log2 sum - margin) for any query of the group
    skip = pr.skipped_pairs(r["box"], r["bbox"], r["qbox"], thr, pd, r["tps"])
    worst = -np.inf
    for qt in range(len(r["qbox"])):
        tiles = np.flatnonzero(skip[qt])
        if not len(tiles):
            continue
        rows = np.concatenate([np.arange(t * 16, min(N, (t + 1) * 16)) for t in tiles])
        qs = slice(qt * 16, min(n, (qt + 1) * 16))
        ex = pr.true_exponents(r["zs"][rows], r["zq"][qs])
        lim = r["tsum"][qs] - margin
        worst = max(worst, float((ex - (lim + pr.bound_slack(N, d, lim))[:, None]).max()))
    assert worst <= 0, (name, worst)
    if name in ("kde-d1", "kde-d2", "kde-d4", "kde-d5-nosub"):
        assert skip.any() and certain < offered                      # the rule does skip something here
