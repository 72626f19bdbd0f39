"""The restatement of the contiguous Gram kernels' launch arithmetic (tests/gram_restatement.py) and the case plan of
tests/test_gram_shapes_gpu.py, without a device: the restated block arithmetic hands every chunk of a range to exactly one block, the plan
reaches every ring state the GPU test asserts at its end on parts of 64 to 304 CUs, the exact leg's integers stay below 2^53 and no planned
table exceeds 128 MiB."""
import numpy as np
import pytest

import gram_restatement as gr

CUS = (64, 104, 228, 256, 304)


@pytest.mark.parametrize("es", [8, 4])
@pytest.mark.parametrize("B", [1, 2, 3, 17, 128, 512])
def test_plain_blocks_take_every_chunk_once(B, es):
    C = gr.chunk_rows(es)
    for n in (0, 1, C - 1, C, C + 1, 5 * C, B * C, B * C + 1, 4 * B * C + C - 1, 9 * B * C + B * C // 2 + 17):
        owner = np.zeros(gr.ceil_div(n, C), dtype=np.int64)
        rows = 0
        for b in range(B):
            first, stride, mine, partial_last, nfull, tail = gr.plain_block(b, B, n, C)
            assert nfull == mine - (1 if partial_last else 0) and (tail > 0) == bool(partial_last) and tail < C
            for i in range(mine):
                owner[(first + i * stride) // C] += 1
            rows += nfull * C + tail
        assert np.all(owner == 1), (B, n)
        assert rows == n
        # only the range's very last chunk can be cut short, and at most one block holds it
        assert sum(1 for b in range(B) if gr.plain_block(b, B, n, C)[3]) == (1 if n % C else 0)


def test_ring_trip_counts():
    # for (i = 0; i + 4 < nfull; i += 2): no trip up to four whole chunks, then one trip per two more; the drain gets 3 or 4
    assert [gr.ring(nf) for nf in range(11)] == [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 3), (1, 4), (2, 3), (2, 4), (3, 3), (3, 4)]
    for nf in range(5, 200):
        trips, left = gr.ring(nf)
        assert trips >= 1 and left in (3, 4) and 2 * trips + left == nf


def test_reduce_tree_and_segment_runs():
    assert [gr.reduce_levels(g) for g in (1, 16, 17, 256, 257, 512, 608, 4096)] == [1, 1, 2, 2, 3, 3, 3, 3]
    for count in range(0, 40):
        runs = gr.seg_runs(count)
        assert len(runs) == 4 and runs[0][0] == 0 and runs[-1][1] == count
        assert all(a[1] == b[0] for a, b in zip(runs, runs[1:])) and all(hi - lo <= gr.ceil_div(count, 4) for lo, hi in runs)
    assert gr.seg_runs(9) == [(0, 3), (3, 6), (6, 9), (9, 9)] and gr.seg_runs(5) == [(0, 2), (2, 4), (4, 5), (5, 5)]
    assert gr.pieces(10, 10) == [] and gr.pieces(3, 4099) == [(3, 4099)] and gr.pieces(3, 4100) == [(3, 4099), (4099, 4100)]
    assert [len(gr.pair_launches(n)) for n in (1, 64, 65, 70, 96, 97, 130)] == [1, 1, 3, 3, 3, 6, 10]
    assert [len(gr.sse_pairs(d)) for d in (65, 70, 97, 130)] == [6, 6, 10, 15]


def test_super_blocks_tile_a_region():
    for length in (0, 1, 63, 64, 65, 1000, 1024, 1667, 4250, 5000, 100003):
        sb = gr.super_blocks(length)
        assert len(sb) == gr.SUPER_BLOCKS and sb[0][0] == 0 and sb[-1][1] == length
        assert all(a[1] == b[0] for a, b in zip(sb, sb[1:])) and all(lo <= hi for lo, hi in sb)
        assert all(hi % 64 == 0 for lo, hi in sb[:-1] if hi < length)


@pytest.mark.parametrize("num_cus", CUS)
def test_the_plan_reaches_every_required_state(num_cus):
    got, req = gr.planned_states(num_cus), gr.required_states(num_cus)
    assert not req - got, sorted(req - got, key=str)
    # what the issue of this test names, spelled out: blocks of 4 .. 9 whole chunks in the capped grid, both parities left to the drain, a cut
    # chunk on the first, a middle and the last block, and a three-level tree where the grid exceeds 256 blocks
    B = gr.GD_BLOCKS_PER_CU * num_cus
    for es in (8, 4):
        C = gr.chunk_rows(es)
        nfulls, cut_at = set(), set()
        for k in gr.K_CAPPED:
            for n, row0 in gr.capped_cases(num_cus, es, k):
                nblocks, _ = gr.plain_blocks(n, num_cus)
                assert gr.plain_grid(nblocks, num_cus) == B <= nblocks    # (k = 4 on a double table asks for exactly B blocks)
                assert nblocks > B or (k == 4 and es == 8)
                for b in range(B):
                    _, _, _, cut, nfull, _ = gr.plain_block(b, B, n, C)
                    nfulls.add(nfull)
                    if cut:
                        cut_at.add(b)
        assert nfulls == {3, 4, 5, 6, 7, 8, 9}                        # 3: in front of the cut chunk of k B C - 1 rows at k = 4
        assert 0 in cut_at and B - 1 in cut_at and any(0 < b < B - 1 for b in cut_at)
        assert {gr.ring(nf) for nf in nfulls} >= {(0, 4), (1, 3), (1, 4), (2, 3), (2, 4), (3, 3)}
        assert gr.reduce_levels(B) == (3 if B > 256 else 2)
    # the uncapped cases stay below the cap on every part
    for n, _ in gr.uncapped_cases():
        nblocks, _ = gr.plain_blocks(n, num_cus)
        assert gr.plain_grid(nblocks, num_cus) == nblocks


@pytest.mark.parametrize("num_cus", CUS)
def test_planned_tables_fit(num_cus):
    for es in (8, 4):
        rows = gr.capped_table_rows(num_cus, es)
        assert rows * gr.NCOL_CAPPED * es <= gr.MAX_TABLE_BYTES, (num_cus, es, rows)
        assert gr.exact_headroom(rows) < 2 ** 53                      # sums of products of integers in [-15, 15]
        assert rows < 2 ** 31
    assert gr.uncapped_table_rows() * gr.NCOL_PLAIN * 8 <= gr.MAX_TABLE_BYTES
    assert gr.SEG_TABLE_ROWS * max(gr.SEG_WIDTHS) * 8 <= gr.MAX_TABLE_BYTES and gr.exact_headroom(gr.SEG_TABLE_ROWS) < 2 ** 53
    # offset + integer must be exact in a float table: |s_j| + 15 far below 2^24
    assert 10 + 66 + 15 < 2 ** 24


@pytest.mark.parametrize("es", [8, 4])
def test_segment_plan(es):
    C = gr.chunk_rows(es)
    L = gr.segment_lengths(es)
    assert 0 in L and all(k * C + t in L for k in range(9) for t in (0, 1, C - 1))
    assert all(k * C + t in L for k in (0, 1, 5) for t in gr.SEG_TAILS + (gr.SEG_TAILS_F32 if es == 4 else ()))
    assert all(m * gr.SEG_ROWS + t in L for m in gr.SEG_PIECES for t in (0, 1, 77))
    segs = gr.segment_cases(es)
    assert len(segs) == 5 * len(L) and all(0 <= r0 <= r1 <= gr.SEG_TABLE_ROWS for r0, r1 in segs)
    for ln in L:   # each length at starts 0 .. 3 mod 4, and at one start off the 128-byte line whatever the element size
        mine = [r0 for r0, r1 in segs if r1 - r0 == ln]
        assert {r0 % 4 for r0 in mine} == {0, 1, 2, 3} and any((r0 * 4) % 128 for r0 in mine) and any(r0 % 64 == 0 for r0 in mine)
    assert {len(gr.pieces(r0, r1)) for r0, r1 in segs} >= {0, 1, 2, 3, 4, 5, 9}


def test_block_gram_equals_the_direct_integer_result():
    rng = np.random.default_rng(3)
    X = rng.integers(-15, 16, size=(5000, 7)).astype(np.int64)
    bg = gr.BlockGram(X, np.float64)
    for r0, r1 in ((0, 0), (0, 1), (5, 1000), (1023, 1025), (1024, 2048), (37, 4999), (0, 5000), (2047, 2049), (3000, 3000)):
        S, G = bg.range(r0, r1)
        assert np.array_equal(S, X[r0:r1].sum(axis=0).astype(np.float64)) and np.array_equal(G, (X[r0:r1].T @ X[r0:r1]).astype(np.float64))
