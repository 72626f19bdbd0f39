"""GPU tier: the d = 8 screen's dense kernel (kde_screen_d8_dense_kernel, the default: PBN_D8_SCREEN_STREAM=2 or unset) against the serial kernel
(PBN_D8_SCREEN_STREAM=0), csrc/kde_screen_d8.inc, DESIGN.md 3.1.

The dense kernel screens consecutive tile pairs - units of 8 tiles from the unit of a batch's first box bit to the unit of its last - where the
serial kernel and the ring screen the listed tiles only.  A tile's bit depends on its own rows and the group's queries alone and live = screened AND
box, so all three must write the same words: box masks and live masks of every launch are compared word for word, slogl as Python floats, on the
cases of test_prune_d8_screen_stream_gpu (partial last batches at 32 769 and 65 537 rows, batches of one tile, odd tile counts, one-batch and
many-batch splits).  The comparison proves nothing on shapes it never meets, so the serial kernel's box masks of the same launches must show the
shapes this kernel's walk turns on: ranges that begin and end inside a batch and at its ends, on odd and even bits, of one unit and of all eight,
a (wave, split) of one unit, of two, of three (the ring of two units of loads: shorter than it, as long, longer), batches out of reach between
two in reach, a unit that reaches beyond the table's last tile (moved back by whole tiles, its bits shifted), and - one screen wave serves two
sweep waves - batches in reach of one of them only and of both, with 49 and 65 queries for a last screen wave that serves two full sweep waves
and one that serves a half and an empty one."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

from test_prune_d8_screen_stream_gpu import CASES as RING_CASES, capture, fetch, tables as ring_tables
from test_prune_d8_sweep_gpu import frames
from test_prune_d8_screen_stream_gpu import lib, pbn  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# one screen wave serves two sweep waves (PBN_SCREEN_NW = 2): 49 queries are 4 query tiles - one screen wave, both of its sweep waves full - and 65
# are 5 - the second screen wave serves a sweep wave of one group and an empty one
NW_CASES = ["nw-32769-49", "nw-32769-65"]
CASES = RING_CASES + NW_CASES


def tables(case):
    if case in NW_CASES:
        _, n_train, n_test = case.split("-")
        return frames("correlated", 8, 1500, int(n_train), int(n_test))
    return ring_tables(case)


def geometry(lib):
    """(sweep waves, splits, batches per split, tiles per split, training tiles, queries) of the launch last captured; arms nothing."""
    dims = np.zeros(6, dtype=np.int64)
    lib.pbn_debug_d8_masks(0, dims.ctypes.data_as(C.c_void_p), 6, 0)
    return tuple(int(v) for v in dims)


@pytest.fixture(scope="module")
def launches(pbn, lib):
    """Per case, computed once: (slogl, box, live) of the dense kernel and of the serial one on the same fitted model and queries, and the launch's
    geometry.  A larger evaluation runs before each of them: the arena then holds another launch's words where the masks will lie, and a word a
    kernel failed to write would show."""
    done = {}

    def get(case):
        if case not in done:
            names, train, test = tables(case)
            k = pbn.ProductKDE(names)
            k.fit(train)
            larger = pd.concat([test, test, test.iloc[:7]], ignore_index=True)
            got = []
            for stream in ("2", "0"):
                k.slogl(larger)
                got.append(capture(lib, k, test, stream))
            done[case] = (got[0], got[1], geometry(lib), k, test)
        return done[case]

    return get


@pytest.mark.parametrize("case", CASES)
def test_masks_are_the_serial_kernels(launches, case):
    (s2, box2, live2), (s0, box0, live0) = launches(case)[:2]
    assert box0.any() and live0.any(), "the screen ran"
    assert not np.any(live0 & ~box0)
    assert np.array_equal(box2, box0), "box words"
    assert np.array_equal(live2, live0), f"live words: {int((live2 != live0).sum())} of {live0.size} differ"
    assert not np.any(live2 & ~box2)
    assert s2 == s0, (s2, s0)


def test_unset_knob_is_the_dense_kernel(launches, lib):
    """With the knob unset the launch writes the words of "2".  Equal words are all this proves: the three kernels write the same words by design,
    so which of them ran is read from a kernel trace (profiles/r13/step_kernels.txt), not from here."""
    (s2, box2, live2), _, _, k, test = launches("edge-32769-33")
    before = os.environ.pop("PBN_D8_SCREEN_STREAM", None)
    lib.pbn_debug_d8_masks(0, None, 0, 1)   # arm
    try:
        su = k.slogl(test)
        boxu, liveu = fetch(lib, 1, np.uint64).reshape(box2.shape), fetch(lib, 2, np.uint64).reshape(live2.shape)
    finally:
        lib.pbn_debug_d8_masks(0, None, 0, 0)
        if before is not None:
            os.environ["PBN_D8_SCREEN_STREAM"] = before
    assert np.array_equal(boxu, box2) and np.array_equal(liveu, live2)
    assert su == s2, (su, s2)


def lowest(u):
    """Position of the lowest set bit (u != 0)."""
    low = u & (~u + np.uint64(1))
    return np.log2(low.astype(np.float64)).astype(np.int64)   # (a power of two: exact)


def highest(u):
    out = np.zeros(u.shape, dtype=np.int64)
    for sh in (32, 16, 8, 4, 2, 1):
        big = (u >> np.uint64(sh)) != 0
        out += np.where(big, sh, 0)
        u = np.where(big, u >> np.uint64(sh), u)
    return out


def test_launches_cover_the_dense_walk(launches):
    """Read from the SERIAL kernel's box masks, so that it says what the inputs are and not what the dense kernel made of them."""
    firsts, lasts, spans, units_per_list = set(), set(), set(), set()
    first_odd = last_even = gaps = beyond = one_wave = both_waves = 0
    for case in CASES:
        _, (_, box, _), (nw, nsplit, bps, tps, ntiles, nq) = launches(case)[:3]   # box: (wave, split, batch, group)
        u = box[..., 0] | box[..., 1]
        reach = u != 0
        uz = u[reach]
        lo, hi = lowest(uz), highest(uz)
        ulo, uhi = lo >> 3, hi >> 3
        firsts |= set(np.unique(ulo).tolist())
        lasts |= set(np.unique(uhi).tolist())
        spans |= set(np.unique(uhi - ulo + 1).tolist())
        first_odd += int((lo & 1).sum())
        last_even += int(((hi & 1) == 0).sum())
        units = np.zeros(u.shape, dtype=np.int64)
        units[reach] = uhi - ulo + 1
        per_list = units.sum(axis=2)                                          # (wave, split)
        units_per_list |= set(np.unique(per_list).tolist())
        first_b = np.argmax(reach, axis=2)
        last_b = reach.shape[2] - 1 - np.argmax(reach[:, :, ::-1], axis=2)
        gap = reach.any(axis=2) & (reach.sum(axis=2) < last_b - first_b + 1)   # a batch out of reach between two in reach
        gaps += int(gap.sum())
        # batches in reach of one only / of both of the two sweep waves a screen wave serves
        pad = reach if nw % 2 == 0 else np.concatenate([reach, np.zeros((1,) + reach.shape[1:], dtype=bool)])
        pair = pad.reshape(-1, 2, nsplit, bps).sum(axis=1)
        one_wave += int((pair == 1).sum())
        both_waves += int((pair == 2).sum())
        # the first tile of every batch in the table, and whether the batch's last unit ends beyond the table's last tile
        tile0 = (np.arange(nsplit)[:, None] * tps + 64 * np.arange(bps)[None, :])[None, :, :] + np.zeros(u.shape, dtype=np.int64)
        over = tile0[reach] + 8 * uhi + 8 - ntiles
        beyond += int((over > 0).sum())
        print(f"{case}: first units {sorted(set(np.unique(ulo).tolist()))}, last units {sorted(set(np.unique(uhi).tolist()))}, units per batch "
              f"{sorted(set(np.unique(uhi - ulo + 1).tolist()))}; first bit odd {int((lo & 1).sum())}, last bit even {int(((hi & 1) == 0).sum())}; units per "
              f"(wave, split) up to 3: {sorted(p for p in np.unique(per_list).tolist() if p <= 3)}, max {int(per_list.max())}; lists with a gap "
              f"{int(gap.sum())}; last units beyond the table {int((over > 0).sum())} (by {sorted(set(over[over > 0].tolist()))} tiles)")
    assert firsts == set(range(8)), f"first units seen: {sorted(firsts)}"
    assert lasts == set(range(8)), f"last units seen: {sorted(lasts)}"
    assert spans == set(range(1, 9)), f"units per batch seen: {sorted(spans)}"
    assert first_odd > 0 and last_even > 0, "the ends of a range on an odd first and an even last bit"
    assert {0, 1, 2, 3} <= units_per_list, f"units per (wave, split) seen: {sorted(p for p in units_per_list if p <= 3)}"
    assert gaps > 0, "no list crosses a batch out of reach (see test_prune_d8_screen_stream_gpu.test_launches_cover_the_ring)"
    assert beyond > 0, "no batch in reach has its last unit beyond the table's last tile"
    print(f"batches in reach of one served sweep wave only {one_wave}, of both {both_waves}")
    assert one_wave > 0 and both_waves > 0, "a batch in reach of one served wave only, and one in reach of both"
