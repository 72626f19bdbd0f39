"""GPU tier: the two-phase d = 8 screen (kde_screen_d8_kernel: box words parked in LDS, then a ring of fragment loads through the MFMAs) against the
serial kernel it replaces (kde_screen_d8_serial_kernel, PBN_D8_SCREEN_STREAM=0), csrc/kde_screen_d8.inc, DESIGN.md 3.1.

The two must write the same words: the box masks and the live masks of every launch are compared word for word, and slogl as Python floats.  The
comparison proves nothing on shapes it never meets, so the same launches' box masks must show every list length around the ring depth - batches of
1 .. 2R + 2 tiles and of 33 and more, (wave, split) lists of 0 and of 1 .. R + 1 pairs (shorter than the ring, the prologue alone, one turn and a
slot), and a list that goes on behind a batch out of reach.  What no dropped block may hold is tests/test_prune_d8_screen_gpu.py's to prove, on the
default kernel.

Inputs settled on (the box masks come from the device; see test_launches_cover_the_ring's output): the Gaussian frames of test_prune_d8_sweep_gpu
at 32 768 / 32 769 / 65 537 training rows x 16 / 17 / 33 / 1 025 queries give the long lists and the padded tiles, and with 33 and 1 025 queries
most of the short ones; `islands`, a built table - a background cloud out of every query's reach and, far from it and from each other, islands of
8 .. 200 rows with 32 queries on each - gives every batch of 1 .. 12 tiles and every list of 0 .. 6 pairs.  None of them, nor `clumps` with a
query group on every second clump, CAN have a list with a gap: the library cuts the training tiles into as many splits as fill the device
(24 blocks of 8 query tiles per CU), down to 64 tiles a split, so with so few queries a split is one or two batches long.  A split of three
batches and more takes queries by the ten thousand: `deep-gauss` (65 537 rows x 32 768 queries: 3 batches a split on 256 CUs, 316 of 24 576 lists
with a gap) and `deep-clumps` (832 queries on each of the 60 clumps: 5 batches a split, 3 398 of 24 960 lists) make the gaps."""
import ctypes as C
import os
import re

import numpy as np
import pandas as pd
import pytest

from test_prune_d8_sweep_gpu import frames, rare_path_frames

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pybnesian_amd", "csrc")
# the ring depth of the default build, from the source: a library built with -DPBN_SCREEN_RING=n would be asked for the lists around this depth
with open(os.path.join(CSRC, "kde_screen_d8.inc")) as _f:
    R = int(re.search(r"^#define PBN_SCREEN_RING (\d+)", _f.read(), flags=re.M).group(1))

EDGES = [(n_train, n_test) for n_train in (32_768, 32_769, 65_537) for n_test in (16, 17, 33, 1_025)]
RARE = [("overflow", [700.0, 850.0, 900.0, 930.0, 960.0, 990.0]), ("nan_weight", [1010.0, 1100.0, 2000.0, 30000.0])]
CASES = [f"edge-{a}-{b}" for a, b in EDGES] + [f"rare-{name}" for name, _ in RARE] + ["islands", "clumps", "deep-gauss", "deep-clumps"]


def islands(seed=5):
    """32 768 cloud rows around the origin and 24 islands on the axes and diagonals at 9 .. 14 cloud deviations, island i holding 8 (i + 1) rows
    within 0.02 of its centre (half a tile to 12 tiles) and 32 queries - one sweep wave - on the same spot.  Every query also sees what the boxes
    of its island's tiles drag in, nothing of the cloud."""
    rng = np.random.default_rng(seed)
    d = 8
    names = [f"v{i}" for i in range(d)]
    rows, queries = [rng.normal(size=(32_768, d))], []
    for i in range(24):
        c = np.zeros(d)
        c[i % d] = (9.0 + 0.2 * i) * (1.0 if (i // d) % 2 == 0 else -1.0)
        if i >= 16:
            c[(i + 3) % d] = 9.0 + 0.2 * i
        rows.append(c + rng.normal(scale=0.02, size=(8 * (i + 1), d)))
        queries.append(c + rng.normal(scale=0.02, size=(32, d)))
    return names, pd.DataFrame(np.vstack(rows), columns=names), pd.DataFrame(np.vstack(queries), columns=names)


def clumps(seed=1, per_clump=0):
    """60 tight clumps at Gaussian centres, mostly out of each other's reach, of 300 and of 2 100 rows in turn (the larger always cover a whole
    64-tile batch).  per_clump = 0: 16 queries - one query group - on every clump of 300 rows.  Otherwise that many queries on every clump:
    enough of them make the splits several batches long, and a wave that reaches the clumps of a split's first and last batch and none of
    those between has a list that goes on behind a batch out of reach."""
    rng = np.random.default_rng(seed)
    d = 8
    names = [f"v{i}" for i in range(d)]
    centres = rng.normal(size=(60, d))
    train = pd.DataFrame(np.vstack([c + rng.normal(scale=0.002, size=(300 if i % 2 == 0 else 2_100, d)) for i, c in enumerate(centres)]), columns=names)
    on = centres if per_clump else centres[::2]
    return names, train, pd.DataFrame(np.vstack([c + rng.normal(scale=0.002, size=(per_clump or 16, d)) for c in on]), columns=names)


def tables(case):
    if case.startswith("edge-"):
        _, n_train, n_test = case.split("-")
        return frames("correlated", 8, 1500, int(n_train), int(n_test))
    if case.startswith("rare-"):
        return rare_path_frames(8, dict(RARE)[case[5:]], 1300)
    if case == "clumps":
        return clumps()
    if case == "deep-gauss":
        return frames("correlated", 8, 1500, 65_537, 32_768)
    if case == "deep-clumps":
        return clumps(per_clump=832)
    return islands()


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib():
    from pybnesian_amd import _lib

    lib = _lib.load()
    lib.pbn_debug_d8_masks.restype = C.c_int64
    lib.pbn_debug_d8_masks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int]
    return lib


def fetch(lib, what, dtype):
    n = lib.pbn_debug_d8_masks(what, None, 0, 1)
    out = np.zeros(n, dtype=dtype)
    lib.pbn_debug_d8_masks(what, out.ctypes.data_as(C.c_void_p), n, 1)
    return out


def capture(lib, k, test, stream):
    """slogl and the masks of one launch with the kernel chosen by PBN_D8_SCREEN_STREAM (read at every evaluation)."""
    before = os.environ.get("PBN_D8_SCREEN_STREAM")
    os.environ["PBN_D8_SCREEN_STREAM"] = stream
    lib.pbn_debug_d8_masks(0, None, 0, 1)   # arm
    try:
        s = k.slogl(test)
        nw, nsplit, bps, tps, ntiles, nq = (int(v) for v in fetch(lib, 0, np.int64))
        box = fetch(lib, 1, np.uint64).reshape(nw, nsplit, bps, 2)
        live = fetch(lib, 2, np.uint64).reshape(nw, nsplit, bps, 2)
    finally:
        lib.pbn_debug_d8_masks(0, None, 0, 0)
        if before is None:
            del os.environ["PBN_D8_SCREEN_STREAM"]
        else:
            os.environ["PBN_D8_SCREEN_STREAM"] = before
    assert nq == len(test)
    return s, box, live


@pytest.fixture(scope="module")
def launches(pbn, lib):
    """Per case, computed once: the (slogl, box, live) of the ring kernel and of the serial one on the same fitted model and queries.  A larger
    evaluation runs before each of them: the arena then holds another launch's words where the masks will lie, and a word a kernel failed to
    write would show."""
    done = {}

    def get(case):
        if case not in done:
            names, train, test = tables(case)
            k = pbn.ProductKDE(names)
            k.fit(train)
            larger = pd.concat([test, test, test.iloc[:7]], ignore_index=True)
            done[case] = []
            for stream in ("1", "0"):
                k.slogl(larger)
                done[case].append(capture(lib, k, test, stream))
        return done[case]

    return get


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.int64)


@pytest.mark.parametrize("case", CASES)
def test_masks_are_the_serial_kernels(launches, case):
    (s1, box1, live1), (s0, box0, live0) = launches(case)
    assert box0.any() and live0.any(), "the screen ran"
    assert not np.any(live0 & ~box0)
    assert np.array_equal(box1, box0), "box words"
    assert np.array_equal(live1, live0), f"live words: {int((live1 != live0).sum())} of {live0.size} differ"
    assert s1 == s0, (s1, s0)


def test_launches_cover_the_ring(launches):
    """Read from the SERIAL kernel's box masks, so that it says what the inputs are and not what the ring made of them."""
    tile_counts, pair_counts, gaps = set(), set(), 0
    for case in CASES:
        box = launches(case)[1][1]                            # (wave, split, batch, group)
        tiles = popcount(box[..., 0] | box[..., 1])           # (wave, split, batch)
        pairs = ((tiles + 1) // 2).sum(axis=2)                # (wave, split)
        reach = tiles > 0
        first = np.argmax(reach, axis=2)
        last = reach.shape[2] - 1 - np.argmax(reach[:, :, ::-1], axis=2)
        gap = reach.any(axis=2) & (reach.sum(axis=2) < last - first + 1)   # a batch out of reach between two in reach
        tile_counts |= set(np.unique(tiles).tolist())
        pair_counts |= set(np.unique(pairs).tolist())
        gaps += int(gap.sum())
        print(f"{case}: tiles per (wave, batch) {sorted(set(np.unique(tiles).tolist()))}; pairs per (wave, split) up to {R + 1}: "
              f"{sorted(p for p in np.unique(pairs).tolist() if p <= R + 1)}, max {int(pairs.max())}; lists with a gap {int(gap.sum())}")
    missing_tiles = [c for c in range(1, 2 * R + 3) if c not in tile_counts]
    missing_pairs = [p for p in range(0, R + 2) if p not in pair_counts]
    assert not missing_tiles, f"no (wave, batch) with {missing_tiles} tiles"
    assert any(c >= 33 for c in tile_counts)
    assert not missing_pairs, f"no (wave, split) with {missing_pairs} pairs"
    assert gaps > 0, ("no list crosses a batch out of reach: `deep-gauss` and `deep-clumps` count on splits of three batches and more, and the "
                      "number of splits follows the device's CU count (256 on MI355X) - on another device give them more queries")
