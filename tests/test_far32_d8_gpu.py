"""GPU tier: the far pass of the pruned sum-only d = 8 sweep (csrc/kde_far32_d8.inc, the far words of csrc/kde_screen_d8.inc).

The screen marks a kept block FAR when every pair of it is proven theta bits below its own query's sum bound and both sides are plain;
the fp64 sweep leaves those blocks to kde_sweep_far32_d8_kernel.  Held here, on real launches at sizes with padded tiles, padded query
columns, an odd last sweep wave and several splits: far within live within box; the far rule pair by pair in fp64 from the dumped rows and
thresholds; no far block on a tile with a row over the cap or padding; the three screen kernels the same far words and the same sum;
the sum inside the far-tail line of the budget against the pass switched off and inside the whole budget against the unpruned sweep; and
with the switch at 0, a NaN query, a row beyond the cap and a launch over the memory cap, the fp64 path."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import CSRC
from test_prune_d8_screen_gpu import margin_of
from test_prune_d8_screen_rowthr_gpu import Dump, env
from test_prune_d8_screen_stream_gpu import fetch
from test_prune_d8_screen_stream_gpu import lib, pbn  # noqa: F401  (fixtures)
from test_prune_d8_sweep_gpu import BUDGET, frames

pytestmark = pytest.mark.gpu

FAR_TAIL = 8e-8   # DESIGN.md 4, "fp32 far tail": what the far terms of a sum may move it by, relative


def header_constant(name):
    with open(f"{CSRC}/kde_kernels.hpp") as f:
        return float(re.search(rf"^#define {name} ([0-9.e+-]+)", f.read(), flags=re.M).group(1))


NCAP = header_constant("PBN_FAR32_NCAP")


def theta_of(lib, n):
    eps, theta = C.c_double(), C.c_double()
    lib.pbn_debug_far32_rule.argtypes = [C.c_double, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.pbn_debug_far32_rule.restype = None
    lib.pbn_debug_far32_rule(NCAP, n, C.byref(eps), C.byref(theta))
    return theta.value


def far_launches(lib, reset=False):
    n = C.c_ulonglong()
    lib.pbn_debug_far32_launches.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    lib.pbn_debug_far32_launches.restype = None
    lib.pbn_debug_far32_launches(C.byref(n), 1 if reset else 0)
    return n.value


class FarDump(Dump):
    """... and the far words of the launch (what = 7; none where it wrote none) and how many far passes it launched."""

    def __init__(self, lib, k, test, stream="2", **kv):
        far_launches(lib, reset=True)
        super().__init__(lib, k, test, stream, **kv)
        self.passes = far_launches(lib)
        far = fetch(lib, 7, np.uint64)
        lib.pbn_debug_d8_masks(0, None, 0, 0)
        self.far = far.reshape(self.live.shape) if far.size else None


@pytest.fixture(scope="module")
def models(pbn):
    """Per training size: the fitted model, the same fitted with pruning off (the switch is read at the fit) and 3 200 queries; fitted once."""
    done = {}

    def get(n_train):
        if n_train not in done:
            names, train, test = frames("correlated", 8, 1600 + n_train % 1000, n_train, 3_200)
            k = pbn.ProductKDE(names)
            k.fit(train)
            with env(PBN_SWEEP_PRUNE="0"):
                k0 = pbn.ProductKDE(names)
                k0.fit(train)
            done[n_train] = (k, k0, test)
        return done[n_train]

    return get


def check_far_rule(d, theta, margin):
    """Every column of every far block below its query's threshold less theta, in fp64; far blocks on plain tiles only.  Returns the far
    and kept block counts."""
    box, live, far = d.tile_bits(d.box), d.tile_bits(d.live), d.tile_bits(d.far)
    assert not np.any(live & ~box) and not np.any(far & ~live), "far within live within box"
    n_rows = np.zeros(d.ntiles * 16)
    n_rows[:len(d.zt)] = 0.5 * np.sum(d.zt * d.zt, axis=1)
    n_rows[len(d.zt):] = np.inf                                      # padding rows
    plain = ~(n_rows.reshape(-1, 16) > NCAP).any(axis=1) & ~np.isnan(n_rows.reshape(-1, 16)).any(axis=1)
    assert not np.any(far & ~plain[None, :]), "a far block on a tile with a row over the cap, a NaN row or padding"
    qrow = d.thr + margin                                            # (what = 6 is the bound less the margin)
    nq = np.zeros(d.nqt * 16)
    nq[:d.nq] = 0.5 * np.sum(d.zq * d.zq, axis=1)
    worst = -np.inf
    for qt in range(d.nqt):
        tiles = np.nonzero(far[qt])[0]
        if not len(tiles):
            continue
        cols = slice(qt * 16, qt * 16 + 16)
        assert np.all(nq[cols] <= NCAP) and np.all(np.abs(qrow[cols]) <= 4 * NCAP), f"query tile {qt}: a far block beside a query the pass does not take"
        gap = d.column_maxima(qt, tiles) - (qrow[cols] - theta)[None, :]
        worst = max(worst, float(gap.max()))
        assert np.all(gap < 0.0), f"query tile {qt}: a far block holds a pair within theta of its query's bound ({gap.max():.3f})"
    return int(far.sum()), int(live.sum()), worst


@pytest.mark.parametrize("n_test", [16, 17, 33, 1_025])
@pytest.mark.parametrize("n_train", [32_768, 32_769, 65_537, 131_087])
def test_far_words_and_sums(lib, models, n_train, n_test):
    k, k0, test = models(n_train)
    q = test.iloc[:n_test]
    theta, margin = theta_of(lib, n_train), margin_of(n_train)
    on = FarDump(lib, k, q)
    assert on.far is not None and on.passes == 1
    n_far, n_live, worst = check_far_rule(on, theta, margin)
    off = FarDump(lib, k, q, PBN_D8_FAR32="0")
    assert off.far is None and off.passes == 0, "with the switch at 0 the far pointer is null and no far kernel runs"
    assert np.array_equal(on.live, off.live) and np.array_equal(on.box, off.box), "the live and box words keep their meaning"
    plain = k0.slogl(q)
    print(f"{n_train} x {n_test}: theta {theta:.2f}, far {n_far} of {n_live} kept blocks ({n_far / max(n_live, 1):.3f}), nearest far pair {worst:.3f} below its "
          f"threshold; slogl far {on.slogl!r} fp64 {off.slogl!r} unpruned {plain!r}: {abs(on.slogl - off.slogl) / abs(off.slogl):.2e} / {abs(on.slogl - plain) / abs(plain):.2e}")
    assert n_far >= 1, "the path is exercised"
    for stream in ("0", "1"):
        other = FarDump(lib, k, q, stream)
        assert np.array_equal(on.far, other.far), f"far words of kernel {stream}: {int((on.far != other.far).sum())} differ"
        assert np.array_equal(on.live, other.live) and on.slogl == other.slogl, (stream, on.slogl, other.slogl)
    assert np.isfinite(on.slogl) and abs(on.slogl - off.slogl) <= FAR_TAIL * abs(off.slogl), (on.slogl, off.slogl)
    assert abs(on.slogl - plain) <= BUDGET * abs(plain), (on.slogl, plain)


def test_nan_query_takes_the_fp64_path(lib, models):
    """A NaN query's tile carries NaN bounds in all sixteen columns: no far block in it, and the launch's sum is what the switch at 0 gives."""
    import pyarrow as pa

    k, _, test = models(32_769)
    vals = test.iloc[:33].to_numpy().copy()
    vals[20, 3] = np.nan
    q = pa.RecordBatch.from_arrays([pa.array(np.ascontiguousarray(vals[:, j])) for j in range(vals.shape[1])], names=list(test.columns))
    on, off = FarDump(lib, k, q), FarDump(lib, k, q, PBN_D8_FAR32="0")
    pos = np.nonzero(np.isnan(on.zq).any(axis=1))[0]
    assert len(pos) == 1
    far = on.tile_bits(on.far)
    assert not far[int(pos[0]) // 16].any(), "the NaN query's tile has no far block"
    assert np.array_equal(on.live, off.live)
    assert (np.isnan(on.slogl) and np.isnan(off.slogl)) or on.slogl == off.slogl, (on.slogl, off.slogl)


def test_rows_beyond_the_cap_take_the_fp64_path(pbn, lib):
    """Queries and training rows on a spot whose 1/2|z|^2 lies beyond the cap, beside an ordinary cloud: no far block on a tile with such a
    row nor in a query tile with such a query, and the sums stay inside the budgets."""
    rng = np.random.default_rng(77)
    d, n = 8, 32_768
    names = [f"v{i}" for i in range(d)]
    import pandas as pd

    tr = rng.normal(size=(n, d))
    spot = np.full(d, 9.0)
    tr[:64] = spot + rng.normal(scale=0.05, size=(64, d))
    te = np.vstack([rng.normal(size=(48, d)), spot + rng.normal(scale=0.05, size=(16, d))])
    train, test = pd.DataFrame(tr, columns=names), pd.DataFrame(te, columns=names)
    k = pbn.ProductKDE(names)
    k.fit(train)
    with env(PBN_SWEEP_PRUNE="0"):
        k0 = pbn.ProductKDE(names)
        k0.fit(train)
    on, off = FarDump(lib, k, test), FarDump(lib, k, test, PBN_D8_FAR32="0")
    n_t, n_q = 0.5 * np.sum(on.zt * on.zt, axis=1), 0.5 * np.sum(on.zq * on.zq, axis=1)
    assert (n_t > NCAP).sum() >= 64 and (n_q > NCAP).sum() == 16, (int((n_t > NCAP).sum()), int((n_q > NCAP).sum()))
    n_far, n_live, _ = check_far_rule(on, theta_of(lib, n), margin_of(n))
    plain = k0.slogl(test)
    print(f"beyond the cap: far {n_far} of {n_live}; far {on.slogl!r} fp64 {off.slogl!r} unpruned {plain!r}")
    assert n_far >= 1
    assert abs(on.slogl - off.slogl) <= FAR_TAIL * abs(off.slogl) and abs(on.slogl - plain) <= BUDGET * abs(plain)


def test_over_the_memory_cap_takes_the_fp64_path(lib, models):
    """Live and far words together beyond PBN_D8_SCREEN_MAX_MB (the dump's box words counted): the screen runs, the far pass does not, and
    the sum is the switch's at 0 bit for bit."""
    k, _, test = models(131_087)
    q = test   # 3 200 queries: 100 sweep waves, 0.39 MB of words each for live, box and far - between a half and a third of one MB
    off = FarDump(lib, k, q, PBN_D8_FAR32="0")
    words_mb = off.live.size * 8 / 1048576.0
    cap = int(np.ceil(2.0 * words_mb))            # (whole MB) live and box words of the dump fit; far words on top do not
    assert 3.0 * words_mb > cap >= 2.0 * words_mb, (words_mb, cap)
    capped = FarDump(lib, k, q, PBN_D8_SCREEN_MAX_MB=str(cap))
    assert capped.far is None and capped.passes == 0
    assert np.array_equal(capped.live, off.live) and capped.slogl == off.slogl
