"""GPU tier: the f16 screen of the pruned sum-only d = 8 sweep (csrc/kde_screen_d8.inc).

kde_screen_d8_kernel walks the boxes the sweep used to walk and takes out of the visit masks every (tile, group) block whose 256 pairs an f16 MFMA
proves below the group's drop threshold; kde_sweep_pruned_d8_kernel then reads the masks.  What must hold: nothing at or above a threshold is ever
dropped (checked pair by pair in fp64 from the masks of a real launch), the sums stay inside the budgets of the pruned sweep, the rare paths and the
edges of tiles, batches and splits behave as before, and with the masks over their memory cap the step is the unscreened one, bit for bit."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from test_prune_d8_sweep_gpu import BUDGET, frames, rare_path_frames, redo_counts

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634


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


def slogl(pbn, names, train, test, monkeypatch=None, **env):
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    try:
        k = pbn.ProductKDE(names)
        k.fit(train)
        return k.slogl(test)
    finally:
        for k_ in env:
            monkeypatch.delenv(k_)


def screened(pbn, lib, monkeypatch, names, train, test, model=None):
    """slogl with the screen on, and the proof that it ran: its own counters moved (a change of the gating that left these tables unscreened would
    otherwise pass every comparison below without testing anything)."""
    kept, tested = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.pbn_debug_d8_screen(None, None, 1)
    monkeypatch.setenv("PBN_SWEEP_COUNT_REDO", "1")
    try:
        s = model() if model else slogl(pbn, names, train, test)
    finally:
        monkeypatch.delenv("PBN_SWEEP_COUNT_REDO")
    lib.pbn_debug_d8_screen(C.byref(kept), C.byref(tested), 1)
    assert 0 < kept.value <= tested.value, (kept.value, tested.value)
    return s


def margin_of(n):
    return 43.0 + np.log2(n / 1e6)   # prune_margin(fp64, N, sum-only)


def fetch(lib, what, dtype):
    n = lib.pbn_debug_d8_masks(what, None, 0, 1)
    out = np.zeros(n, dtype=dtype)
    lib.pbn_debug_d8_masks(what, out.ctypes.data_as(C.c_void_p), n, 1)
    return out


def test_no_dropped_block_holds_a_live_pair(pbn, lib, monkeypatch):
    """The table of test_visits_are_the_parents.  Every block that passes the box test is recomputed in fp64 from the model's sorted, whitened rows."""
    d = 8
    rng = np.random.default_rng(940 + d)
    names = [f"v{i}" for i in range(d)]
    mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
    train = pd.DataFrame(rng.normal(size=(100_000, d)) @ mix.T, columns=names)
    test = pd.DataFrame(rng.normal(size=(2_000, d)) @ mix.T, columns=names)
    k = pbn.ProductKDE(names)
    k.fit(train)
    # a larger evaluation first: the arena then holds another launch's words where this one's masks will lie, and a word the screen failed to
    # write (the batch slots past the table's end in the short last split) would show as live outside box
    k.slogl(pd.concat([test, test, test.iloc[:1_000]], ignore_index=True))
    lib.pbn_debug_d8_masks(0, None, 0, 1)   # arm
    try:
        k.slogl(test)
        dims = fetch(lib, 0, np.int64)
        nw, nsplit, bps, tps, ntiles, nq = (int(v) for v in dims)
        box = fetch(lib, 1, np.uint64).reshape(nw, nsplit, bps, 2)
        live = fetch(lib, 2, np.uint64).reshape(nw, nsplit, bps, 2)
        thr = fetch(lib, 3, np.float64)
        zq = fetch(lib, 4, np.float64).reshape(nq, 8)
        zt = fetch(lib, 5, np.float64).reshape(-1, 8)
    finally:
        lib.pbn_debug_d8_masks(0, None, 0, 0)
    assert nq == 2_000 and len(zt) == 100_000 and ntiles == 6_250
    assert not np.any(live & ~box), "live is a subset of box"
    nqt = (nq + 15) // 16
    zt_t = np.zeros((ntiles * 16, 8))
    zt_t[:len(zt)] = zt
    nt = -0.5 * np.sum(zt_t * zt_t, axis=1)
    nt[len(zt):] = -np.inf                                  # padding rows hold no term
    zq_t = np.zeros((nqt * 16, 8))
    zq_t[:nq] = zq
    nqv = -0.5 * np.sum(zq_t * zq_t, axis=1)
    nqv[nq:] = -np.inf
    zt_t, nt, zq_t, nqv = zt_t.reshape(ntiles, 16, 8), nt.reshape(ntiles, 16), zq_t.reshape(nqt, 16, 8), nqv.reshape(nqt, 16)

    def bits(m):
        return np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(nw, nsplit, bps, 2, 8), axis=-1, bitorder="little").astype(bool)

    bb, lb = bits(box), bits(live)
    w, sp, jb, g, bit = np.nonzero(bb)
    keep = w * 2 + g < nqt                                   # (the second group of the last wave repeats the last query tile)
    w, sp, jb, g, bit = (a[keep] for a in (w, sp, jb, g, bit))
    tile, qt = sp * tps + jb * 64 + bit, w * 2 + g
    assert tile.max() < ntiles
    kept = lb[w, sp, jb, g, bit]
    alive = np.zeros(len(tile), dtype=bool)
    for i in range(0, len(tile), 20_000):
        t_, q_ = tile[i:i + 20_000], qt[i:i + 20_000]
        s = np.einsum("bik,bjk->bij", zt_t[t_], zq_t[q_]) + nt[t_][:, :, None] + nqv[q_][:, None, :]
        alive[i:i + 20_000] = s.reshape(len(t_), -1).max(axis=1) >= thr[q_]
    n_box, n_dead, n_drop = len(tile), int((~alive).sum()), int((~kept).sum())
    print(f"box-visited blocks {n_box}; dead by brute force {n_dead} ({n_dead / n_box:.3f}); dropped by the screen {n_drop} ({n_drop / n_box:.3f}, "
          f"{n_drop / max(n_dead, 1):.3f} of the dead)")
    assert not np.any(alive & ~kept), "a dropped block holds a pair at or above its group's threshold"
    assert n_drop >= 0.10 * n_box


@pytest.mark.parametrize("kind", ["correlated", "independent", "heavy-tailed"])
def test_results_stay_inside_the_budgets(pbn, lib, monkeypatch, kind):
    names, train, test = frames(kind, 8, 1100)
    on = screened(pbn, lib, monkeypatch, names, train, test)
    plain = slogl(pbn, names, train, test, monkeypatch, PBN_SWEEP_PRUNE="0")
    off = slogl(pbn, names, train, test, monkeypatch, PBN_D8_SCREEN="0")
    guard = slogl(pbn, names, train, test, monkeypatch, PBN_MAGIC_GUARD="0")
    n = len(train)
    print(f"{kind}: screened {on!r}; vs unpruned {abs(on - plain) / abs(plain):.3e}; vs unscreened {abs(on - off) / abs(off):.3e} (bound {n * 2.0 ** -margin_of(n):.3e})")
    assert np.isfinite(on) and abs(on - plain) <= BUDGET * abs(plain)
    assert abs(on - off) <= n * 2.0 ** -margin_of(n) * abs(off)
    assert on == guard


def test_nothing_live_is_lost(pbn, lib, monkeypatch):
    """Bandwidth I, every query next to ONE training row, and 40 000 rows on a sphere around it whose terms sit 0.75 exponent units INSIDE the
    margin: nothing may be dropped, and a pruned sum from which nothing is dropped is the unpruned one to rounding."""
    rng = np.random.default_rng(21)
    d, n_ring = 8, 40_000
    n = n_ring + 1
    e = margin_of(n) - 0.75
    r = np.sqrt(2.0 * e / LOG2E)
    u = rng.normal(size=(n_ring, d))
    ring = r * u / np.linalg.norm(u, axis=1, keepdims=True)
    train = np.vstack([np.zeros((1, d)), ring])
    test = rng.normal(scale=0.002, size=(1_000, d))
    # the exact arithmetic keeps every row: its exponent against the query's log2 sum
    s = -0.5 * LOG2E * (np.sum(test * test, axis=1)[:, None] - 2.0 * test @ train.T + np.sum(train * train, axis=1)[None, :])
    log2sum = np.log2(np.sum(np.exp2(s - s.max(axis=1, keepdims=True)), axis=1)) + s.max(axis=1)
    assert np.all(s >= (log2sum - margin_of(n))[:, None] + 0.5)
    names = [f"v{i}" for i in range(d)]

    def run():
        k = pbn.KDE(names)
        k.fit(pd.DataFrame(train, columns=names))
        k.bandwidth = np.eye(d)
        return k.slogl(pd.DataFrame(test, columns=names))

    on = screened(pbn, lib, monkeypatch, None, None, None, model=run)
    monkeypatch.setenv("PBN_SWEEP_PRUNE", "0")
    plain = run()
    monkeypatch.delenv("PBN_SWEEP_PRUNE")
    print(f"screened {on!r} unpruned {plain!r} relative {abs(on - plain) / abs(plain):.3e}")
    assert abs(on - plain) <= 1e-11 * abs(plain)


@pytest.mark.parametrize("n_test", [16, 17, 33, 1_025])
@pytest.mark.parametrize("n_train", [32_768, 32_769, 65_537, 131_087])
def test_edges(pbn, lib, monkeypatch, n_train, n_test):
    """An odd number of passing tiles (a half-empty MFMA), a padded last tile, one query group in the last wave, one split's worth of batches and
    several splits, a short last split.  NOT covered: a second super-batch of one split (the second turn of the `sb += 4096` loops and the sweep's
    reload of its mask words) - the shipped library keeps a pruned split at 1 024 tiles (PRUNE_MAX_TILES, a compile-time constant outside
    -DPBN_EXPERIMENTS builds), so a split holds at most 16 batches at any table size and no launch of it reaches that turn."""
    names, train, test = frames("correlated", 8, 1200, n_train, n_test)
    on = screened(pbn, lib, monkeypatch, names, train, test)
    plain = slogl(pbn, names, train, test, monkeypatch, PBN_SWEEP_PRUNE="0")
    off = slogl(pbn, names, train, test, monkeypatch, PBN_D8_SCREEN="0")
    assert np.isfinite(on) and abs(on - plain) <= BUDGET * abs(plain), (on, plain)
    assert abs(on - off) <= n_train * 2.0 ** -margin_of(n_train) * abs(off), (on, off)


@pytest.mark.parametrize("case,norms", [("overflow", [700.0, 850.0, 900.0, 930.0, 960.0, 990.0]), ("nan_weight", [1010.0, 1100.0, 2000.0, 30000.0])])
def test_rare_paths_with_the_screen(pbn, lib, monkeypatch, case, norms):
    names, train, test = rare_path_frames(8, norms, 1300)
    redo_counts(lib)
    on = screened(pbn, lib, monkeypatch, names, train, test)
    redo, units = redo_counts(lib)
    plain = slogl(pbn, names, train, test, monkeypatch, PBN_SWEEP_PRUNE="0")
    print(f"{case}: batches redone {redo} of {units}; relative {abs(on - plain) / abs(plain):.3e}")
    assert units > 0 and redo > 0
    assert np.isfinite(on) and abs(on - plain) <= BUDGET * abs(plain)


def test_over_the_memory_cap_the_step_runs_unscreened(pbn, lib, monkeypatch):
    names, train, test = frames("correlated", 8, 1400)
    kept, tested = C.c_ulonglong(0), C.c_ulonglong(0)
    lib.pbn_debug_d8_screen(None, None, 1)
    capped = slogl(pbn, names, train, test, monkeypatch, PBN_D8_SCREEN_MAX_MB="0", PBN_SWEEP_COUNT_REDO="1")
    lib.pbn_debug_d8_screen(C.byref(kept), C.byref(tested), 1)
    assert tested.value == 0                                  # the screen did not run
    off = slogl(pbn, names, train, test, monkeypatch, PBN_D8_SCREEN="0")
    on = slogl(pbn, names, train, test, monkeypatch, PBN_SWEEP_COUNT_REDO="1")
    lib.pbn_debug_d8_screen(C.byref(kept), C.byref(tested), 1)
    assert capped == off
    assert 0 < kept.value < tested.value and np.isfinite(on)   # ... and does by default
