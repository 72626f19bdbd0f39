"""Counts of the d = 8 f16 screen on the GPU: blocks kept / tested (PBN_SWEEP_COUNT_REDO=1, pbn_debug_d8_screen), of the launch as shipped and of
the same launch with the columns screened against their group's threshold (PBN_D8_SCREEN_ROWTHR=0), and, from the dumped box
masks (pbn_debug_d8_masks), the MFMA iterations the screen issues: sum over (wave, batch) of ceil(popcount(box0 | box1) / 2) - and what the
forms of a screen without a pair list would issue instead (round 13): MFMAs and operand bytes (1 KiB per fragment load) with one screen wave
serving NW = 1 or 2 sweep waves.
    python tools/screen_d8_counts.py bench      bench.py's 1e6 x 1e5 table
    python tools/screen_d8_counts.py test       the 100 000 x 2 000 table of tests/test_prune_d8_screen_gpu.py::test_no_dropped_block_holds_a_live_pair"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (before the library, as in tools/prune_d8_visits.py)
import pybnesian_amd as pbn  # noqa: E402
from pybnesian_amd import _lib  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "test"
lib = _lib.load()
lib.pbn_debug_d8_masks.restype = C.c_int64
lib.pbn_debug_d8_masks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int]

if which == "bench":
    import bench

    ctx = pbn.Context(0)
    dev = torch.device("cuda", 0)
    n_train, n_test = 1_000_000, 100_000
    train_t, test_t = bench.make_tables(torch, dev, n_train, n_test, 0, 1, torch.float64)
    torch.cuda.synchronize()
    names = [f"v{i}" for i in range(bench.D)]
    train = pbn.DeviceTable.from_device_pointer(ctx, train_t.data_ptr(), n_train, names, n_train, _lib.PBN_F64, keepalive=train_t)
    test = pbn.DeviceTable.from_device_pointer(ctx, test_t.data_ptr(), n_test, names, n_test, _lib.PBN_F64, keepalive=test_t)
    kde = pbn.ProductKDE(names)
    kde.fit_table(train)
    out = torch.zeros(1, dtype=torch.float64, device=dev)

    def run():
        kde.slogl_table_async(test, out.data_ptr())
        ctx.sync()
        return out.item()
else:
    import pandas as pd

    d = 8
    rng = np.random.default_rng(940 + d)
    names = [f"v{i}" for i in range(d)]
    mix = np.tril(np.full((d, d), 0.3), -1) + np.eye(d)
    train = pd.DataFrame(rng.normal(size=(100_000, d)) @ mix.T, columns=names)
    test = pd.DataFrame(rng.normal(size=(2_000, d)) @ mix.T, columns=names)
    kde = pbn.ProductKDE(names)
    kde.fit(train)

    def run():
        return kde.slogl(test)

def counted():
    """slogl and the counters of one step: blocks kept / tested by the screen, box-visited / offered."""
    os.environ["PBN_SWEEP_COUNT_REDO"] = "1"
    lib.pbn_debug_d8_screen(None, None, 1)
    lib.pbn_debug_sweep_visits(None, None, 1)
    s = run()
    kept, tested, v, t = (C.c_ulonglong(0) for _ in range(4))
    lib.pbn_debug_d8_screen(C.byref(kept), C.byref(tested), 1)
    lib.pbn_debug_sweep_visits(C.byref(v), C.byref(t), 1)
    os.environ["PBN_SWEEP_COUNT_REDO"] = "0"
    return s, kept.value, tested.value, v.value, t.value


s, kept, tested, v, t = counted()
print(f"{which}: slogl {s!r}; box-visited {v} of {t} offered ({v / max(t, 1):.4f}); "
      f"screen kept {kept} of {tested} tested ({kept / max(tested, 1):.4f})")
# round 16: of the kept blocks, those the screen's far words hand to the fp32 pass (pbn_debug_d8_screen_far; PBN_D8_FAR32=0: none, the fp64 step)
if hasattr(lib, "pbn_debug_d8_screen_far"):
    far = C.c_ulonglong(0)
    os.environ["PBN_SWEEP_COUNT_REDO"] = "1"
    lib.pbn_debug_d8_screen_far(None, 1)
    s_far = run()
    lib.pbn_debug_d8_screen_far(C.byref(far), 1)
    os.environ["PBN_SWEEP_COUNT_REDO"] = "0"
    os.environ["PBN_D8_FAR32"] = "0"
    s_f64 = run()
    del os.environ["PBN_D8_FAR32"]
    print(f"  far blocks {far.value} of {kept} kept ({far.value / max(kept, 1):.4f}); slogl with the far pass {s_far!r}, PBN_D8_FAR32=0 {s_f64!r}: "
          f"relative difference {abs(s_far - s_f64) / abs(s_f64):.3e}")
# round 14: the same launch with every column against its GROUP's threshold (PBN_D8_SCREEN_ROWTHR=0, read per evaluation)
before = os.environ.get("PBN_D8_SCREEN_ROWTHR")
os.environ["PBN_D8_SCREEN_ROWTHR"] = "0"
try:
    s0, kept0, tested0, _, _ = counted()
finally:
    if before is None:
        del os.environ["PBN_D8_SCREEN_ROWTHR"]
    else:
        os.environ["PBN_D8_SCREEN_ROWTHR"] = before
print(f"  PBN_D8_SCREEN_ROWTHR=0: slogl {s0!r}; screen kept {kept0} of {tested0} tested ({kept0 / max(tested0, 1):.4f}); "
      f"kept per-query / kept group {kept / max(kept0, 1):.4f}; slogl relative difference {abs(s - s0) / abs(s0):.3e}")


def fetch(what, dtype):
    n = lib.pbn_debug_d8_masks(what, None, 0, 1)
    a = np.zeros(n, dtype=dtype)
    lib.pbn_debug_d8_masks(what, a.ctypes.data_as(C.c_void_p), n, 1)
    return a


lib.pbn_debug_d8_masks(0, None, 0, 1)
try:
    run()
    nw, nsplit, bps, tps, ntiles, nq = (int(x) for x in fetch(0, np.int64))
    box = fetch(1, np.uint64).reshape(nw, nsplit, bps, 2)
    live = fetch(2, np.uint64).reshape(nw, nsplit, bps, 2)
finally:
    lib.pbn_debug_d8_masks(0, None, 0, 0)


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.int64)


tiles = popcount(box[..., 0] | box[..., 1])          # per (wave, split, batch)
iters = (tiles + 1) // 2
blocks = int(popcount(box).sum())
per_split = iters.sum(axis=2)
print(f"  launch: {nw} waves x {nsplit} splits x {bps} batches of a split ({tps} tiles per split, {ntiles} tiles, {nq} queries)")
print(f"  blocks in the box masks {blocks} (live {int(popcount(live).sum())}); batches in reach {int((tiles > 0).sum())} of {tiles.size}")
print(f"  MFMA iterations {int(iters.sum())}: {blocks / max(int(iters.sum()), 1):.3f} blocks per iteration; tiles per batch in reach: "
      f"mean {tiles[tiles > 0].mean():.2f}, odd {float((tiles[tiles > 0] & 1).mean()):.3f}")
print(f"  iterations per (wave, split): mean {per_split.mean():.1f}, median {np.median(per_split):.0f}, max {per_split.max()}, "
      f"zero {float((per_split == 0).mean()):.3f}")


# ---- round 13: a screen that walks consecutive tile pairs (2p, 2p + 1) of a batch in reach instead of a list of the pairs that pass
def smear(u):
    for sh in (1, 2, 4, 8, 16, 32):
        u = u | (u >> np.uint64(sh))
    return u


def first_pair(u):   # of the lowest set bit (u != 0)
    return popcount((u & (~u + np.uint64(1))) - np.uint64(1)) >> 1


def last_pair(u):    # of the highest set bit (u != 0)
    return (popcount(smear(u)) - 1) >> 1


u1 = box[..., 0] | box[..., 1]                                   # (wave, split, batch): tiles in reach of a sweep wave
# pairs a batch holds at all: the last batch of a split (of the table) is partial
split_tiles = np.minimum(tps, np.maximum(ntiles - tps * np.arange(nsplit), 0))
batch_tiles = np.clip(split_tiles[:, None] - 64 * np.arange(bps)[None, :], 0, 64)      # (split, batch)
batch_pairs = (batch_tiles + 1) // 2


def forms(u, served):
    """u: (screen wave, split, batch) the tiles whose fragments the wave loads; served: how many of its sweep waves reach the batch.
    Returns {form: (MFMAs, loads)}."""
    on = u != 0
    uz = np.where(on, u, np.uint64(1))
    cur = (popcount(u) + 1) // 2
    full = np.where(on, np.broadcast_to(batch_pairs, u.shape), 0)
    rng = np.where(on, last_pair(uz) - first_pair(uz) + 1, 0)
    unit = np.where(on, 4 * ((last_pair(uz) >> 2) - (first_pair(uz) >> 2) + 1), 0)   # units of four pairs: what kde_screen_d8_dense_kernel walks
    # (a non-empty quarter of a partial batch holds no more pairs than the batch has left)
    quarters = sum(np.where(((u >> np.uint64(16 * k)) & np.uint64(0xFFFF)) != 0, np.clip(np.broadcast_to(batch_pairs, u.shape) - 8 * k, 0, 8), 0)
                   for k in range(4))
    return {name: (int((loads * served).sum()), int(loads.sum()))
            for name, loads in (("listed pairs (the ring)", cur), ("all pairs of the batch", full), ("first to last set pair", rng), ("first to last set unit", unit), ("non-empty quarters", quarters))}


print("  forms of the screen: MFMAs and operand bytes a step (1 KiB per fragment load); NW = sweep waves served by one screen wave")
on1 = (u1 != 0).astype(np.int64)
res = {1: forms(u1, on1)}
pad = u1 if nw % 2 == 0 else np.concatenate([u1, np.zeros((1,) + u1.shape[1:], dtype=u1.dtype)])
pad = pad.reshape(-1, 2, nsplit, bps)
res[2] = forms(pad[:, 0] | pad[:, 1], (pad != 0).sum(axis=1).astype(np.int64))
for NW, r in res.items():
    for name, (mf, ld) in r.items():
        note = "  (at NW = 2 the pairs of either wave's list, each MFMA'd once per wave in reach: an upper bound of a joint list)" if NW == 2 and name.startswith("listed") else ""
        print(f"    NW = {NW}  {name:26s} {mf:12d} MFMAs  {ld:12d} loads  {ld * 1024 / 1e9:8.2f} GB{note}")
both = int(((pad != 0).sum(axis=1) == 2).sum())
print(f"    NW = 2: batches in reach of both served waves {both}, of one only {int(((pad != 0).sum(axis=1) == 1).sum())}")
uz = u1[u1 != 0]
print(f"    batches in reach whose first set bit is odd {float((popcount((uz & (~uz + np.uint64(1))) - np.uint64(1)) & 1).mean()):.3f}, "
      f"whose last set bit is even {float(((popcount(smear(uz)) - 1) & 1 == 0).mean()):.3f}; with an empty 16-tile quarter "
      f"{float((sum(((uz >> np.uint64(16 * k)) & np.uint64(0xFFFF)) == 0 for k in range(4)) > 0).mean()):.3f}")
