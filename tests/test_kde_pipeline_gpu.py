"""GPU tier: the front lanes of the handle evaluations (pbn_ctx::front, FrontStage in csrc/kde_model.hip).

Consecutive asynchronous evaluations on one context enqueue their query sides (keys, sort, pack, prepass, window pass) on two front lanes beside
the previous evaluation's sweep; what every kernel computes is untouched, so every result must be the serial one BIT FOR BIT.  The serial sequence
is the same calls with PBN_KDE_PIPELINE=0 and a synchronisation after every call.  Held here: eight back-to-back calls on tables of eight sizes (a
single partial tile, arena growth in the third and sixth call, each lane reused at k + 2, a changing number of splits) on a screened d = 8 handle,
a pruned d = 3 handle, a split CKDE handle and an unpruned handle (no lane); and the ordering against the other entry points: a refit, a test
table overwritten in place, two handles of one context in turn, blocking calls behind an asynchronous one, the capture aids, a destroyed context."""
import ctypes as C
import os

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

SIZES = (3_000, 1_000, 5_000, 17, 3_000, 9_000, 1, 2_500)
N_TRAIN = 40_000    # above the 32 768 rows from which the handles prune (PBN_PRUNE_MIN_ROWS)
NAMES = [f"v{i}" for i in range(8)]


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def table(n, seed):
    rng = np.random.default_rng(seed)
    mix = np.tril(np.full((8, 8), 0.3), -1) + np.eye(8)
    return pd.DataFrame(rng.normal(size=(n, 8)) @ mix.T, columns=NAMES)


@pytest.fixture(scope="module")
def pbn():
    import pybnesian_amd

    pybnesian_amd.load_library()
    return pybnesian_amd


@pytest.fixture(scope="module")
def lib():
    from pybnesian_amd import _lib

    L = _lib.load()
    L.pbn_debug_front_lanes.restype = None
    L.pbn_debug_front_lanes.argtypes = [C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.c_int]
    L.pbn_debug_far32_launches.restype = None
    L.pbn_debug_far32_launches.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    L.pbn_debug_prune_stages.restype = C.c_int64
    L.pbn_debug_prune_stages.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int]
    L.pbn_debug_d8_masks.restype = C.c_int64
    L.pbn_debug_d8_masks.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int]
    return L


def front_lanes(lib, reset=False):
    """(evaluations whose query side went to a front lane, those of them that did not wait for the context's stream) since the last reset"""
    e, c = C.c_ulonglong(), C.c_ulonglong()
    lib.pbn_debug_front_lanes(C.byref(e), C.byref(c), 1 if reset else 0)
    return e.value, c.value


def far_launches(lib, reset=False):
    n = C.c_ulonglong()
    lib.pbn_debug_far32_launches(C.byref(n), 1 if reset else 0)
    return n.value


@pytest.fixture(scope="module")
def world(pbn):
    """One context: the training table, the eight test tables, and the four handles, fitted once."""
    from pybnesian_amd.dataset import DeviceTable, default_context

    ctx = default_context()
    train = table(N_TRAIN, 11)
    train_t, _ = DeviceTable.from_dataframe(ctx, train, NAMES)
    small_t, _ = DeviceTable.from_dataframe(ctx, train.iloc[:5_000], NAMES)
    tests = [DeviceTable.from_dataframe(ctx, table(n, 100 + i), NAMES)[0] for i, n in enumerate(SIZES)]
    d8 = pbn.ProductKDE(NAMES)
    d8.fit_table(train_t)
    d3 = pbn.KDE(NAMES[:3])
    d3.fit_table(train_t)
    ckde = pbn.CKDE("v0", ["v1", "v2"])
    ckde.fit_table(train_t)
    small = pbn.ProductKDE(NAMES)
    small.fit_table(small_t)
    return dict(ctx=ctx, train=train_t, tests=tests, d8=d8, d3=d3, ckde=ckde, small=small)


def enqueue(k, t, out_ptr):
    """pbn_kde_slogl_async of any fitted handle (KDE, ProductKDE, CKDE) on all rows of a device table"""
    from pybnesian_amd import _lib

    _lib.check(_lib.load().pbn_kde_slogl_async(k._handle, t.handle, _lib.int_array(t.index(k._variables)), 0, t.num_rows, C.c_void_p(out_ptr)))


def run(ctx, calls, piped):
    """calls: (handle, table) pairs.  piped: back to back with one synchronisation at the end; else the serial sequence."""
    import torch

    out = torch.zeros(len(calls), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with env(PBN_KDE_PIPELINE="1" if piped else "0"):
        for i, (k, t) in enumerate(calls):
            enqueue(k, t, out.data_ptr() + 8 * i)
            if not piped:
                ctx.sync()
        ctx.sync()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def serial(world):
    """The serial sums of the eight tables, per handle kind; computed once."""
    done = {}

    def get(kind):
        if kind not in done:
            done[kind] = run(world["ctx"], [(world[kind], t) for t in world["tests"]], piped=False)
        return done[kind]

    return get


@pytest.mark.parametrize("kind", ["d8", "d3", "ckde", "small"])
def test_back_to_back_is_the_serial_sequence(lib, world, serial, kind):
    want = serial(kind)
    assert np.all(np.isfinite(want))
    front_lanes(lib, reset=True)
    far_launches(lib, reset=True)
    got = run(world["ctx"], [(world[kind], t) for t in world["tests"]], piped=True)
    evals, chained = front_lanes(lib)
    print(kind, "front-lane evaluations", evals, "chained", chained, "sums", got.tolist())
    if kind == "d8":
        assert far_launches(lib) == len(SIZES), "every call took the pruned, screened path with its far pass"
        assert (evals, chained) == (8, 7)
    elif kind == "d3":
        assert (evals, chained) == (8, 7)
    elif kind == "ckde":
        assert (evals, chained) == (16, 15), "joint and marginal sweep of every call, one lane each"
    else:
        assert evals == 0, "an unpruned evaluation has no front stage"
    assert np.array_equal(got, want), (got - want).tolist()
    front_lanes(lib, reset=True)
    off = run(world["ctx"], [(world[kind], t) for t in world["tests"][:2]], piped=False)
    assert front_lanes(lib)[0] == 0 and np.array_equal(off, want[:2]), "PBN_KDE_PIPELINE=0: no lane"


def test_a_refit_between_two_calls(pbn, world):
    from pybnesian_amd.dataset import DeviceTable

    ctx, t = world["ctx"], world["tests"][0]
    train2, _ = DeviceTable.from_dataframe(ctx, table(N_TRAIN, 12) * 1.25, NAMES)

    def sequence(piped):
        import torch

        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        k = pbn.ProductKDE(NAMES)
        k.fit_table(world["train"])
        with env(PBN_KDE_PIPELINE="1" if piped else "0"):
            enqueue(k, t, out.data_ptr())
            if not piped:
                ctx.sync()
            k.fit_table(train2)
            enqueue(k, t, out.data_ptr() + 8)
            ctx.sync()
        return out.cpu().numpy()

    want, got = sequence(False), sequence(True)
    assert want[0] != want[1] and np.array_equal(got, want), (got, want)


def test_a_test_table_overwritten_in_place(lib, world):
    import torch

    from pybnesian_amd import _lib
    from pybnesian_amd.dataset import DeviceTable

    ctx, k, n = world["ctx"], world["d8"], 3_000
    a = torch.tensor(table(n, 21).to_numpy().T.copy(), dtype=torch.float64, device="cuda")   # [8][n]: column c at base + c n
    b = torch.tensor(table(n, 22).to_numpy().T.copy(), dtype=torch.float64, device="cuda")

    def sequence(piped):
        buf = a.clone()
        out = torch.zeros(2, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        t = DeviceTable.from_device_pointer(ctx, buf.data_ptr(), n, NAMES, n, _lib.PBN_F64, keepalive=buf)
        with env(PBN_KDE_PIPELINE="1" if piped else "0"):
            enqueue(k, t, out.data_ptr())
            ctx.sync()                      # the writer waits for the readers ...
            buf.copy_(b)
            torch.cuda.synchronize()        # ... and the next reader for the writer
            enqueue(k, t, out.data_ptr() + 8)
            ctx.sync()
        return out.cpu().numpy()

    want, got = sequence(False), sequence(True)
    assert want[0] != want[1] and np.array_equal(got, want), (got, want)


def test_two_handles_in_turn(lib, world):
    calls = [(world["d8" if i % 2 == 0 else "d3"], world["tests"][i]) for i in range(6)]
    want = run(world["ctx"], calls, piped=False)
    front_lanes(lib, reset=True)
    got = run(world["ctx"], calls, piped=True)
    assert front_lanes(lib) == (6, 5)
    assert np.array_equal(got, want), (got, want)


def test_blocking_calls_behind_an_asynchronous_one(world):
    import torch

    ctx, k, (t0, t1) = world["ctx"], world["d8"], world["tests"][:2]

    def sequence(piped):
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        with env(PBN_KDE_PIPELINE="1" if piped else "0"):
            enqueue(k, t0, out.data_ptr())
            if not piped:
                ctx.sync()
            s = k.slogl_table(t1)
            enqueue(k, t0, out.data_ptr())
            if not piped:
                ctx.sync()
            rows = k.logl_table(t1)
            ctx.sync()
        return out.cpu().numpy(), s, rows

    (wa, ws, wr), (ga, gs, gr) = sequence(False), sequence(True)
    assert np.array_equal(ga, wa) and gs == ws and np.array_equal(gr, wr)


STAGE_ITEMS = ((0, np.int64), (1, np.float64), (4, np.float64), (5, np.uint32), (6, np.uint32), (7, np.int32), (8, np.float64), (9, np.float64),
               (10, np.float64), (11, np.float64), (12, np.int64), (13, np.float64), (14, np.float64))


def stage_records(lib):
    """Everything the last captured evaluation left (pbn_debug_prune_stages, side 1), bit patterns"""
    rec = []
    for what, dtype in STAGE_ITEMS:
        n = lib.pbn_debug_prune_stages(1, 0, what, None, 0, -1)
        assert n >= 0, what
        a = np.zeros(max(int(n), 1), dtype=dtype)
        assert lib.pbn_debug_prune_stages(1, 0, what, a.ctypes.data, n, -1) == n
        rec.append(a[:n].tobytes())
    return rec


def mask_records(lib):
    rec = []
    for what, dtype in ((0, np.int64), (1, np.uint64), (2, np.uint64), (6, np.float64), (7, np.uint64), (8, np.float64)):
        n = lib.pbn_debug_d8_masks(what, None, 0, 1)
        a = np.zeros(max(int(n), 1), dtype=dtype)
        lib.pbn_debug_d8_masks(what, a.ctypes.data, n, 1)
        rec.append(a[:n].tobytes())
    return rec


def test_capture_aids_between_two_calls(lib, world):
    """An armed aid synchronises and reads scratch: the armed evaluation stays on the context's stream, behind the call before it, and
    captures what a serial call's does; the calls around it keep their sums."""
    import torch

    ctx, k, (t0, t1, t2) = world["ctx"], world["d8"], world["tests"][:3]

    def sequence(piped):
        out = torch.zeros(5, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        caps = []
        with env(PBN_KDE_PIPELINE="1" if piped else "0"):
            try:
                enqueue(k, t0, out.data_ptr())
                if not piped:
                    ctx.sync()
                lib.pbn_debug_prune_stages(0, 0, -1, None, 0, 0)
                lib.pbn_debug_prune_stages(0, 0, -1, None, 0, 1)      # armed
                enqueue(k, t1, out.data_ptr() + 8)
                caps.append(stage_records(lib))
                lib.pbn_debug_prune_stages(0, 0, -1, None, 0, 0)      # disarmed, records forgotten
                enqueue(k, t2, out.data_ptr() + 16)
                if not piped:
                    ctx.sync()
                lib.pbn_debug_d8_masks(0, None, 0, 1)                 # armed
                enqueue(k, t1, out.data_ptr() + 24)
                caps.append(mask_records(lib))
                lib.pbn_debug_d8_masks(0, None, 0, 0)
                enqueue(k, t0, out.data_ptr() + 32)
                ctx.sync()
            finally:
                lib.pbn_debug_prune_stages(0, 0, -1, None, 0, 0)
                lib.pbn_debug_d8_masks(0, None, 0, 0)
        return out.cpu().numpy(), caps

    front_lanes(lib, reset=True)
    (want, wcaps) = sequence(False)
    assert front_lanes(lib)[0] == 0
    (got, gcaps) = sequence(True)
    assert front_lanes(lib)[0] == 3, "the three unarmed calls; the armed ones stay on the context's stream"
    assert np.array_equal(got, want), (got, want)
    assert all(len(b) for b in wcaps[0][:4]) and len(wcaps[1][1]) > 0, "the serial call captured something"
    assert gcaps[0] == wcaps[0], "pbn_debug_prune_stages: the armed call's records"
    assert gcaps[1] == wcaps[1], "pbn_debug_d8_masks: the armed call's masks and partial rows"


def test_a_context_destroyed_behind_its_synchronisation(pbn, world, serial):
    import gc

    from pybnesian_amd.dataset import Context, DeviceTable

    want = serial("d8")[:4]
    ctx = Context(0)
    train_t, _ = DeviceTable.from_dataframe(ctx, table(N_TRAIN, 11), NAMES)
    tests = [DeviceTable.from_dataframe(ctx, table(n, 100 + i), NAMES)[0] for i, n in enumerate(SIZES[:4])]
    k = pbn.ProductKDE(NAMES)
    k.fit_table(train_t)
    got = run(ctx, [(k, t) for t in tests], piped=True)
    del k, tests, train_t, ctx      # handles first or last: the context goes with its last reference, its front lanes with it
    gc.collect()
    assert np.array_equal(got, want), (got, want)
    # the default context still works after another one's lanes are gone
    again = run(world["ctx"], [(world["d8"], t) for t in world["tests"][:4]], piped=True)
    assert np.array_equal(again, want)
