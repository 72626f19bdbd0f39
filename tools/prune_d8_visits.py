"""Visited (tile, group) fraction of the C2 sweep on the GPU (PBN_SWEEP_COUNT_REDO=1): bench.py's table and model, one slogl.
Compare with the realistic variant of tools/prune_d8_estimate.py.  python tools/prune_d8_visits.py"""
import ctypes as C
import os
import sys

os.environ["PBN_SWEEP_COUNT_REDO"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import pybnesian_amd as pbn  # noqa: E402
from pybnesian_amd import _lib  # noqa: E402

lib = _lib.load()
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
lib.pbn_debug_sweep_visits(None, None, 1)
kde.slogl_table_async(test, out.data_ptr())
ctx.sync()
v, t = C.c_ulonglong(0), C.c_ulonglong(0)
lib.pbn_debug_sweep_visits(C.byref(v), C.byref(t), 0)
print(f"C2 slogl {out.item():.10f}: (tile, group) blocks visited {v.value} of {t.value} offered = {v.value / max(t.value, 1):.4f}")
