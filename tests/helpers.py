"""Shared helpers for the parity tests (data frames from the golden arrays, tolerances) and for the ISA tests (a unit's gfx950 listing)."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pandas as pd

COLS = ["a", "b", "c", "d"]
VARSETS = [["a"], ["b", "a"], ["c", "a", "b"], ["d", "a", "b", "c"]]
CKDE_SETS = [("a", []), ("b", ["a"]), ("c", ["a", "b"]), ("d", ["a", "b", "c"])]

# BASELINE.json north_star: slogl within 1e-6 relative (fp64) / 1e-3 (fp32)
RTOL_F64 = 1e-6
RTOL_F32 = 1e-3


def frame(arr, dtype=None):
    df = pd.DataFrame(np.asarray(arr), columns=COLS)
    return df.astype(dtype) if dtype else df


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pybnesian_amd", "csrc")
# the units csrc/Makefile builds with -fno-slp-vectorize (its KDE_UNITS)
KDE_UNITS = ("kde_kernels", "kde_moment", "kde_prepass", "kde_cdf", "kde_finish")


@functools.lru_cache(maxsize=None)
def unit_asm(unit):
    """The gfx950 assembly of pybnesian_amd/csrc/<unit>.hip, compiled with the Makefile's flags (cross-compile: no GPU needed); once per process."""
    extra = ["-fno-slp-vectorize"] if unit in KDE_UNITS else []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        p = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", *extra, "-S", "--cuda-device-only",
                            unit + ".hip", "-o", out], cwd=CSRC, capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        with open(out) as f:
            return f.read()
