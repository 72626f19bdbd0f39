"""CPU tier (cross-compile only): ISA invariants of LinearCorrelation's batch over tables with nulls (csrc/lincor_null_batch.hip), and
its plain-C++ host half under the sanitizers.

lincor_null_moments_kernel<T, M> keeps 1 + M + M (M + 1) / 2 fp64 accumulators per lane (45 at M = 8) and lincor_null_finish_kernel<M>
the block and two eigenvector rows, all indexed by compile-time constants: one dynamic index and they move to scratch memory - correct
results at a fraction of the speed, and no other test would say so.  The arithmetic is fp64 on the vector ALU for float32 tables too
(the values are converted on the way out of LDS); a matrix-unit or single-precision rewrite would change the rounding the band of
pbn_mi_lincor_band() is measured against.

VGPR bound: the design claims three waves per SIMD for the moments kernels at every M - 512 registers / 3 = 170, in
allocation granules of 8 -> at most 168; the compiler's own report gives 152 for the widest (float32, M = 8).  The finish kernel runs
once per test, not once per (test, row): it only has to stay out of scratch memory (512 registers, one wave per SIMD)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybnesian_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "lincor_null_batch.s"
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only", "lincor_null_batch.hip", "-o", str(out)],
                       cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out.read_text()


def kernels(asm, pattern):
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*%s\S*)\n(.*?)\.end_amdhsa_kernel" % pattern, asm, flags=re.S))
    return {name: (hdr, re.search(r"\n%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), asm, flags=re.S).group(1)) for name, hdr in headers.items()}


def field(hdr, name):
    return int(re.search(r"%s (\d+)" % name, hdr).group(1))


def check_per_test_kernel(name, hdr, body, vgpr_max):
    assert field(hdr, "private_segment_fixed_size") == 0, name
    assert field(hdr, "next_free_vgpr") <= vgpr_max, (name, field(hdr, "next_free_vgpr"))
    assert re.search(r"uses_dynamic_stack 0|dynamic_stack\s+0", hdr) or "dynamic_stack" not in hdr, name
    assert "scratch_" not in body, f"{name}: a per-lane array went to scratch memory"
    assert "s_swappc" not in body, f"{name}: a call left in the kernel"
    assert re.search(r"\bv_fmac?_f64", body), name      # (v_fmac_f64 is the accumulate-in-place encoding of the same fused operation)
    assert "v_mfma" not in body, name
    assert not re.search(r"\bv_(pk_)?(fma|mul|add|sub|mac|fmac)_f32\b", body), f"{name}: single-precision arithmetic"


def test_moments_kernels_live_in_registers(ensure_built, asm):
    from pybnesian_amd import _lib

    k_dev = _lib.load().pbn_lincor_batch_max_cond()
    ks = kernels(asm, r"lincor_null_moments_kernelI[df]Li\d+E")
    for t in "df":      # float64 and float32 tables: one specialisation per M = 2 ... K_DEV + 2 each
        sizes = sorted(int(re.search(r"kernelI%sLi(\d+)E" % t, n).group(1)) for n in ks if "kernelI%sLi" % t in n)
        assert sizes == list(range(2, k_dev + 3)), (t, sizes)
    assert len(ks) == 2 * (k_dev + 1)
    for name, (hdr, body) in ks.items():
        check_per_test_kernel(name, hdr, body, 168)     # three waves per SIMD
        assert field(hdr, "group_segment_fixed_size") == 0, name      # the tile is dynamic LDS, sized by the handle's columns
        assert "ds_read" in body or "ds_load" in body, f"{name}: the rows are not read from LDS"
        assert "atomic" not in body, f"{name}: an atomic in the order of additions"


def test_finish_kernels_live_in_registers(ensure_built, asm):
    from pybnesian_amd import _lib

    k_dev = _lib.load().pbn_lincor_batch_max_cond()
    ks = kernels(asm, r"lincor_null_finish_kernelILi\d+E")
    sizes = sorted(int(re.search(r"kernelILi(\d+)E", n).group(1)) for n in ks)
    assert sizes == list(range(2, k_dev + 3))
    for name, (hdr, body) in ks.items():
        check_per_test_kernel(name, hdr, body, 512)
        assert field(hdr, "group_segment_fixed_size") == 0, name
        assert "atomic" not in body, name


def test_tile_fits_the_lds_of_a_cu_four_times(ensure_built):
    """The dynamic LDS of a moments workgroup is TILE rows of all columns, at most of the column cap in doubles (the constants of
    csrc/lincor_null_host.hpp, read from the file: no device is needed)."""
    src = open(os.path.join(CSRC, "lincor_null_host.hpp")).read()
    tile = int(re.search(r"constexpr int TILE = (\d+);", src).group(1))
    cap = int(re.search(r"constexpr int NC_MAX = (\d+);", src).group(1))
    assert 4 * tile * cap * 8 <= LDS_PER_CU
    assert tile * cap * 8 <= 64 * 1024      # one workgroup's own limit


def test_host_half_under_the_sanitizers(tmp_path):
    """tests/c/lincor_null_host_main.cpp: the row partition (no dirty row, one, all), the slices, the grouping and the launch chunking
    as a stand-alone program compiled with -fsanitize=address,undefined; it runs on the CPU."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "lincor_null_host_main"
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "c", "lincor_null_host_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-500:], r.stderr[-2000:])
