"""CPU tier (cross-compile only): ISA invariants of the batched LinearCorrelation kernel (csrc/lincor_batch.hip).

One test per lane means every lane keeps its (k+2) x (k+2) block and two rows of eigenvectors in registers.  That holds only while every
index into those per-lane arrays is a compile-time constant: one dynamic index, or one specialisation that outgrows the register file,
and the block moves to scratch memory - correct results, a fraction of the speed, and no test would say so.  The arithmetic must also
stay fp64 on the vector ALU: a matrix-unit or mixed-precision rewrite would change rounding, which the engine's re-evaluation band is
measured against."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybnesian_amd", "csrc")


@pytest.fixture(scope="module")
def batch_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "lincor_batch.s"
    p = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "lincor_batch.hip", "-o", str(out)], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out.read_text()


def test_every_specialisation_lives_in_registers(ensure_built, batch_asm):
    from pybnesian_amd import _lib

    k_dev = _lib.load().pbn_lincor_batch_max_cond()
    assert k_dev >= 6
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*lincor_batch_kernelILi\d+E\S*)\n(.*?)\.end_amdhsa_kernel", batch_asm, flags=re.S))
    sizes = sorted(int(re.search(r"lincor_batch_kernelILi(\d+)E", name).group(1)) for name in headers)
    assert sizes == list(range(2, k_dev + 3))          # one per k = 0 ... K_DEV, specialised on m = k + 2
    assert len(headers) == k_dev + 1
    for name, hdr in headers.items():
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 168, name      # at least three waves per SIMD
        assert re.search(r"uses_dynamic_stack 0|dynamic_stack\s+0", hdr) or "dynamic_stack" not in hdr, name
        body = re.search(r"\n%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), batch_asm, flags=re.S).group(1)
        assert "scratch_" not in body, f"{name}: a per-lane array went to scratch memory"
        assert "s_swappc" not in body, f"{name}: a call left in the kernel"
        assert "v_fma_f64" in body, name
        assert "v_mfma" not in body, name
        assert not re.search(r"\bv_(fma|mul|add)_f32\b", body), f"{name}: single-precision arithmetic"
