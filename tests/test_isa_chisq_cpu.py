"""CPU tier (cross-compile only): ISA invariants of the batched joint-count kernel of ChiSquare (csrc/chisq.hip).

The kernel is latency-bound on its code loads and on LDS adds: what hides both is eight waves per SIMD, which needs at most 64 VGPRs
and no scratch memory, and LDS adds that return nothing (a returning add makes the wave wait for a value nobody reads).  None of that
changes a result, so no numerical test would notice its loss.  Everything but the last check is read from the kernel descriptors."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybnesian_amd", "csrc")


@pytest.fixture(scope="module")
def count_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "chisq.s"
    p = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "chisq.hip", "-o", str(out)], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out.read_text()


def test_both_code_widths_keep_eight_waves_and_add_without_return(count_asm):
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*chisq_count_kernelI[a-z]E\S*)\n(.*?)\.end_amdhsa_kernel", count_asm, flags=re.S))
    widths = sorted(re.search(r"chisq_count_kernelI([a-z])E", name).group(1) for name in headers)
    assert widths == ["h", "i"]                      # unsigned char (the byte mirror) and int (codes as uploaded)
    for name, hdr in headers.items():
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 64, name      # eight waves per SIMD
        body = re.search(r"\n%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), count_asm, flags=re.S).group(1)
        assert "ds_add_u32" in body, name
        assert "ds_add_rtn_u32" not in body, f"{name}: an LDS add waits for its old value"
