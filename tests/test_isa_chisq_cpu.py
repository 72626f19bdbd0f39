"""CPU tier (cross-compile only): ISA invariants of the joint-count kernel (csrc/joint_counts.hip) that counts ChiSquare's contingency
tables and the family tables of the score engine, and the unit's plain-C++ half under the host sanitizers.

The kernel is latency-bound on its code loads and on LDS adds: what hides both is eight waves per SIMD, which needs at most 64 VGPRs
and no scratch memory, and LDS adds that return nothing (a returning add makes the wave wait for a value nobody reads).  None of that
changes a result, so no numerical test would notice its loss.  Everything but the last check is read from the kernel descriptors."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pybnesian_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# joint_count_kernel<CodeT, LDS, POLICY> as the Itanium ABI spells it: code type h (unsigned char: the byte mirror) or i (int: the codes as
# uploaded), the LDS flag as Lb0 / Lb1, the policy as its enumerator's value (0 NONE, 1 BY_CARD)
INSTANCE = r"joint_count_kernelI([hi])Lb([01])ELNS\d+_6PolicyE([01])E"


@pytest.fixture(scope="module")
def count_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "joint_counts.s"
    p = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only",
                        "joint_counts.hip", "-o", str(out)], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return out.read_text()


def test_both_code_widths_keep_eight_waves_and_add_without_return(count_asm):
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*joint_count_kernel\S*)\n(.*?)\.end_amdhsa_kernel", count_asm, flags=re.S))
    found = set()
    for name, hdr in headers.items():
        inst = re.search(INSTANCE, name)
        assert inst, name
        width, lds, policy = inst.groups()
        found.add((width, lds, policy))
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 64, name      # eight waves per SIMD
        if lds == "1":
            body = re.search(r"\n%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), count_asm, flags=re.S).group(1)
            assert "ds_add_u32" in body, name
            assert "ds_add_rtn_u32" not in body, f"{name}: an LDS add waits for its old value"
    assert len(found) == len(headers)
    # both code widths of each policy in use, in the LDS form (ChiSquare, small families) and the global form (large families)
    assert found == {(w, l, p) for w in "hi" for l in "01" for p in "01"}


def test_host_half_under_the_sanitizers(tmp_path):
    """tests/c/joint_counts_host_main.cpp: the slice planner against the rule as test_chisq_batch_gpu.py's slicing() states it, regions
    that start on any row, and copies_for, as a stand-alone program compiled with -fsanitize=address,undefined; it runs on the CPU."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    exe = tmp_path / "joint_counts_host_main"
    p = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "-x", "c++", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + CSRC, os.path.join(ROOT, "tests", "c", "joint_counts_host_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout[-500:], r.stderr[-2000:])
