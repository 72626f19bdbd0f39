"""CPU tier: the gfx950 listing of the d = 8 f16 screen's two kernels (csrc/kde_screen_d8.inc), cross-compiled with the Makefile's flags.

kde_screen_d8_kernel keeps PBN_SCREEN_RING fragment loads in flight through its MFMA loop.  That is a property of what the compiler made of the
source, not of the source: the serial kernel's prefetch was written out too and was rotated away, every MFMA behind `s_waitcnt vmcnt(0)`.  So the
listing is held to it - the wait counts, the block maximum (8 v_maximum3_f32 per MFMA, no input quieted by `v_max_f32 x, y, y`) and the register
budget of four waves per SIMD.  Only those: nothing here looks at other instructions."""
import os
import re

import pytest

from helpers import CSRC, unit_asm

STREAM = "_ZN3pbn20kde_screen_d8_kernelENS_9SweepArgsE"
SERIAL = "_ZN3pbn27kde_screen_d8_serial_kernelENS_9SweepArgsE"
MFMA = "v_mfma_f32_32x32x16_f16"


@pytest.fixture(scope="module")
def kde_asm():
    return unit_asm("kde_kernels")


def ring_depth():
    """The default of the source, which is what unit_asm compiles; a build with -DPBN_SCREEN_RING=n is not what this file looks at."""
    with open(os.path.join(CSRC, "kde_screen_d8.inc")) as f:
        return int(re.search(r"^#define PBN_SCREEN_RING (\d+)", f.read(), flags=re.M).group(1))


def kernel(asm, name):
    hdr = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, flags=re.S).group(1)
    body = next(f for f in re.split(r"\n(?=_Z[A-Za-z0-9_]+:)", asm) if f.startswith(name + ":")).split(".Lfunc_end")[0]
    return hdr, body


def innermost_loops(body):
    """The instructions of every loop of a kernel's listing, by the label of the loop's header: the compiler marks each basic block with its
    innermost loop (`; in Loop: Header=BBn_m`) and a header with `Loop Header` on its own label, wherever it places the blocks."""
    loops, cur = {}, None
    for line in body.splitlines():
        m = re.match(r"\s*(?:\.L(BB\d+_\d+):|; %bb\.\d+:)\s*(?:;\s*(.*))?$", line)
        if m:
            label, note = m.group(1), m.group(2) or ""
            inside = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            cur = inside.group(1) if inside else label if ("Loop Header" in note or "Parent Loop" in note) else None
            continue
        if cur is not None and line.strip() and not line.strip().startswith(";"):
            loops.setdefault(cur, []).append(line.strip())
    return loops


def test_ring_loop_waits_with_counted_vmcnt(kde_asm):
    R = ring_depth()
    assert R >= 2
    hdr, body = kernel(kde_asm, STREAM)
    assert body.count(MFMA) == R, "the MFMAs of the kernel are the ring's slots"
    with_mfma = [ins for ins in innermost_loops(body).values() if any(MFMA in i for i in ins)]
    assert len(with_mfma) == 1, "one loop holds the MFMAs"
    loop = with_mfma[0]
    assert sum(MFMA in i for i in loop) == R
    waits = [int(n) for i in loop for n in re.findall(r"vmcnt\((\d+)\)", i)]
    print(f"ring {R}: {len(loop)} instructions a turn, vmcnt waits {waits}")
    assert waits and all(n >= R - 1 and n != 0 for n in waits), waits
    assert sum(i.startswith("v_maximum3_f32") for i in loop) == 8 * R
    assert not [i for i in loop if re.match(r"v_max_f32\S* v\d+, (v\d+), \1$", i)], "no input of the maximum is quieted"


def test_register_budget(kde_asm):
    for name in (STREAM, SERIAL):
        hdr, body = kernel(kde_asm, name)
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 128, name   # four waves per SIMD
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0 and "scratch_" not in body, name


def test_serial_kernel_is_kept(kde_asm):
    hdr, body = kernel(kde_asm, SERIAL)
    assert MFMA in body
