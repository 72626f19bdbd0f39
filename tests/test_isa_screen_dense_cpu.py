"""CPU tier: the gfx950 listing of the d = 8 screen's dense kernel (kde_screen_d8_dense_kernel, csrc/kde_screen_d8.inc), cross-compiled
with the Makefile's flags.

The dense kernel exists because the ring's slot is long: what it must keep is a short MFMA loop whose loads stay in flight.  Held to the listing:
one innermost loop with the kernel's MFMAs, every vmcnt wait in it counted (non-zero), 8 v_maximum3_f32 per MFMA and no input quieted, the
registers of the occupancy it is launched for without scratch, and at most half the ring kernel's instructions per MFMA - the ring's own loop,
parsed from the same listing, is the yardstick.  Nothing here looks at other instructions."""
import os
import re

import pytest

from helpers import CSRC, unit_asm
from test_isa_screen_cpu import MFMA, STREAM, innermost_loops, kernel


def shipped_nw():
    """The default of the source, which is what unit_asm compiles."""
    with open(os.path.join(CSRC, "kde_screen_d8.inc")) as f:
        return int(re.search(r"^#define PBN_SCREEN_NW (\d+)", f.read(), flags=re.M).group(1))


def dense_name():
    name = "kde_screen_d8_dense_kernel"
    return "_ZN3pbn%d%sILi%dEEEvNS_9SweepArgsE" % (len(name), name, shipped_nw())


@pytest.fixture(scope="module")
def kde_asm():
    return unit_asm("kde_kernels")


def mfma_loop(asm, name):
    hdr, body = kernel(asm, name)
    with_mfma = [ins for ins in innermost_loops(body).values() if any(MFMA in i for i in ins)]
    assert len(with_mfma) == 1, f"{name}: one loop holds the MFMAs"
    assert sum(MFMA in i for i in with_mfma[0]) == body.count(MFMA), f"{name}: every MFMA of the kernel is in that loop"
    return hdr, body, with_mfma[0]


def test_dense_loop(kde_asm):
    hdr, body, loop = mfma_loop(kde_asm, dense_name())
    n = sum(MFMA in i for i in loop)
    waits = [int(v) for i in loop for v in re.findall(r"vmcnt\((\d+)\)", i)]
    print(f"dense NW = {shipped_nw()}: {len(loop)} instructions for {n} MFMAs ({len(loop) / n:.1f} per MFMA), vmcnt waits {waits}")
    assert waits and all(v != 0 for v in waits), waits
    assert sum(i.startswith("v_maximum3_f32") for i in loop) == 8 * n
    assert not [i for i in loop if re.match(r"v_max_f32\S* v\d+, (v\d+), \1$", i)], "no input of the maximum is quieted"


def test_dense_loop_is_half_the_rings(kde_asm):
    _, _, dense = mfma_loop(kde_asm, dense_name())
    _, _, ring = mfma_loop(kde_asm, STREAM)
    per_dense = len(dense) / sum(MFMA in i for i in dense)
    per_ring = len(ring) / sum(MFMA in i for i in ring)
    print(f"instructions per MFMA: dense {per_dense:.2f}, ring {per_ring:.2f}")
    assert per_dense <= 0.5 * per_ring, (per_dense, per_ring)


def test_register_budget(kde_asm):
    hdr, body = kernel(kde_asm, dense_name())
    with open(os.path.join(CSRC, "kde_screen_d8.inc")) as f:
        waves = int(re.search(r"^#define PBN_SCREEN_WAVES (\d+)", f.read(), flags=re.M).group(1))   # the kernel's launch bound
    assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 512 // waves, (hdr, waves)
    assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0 and "scratch_" not in body
