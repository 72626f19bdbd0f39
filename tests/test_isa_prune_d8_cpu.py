"""CPU tier (cross-compile only): the listing of the pruned sum-only d = 8 sweep - bench.py's headline kernel.

kde_sweep_pruned_d8_kernel (KS = 2, QG = 2, norms as weights, pruned, sum-only, eight box dimensions) spends its time in three places, and each has a form that the
source asks for but only the listing shows (profiles/r9/):
  * the (tile, group) bodies: a BLIND loop (the weighted FMA chain runs into the running sum: no compare of a tile sum, no branch on it), of
    which the batches proven by batch_bare_wmul take exp2_magic WITHOUT its clamp, and the checked loop as the redo path;
  * the box tests of the walk: ONE round trip each - all box words of a test are requested before the first wait for any of them (with a
    run-time number of box dimensions every dimension was a basic block of its own with its own loads and waits: eight dependent trips);
  * its registers: three waves per SIMD, nothing in scratch, the 64-bit visit masks in scalar registers.
Every assertion below fails on the source before round 9 (no blind loop for this shape, eight wait-separated load groups per test)."""
import re

import pytest

from helpers import unit_asm

# What launch_sweep_tf starts for the d = 8 sum-only sweep: kde_sweep_pruned_d8_kernel (the box dimensions at compile time) where the source has
# it, else kde_sweep_kernel<double, 2, COND = false, QG = 2, FOLD = false, PRUNE = true, WMUL = true, EF32 = true>
HEADLINE = ("_ZN3pbn26kde_sweep_pruned_d8_kernelENS_9SweepArgsE", "_ZN3pbn16kde_sweep_kernelIdLi2ELb0ELi2ELb0ELb1ELb1ELb1EEEvNS_9SweepArgsE")


@pytest.fixture(scope="module")
def kde_asm():
    return unit_asm("kde_kernels")   # the unit that holds the fp64 sweeps


def headline(asm):
    """(name, resource header, basic blocks) of the headline kernel."""
    names = [n for n in HEADLINE if ".amdhsa_kernel %s\n" % n in asm]
    assert names, "the pruned sum-only d = 8 sweep is not instantiated"
    name = names[0]
    hdr = re.search(r"\.amdhsa_kernel %s\n(.*?)\.end_amdhsa_kernel" % re.escape(name), asm, flags=re.S).group(1)
    body = next(f for f in re.split(r"\n(?=_Z[A-Za-z0-9_]+:)", asm) if f.startswith(name + ":")).split(".Lfunc_end")[0]
    return name, hdr, re.split(r"\n(?=\.LBB\d+_\d+:)", body)


def pair_bodies(blocks):
    """The basic blocks that hold one (tile, group) body: the shape's two MFMAs and the four 2^x of exp2_magic."""
    return [b for b in blocks if len(re.findall(r"\bv_mfma_f64", b)) == 2 and len(re.findall(r"\bv_exp_f32", b)) == 4 and "v_alignbit_b32" in b]


def test_headline_sweep_keeps_three_waves_and_no_scratch(kde_asm):
    """Keys on the kernel's resource header and on the whole function: 168 VGPRs is the cap of the three waves per SIMD its launch bounds ask for;
    and on the blind loop being there at all - before round 9 the register count was met by NOT having it."""
    name, hdr, blocks = headline(kde_asm)
    assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
    assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 168, name
    assert not any("scratch_" in b for b in blocks), name
    assert [b for b in pair_bodies(blocks) if not re.search(r"\bv_cmp_\w+_f64", b)], f"{name}: fits its registers without a blind loop"


def test_headline_sweep_has_blind_bare_and_checked_bodies(kde_asm):
    """Keys on what follows the MFMAs of a (tile, group) body.  Checked: v_cmp_*_f64 of the tile sum against 2^900 and a branch on it.  Blind: four
    FMAs (weight x 2^x into the running sum), no fp64 compare in the block.  Bare: blind and no v_med3_i32 (the clamp of exp2_magic).  The visit
    masks are tested with scalar instructions in all of them (v_cmp_ne_u64 = masks in vector registers: profiles/r6/magic_exp2.txt, -25 %)."""
    name, _, blocks = headline(kde_asm)
    bodies = pair_bodies(blocks)
    checked = [b for b in bodies if re.search(r"\bv_cmp_\w+_f64", b)]
    blind = [b for b in bodies if not re.search(r"\bv_cmp_\w+_f64", b)]
    bare = [b for b in blind if "v_med3_i32" not in b]
    clamped = [b for b in blind if "v_med3_i32" in b]
    # run_batch holds four bodies (two fragment buffers x the first / a later group of the tile)
    assert len(checked) >= 4 and len(clamped) >= 4 and len(bare) >= 4, (name, len(checked), len(clamped), len(bare))
    for b in bodies:
        assert "Loop" in "\n".join(b.split("\n")[:3]), name
        assert "v_cmp_ne_u64" not in b and "scratch_" not in b, name
    for b in blind:
        assert len(re.findall(r"\bv_fmac_f64|\bv_fma_f64", b)) == 4 and not re.search(r"\bv_add_f64", b), name   # the chain runs into the sum
    for b in checked:
        assert len(re.findall(r"\bv_med3_i32", b)) == 4, name   # the redo path keeps the clamp
    for b in clamped:
        assert len(re.findall(r"\bv_med3_i32", b)) == 4, name


def test_headline_sweep_box_tests_take_one_round_trip(kde_asm):
    """Keys on the box tests' basic blocks: no MFMA, an fp64 compare (the ballot's), and the 2 x 8 doubles of a tile's or a batch's box as eight
    global_load_dwordx4.  Between the first and the last of these loads there is no s_waitcnt on vmcnt - the test waits once.  (The groups' own boxes
    and thresholds come from LDS: they count on lgkmcnt.)  Seven tests: batch_in_reach and batch_bare_wmul per group, prune_group_mask per group,
    prune_group_masks_joint."""
    name, _, blocks = headline(kde_asm)
    tests = [b for b in blocks if "v_mfma" not in b and re.search(r"\bv_cmp_\w+_f64", b) and len(re.findall(r"\bglobal_load_dwordx4", b)) >= 8]
    assert len(tests) >= 7, (name, len(tests))
    for b in tests:
        lines = b.split("\n")
        loads = [i for i, l in enumerate(lines) if re.search(r"\bglobal_load_dword", l)]
        between = lines[loads[0]:loads[-1]]
        assert not [l for l in between if re.search(r"s_waitcnt[^\n]*vmcnt", l)], (name, lines[0])
        assert len(loads) <= 9, (name, lines[0], len(loads))   # the box, at most one word more: the groups' sides are not vector-memory loads
