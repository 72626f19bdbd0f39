"""CPU tier: the plan of the one-pass Gaussian network evaluation (pybnesian_amd/gaussian_model.py - pure Python), its switch, and
the resource figures of gnet_logl_kernel (csrc/gaussian_model.hip) read from the kernel descriptors of a cross-compile.

The kernel is a streaming loop with next to no arithmetic: what hides its load latency is eight waves per SIMD, which needs at most
64 VGPRs and no scratch memory.  Losing that changes no result, so no numerical test would notice."""
import re

import pytest
from helpers import unit_asm

from pybnesian_amd import gaussian_model as gm


def test_plan_numbers_columns_by_first_use():
    plan = gm.build_plan([("b", ["a", "z"]), ("a", []), ("c", ["b"])])
    assert plan.columns == ["b", "a", "z", "c"]
    assert plan.var == [0, 1, 3]                      # node order differs from column order
    assert plan.par_off == [0, 2, 2, 3]
    assert plan.parents == [1, 2, 0]                  # evidence in the factor's order, not sorted
    assert plan.within_caps


def test_plan_interface_columns_have_no_node():
    plan = gm.build_plan([("x_t_0", ["x_t_1", "y_t_1"]), ("y_t_0", ["x_t_0", "y_t_2"])])
    assert plan.columns == ["x_t_0", "x_t_1", "y_t_1", "y_t_0", "y_t_2"]
    assert plan.var == [0, 3]
    assert sorted(set(range(len(plan.columns))) - set(plan.var)) == [1, 2, 4]
    assert plan.parents == [1, 2, 0, 4]


def test_plan_coefficient_offsets():
    fams = [("a", []), ("b", ["a"]), ("c", ["a", "b"]), ("d", []), ("e", ["d", "c", "a"])]
    plan = gm.build_plan(fams)
    # node i's p_i + 1 coefficients start at par_off[i] + i: the concatenation of the factors' betas
    assert plan.beta_off == [0, 1, 3, 6, 7]
    assert plan.beta_off == [plan.par_off[i] + i for i in range(len(fams))]
    sizes = [len(ev) + 1 for _, ev in fams]
    assert [sum(sizes[:i]) for i in range(len(fams))] == plan.beta_off


def test_plan_family_cap():
    ok = gm.build_plan([("y", [f"x{i}" for i in range(63)])])
    assert ok.within_caps and len(ok.columns) == 64
    wide = gm.build_plan([("a", []), ("y", [f"x{i}" for i in range(64)])])
    assert not wide.within_caps                       # 65 columns in one family: beyond pbn_lg_logl's cap


def test_enabled_follows_the_environment_per_call(monkeypatch):
    monkeypatch.delenv("PBN_GAUSSIAN_MODEL", raising=False)
    assert gm.enabled()
    monkeypatch.setenv("PBN_GAUSSIAN_MODEL", "0")
    assert not gm.enabled()
    monkeypatch.setenv("PBN_GAUSSIAN_MODEL", "1")
    assert gm.enabled()


@pytest.fixture(scope="module")
def gnet_asm():
    return unit_asm("gaussian_model")


def test_every_instantiation_keeps_eight_waves_and_no_scratch(gnet_asm):
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*gnet_logl_kernelI[a-z]Lb[01]E\S*)\n(.*?)\.end_amdhsa_kernel", gnet_asm, flags=re.S))
    kinds = sorted(re.search(r"gnet_logl_kernelI([a-z])Lb([01])E", name).groups() for name in headers)
    assert kinds == [("d", "0"), ("d", "1"), ("f", "0"), ("f", "1")]     # double / float x per-row sums / per-node block sums
    for name, hdr in headers.items():
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= 64, name      # eight waves per SIMD
