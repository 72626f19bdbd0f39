"""CPU tier: the plan of the one-pass CLG network evaluation (pybnesian_amd/clg_model.py - pure Python), its switch, and the resource
figures of clgnet_logl_kernel (csrc/clg_model.hip) read from the kernel descriptors of a cross-compile.

The kernel is a streaming loop with next to no arithmetic: waves in flight hide its load latency.  Scratch memory or a fall in the
waves per SIMD changes no result, so no numerical test would notice."""
import re

import numpy as np
import pytest
from helpers import unit_asm

from pybnesian_amd import clg_model as cm


def test_plan_numbers_both_column_kinds_by_first_use():
    cards = {"A": 2, "B": 3, "C": 4}
    fams = [("y", ["B", "A"], ["x", "w"]),      # CLG: discrete parents B, A; continuous parents x, w
            ("A", [], None),                    # discrete root
            ("x", [], []),                      # plain LG, no parents
            ("C", ["A", "B"], None),            # discrete child
            ("w", ["C"], ["x"])]
    plan = cm.build_plan(fams, cards)
    assert plan.dcolumns == ["B", "A", "C"] and plan.cardinality == [3, 2, 4]
    assert plan.ccolumns == ["y", "x", "w"]
    assert plan.kind == [cm.CLG, cm.DISCRETE, cm.CLG, cm.DISCRETE, cm.CLG]
    assert plan.var == [0, 1, 1, 2, 2]              # each in its own table's numbering
    assert plan.dpar_off == [0, 2, 2, 2, 4, 5] and plan.dparents == [0, 1, 1, 0, 2]     # the factor's order, not sorted
    assert plan.cpar_off == [0, 2, 2, 2, 2, 3] and plan.cparents == [1, 2, 1]
    assert plan.configs == [6, 2, 1, 24, 4]
    assert plan.cfg_off == [0, 6, 6, 7, 7, 11]      # discrete nodes carry no configuration marks
    assert plan.param_off == [0, 6 * 4, 6 * 4 + 2, 6 * 4 + 2 + 2, 28 + 24, 52 + 4 * 3]
    assert plan.within_caps


def test_plan_interface_columns_have_no_node():
    plan = cm.build_plan([("x_t_0", ["D_t_1"], ["x_t_1"]), ("D_t_0", ["D_t_1", "E_t_2"], None)], {"D_t_0": 2, "D_t_1": 2, "E_t_2": 5})
    assert plan.dcolumns == ["D_t_1", "D_t_0", "E_t_2"] and plan.ccolumns == ["x_t_0", "x_t_1"]
    assert plan.var == [0, 1]
    discrete_with_node = {plan.var[i] for i in range(2) if plan.kind[i] == cm.DISCRETE}
    assert sorted(set(range(3)) - discrete_with_node) == [0, 2]
    assert plan.cparents == [1]                     # x_t_1: a continuous column without a node


def test_configuration_strides_are_those_of_the_adaptator():
    """_DiscreteAdaptator._config: idx = sum codes_j * stride_j, the FIRST discrete parent fastest."""
    import pyarrow as pa

    from pybnesian_amd.factors import CLinearGaussianCPD

    cats = {"P": ["a", "b", "c"], "Q": ["u", "v"], "R": ["k", "l", "m", "n"]}
    rng = np.random.default_rng(0)
    codes = {k: rng.integers(0, len(v), 50) for k, v in cats.items()}
    rb = pa.RecordBatch.from_arrays([pa.DictionaryArray.from_arrays(pa.array(codes[k], type=pa.int8()), pa.array(cats[k])) for k in cats], names=list(cats))
    f = CLinearGaussianCPD("y", ["Q", "x", "R", "P"])
    f._disc, f._cont, f._categories = ["Q", "R", "P"], ["x"], [cats["Q"], cats["R"], cats["P"]]
    idx, valid = f._config(rb)
    plan = cm.build_plan([("y", f._disc, f._cont)], {k: len(v) for k, v in cats.items()})
    assert plan.strides == [[1, 2, 8]] and plan.configs == [24]
    mine = sum(codes[plan.dcolumns[c]] * s for c, s in zip(plan.dparents, plan.strides[0]))
    assert valid.all() and np.array_equal(idx, mine)
    # a discrete node: the variable fastest, then the parents as given (DiscreteFactor._indices)
    plan = cm.build_plan([("P", ["R", "Q"], None)], {k: len(v) for k, v in cats.items()})
    assert plan.strides == [[1, 3, 12]] and plan.dcolumns == ["P", "R", "Q"]


def test_caps():
    cards = {f"D{i}": 2 for i in range(9)}
    ok = cm.build_plan([("D0", [f"D{i}" for i in range(1, 8)], None), ("y", [f"D{i}" for i in range(7)], [f"x{i}" for i in range(63)])], cards)
    assert ok.within_caps and ok.configs == [256, 128]
    assert not cm.build_plan([("D0", [f"D{i}" for i in range(1, 9)], None), ("y", [], [])], cards).within_caps       # 9 discrete family variables
    assert not cm.build_plan([("y", [f"D{i}" for i in range(8)], [])], cards).within_caps                            # 8 discrete parents
    assert not cm.build_plan([("y", ["D0"], [f"x{i}" for i in range(64)])], cards).within_caps                       # 65 continuous columns
    assert cm.build_plan([("y", ["A", "B"], [])], {"A": 1024, "B": 1024}).within_caps                                # 2^20 configurations
    assert not cm.build_plan([("y", ["A", "B"], [])], {"A": 1024, "B": 1025}).within_caps
    assert not cm.build_plan([("y", ["A", "B", "C"], [])], {"A": 1024, "B": 1024, "C": 4}).within_caps
    many = [(f"y{i}", ["A", "B"], [f"x{j}" for j in range(61)]) for i in range(4)]                                   # 4 x 2^20 x 64 doubles = 2^28 ...
    assert cm.build_plan(many, {"A": 1024, "B": 1024}).within_caps
    assert not cm.build_plan(many + [("D", [], None)], {"A": 1024, "B": 1024, "D": 2}).within_caps                   # ... and two cells more
    assert not cm.build_plan([("y", ["A", "A"], [])], {"A": 2}).within_caps                                          # a column twice
    assert not cm.build_plan([("y", ["A"], [])], {"A": 0}).within_caps                                               # no categories


def test_enabled_follows_the_environment_per_call(monkeypatch):
    monkeypatch.delenv("PBN_CLG_MODEL", raising=False)
    assert cm.enabled()
    monkeypatch.setenv("PBN_CLG_MODEL", "0")
    assert not cm.enabled()
    monkeypatch.setenv("PBN_CLG_MODEL", "1")
    assert cm.enabled()


@pytest.fixture(scope="module")
def clgnet_asm():
    return unit_asm("clg_model")


def test_no_instantiation_uses_scratch_and_the_waves_per_simd_hold(clgnet_asm):
    """Descriptors only.  The block-sum instantiations fit eight waves per SIMD (at most 64 VGPRs); the per-row ones hold four running
    sums more and a per-lane address for every coefficient, and are built for seven (at most 72): DESIGN.md 3.16 has the counts."""
    headers = dict(re.findall(r"\.amdhsa_kernel (\S*clgnet_logl_kernelI[a-z]Lb[01]E\S*)\n(.*?)\.end_amdhsa_kernel", clgnet_asm, flags=re.S))
    kinds = sorted(re.search(r"clgnet_logl_kernelI([a-z])Lb([01])E", name).groups() for name in headers)
    assert kinds == [("d", "0"), ("d", "1"), ("f", "0"), ("f", "1")]     # double / float x per-row sums / per-node block sums
    for name, hdr in headers.items():
        sums = re.search(r"clgnet_logl_kernelI[a-z]Lb([01])E", name).group(1) == "1"
        assert int(re.search(r"private_segment_fixed_size (\d+)", hdr).group(1)) == 0, name
        assert int(re.search(r"next_free_vgpr (\d+)", hdr).group(1)) <= (64 if sums else 72), name
