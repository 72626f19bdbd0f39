"""CPU tier: the entry points of the count-only tests of pbn_mi_pvalue_batch (csrc/mi.hip) are declared in
include/pbn_hip.h, each under a comment that cites the reference lines it stands for, are exported by the built library and are bound in
pybnesian_amd._lib.  The test aid pbn_debug_mi_discrete is exported and stays out of the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbn_mi_discrete_batch_stats", "pbn_mi_discrete_set_batch_threshold", "pbn_mi_discrete_batch_max_cells")
CITED = ("mutual_information.cpp:926-1055,1093-1137", "discrete_indices.cpp:134-150")


def header():
    return open(os.path.join(ROOT, "include", "pbn_hip.h")).read()


def test_declared_with_their_reference_citation():
    txt = header()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void|double|int64_t)\s+" + name + r"\s*\(", txt, flags=re.S)
        assert m, f"{name} is not declared under a comment of its own"
        for cite in CITED:
            assert cite in m.group(1), f"the comment of {name} does not cite {cite}"
    assert "pbn_debug_mi_discrete" not in txt


def test_exported_and_bound(ensure_built):
    import pybnesian_amd._lib as L

    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES + ("pbn_debug_mi_discrete",):
        assert hasattr(lib, name), f"{name} is not exported"
    for name in NAMES:
        assert name in L.SIGNATURES
    assert "pbn_debug_mi_discrete" not in L.SIGNATURES
    # no device needed: a constant of the build
    fn = lib.pbn_mi_discrete_batch_max_cells
    fn.restype = ctypes.c_int
    assert fn() >= 4096
    import pybnesian_amd as pbn

    assert callable(pbn.MutualInformation.batch_stats) and callable(pbn.MutualInformation.set_batch_threshold)
    assert pbn.ChiSquare.batch_stats is not pbn.MutualInformation.batch_stats       # ChiSquare keeps its own counters
