"""CPU tier: the host side of the device row grouping behind HCKDE / CLinearGaussianCPD.fit / logl / slogl (pybnesian_amd/
adaptator_group.py, csrc/row_groups.hip) - no device.

The predicate `served` is decided on record batches alone; the numpy restatement of the grouping's key (`keys`, which the GPU tests
reuse as their comparator) equals _DiscreteAdaptator._config (factors/discrete/DiscreteAdaptator.hpp:201-260 over
factors/discrete/discrete_indices.cpp:93-204) on random codes with nulls; the new entry points are declared under their reference
citation, exported by the built library and bound."""
import ctypes
import os
import re

import numpy as np
import pyarrow as pa
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pbn_dtable_group_rows", "pbn_rowgroups_offsets", "pbn_rowgroups_rows", "pbn_table_take_group", "pbn_rowgroups_destroy")
CITED = ("discrete_indices.cpp:93-204", "DiscreteAdaptator.hpp:201-348")


@pytest.fixture(scope="module")
def ag():
    from pybnesian_amd import adaptator_group

    return adaptator_group


def dictionary(codes, categories, nulls=None):
    idx = pa.array(np.asarray(codes, dtype=np.int32), mask=None if nulls is None else np.asarray(nulls, dtype=bool))
    return pa.DictionaryArray.from_arrays(idx, pa.array(categories))


def batch(rows=40, cards=(3, 2), ftype=np.float64, seed=0, mixed=False):
    """Discrete columns D0, D1, ... with the given cardinalities and float columns x, y, z."""
    rng = np.random.default_rng(seed)
    cols = {f"D{k}": dictionary(rng.integers(0, c, size=rows), [f"c{k}_{i}" for i in range(c)]) for k, c in enumerate(cards)}
    for name in "xyz":
        cols[name] = pa.array(rng.normal(size=rows).astype(np.float32 if (mixed and name == "y") else ftype))
    return pa.RecordBatch.from_pydict(cols)


def fitted(factor, rb, disc, cont):
    """The state _DiscreteAdaptator.fit leaves, set by hand: the predicate reads nothing else."""
    factor._disc, factor._cont = list(disc), list(cont)
    factor._categories = [rb.column(rb.schema.get_field_index(d)).dictionary.to_pylist() for d in disc]
    factor._factors = [None] * int(np.prod([len(c) for c in factor._categories]))
    factor._fitted = True
    return factor


@pytest.mark.parametrize("kind", ["HCKDE", "CLinearGaussianCPD"])
@pytest.mark.parametrize("ftype", [np.float64, np.float32])
def test_served(ag, kind, ftype):
    import pybnesian_amd as pbn

    rb = batch(ftype=ftype)
    f = getattr(pbn, kind)("x", ["D0", "y", "D1", "z"])
    assert ag.served(f, rb, fitting=True)
    assert not ag.served(f, rb, fitting=False)            # not fitted
    fitted(f, rb, ["D0", "D1"], ["y", "z"])
    assert ag.served(f, rb, fitting=False)
    assert ag.MAX_CONFIGS >= 4096 and ag.MAX_DISCRETE_PARENTS == 7


@pytest.mark.parametrize("kind", ["HCKDE", "CLinearGaussianCPD"])
def test_not_served(ag, kind):
    import pybnesian_amd as pbn

    cls = getattr(pbn, kind)

    class Derived(cls):
        pass

    rb = batch()
    assert not ag.served(Derived("x", ["D0", "y"]), rb)                                   # a subclass keeps the loop
    assert not ag.served(cls("x", ["y", "z"]), rb)                                        # no discrete evidence
    assert not ag.served(cls("x", ["D0", "missing"]), rb)                                 # (the loop raises)
    eight = batch(cards=(2,) * 8)
    assert ag.served(cls("x", [f"D{k}" for k in range(7)] + ["y"]), eight)
    assert not ag.served(cls("x", [f"D{k}" for k in range(8)] + ["y"]), eight)            # 8 discrete parents
    wide = batch(cards=(128, 64, 2))
    assert ag.served(cls("x", ["D0", "D1"]), wide) and 128 * 64 == ag.MAX_CONFIGS         # G at the cap
    assert not ag.served(cls("x", ["D0", "D1", "D2"]), wide)                              # G above the cap
    assert not ag.served(cls("x", ["D0", "y"]), batch(mixed=True))                        # mixed float types
    assert ag.served(cls("x", ["D0", "z"]), batch(mixed=True))                            # (the family's own columns are of one type)
    f = fitted(cls("x", ["D0", "y"]), rb, ["D0"], ["y"])
    assert ag.served(f, rb, fitting=False)
    other = batch()
    k = other.schema.get_field_index("D0")
    other = other.set_column(k, "D0", dictionary(other.column(k).indices.to_numpy(), ["c0_0", "c0_1", "other"]))
    assert not ag.served(f, other, fitting=False)                                         # categories that differ from the fitted ones
    with pytest.raises(ValueError, match="does not contain the same categories"):
        f._config(other)                                                                  # (what the loop then raises)


def test_the_switch_is_read_per_call(ag, monkeypatch):
    monkeypatch.delenv("PBN_ADAPTATOR_GROUP", raising=False)
    assert ag.enabled()
    monkeypatch.setenv("PBN_ADAPTATOR_GROUP", "0")
    assert not ag.enabled()
    monkeypatch.setenv("PBN_ADAPTATOR_GROUP", "1")
    assert ag.enabled()
    assert set(ag.counters) >= {"partitions", "rows_grouped", "tables_gathered", "loop_fallbacks"}


@pytest.mark.parametrize("cards", [(3,), (3, 2), (2, 5, 3), (4, 1, 3, 2), (2, 3, 2, 2, 3, 2, 2)])
def test_keys_restate_the_adaptators_configuration_index(ag, cards):
    import pybnesian_amd as pbn
    from pybnesian_amd.network_pass import codes

    rng = np.random.default_rng(len(cards))
    rows = 500
    names = [f"D{k}" for k in range(len(cards))]
    cols = {}
    for name, card in zip(names, cards):
        cols[name] = dictionary(rng.integers(0, card, size=rows), [f"{name}_{i}" for i in range(card)], nulls=rng.random(rows) < 0.1)
    cols["x"] = pa.array(rng.normal(size=rows))
    rb = pa.RecordBatch.from_pydict(cols)
    f = fitted(pbn.HCKDE("x", names), rb, names, [])
    idx, valid = f._config(rb)
    arrays = [codes(rb.column(rb.schema.get_field_index(n))) for n in names]
    assert all(a.dtype == np.int32 and a.min() == -1 for a in arrays)
    key, grouped = ag.keys(arrays, cards)
    assert np.array_equal(grouped, valid) and not valid.all() and valid.any()
    assert np.array_equal(key, idx)
    st, cells = ag.strides(cards)
    assert cells == int(np.prod(cards)) and st == [int(np.prod(cards[:j])) for j in range(len(cards))]
    # the grouping the device must give is the loop's row selection, configuration after configuration
    offsets, order = ag.grouping(key, grouped, cells)
    assert offsets[0] == 0 and offsets[-1] == valid.sum() and order.dtype == np.int32
    for c in range(cells):
        assert np.array_equal(order[offsets[c]: offsets[c + 1]], np.nonzero(valid & (idx == c))[0])
    # a validity mask takes rows out of the groups and leaves the keys alone
    keep = rng.random(rows) < 0.7
    key2, grouped2 = ag.keys(arrays, cards, keep)
    assert np.array_equal(key2, key) and np.array_equal(grouped2, valid & keep)


def test_declared_with_their_reference_citation():
    txt = open(os.path.join(ROOT, "include", "pbn_hip.h")).read()
    for name in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|void|double|int64_t)\s+" + name + r"\s*\(", txt, flags=re.S)
        assert m, f"{name} is not declared under a comment of its own"
        for cite in CITED:
            assert cite in m.group(1), f"the comment of {name} does not cite {cite}"
    m = re.search(r"#define\s+PBN_ROWGROUPS_MAX_CONFIGS\s+(\d+)", txt)
    assert m and int(m.group(1)) >= 4096


def test_exported_and_bound(ensure_built, ag):
    import pybnesian_amd._lib as L

    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES
    txt = open(os.path.join(ROOT, "include", "pbn_hip.h")).read()
    assert int(re.search(r"#define\s+PBN_ROWGROUPS_MAX_CONFIGS\s+(\d+)", txt).group(1)) == ag.MAX_CONFIGS
    # null arguments are refused before anything touches a device
    fn = lib.pbn_dtable_group_rows
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert fn(None, 1, None, None, None) == L.PBN_ERR_INVALID
