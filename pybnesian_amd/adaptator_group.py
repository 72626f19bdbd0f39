"""fit / logl / slogl of a factor with one base factor per configuration of its discrete evidence - HCKDE, and a CLinearGaussianCPD used
on its own - on ONE device partition of the rows (csrc/row_groups.hip) instead of _DiscreteAdaptator's loop
(factors/discrete/DiscreteAdaptator.hpp:201-348): per configuration a scan of all rows on the host, an arrow take of the whole frame, an
upload of the slice, and only then a kernel.

A call uploads one code table of the discrete evidence (a null is -1) and one table of the family's continuous columns - inside
BayesianNetwork.fit / logl / slogl both are the scope's shared ones (dataset.shared_upload) - groups the rows once
(pbn_dtable_group_rows) and gathers each configuration's rows device to device (pbn_table_take_group) into the table the base factor's
`fit_table` / `logl_table` / `slogl_table` takes.  That table is byte for byte the one the loop's upload of the slice gives, and the base
factor enters through the same code: the results are the loop's bits.

`PBN_ADAPTATOR_GROUP=0` (read per call) restores the loop.  `served` says, without a device, whether a factor and a frame take this
route; everything else keeps the loop, which also raises whatever is to be raised."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .network_pass import CodeTable, codes, float_type

MAX_DISCRETE_PARENTS = 7   # pbn_dtable_group_rows: key columns
MAX_CONFIGS = 8192         # PBN_ROWGROUPS_MAX_CONFIGS: the LDS counters of a workgroup

# what the calls of this process did (tests, tools): device partitions, the rows they put into groups, tables gathered from them, calls
# with the switch on that the loop served, code tables uploaded (one per stand-alone call, one per model call)
counters = {"partitions": 0, "rows_grouped": 0, "tables_gathered": 0, "loop_fallbacks": 0, "code_tables": 0}


def enabled():
    return os.environ.get("PBN_ADAPTATOR_GROUP", "1").strip() != "0"


def strides(cards):
    """The adaptator's index (_DiscreteAdaptator._config): the first column fastest, stride_j = the product of the cardinalities before
    it.  Returns (strides, number of configurations)."""
    out, cells = [], 1
    for card in cards:
        out.append(cells)
        cells *= int(card)
    return out, cells


def keys(code_arrays, cards, valid=None):
    """The numpy restatement of the grouping's key: (key, grouped) per row from int32 code arrays with -1 for a null - key = sum code_j
    stride_j with a null counting as code 0, grouped = no code is -1 and, when `valid` (a boolean array) is given, the row's entry is
    set: _DiscreteAdaptator._config's (idx, valid).  The key of a row that is not grouped means nothing."""
    st, _ = strides(cards)
    n = len(code_arrays[0]) if code_arrays else 0
    key = np.zeros(n, dtype=np.int64)
    grouped = np.ones(n, dtype=bool) if valid is None else np.array(valid, dtype=bool)
    for col, stride in zip(code_arrays, st):
        col = np.asarray(col)
        grouped &= col >= 0
        key += np.where(col >= 0, col, 0).astype(np.int64) * stride
    return key, grouped


def grouping(key, grouped, n_configs):
    """What the device partition must give for these keys: (offsets, rows) - the grouped rows in stable key order and the cumulative
    counts of the configurations."""
    rows = np.nonzero(grouped)[0]
    rows = rows[np.argsort(key[rows], kind="stable")].astype(np.int32)
    offsets = np.zeros(n_configs + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(key[grouped], minlength=n_configs))
    return offsets, rows


# ---- the predicate -------------------------------------------------------------------------------------------------------------------------

def _family(factor, rb, fitting):
    """(discrete evidence, continuous evidence, cardinalities) of `factor` on `rb` when this route serves it, else None.  fitting: the
    evidence is split by the frame's types as _DiscreteAdaptator.fit splits it; otherwise the fitted split is used and the frame's
    categories must be the fitted ones."""
    import pyarrow as pa

    from .factors import HCKDE, CLinearGaussianCPD

    if type(factor) is not HCKDE and type(factor) is not CLinearGaussianCPD:
        return None
    if fitting:
        disc, cont = [], []
        for e in factor.evidence():
            idx = rb.schema.get_field_index(e)
            if idx < 0:
                return None
            t = rb.schema.field(idx).type
            if pa.types.is_dictionary(t):
                disc.append(e)
            elif pa.types.is_floating(t):
                cont.append(e)
            else:
                return None
    else:
        if not factor.fitted():
            return None
        disc, cont = list(factor._disc), list(factor._cont)
    if not 1 <= len(disc) <= MAX_DISCRETE_PARENTS or len(set(disc)) != len(disc):
        return None
    cards = []
    for k, name in enumerate(disc):
        idx = rb.schema.get_field_index(name)
        if idx < 0 or not pa.types.is_dictionary(rb.schema.field(idx).type):
            return None
        dictionary = rb.column(idx).dictionary
        if not fitting and dictionary.to_pylist() != factor._categories[k]:
            return None                      # the loop raises: "does not contain the same categories"
        cards.append(len(dictionary))
    if not 1 <= strides(cards)[1] <= MAX_CONFIGS:
        return None
    if float_type(rb, [factor.variable()] + cont) is None:
        return None
    return disc, cont, cards


def served(factor, rb, fitting=True):
    """Whether fit (fitting) or logl / slogl of `factor` on the record batch `rb` takes the device partition.  Pure Python: no device,
    no library.  Served: the factor is exactly HCKDE or exactly CLinearGaussianCPD (a Python subclass keeps the loop), it has between 1
    and 7 discrete evidence columns with at most MAX_CONFIGS configurations between them, its variable and continuous evidence are all
    float64 or all float32, and - for logl / slogl - it is fitted and the frame's categories are the fitted ones."""
    return _family(factor, rb, fitting) is not None


# ---- a call ----------------------------------------------------------------------------------------------------------------------------------

def _count_code_table():
    counters["code_tables"] += 1


def _code_table(ctx, rb, disc):
    """(code table, its columns of `disc`, whether the caller owns it).  Inside a shared_upload scope on this frame the table of ALL the
    scope's dictionary columns, built at the first call that asks and closed with the scope; otherwise one of `disc` alone."""
    import pyarrow as pa

    from .dataset import shared_slot

    slot = shared_slot(ctx, rb)
    if slot is not None:
        if "code_table" not in slot:
            wanted = slot["columns"]
            names = [f.name for f in rb.schema if pa.types.is_dictionary(f.type) and (wanted is None or f.name in wanted)]
            cards = [len(rb.column(rb.schema.get_field_index(n)).dictionary) for n in names]
            slot["code_table"] = None
            if names and min(cards) >= 1:
                arrays = [codes(rb.column(rb.schema.get_field_index(n))) for n in names]
                slot["code_table"] = CodeTable(ctx, arrays, cards, rb.num_rows, created=_count_code_table)
                slot["code_table"].names = names
        shared = slot["code_table"]
        if shared is not None and all(d in shared.names for d in disc):
            return shared, [shared.names.index(d) for d in disc], False
    arrays = [codes(rb.column(rb.schema.get_field_index(d))) for d in disc]
    cards = [len(rb.column(rb.schema.get_field_index(d)).dictionary) for d in disc]
    return CodeTable(ctx, arrays, cards, rb.num_rows, created=_count_code_table), list(range(len(disc))), True


class _Partition:
    """One call's device state: the continuous table, the code table and the rows grouped by configuration.  `offsets` (G + 1) on the
    host; table(c) gathers configuration c's rows of the family's columns; rows() downloads the grouped list once."""

    def __init__(self, factor, rb, disc, cont):
        from .dataset import DeviceTable, combined_mask, default_context

        self.handle, self.ctable, self._owns_ctable = None, None, False
        self.columns = [factor.variable()] + list(cont)
        ctx = default_context()
        # inside a shared_upload scope: the scope's table (its columns are null-free); otherwise the family's columns, every row
        self.source, _ = DeviceTable.from_dataframe(ctx, rb, self.columns, drop_null=False)
        self.cidx = _lib.int_array(self.source.index(self.columns))
        self.mask = combined_mask(rb, self.columns)   # rows with a null in a continuous column of the family are in no group
        bitmap = np.packbits(self.mask, bitorder="little") if self.mask is not None else None
        self.ctable, dcols, self._owns_ctable = _code_table(ctx, rb, disc)
        self.disc_codes = [self.ctable._codes[k] for k in dcols]
        lib = _lib.load()
        try:
            h = C.c_void_p()
            _lib.check(lib.pbn_dtable_group_rows(self.ctable.handle, len(dcols), _lib.int_array(dcols), bitmap.ctypes.data if bitmap is not None else None,
                                                 C.byref(h)))
            self.handle = h
            n_configs = C.c_int64(0)
            _lib.check(lib.pbn_rowgroups_offsets(self.handle, C.byref(n_configs), None))
            self.offsets = np.zeros(n_configs.value + 1, dtype=np.int64)
            _lib.check(lib.pbn_rowgroups_offsets(self.handle, C.byref(n_configs), self.offsets.ctypes.data_as(C.POINTER(C.c_int64))))
        except Exception:
            self.close()
            raise
        counters["partitions"] += 1
        counters["rows_grouped"] += int(self.offsets[-1])

    def count(self, c):
        return int(self.offsets[c + 1] - self.offsets[c])

    def table(self, c):
        from .dataset import DeviceTable

        h = C.c_void_p()
        _lib.check(_lib.load().pbn_table_take_group(self.source.handle, self.cidx, len(self.columns), self.handle, int(c), C.byref(h)))
        counters["tables_gathered"] += 1
        return DeviceTable(self.source.ctx, h, self.columns, self.source.dtype)

    def rows(self):
        out = np.zeros(int(self.offsets[-1]), dtype=np.int32)
        _lib.check(_lib.load().pbn_rowgroups_rows(self.handle, out.ctypes.data if out.size else None))
        return out

    def close(self):
        if self.handle:
            _lib.load().pbn_rowgroups_destroy(self.handle)
            self.handle = None
        if self._owns_ctable:
            self.ctable.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _route(factor, rb, fitting):
    """The family when this call takes the device partition; None - and, with the switch on, one more `loop_fallbacks` - for the loop."""
    if not enabled():
        return None
    family = _family(factor, rb, fitting)
    if family is None:
        counters["loop_fallbacks"] += 1
    return family


def fit(factor, rb):
    """_DiscreteAdaptator.fit of `factor` on the record batch `rb`; False when the loop must run (nothing was touched).  The factor ends
    as the loop leaves it: `_disc`, `_cont`, `_categories`, and per configuration a base factor or None - no rows, or a fit the factor's
    `_fit_base` rule drops (HCKDE: SingularCovarianceData; CLinearGaussianCPD: a variance below 1.49e-8 or infinite)."""
    family = _route(factor, rb, True)
    if family is None:
        return False
    disc, cont, cards = family
    factor._disc, factor._cont = disc, cont
    factor._categories = [rb.column(rb.schema.get_field_index(d)).dictionary.to_pylist() for d in disc]
    factor._factors = []
    with _Partition(factor, rb, disc, cont) as part:
        # rows with a null in a continuous column are in no group, where the loop hands them to the base factor, which compacts them
        # away: a configuration whose rows are ALL such is still fitted - on no rows - as the loop fits it
        present = part.offsets[1:] > part.offsets[:-1]
        if part.mask is not None:
            key, grouped = keys(part.disc_codes, cards)
            present = present | (np.bincount(key[grouped], minlength=len(present)) > 0)
        for c in range(len(present)):
            if not present[c]:
                factor._factors.append(None)
                continue
            base = factor._base(cont)
            factor._factors.append(base if factor._fit_base(base, part.table(c), table=True) else None)
    factor._fitted = True
    return True


def logl(factor, rb):
    """_DiscreteAdaptator.logl: per row the value of its configuration's base factor; NaN for a row with a null in the family, and for
    a configuration without a factor.  None when the loop must run."""
    family = _route(factor, rb, False)
    if family is None:
        return None
    disc, cont, _ = family
    out = np.full(rb.num_rows, np.nan)
    with _Partition(factor, rb, disc, cont) as part:
        rows = part.rows()
        for c, base in enumerate(factor._factors):
            lo, hi = int(part.offsets[c]), int(part.offsets[c + 1])
            if hi > lo and base is not None:
                out[rows[lo:hi]] = base.logl_table(part.table(c))
    return out


def slogl(factor, rb):
    """_DiscreteAdaptator.slogl: the configurations' sums added in configuration order from 0.0.  None when the loop must run."""
    family = _route(factor, rb, False)
    if family is None:
        return None
    disc, cont, _ = family
    total = 0.0
    with _Partition(factor, rb, disc, cont) as part:
        for c, base in enumerate(factor._factors):
            if part.count(c) and base is not None:
                total += base.slogl_table(part.table(c))
    return total
