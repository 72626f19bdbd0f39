"""What the one-pass network evaluations share (discrete_model.py, gaussian_model.py, clg_model.py):
the numbering of a plan's columns, the checks on the arrow side, dictionary codes and their pbn_dtable, the base of the device handles,
the driver of an evaluation over continuous columns, and the one place that says which pass a network takes (`one_pass`).

Each of the three modules keeps what is its own: its switch, counters and caps, the packing of its parameters and its reasons to fall
back to the per-factor loop."""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib


class Plan(SimpleNamespace):
    """The arrays a pbn_*_create takes for a list of families: a plain record, its fields named by the module's build_plan."""


class FirstUse(dict):
    """name -> its number, numbers given in order of first use: index[name] numbers a name that is new, list(index) are the columns in
    that order.  A conditional network's interface columns are numbered like any other, so they are columns without a node."""

    def __missing__(self, name):
        number = self[name] = len(self)
        return number


def model_families(model, nodes):
    """[(node, evidence of its factor)] - the factor's evidence order, which is its CPT's layout or its beta's."""
    return [(n, list(model._cpds[n].evidence())) for n in nodes]


def float_type(rb, columns):
    """The arrow type of `columns` in `rb` when every one is present and they are all float64 or all float32; otherwise None."""
    import pyarrow as pa

    types = set()
    for name in columns:
        idx = rb.schema.get_field_index(name)
        if idx < 0:
            return None
        types.add(rb.schema.field(idx).type)
    if len(types) != 1:
        return None
    t = next(iter(types))
    return t if pa.types.is_float64(t) or pa.types.is_float32(t) else None


def has_nulls(rb, columns):
    return any(rb.column(rb.schema.get_field_index(c)).null_count for c in columns)


def codes(col):
    """int32 dictionary indices of an arrow DictionaryArray, -1 where the row is null."""
    idx = col.indices
    if col.null_count:
        valid = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        return np.ascontiguousarray(np.where(valid, idx.fill_null(0).to_numpy(zero_copy_only=False), -1), dtype=np.int32)
    return np.ascontiguousarray(idx.to_numpy(zero_copy_only=False), dtype=np.int32)


def scatter_rows(vals, mask, n_rows):
    """Per-row values of the rows `mask` kept, back at their places among n_rows; the dropped rows are NaN.  mask None: every row was kept."""
    if mask is None:
        return vals
    out = np.full(n_rows, np.nan)
    out[mask] = vals
    return out


class Handle:
    """Owns what <prefix>_create gave.  close() adds the handle's <prefix>_stats to the owning module's `counters` under the two keys
    `stat_keys` (None: a handle without stats) and calls <prefix>_destroy; a context manager closes on exit."""
    prefix, counters, stat_keys = None, None, None

    def __init__(self, *args):
        h = C.c_void_p()
        _lib.check(getattr(_lib.load(), self.prefix + "_create")(*args, C.byref(h)))
        self.handle = h

    def close(self):
        if self.handle:
            lib = _lib.load()
            if self.stat_keys:
                launches, rows = C.c_int64(0), C.c_int64(0)
                _lib.check(getattr(lib, self.prefix + "_stats")(self.handle, C.byref(launches), C.byref(rows)))
                self.counters[self.stat_keys[0]] += launches.value
                self.counters[self.stat_keys[1]] += rows.value
            getattr(lib, self.prefix + "_destroy")(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class CodeTable(Handle):
    """A pbn_dtable of int32 code arrays (-1 = null), one per column.  `created` is called once the table exists (a module's counter)."""
    prefix = "pbn_dtable"

    def __init__(self, ctx, code_arrays, cardinality, n_rows, created=None):
        self._codes = code_arrays
        ptrs = (C.c_void_p * len(code_arrays))(*[a.ctypes.data for a in code_arrays])
        super().__init__(ctx.handle, int(n_rows), len(code_arrays), ptrs, _lib.int_array(cardinality))
        self.n_rows = int(n_rows)
        if created:
            created()

    def family_counts(self, plan):
        """The tables of the plan's families (var, par_off, parents), concatenated at plan.cpt_off (int64)."""
        total = plan.cpt_off[-1]
        off = np.zeros(len(plan.var) + 1, dtype=np.int64)
        out = np.zeros(max(total, 1), dtype=np.int64)
        form = np.zeros(max(len(plan.var), 1), dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        _lib.check(_lib.load().pbn_dtable_family_counts(self.handle, len(plan.var), _lib.int_array(plan.var), _lib.int_array(plan.par_off),
                                                        _lib.int_array(plan.parents or [0]), off.ctypes.data_as(i64p), out.ctypes.data_as(i64p),
                                                        int(total), form.ctypes.data_as(C.POINTER(C.c_int))))
        return out[:total]


def evaluate_continuous(rb, ccolumns, make_net, what, dcols=None, cardinality=None):
    """One evaluation of a network with continuous columns.  `ccolumns` are uploaded (the rows null in any of them dropped); with
    `dcols` - arrow dictionary columns in the plan's order - the kept rows' codes go into a CodeTable beside them, nulls as -1.
    make_net(ctx) creates the network's handle; `what` names its call: "logl" gives the rows' values with NaN in the dropped rows,
    "node_slogl" the nodes' sums.  The call takes (table), or (code table, table).

    None when the per-factor loop must run: the nodes' sums are asked over continuous nulls (each factor then sums over its own
    family's valid rows), or a shared upload holds other columns than these (the plan's numbering would not hold)."""
    from .dataset import DeviceTable, default_context

    if what == "node_slogl" and has_nulls(rb, ccolumns):
        return None
    ctx = default_context()
    table, mask = DeviceTable.from_dataframe(ctx, rb, ccolumns)
    if list(table.names) != list(ccolumns):
        return None
    if dcols is None:
        with make_net(ctx) as net:
            vals = getattr(net, what)(table)
    else:
        kept = [codes(c) for c in dcols]
        if mask is not None:
            kept = [np.ascontiguousarray(c[mask]) for c in kept]
        with CodeTable(ctx, kept, cardinality, table.num_rows) as ctable, make_net(ctx) as net:
            vals = getattr(net, what)(ctable, table)
    return scatter_rows(vals, mask, rb.num_rows) if what == "logl" else vals


# ---- which pass a network takes ----------------------------------------------------------------------------------------------------------

DISCRETE, GAUSSIAN, CLG = "discrete_model", "gaussian_model", "clg_model"
Served = namedtuple("Served", "name value is_total")   # is_total: `value` is the network's sum already, not the nodes' sums


def one_pass(model, df, what, only=None):
    """The network's "logl" or "slogl" (`what`) from the first pass - of those named in `only`, default all - whose switch is on, whose
    predicate holds for `model` and whose call does not return None: a Served.  None: run the per-factor loop.  The discrete pass's
    "slogl" is the total the C side added (is_total); the other two give the nodes' sums and leave the adding to the caller, whose
    order is part of its result's bits.  `df` is turned into a record batch only for a pass that is taken."""
    from . import clg_model as cm
    from . import discrete_model as dm
    from . import gaussian_model as gm
    from .dataset import as_record_batch

    # in order of precedence: (name, switch, predicate, per-row call, call for the sums, the sums' call gives the total); the
    # modules' attributes are read at each call
    for name, enabled, predicate, logl, slogl, is_total in ((DISCRETE, dm.enabled, dm.all_discrete_factors, dm.network_logl, dm.network_slogl, True),
                                                            (GAUSSIAN, gm.enabled, gm.all_lg_factors, gm.network_logl, gm.network_node_slogl, False),
                                                            (CLG, cm.enabled, cm.clg_factors, cm.network_logl, cm.network_node_slogl, False)):
        if only is not None and name not in only:
            continue
        if enabled() and predicate(model):
            sums = what == "slogl"
            out = (slogl if sums else logl)(model, as_record_batch(df))
            if out is not None:
                return Served(name, out, sums and is_total)
    return None
