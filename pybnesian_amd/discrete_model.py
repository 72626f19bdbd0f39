"""Fit and evaluation of a network whose factors are all DiscreteFactor, in one device pass (csrc/discrete_model.hip,
DESIGN.md §3.13): BayesianNetwork.fit / logl / slogl (models/BayesianNetwork.hpp:960-994) route here instead of looping
over DiscreteFactor.fit / logl (factors/discrete/DiscreteFactor.cpp:34-171, learning/parameters/mle_DiscreteFactor.cpp:5-41).

One pbn_dtable and one pbn_dnet per call; no handle is kept on the model.  `PBN_DISCRETE_MODEL=0` (read per call) restores
the per-factor loop."""
import ctypes as C
import os

import numpy as np

from . import _lib

MAX_FAMILY_VARS = 8             # pbn_dnet_create: the variable and 7 parents
MAX_FAMILY_CELLS = 2 ** 31 - 1  # pbn_dnet_create: cells of one CPT

# what the calls of this process did (tests, tools): handles created and the pbn_dnet_stats of the evaluations
counters = {"dtable_created": 0, "dnet_created": 0, "logl_launches": 0, "rows_evaluated": 0}


def enabled():
    return os.environ.get("PBN_DISCRETE_MODEL", "1").strip() != "0"


class Plan:
    """The arrays pbn_dtable_family_counts / pbn_dnet_create take for a list of families over `columns`."""

    def __init__(self, columns, cardinality, var, par_off, parents, cpt_off, within_caps):
        self.columns, self.cardinality = columns, cardinality
        self.var, self.par_off, self.parents, self.cpt_off = var, par_off, parents, cpt_off
        self.within_caps = within_caps


def build_plan(families, cards):
    """families: [(variable, [evidence...])] in node order, evidence in the FACTOR's order (a CPT follows it); cards: column
    name -> number of categories.  Columns are numbered in order of first use, so a conditional network's interface columns
    are columns without a node.  Pure Python: no device, no library.

    within_caps is False when a family has more than 8 variables, more than 2^31 - 1 cells or a column without categories:
    such a network keeps the per-factor loop."""
    columns, index = [], {}
    var, par_off, parents, cpt_off = [], [0], [], [0]
    within = True
    for variable, evidence in families:
        names = [variable] + list(evidence)
        for name in names:
            if name not in index:
                index[name] = len(columns)
                columns.append(name)
        cells = 1
        for name in names:
            cells *= int(cards[name])
        if len(names) > MAX_FAMILY_VARS or cells > MAX_FAMILY_CELLS or cells < 1 or len(set(names)) != len(names):
            within = False
        var.append(index[variable])
        parents.extend(index[e] for e in evidence)
        par_off.append(len(parents))
        cpt_off.append(cpt_off[-1] + cells)
    return Plan(columns, [int(cards[c]) for c in columns], var, par_off, parents, cpt_off, within)


def model_families(model, nodes):
    """[(node, evidence of its factor)] - the factor's evidence order, which is its CPT's layout."""
    return [(n, list(model._cpds[n].evidence())) for n in nodes]


def all_discrete_factors(model):
    """Every node holds a factor that is exactly DiscreteFactor (a Python subclass stays on the per-factor loop)."""
    from .factors import DiscreteFactor

    cpds = getattr(model, "_cpds", None) or {}
    return bool(model._nodes) and all(type(cpds.get(n)) is DiscreteFactor for n in model._nodes)


def _codes(col):
    """int32 dictionary indices of an arrow DictionaryArray, -1 where the row is null."""
    idx = col.indices
    if col.null_count:
        valid = np.asarray(col.is_valid().to_numpy(zero_copy_only=False), dtype=bool)
        return np.ascontiguousarray(np.where(valid, idx.fill_null(0).to_numpy(zero_copy_only=False), -1), dtype=np.int32)
    return np.ascontiguousarray(idx.to_numpy(zero_copy_only=False), dtype=np.int32)


class _DTable:
    def __init__(self, cols, cardinality, n_rows):
        from .dataset import default_context

        self._ctx = default_context()
        self._codes = [_codes(c) for c in cols]
        ptrs = (C.c_void_p * len(cols))(*[a.ctypes.data for a in self._codes])
        h = C.c_void_p()
        _lib.check(_lib.load().pbn_dtable_create(self._ctx.handle, int(n_rows), len(cols), ptrs, _lib.int_array(cardinality), C.byref(h)))
        self.handle, self.n_rows = h, int(n_rows)
        counters["dtable_created"] += 1

    def family_counts(self, plan):
        """The families' tables, concatenated at plan.cpt_off (int64)."""
        total = plan.cpt_off[-1]
        off = np.zeros(len(plan.var) + 1, dtype=np.int64)
        out = np.zeros(max(total, 1), dtype=np.int64)
        form = np.zeros(max(len(plan.var), 1), dtype=np.int32)
        i64p = C.POINTER(C.c_int64)
        _lib.check(_lib.load().pbn_dtable_family_counts(self.handle, len(plan.var), _lib.int_array(plan.var), _lib.int_array(plan.par_off),
                                                        _lib.int_array(plan.parents or [0]), off.ctypes.data_as(i64p), out.ctypes.data_as(i64p),
                                                        int(total), form.ctypes.data_as(C.POINTER(C.c_int))))
        return out[:total]

    def close(self):
        if self.handle:
            _lib.load().pbn_dtable_destroy(self.handle)
            self.handle = None


class _DNet:
    def __init__(self, plan, logprob):
        from .dataset import default_context

        self._ctx = default_context()
        lp = np.ascontiguousarray(logprob, dtype=np.float64)
        cpt_off = np.ascontiguousarray(plan.cpt_off, dtype=np.int64)
        h = C.c_void_p()
        _lib.check(_lib.load().pbn_dnet_create(self._ctx.handle, len(plan.columns), _lib.int_array(plan.cardinality), len(plan.var),
                                               _lib.int_array(plan.var), _lib.int_array(plan.par_off), _lib.int_array(plan.parents or [0]),
                                               cpt_off.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(lp), C.byref(h)))
        self.handle = h
        counters["dnet_created"] += 1

    def logl(self, table):
        out = np.empty(table.n_rows, dtype=np.float64)
        _lib.check(_lib.load().pbn_dnet_logl(self.handle, table.handle, _lib.dptr(out)))
        return out

    def slogl(self, table):
        total = C.c_double(0.0)
        _lib.check(_lib.load().pbn_dnet_slogl(self.handle, table.handle, C.byref(total), None))
        return total.value

    def close(self):
        if self.handle:
            launches, rows = C.c_int64(0), C.c_int64(0)
            _lib.check(_lib.load().pbn_dnet_stats(self.handle, C.byref(launches), C.byref(rows)))
            counters["logl_launches"] += launches.value
            counters["rows_evaluated"] += rows.value
            _lib.load().pbn_dnet_destroy(self.handle)
            self.handle = None


def fit_network(model, rb, todo):
    """Fit the (exactly-DiscreteFactor, already constructed) factors of the nodes `todo` from ONE family-count call; False when
    a family is beyond the caps (the caller then runs the per-factor loop).  The factors end bit-identical to DiscreteFactor.fit."""
    from .factors import _dictionary_column, _logprob_from_counts

    families = model_families(model, todo)
    cols = {}
    for variable, evidence in families:          # the order DiscreteFactor._indices meets the columns in: the same first error
        for name in [variable] + evidence:
            if name not in cols:
                cols[name] = _dictionary_column(rb, name)
    cards = {name: len(c.dictionary) for name, c in cols.items()}
    plan = build_plan(families, cards)
    if not plan.within_caps:
        return False
    table = _DTable([cols[c] for c in plan.columns], plan.cardinality, rb.num_rows)
    try:
        counts = table.family_counts(plan)
    finally:
        table.close()
    categories = {name: c.dictionary.to_pylist() for name, c in cols.items()}
    for i, (variable, evidence) in enumerate(families):
        f = model._cpds[variable]
        names = [variable] + evidence
        f._fitted = False
        f._categories = [list(categories[n]) for n in names]
        f._cards = [cards[n] for n in names]
        f._logprob = _logprob_from_counts(counts[plan.cpt_off[i]: plan.cpt_off[i + 1]], f._cards[0])
        f._fitted = True
    return True


def _evaluation(model, rb):
    """(plan, table columns, concatenated logprob) of a fitted all-DiscreteFactor model on `rb`, after DiscreteFactor._indices'
    category check; None when a family is beyond the caps."""
    from .factors import _dictionary_column

    families = model_families(model, model._nodes)
    cols, dictionaries, cards = {}, {}, {}
    for variable, evidence in families:
        f = model._cpds[variable]
        for name, cats in zip([variable] + evidence, f._categories):
            if name not in cols:
                cols[name] = _dictionary_column(rb, name)
                dictionaries[name] = cols[name].dictionary.to_pylist()
                cards[name] = len(dictionaries[name])
            if dictionaries[name] != cats:
                raise ValueError(f"Variable {name} does not contain the same categories.")  # discrete_indices.cpp:206-227
    plan = build_plan(families, cards)
    if not plan.within_caps:
        return None
    logprob = np.concatenate([np.asarray(model._cpds[v]._logprob, dtype=np.float64).reshape(-1) for v, _ in families])
    if logprob.size != plan.cpt_off[-1]:
        return None   # a factor whose table is not its categories' (set by hand): the per-factor loop reports it
    return plan, [cols[c] for c in plan.columns], logprob


def _evaluate(model, rb, what):
    ev = _evaluation(model, rb)
    if ev is None:
        return None
    plan, cols, logprob = ev
    table = _DTable(cols, plan.cardinality, rb.num_rows)
    try:
        net = _DNet(plan, logprob)
        try:
            return getattr(net, what)(table)
        finally:
            net.close()
    finally:
        table.close()


def network_logl(model, rb):
    """Per-row log-likelihood: the nodes' values added in node order on the device; None when the per-factor loop must run."""
    return _evaluate(model, rb, "logl")


def network_slogl(model, rb):
    return _evaluate(model, rb, "slogl")
