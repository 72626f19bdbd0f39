"""Fit and evaluation of a network whose factors are all DiscreteFactor, in one device pass (csrc/discrete_model.hip,
DESIGN.md §3.13): BayesianNetwork.fit / logl / slogl (models/BayesianNetwork.hpp:960-994) route here instead of looping
over DiscreteFactor.fit / logl (factors/discrete/DiscreteFactor.cpp:34-171, learning/parameters/mle_DiscreteFactor.cpp:5-41).

One pbn_dtable and one pbn_dnet per call; no handle is kept on the model.  `PBN_DISCRETE_MODEL=0` (read per call) restores
the per-factor loop.  The code table, the handle base and the numbering of the columns are network_pass.py's, shared with
gaussian_model.py and clg_model.py; here are the caps, the CPTs' packing and the reasons to keep the loop."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .network_pass import CodeTable, FirstUse, Handle, Plan, codes, model_families  # noqa: F401 - Plan, model_families: this module's names too

MAX_FAMILY_VARS = 8             # pbn_dnet_create: the variable and 7 parents
MAX_FAMILY_CELLS = 2 ** 31 - 1  # pbn_dnet_create: cells of one CPT

# what the calls of this process did (tests, tools): handles created and the pbn_dnet_stats of the evaluations
counters = {"dtable_created": 0, "dnet_created": 0, "logl_launches": 0, "rows_evaluated": 0}


def enabled():
    return os.environ.get("PBN_DISCRETE_MODEL", "1").strip() != "0"


def build_plan(families, cards):
    """families: [(variable, [evidence...])] in node order, evidence in the FACTOR's order (a CPT follows it); cards: column
    name -> number of categories.  Columns are numbered in order of first use, so a conditional network's interface columns
    are columns without a node.  Pure Python: no device, no library.

    within_caps is False when a family has more than 8 variables, more than 2^31 - 1 cells or a column without categories:
    such a network keeps the per-factor loop."""
    index = FirstUse()
    var, par_off, parents, cpt_off = [], [0], [], [0]
    within = True
    for variable, evidence in families:
        names = [variable] + list(evidence)
        ids = [index[name] for name in names]
        cells = 1
        for name in names:
            cells *= int(cards[name])
        if len(names) > MAX_FAMILY_VARS or cells > MAX_FAMILY_CELLS or cells < 1 or len(set(names)) != len(names):
            within = False
        var.append(ids[0])
        parents.extend(ids[1:])
        par_off.append(len(parents))
        cpt_off.append(cpt_off[-1] + cells)
    columns = list(index)
    return Plan(columns=columns, cardinality=[int(cards[c]) for c in columns], var=var, par_off=par_off, parents=parents,
                cpt_off=cpt_off, within_caps=within)


def all_discrete_factors(model):
    """Every node holds a factor that is exactly DiscreteFactor (a Python subclass stays on the per-factor loop)."""
    from .factors import DiscreteFactor

    cpds = getattr(model, "_cpds", None) or {}
    return bool(model._nodes) and all(type(cpds.get(n)) is DiscreteFactor for n in model._nodes)


def _count_dtable():
    counters["dtable_created"] += 1


def _code_table(cols, plan, n_rows):
    from .dataset import default_context

    return CodeTable(default_context(), [codes(c) for c in cols], plan.cardinality, n_rows, _count_dtable)


class _DNet(Handle):
    prefix, counters, stat_keys = "pbn_dnet", counters, ("logl_launches", "rows_evaluated")

    def __init__(self, plan, logprob):
        from .dataset import default_context

        lp = np.ascontiguousarray(logprob, dtype=np.float64)
        cpt_off = np.ascontiguousarray(plan.cpt_off, dtype=np.int64)
        super().__init__(default_context().handle, len(plan.columns), _lib.int_array(plan.cardinality), len(plan.var), _lib.int_array(plan.var),
                         _lib.int_array(plan.par_off), _lib.int_array(plan.parents or [0]), cpt_off.ctypes.data_as(C.POINTER(C.c_int64)),
                         _lib.dptr(lp))
        counters["dnet_created"] += 1

    def logl(self, table):
        out = np.empty(table.n_rows, dtype=np.float64)
        _lib.check(_lib.load().pbn_dnet_logl(self.handle, table.handle, _lib.dptr(out)))
        return out

    def slogl(self, table):
        total = C.c_double(0.0)
        _lib.check(_lib.load().pbn_dnet_slogl(self.handle, table.handle, C.byref(total), None))
        return total.value


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
    with _code_table([cols[c] for c in plan.columns], plan, rb.num_rows) as table:
        counts = table.family_counts(plan)
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
    with _code_table(cols, plan, rb.num_rows) as table, _DNet(plan, logprob) as net:
        return getattr(net, what)(table)


def network_logl(model, rb):
    """Per-row log-likelihood: the nodes' values added in node order on the device; None when the per-factor loop must run."""
    return _evaluate(model, rb, "logl")


def network_slogl(model, rb):
    return _evaluate(model, rb, "slogl")
