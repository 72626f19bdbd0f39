"""Evaluation of a network whose factors are all LinearGaussianCPD, in one device pass (csrc/gaussian_model.hip):
BayesianNetwork.logl / slogl (models/BayesianNetwork.hpp:997-1022) and the transition part of DynamicBayesianNetwork.logl / slogl
route here instead of looping over LinearGaussianCPD.logl / slogl (factors/continuous/LinearGaussianCPD.cpp:92-149).

One upload of the network's columns and one pbn_gnet per call; no handle is kept on the model.  `PBN_GAUSSIAN_MODEL=0` (read per
call) restores the per-factor loop."""
import ctypes as C
import os

import numpy as np

from . import _lib

MAX_FAMILY_COLUMNS = 64   # pbn_gnet_create / pbn_lg_logl: the variable and 63 parents

# what the calls of this process did (tests, tools): handles created and the pbn_gnet_stats of the evaluations
counters = {"gnet_created": 0, "launches": 0, "rows_evaluated": 0}


def enabled():
    return os.environ.get("PBN_GAUSSIAN_MODEL", "1").strip() != "0"


class Plan:
    """The arrays pbn_gnet_create takes for a list of families over `columns`; node i's coefficients start at beta_off[i]."""

    def __init__(self, columns, var, par_off, parents, beta_off, within_caps):
        self.columns = columns
        self.var, self.par_off, self.parents, self.beta_off = var, par_off, parents, beta_off
        self.within_caps = within_caps


def build_plan(families):
    """families: [(variable, [evidence...])] in node order, evidence in the FACTOR's order (its beta follows it).  Columns are
    numbered in order of first use, so a conditional network's interface columns are columns without a node.  Pure Python: no
    device, no library.

    within_caps is False when a family has more than 64 columns: such a network keeps the per-factor loop."""
    columns, index = [], {}
    var, par_off, parents, beta_off = [], [0], [], []
    within = True
    for i, (variable, evidence) in enumerate(families):
        names = [variable] + list(evidence)
        for name in names:
            if name not in index:
                index[name] = len(columns)
                columns.append(name)
        if len(names) > MAX_FAMILY_COLUMNS:
            within = False
        beta_off.append(par_off[-1] + i)
        var.append(index[variable])
        parents.extend(index[e] for e in evidence)
        par_off.append(len(parents))
    return Plan(columns, var, par_off, parents, beta_off, within)


def model_families(model, nodes):
    """[(node, evidence of its factor)] - the factor's evidence order, which is its beta's."""
    return [(n, list(model._cpds[n].evidence())) for n in nodes]


def all_lg_factors(model):
    """Every node holds a factor that is exactly LinearGaussianCPD (a Python subclass stays on the per-factor loop)."""
    from .factors import LinearGaussianCPD

    cpds = getattr(model, "_cpds", None) or {}
    return bool(model._nodes) and all(type(cpds.get(n)) is LinearGaussianCPD for n in model._nodes)


class _GNet:
    def __init__(self, ctx, plan, beta, variance):
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        variance = np.ascontiguousarray(variance, dtype=np.float64)
        h = C.c_void_p()
        _lib.check(_lib.load().pbn_gnet_create(ctx.handle, len(plan.columns), len(plan.var), _lib.int_array(plan.var), _lib.int_array(plan.par_off),
                                               _lib.int_array(plan.parents or [0]), _lib.dptr(beta), _lib.dptr(variance), C.byref(h)))
        self.handle, self.n_nodes = h, len(plan.var)
        counters["gnet_created"] += 1

    def logl(self, table):
        out = np.empty(table.num_rows, dtype=np.float64)
        _lib.check(_lib.load().pbn_gnet_logl(self.handle, table.handle, _lib.dptr(out)))
        return out

    def node_slogl(self, table):
        out = np.zeros(self.n_nodes, dtype=np.float64)
        _lib.check(_lib.load().pbn_gnet_slogl(self.handle, table.handle, _lib.dptr(out)))
        return out

    def close(self):
        if self.handle:
            launches, rows = C.c_int64(0), C.c_int64(0)
            _lib.check(_lib.load().pbn_gnet_stats(self.handle, C.byref(launches), C.byref(rows)))
            counters["launches"] += launches.value
            counters["rows_evaluated"] += rows.value
            _lib.load().pbn_gnet_destroy(self.handle)
            self.handle = None


def _evaluation(model, rb):
    """(plan, beta, variance) of a fitted all-LinearGaussianCPD model on `rb`; None when the per-factor loop must run (and raise
    what it raises): a family beyond the cap, a column that is missing, or columns that are not all float64 or all float32."""
    import pyarrow as pa

    families = model_families(model, model._nodes)
    plan = build_plan(families)
    if not plan.within_caps:
        return None
    types = set()
    for name in plan.columns:
        idx = rb.schema.get_field_index(name)
        if idx < 0:
            return None
        types.add(rb.schema.field(idx).type)
    if len(types) != 1:
        return None
    t = next(iter(types))
    if not (pa.types.is_float64(t) or pa.types.is_float32(t)):
        return None
    betas, variances = [], []
    for (variable, evidence) in families:
        f = model._cpds[variable]
        b = np.asarray(f.beta, dtype=np.float64).reshape(-1)
        if b.size != len(evidence) + 1:
            return None   # coefficients set by hand that do not fit the evidence: the per-factor loop reports it
        betas.append(b)
        variances.append(float(f.variance))
    return plan, np.concatenate(betas), np.asarray(variances, dtype=np.float64)


def _has_nulls(rb, columns):
    return any(rb.column(rb.schema.get_field_index(c)).null_count for c in columns)


def _run(plan, beta, variance, rb, what):
    from .dataset import DeviceTable, default_context

    ctx = default_context()
    table, mask = DeviceTable.from_dataframe(ctx, rb, plan.columns)
    if list(table.names) != list(plan.columns):
        return None   # a shared upload of other columns: the plan's numbering would not hold
    net = _GNet(ctx, plan, beta, variance)
    try:
        return getattr(net, what)(table), mask
    finally:
        net.close()


def network_logl(model, rb):
    """Per-row log-likelihood: the nodes' values added in node order on the device, NaN where a row is null in any column of the
    network (it is NaN in that factor's logl and so in the loop's sum); None when the per-factor loop must run."""
    ev = _evaluation(model, rb)
    if ev is None:
        return None
    res = _run(*ev, rb, "logl")
    if res is None:
        return None
    vals, mask = res
    if mask is None:
        return vals
    out = np.full(rb.num_rows, np.nan)
    out[mask] = vals
    return out


def network_node_slogl(model, rb):
    """The nodes' summed log-likelihoods in node order (float64 array), each LinearGaussianCPD.slogl's bits; None when the loop must
    run: also when a column of the network has nulls (each factor then sums over its own family's valid rows)."""
    ev = _evaluation(model, rb)
    if ev is None or _has_nulls(rb, ev[0].columns):
        return None
    res = _run(*ev, rb, "node_slogl")
    return None if res is None else res[0]
