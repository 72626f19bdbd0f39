"""Evaluation of a network whose factors are all LinearGaussianCPD, in one device pass (csrc/gaussian_model.hip):
BayesianNetwork.logl / slogl (models/BayesianNetwork.hpp:997-1022) and the transition part of DynamicBayesianNetwork.logl / slogl
route here instead of looping over LinearGaussianCPD.logl / slogl (factors/continuous/LinearGaussianCPD.cpp:92-149).

One upload of the network's columns and one pbn_gnet per call; no handle is kept on the model.  `PBN_GAUSSIAN_MODEL=0` (read per
call) restores the per-factor loop.  The upload, the handle base and the numbering of the columns are network_pass.py's, shared with
discrete_model.py and clg_model.py; here are the cap, the coefficients' packing and the reasons to keep the loop."""
import os

import numpy as np

from . import _lib
from .network_pass import FirstUse, Handle, Plan, evaluate_continuous, float_type, model_families  # noqa: F401 - Plan, model_families: this module's names too

MAX_FAMILY_COLUMNS = 64   # pbn_gnet_create / pbn_lg_logl: the variable and 63 parents

# what the calls of this process did (tests, tools): handles created and the pbn_gnet_stats of the evaluations
counters = {"gnet_created": 0, "launches": 0, "rows_evaluated": 0}


def enabled():
    return os.environ.get("PBN_GAUSSIAN_MODEL", "1").strip() != "0"


def build_plan(families):
    """families: [(variable, [evidence...])] in node order, evidence in the FACTOR's order (its beta follows it).  Columns are
    numbered in order of first use, so a conditional network's interface columns are columns without a node.  Pure Python: no
    device, no library.

    within_caps is False when a family has more than 64 columns: such a network keeps the per-factor loop."""
    index = FirstUse()
    var, par_off, parents, beta_off = [], [0], [], []
    within = True
    for i, (variable, evidence) in enumerate(families):
        ids = [index[name] for name in [variable] + list(evidence)]
        if len(ids) > MAX_FAMILY_COLUMNS:
            within = False
        beta_off.append(par_off[-1] + i)   # node i's coefficients start here
        var.append(ids[0])
        parents.extend(ids[1:])
        par_off.append(len(parents))
    return Plan(columns=list(index), var=var, par_off=par_off, parents=parents, beta_off=beta_off, within_caps=within)


def all_lg_factors(model):
    """Every node holds a factor that is exactly LinearGaussianCPD (a Python subclass stays on the per-factor loop)."""
    from .factors import LinearGaussianCPD

    cpds = getattr(model, "_cpds", None) or {}
    return bool(model._nodes) and all(type(cpds.get(n)) is LinearGaussianCPD for n in model._nodes)


class _GNet(Handle):
    prefix, counters, stat_keys = "pbn_gnet", counters, ("launches", "rows_evaluated")

    def __init__(self, ctx, plan, beta, variance):
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        variance = np.ascontiguousarray(variance, dtype=np.float64)
        super().__init__(ctx.handle, len(plan.columns), len(plan.var), _lib.int_array(plan.var), _lib.int_array(plan.par_off),
                         _lib.int_array(plan.parents or [0]), _lib.dptr(beta), _lib.dptr(variance))
        self.n_nodes = len(plan.var)
        counters["gnet_created"] += 1

    def logl(self, table):
        out = np.empty(table.num_rows, dtype=np.float64)
        _lib.check(_lib.load().pbn_gnet_logl(self.handle, table.handle, _lib.dptr(out)))
        return out

    def node_slogl(self, table):
        out = np.zeros(self.n_nodes, dtype=np.float64)
        _lib.check(_lib.load().pbn_gnet_slogl(self.handle, table.handle, _lib.dptr(out)))
        return out


def _evaluation(model, rb):
    """(plan, beta, variance) of a fitted all-LinearGaussianCPD model on `rb`; None when the per-factor loop must run (and raise
    what it raises): a family beyond the cap, a column that is missing, or columns that are not all float64 or all float32."""
    families = model_families(model, model._nodes)
    plan = build_plan(families)
    if not plan.within_caps or float_type(rb, plan.columns) is None:
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


def _evaluate(model, rb, what):
    ev = _evaluation(model, rb)
    if ev is None:
        return None
    plan, beta, variance = ev
    return evaluate_continuous(rb, plan.columns, lambda ctx: _GNet(ctx, plan, beta, variance), what)


def network_logl(model, rb):
    """Per-row log-likelihood: the nodes' values added in node order on the device, NaN where a row is null in any column of the
    network (it is NaN in that factor's logl and so in the loop's sum); None when the per-factor loop must run."""
    return _evaluate(model, rb, "logl")


def network_node_slogl(model, rb):
    """The nodes' summed log-likelihoods in node order (float64 array), each LinearGaussianCPD.slogl's bits; None when the loop must
    run: also when a column of the network has nulls (each factor then sums over its own family's valid rows)."""
    return _evaluate(model, rb, "node_slogl")
