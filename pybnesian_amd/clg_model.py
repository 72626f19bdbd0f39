"""Evaluation of a network of DiscreteFactors and (C)LinearGaussianCPDs - a CLGNetwork - in one device pass (csrc/clg_model.hip,
DESIGN.md §3.16): BayesianNetwork.logl / slogl (models/BayesianNetwork.hpp:997-1022) and the transition part of
DynamicBayesianNetwork.logl / slogl route here instead of looping over DiscreteFactor.logl (factors/discrete/DiscreteFactor.cpp:91-171)
and, per configuration of a continuous node's discrete parents, LinearGaussianCPD.logl on a slice of the table
(factors/discrete/DiscreteAdaptator.hpp:327-348, factors/continuous/LinearGaussianCPD.cpp:92-149).

One upload of the continuous columns, one pbn_dtable of the discrete codes and one pbn_clgnet per call; no handle is kept on the
model.  `PBN_CLG_MODEL=0` (read per call) restores the per-factor loop.  Networks whose factors are all DiscreteFactor or all
LinearGaussianCPD are not served here: they keep discrete_model.py / gaussian_model.py and their switches.  The upload, the code
table, the handle base and the numbering of the columns are network_pass.py's, shared with those two; here are the caps, the
parameters' packing and the reasons to keep the loop."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .network_pass import FirstUse, Handle, Plan, evaluate_continuous, float_type  # noqa: F401 - Plan: this module's name too

MAX_DISCRETE_FAMILY = 8        # pbn_clgnet_create: a discrete node's variable and 7 parents
MAX_DISCRETE_PARENTS = 7       # ... a CLG node's discrete parents
MAX_CONTINUOUS_FAMILY = 64     # ... a CLG node's variable and 63 continuous parents (pbn_lg_logl's cap)
MAX_CONFIGS = 2 ** 20          # PBN_CLGNET_MAX_CONFIGS: configurations of one CLG node
MAX_PARAMS = 2 ** 28           # PBN_CLGNET_MAX_PARAMS: doubles on the device, a CPT cell one and a record p + 3

DISCRETE, CLG = 0, 1

# what the calls of this process did (tests, tools): handles created and the pbn_clgnet_stats of the evaluations
counters = {"clgnet_created": 0, "launches": 0, "rows_evaluated": 0}


def enabled():
    return os.environ.get("PBN_CLG_MODEL", "1").strip() != "0"


# A plan's fields: the code columns `dcolumns` with their `cardinality` and the continuous columns `ccolumns`; per node its kind and
# var; strides[i]: of node i's key columns (a discrete node: the variable, then its parents; a CLG node: its discrete parents),
# configs[i]: their product.  Node i's parameters are param_off[i] .. param_off[i + 1]: configs[i] CPT cells, or configs[i] records
# of p + 2 doubles; its configuration marks cfg_off[i] .. cfg_off[i + 1] (none for a discrete node).


def build_plan(families, cards):
    """families: [(variable, [discrete parents], None)] for a discrete node and [(variable, [discrete parents], [continuous
    parents])] for a CLG node, in node order; the discrete parents in the FACTOR's order (a CPT follows its evidence, a
    CLinearGaussianCPD's configuration index its `_disc`, the first fastest: _DiscreteAdaptator._config), the continuous ones in the
    order of the coefficients.  cards: discrete column name -> number of categories.  Discrete and continuous columns are each
    numbered in order of first use, so a conditional network's interface columns are columns without a node.  Pure Python: no
    device, no library.

    within_caps is False when a family is beyond pbn_clgnet_create's caps (module constants above), names a column twice or has a
    column without categories: such a network keeps the per-factor loop."""
    dindex, cindex = FirstUse(), FirstUse()
    kind, var, dpar_off, dparents, cpar_off, cparents = [], [], [0], [], [0], []
    strides, configs, cfg_off, param_off = [], [], [0], [0]
    within, device_params = True, 0
    for variable, disc, cont in families:
        disc = list(disc)
        clg = cont is not None
        keys = disc if clg else [variable] + disc
        key_ids = [dindex[name] for name in keys]
        if clg:
            cont = list(cont)
            cont_ids = [cindex[name] for name in [variable] + cont]
            if len(disc) > MAX_DISCRETE_PARENTS or 1 + len(cont) > MAX_CONTINUOUS_FAMILY:
                within = False
        elif len(keys) > MAX_DISCRETE_FAMILY:
            within = False
        if len(set(keys)) != len(keys):
            within = False
        st, cells = [], 1
        for name in keys:
            st.append(cells)
            cells *= int(cards[name])
        if cells < 1 or (clg and cells > MAX_CONFIGS):
            within = False
        kind.append(CLG if clg else DISCRETE)
        var.append(cont_ids[0] if clg else key_ids[0])
        dparents.extend(key_ids if clg else key_ids[1:])
        dpar_off.append(len(dparents))
        if clg:
            cparents.extend(cont_ids[1:])
        cpar_off.append(len(cparents))
        strides.append(st)
        configs.append(cells)
        cfg_off.append(cfg_off[-1] + (cells if clg else 0))
        param_off.append(param_off[-1] + (cells * (len(cont) + 2) if clg else cells))
        device_params += cells * (len(cont) + 3) if clg else cells
    dcolumns, ccolumns = list(dindex), list(cindex)
    if device_params > MAX_PARAMS or not dcolumns or not ccolumns:
        within = False
    return Plan(dcolumns=dcolumns, cardinality=[int(cards[c]) for c in dcolumns], ccolumns=ccolumns, kind=kind, var=var, dpar_off=dpar_off,
                dparents=dparents, cpar_off=cpar_off, cparents=cparents, strides=strides, configs=configs, cfg_off=cfg_off, param_off=param_off,
                within_caps=within)


def clg_factors(model):
    """Every node holds a factor that is exactly DiscreteFactor, LinearGaussianCPD or CLinearGaussianCPD (a Python subclass, an HCKDE
    or a CKDE keeps the per-factor loop), and the network is neither all-DiscreteFactor nor all-LinearGaussianCPD (those have their
    own one-pass paths and switches)."""
    from .factors import CLinearGaussianCPD, DiscreteFactor, LinearGaussianCPD

    cpds = getattr(model, "_cpds", None) or {}
    types = [type(cpds.get(n)) for n in model._nodes]
    if not types or any(t not in (DiscreteFactor, LinearGaussianCPD, CLinearGaussianCPD) for t in types):
        return False
    return not all(t is DiscreteFactor for t in types) and not all(t is LinearGaussianCPD for t in types)


def _factor_family(f):
    """(variable, discrete parents, continuous parents or None, categories of the key columns, the per-configuration
    LinearGaussianCPDs or None); None for a factor that does not carry what its kind carries."""
    from .factors import DiscreteFactor, LinearGaussianCPD

    variable = f.variable()
    if type(f) is DiscreteFactor:
        cats = getattr(f, "_categories", None)
        evidence = list(f.evidence())
        if cats is None or len(cats) != 1 + len(evidence):
            return None
        return variable, evidence, None, cats, None
    if type(f) is LinearGaussianCPD:
        return variable, [], list(f.evidence()), [], [f]
    disc, cont, factors, cats = (getattr(f, a, None) for a in ("_disc", "_cont", "_factors", "_categories"))
    if disc is None or cont is None or factors is None or cats is None or len(cats) != len(disc):
        return None
    return variable, list(disc), list(cont), cats, list(factors)


def _evaluation(model, rb):
    """(plan, discrete arrow columns, params, present) of a fitted qualifying model on `rb`; None when the per-factor loop must run
    (and raise what it raises): a column that is missing, a discrete column that is not a dictionary or whose categories are not the
    factor's, continuous columns that are not all float64 or all float32, parameters that do not fit their family, a family beyond
    the caps."""
    import pyarrow as pa

    from .factors import LinearGaussianCPD

    described = [_factor_family(model._cpds[n]) for n in model._nodes]
    if any(d is None for d in described):
        return None
    dcols, cards = {}, {}
    for variable, disc, cont, cats, _ in described:
        for name, want in zip(disc if cont is not None else [variable] + disc, cats):
            if name not in dcols:
                idx = rb.schema.get_field_index(name)
                if idx < 0 or not pa.types.is_dictionary(rb.schema.field(idx).type):
                    return None
                dcols[name] = (rb.column(idx), rb.column(idx).dictionary.to_pylist())
                cards[name] = len(dcols[name][1])
            if dcols[name][1] != list(want):
                return None   # the loop raises "does not contain the same categories"
    plan = build_plan([(v, d, c) for v, d, c, _, _ in described], cards)
    if not plan.within_caps or float_type(rb, plan.ccolumns) is None:
        return None
    params = np.zeros(plan.param_off[-1], dtype=np.float64)
    present = np.zeros(max(plan.cfg_off[-1], 1), dtype=np.uint8)
    for i, (variable, disc, cont, _, factors) in enumerate(described):
        lo, hi = plan.param_off[i], plan.param_off[i + 1]
        if cont is None:
            lp = np.asarray(model._cpds[variable]._logprob, dtype=np.float64).reshape(-1)
            if lp.size != hi - lo:
                return None   # a table that is not its categories' (set by hand): the per-factor loop reports it
            params[lo:hi] = lp
            continue
        if len(factors) != plan.configs[i]:
            return None
        w = len(cont) + 2
        for c, sub in enumerate(factors):
            if sub is None:
                continue   # a configuration without rows, or whose fit was dropped: its rows are NaN
            if type(sub) is not LinearGaussianCPD or not sub.fitted() or sub.variable() != variable or list(sub.evidence()) != cont:
                return None
            b = np.asarray(sub.beta, dtype=np.float64).reshape(-1)
            if b.size != len(cont) + 1:
                return None   # coefficients set by hand that do not fit the evidence: the per-factor loop reports it
            params[lo + c * w: lo + c * w + w - 1] = b
            params[lo + c * w + w - 1] = float(sub.variance)
            present[plan.cfg_off[i] + c] = 1
    return plan, [dcols[c][0] for c in plan.dcolumns], params, present


class _CLGNet(Handle):
    prefix, counters, stat_keys = "pbn_clgnet", counters, ("launches", "rows_evaluated")

    def __init__(self, ctx, plan, params, present):
        self._keep = (np.ascontiguousarray(params, dtype=np.float64), np.ascontiguousarray(present, dtype=np.uint8),
                      np.ascontiguousarray(plan.param_off, dtype=np.int64))
        params, present, param_off = self._keep
        super().__init__(
            ctx.handle, len(plan.dcolumns), _lib.int_array(plan.cardinality), len(plan.ccolumns), len(plan.var), _lib.int_array(plan.kind),
            _lib.int_array(plan.var), _lib.int_array(plan.dpar_off), _lib.int_array(plan.dparents or [0]), _lib.int_array(plan.cpar_off),
            _lib.int_array(plan.cparents or [0]), _lib.int_array(plan.cfg_off), present.ctypes.data_as(C.POINTER(C.c_ubyte)),
            param_off.ctypes.data_as(C.POINTER(C.c_int64)), _lib.dptr(params))
        self.n_nodes = len(plan.var)
        counters["clgnet_created"] += 1

    def logl(self, codes, table):
        out = np.empty(table.num_rows, dtype=np.float64)
        _lib.check(_lib.load().pbn_clgnet_logl(self.handle, codes.handle, table.handle, _lib.dptr(out)))
        return out

    def node_slogl(self, codes, table):
        out = np.zeros(self.n_nodes, dtype=np.float64)
        _lib.check(_lib.load().pbn_clgnet_slogl(self.handle, codes.handle, table.handle, _lib.dptr(out)))
        return out


def _evaluate(model, rb, what):
    ev = _evaluation(model, rb)
    if ev is None:
        return None
    plan, dcols, params, present = ev
    return evaluate_continuous(rb, plan.ccolumns, lambda ctx: _CLGNet(ctx, plan, params, present), what, dcols, plan.cardinality)


def network_logl(model, rb):
    """Per-row log-likelihood: the nodes' values added in node order on the device, NaN where a row is null in any continuous
    column of the network (it is NaN in that factor's logl and so in the loop's sum); None when the per-factor loop must run."""
    return _evaluate(model, rb, "logl")


def network_node_slogl(model, rb):
    """The nodes' summed log-likelihoods in node order (float64 array), a NaN row counting 0 as in DiscreteFactor.slogl's nansum and
    the adaptator's skipped configurations; None when the loop must run: also when a continuous column of the network has nulls (each
    factor then sums over its own family's valid rows).  Nulls in discrete columns are served."""
    return _evaluate(model, rb, "node_slogl")
