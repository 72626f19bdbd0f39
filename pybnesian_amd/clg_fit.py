"""Fit of a network's conditional linear Gaussian nodes in one device pass (csrc/clg_fit.hip): BayesianNetwork.fit
(models/BayesianNetwork.hpp:960-994) hands its unfitted factors to `fit_nodes` once, before the per-factor loop, instead of running
_DiscreteAdaptator.fit (factors/discrete/DiscreteAdaptator.hpp:201-276) per node: per configuration of the node's discrete parents a
pass over all rows on the host, an arrow take, an upload of the slice, one Gram launch and a wait.

One pbn_dtable of the discrete codes and one pbn_clg_fit call on the continuous upload - the shared one inside BayesianNetwork.fit -
per call of `fit_nodes`.  The decision is per NODE: a node is served when its factor is exactly CLinearGaussianCPD with at least one
discrete parent, its family is within the caps below, its continuous columns are present, of one float type and without nulls, and its
discrete parents are dictionary columns; every other node keeps the per-factor loop, which also raises whatever is to be raised.  In a
call that serves at least one such node the unfitted nodes that are exactly DiscreteFactor are fitted from ONE family-count call on the
same code table.  `PBN_CLG_FIT=0` (read per call) restores the loop.  The numbering of the columns, the code table and the arrow-side
checks are network_pass.py's; here are the caps, the packing of the cells and the reasons to keep the loop."""
import ctypes as C
import os

import numpy as np

from . import _lib
from .network_pass import CodeTable, FirstUse, Plan, codes, float_type, has_nulls

MAX_FAMILY = 8                 # pbn_clg_fit: a node's variable and 7 continuous parents
MAX_DISCRETE_PARENTS = 7       # ... its discrete parents (at least one)
MAX_CONFIGS = 256              # PBN_CLG_FIT_MAX_CONFIGS: configurations of one node
TILE_ROWS = 1024               # PBN_CLG_FIT_TILE_ROWS: rows of a workgroup's tile (the tests' launch shapes)
MAX_DISCRETE_FAMILY = 8        # pbn_dtable_family_counts' device form: the variable and 7 parents
MAX_DISCRETE_CELLS = 2 ** 31 - 1
MAX_CHUNKS = 512               # clg_fit.hip's FIT_MAX_CHUNKS: chunk records of a cell
MAX_RECORD_BYTES = 2 ** 30     # device memory one call may take for its chunk records; the nodes beyond it keep the loop
VARIANCE_TOL = 1.4901161193847656e-08   # CLinearGaussianCPD._fit_base: a fit below it, or an infinite one, is dropped

# what the calls of this process did (tests, tools)
counters = {"calls": 0, "launches": 0, "nodes_served": 0, "cells_fitted": 0, "cells_refitted": 0, "discrete_nodes_fitted": 0}


def enabled():
    return os.environ.get("PBN_CLG_FIT", "1").strip() != "0"


def _cells(names, cards):
    cells = 1
    for name in names:
        cells *= int(cards[name])
    return cells


def record_bytes(cells, d, rows):
    """Device memory pbn_clg_fit takes for the chunk records of a node of `cells` configurations and d continuous columns on a table of
    `rows` rows: chunks x cells x (1 + d + d (d + 1) / 2) doubles, with clg_fit.hip's chunks - ceil(tiles / 512) tiles of 1 024 rows each."""
    tiles = -(-int(rows) // TILE_ROWS)
    chunks = -(-tiles // -(-tiles // MAX_CHUNKS)) if tiles else 0
    return 8 * chunks * int(cells) * (1 + d + d * (d + 1) // 2)


def within_caps(family, cards):
    """One family of build_plan's against the caps of pbn_clg_fit (a CLG node) or of the family counts (a discrete node)."""
    variable, disc, cont = family
    disc = list(disc)
    if cont is None:
        names = [variable] + disc
        return len(names) <= MAX_DISCRETE_FAMILY and len(set(names)) == len(names) and 1 <= _cells(names, cards) <= MAX_DISCRETE_CELLS
    return (1 <= len(disc) <= MAX_DISCRETE_PARENTS and 1 + len(cont) <= MAX_FAMILY and len(set(disc)) == len(disc)
            and 1 <= _cells(disc, cards) <= MAX_CONFIGS)


def build_plan(families, cards):
    """families: [(variable, [discrete parents], [continuous parents])] for a CLG node and [(variable, [discrete parents], None)] for
    a discrete node; the discrete parents in the FACTOR's order (a CLinearGaussianCPD's configuration index follows its `_disc`, the
    first fastest: _DiscreteAdaptator._config; a CPT its evidence), the continuous ones in the order of the coefficients.  cards:
    discrete column name -> number of categories.  Pure Python: no device, no library.

    The decision is per family: `served[i]` is False for a family beyond the caps (within_caps), which then takes no part in the plan -
    its columns are not numbered either.  Discrete and continuous columns are each numbered in order of first use by the served
    families.  The CLG nodes, in order: `nodes` (their positions in `families`), var / cpar_off / cparents (continuous numbers),
    dpar_off / dparents (discrete numbers), strides[k] and configs[k]; node k's cells are cell_off[k] .. cell_off[k + 1], its records
    (p + 2 doubles a cell) param_off[k] .. param_off[k + 1].  The discrete nodes: `discrete`, a plan CodeTable.family_counts takes
    (var, par_off, parents, cpt_off) with `nodes` beside it."""
    dindex, cindex = FirstUse(), FirstUse()
    served = [within_caps(f, cards) for f in families]
    nodes, var, dpar_off, dparents, cpar_off, cparents = [], [], [0], [], [0], []
    strides, configs, cell_off, param_off = [], [], [0], [0]
    dnodes, dvar, dfam_off, dfam, cpt_off = [], [], [0], [], [0]
    for i, (variable, disc, cont) in enumerate(families):
        if not served[i]:
            continue
        disc = list(disc)
        if cont is None:
            ids = [dindex[name] for name in [variable] + disc]
            dnodes.append(i)
            dvar.append(ids[0])
            dfam.extend(ids[1:])
            dfam_off.append(len(dfam))
            cpt_off.append(cpt_off[-1] + _cells([variable] + disc, cards))
            continue
        cont = list(cont)
        key_ids = [dindex[name] for name in disc]
        cont_ids = [cindex[name] for name in [variable] + cont]
        st, cells = [], 1
        for name in disc:
            st.append(cells)
            cells *= int(cards[name])
        d = len(cont_ids)
        nodes.append(i)
        var.append(cont_ids[0])
        dparents.extend(key_ids)
        dpar_off.append(len(dparents))
        cparents.extend(cont_ids[1:])
        cpar_off.append(len(cparents))
        strides.append(st)
        configs.append(cells)
        cell_off.append(cell_off[-1] + cells)
        param_off.append(param_off[-1] + cells * (d + 1))
    dcolumns = list(dindex)
    return Plan(served=served, dcolumns=dcolumns, cardinality=[int(cards[c]) for c in dcolumns], ccolumns=list(cindex), nodes=nodes, var=var,
                dpar_off=dpar_off, dparents=dparents, cpar_off=cpar_off, cparents=cparents, strides=strides, configs=configs, cell_off=cell_off,
                param_off=param_off,
                discrete=Plan(nodes=dnodes, var=dvar, par_off=dfam_off, parents=dfam, cpt_off=cpt_off))


def _dictionary(rb, name):
    """The arrow dictionary column `name` of rb; None when it is missing or not a dictionary (the loop raises)."""
    import pyarrow as pa

    idx = rb.schema.get_field_index(name)
    if idx < 0 or not pa.types.is_dictionary(rb.schema.field(idx).type):
        return None
    return rb.column(idx)


def _clg_family(f, rb):
    """(variable, discrete parents, continuous parents, float type) of a CLinearGaussianCPD as _DiscreteAdaptator.fit would split its
    evidence on `rb`; None when the loop must run: an evidence column that is missing or neither a dictionary nor floating (the loop
    raises), no discrete parent, continuous columns that are missing, not all float64 or all float32, or hold nulls - or whose FIRST
    row is not finite (a non-null NaN or inf): that value is the pass's pilot shift of the column and would reach every configuration,
    where the loop confines it to the one that holds the row."""
    import math

    import pyarrow as pa

    disc, cont = [], []
    for e in f.evidence():
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
    columns = [f.variable()] + cont
    ftype = float_type(rb, columns)
    if not disc or ftype is None or has_nulls(rb, columns):
        return None
    if rb.num_rows and not all(math.isfinite(rb.column(rb.schema.get_field_index(c))[0].as_py()) for c in columns):
        return None
    return f.variable(), disc, cont, ftype


def plan_nodes(model, rb, todo):
    """Which of the nodes `todo` (their factors built, unfitted) one pass serves on `rb`, without a device: (plan, families, names)
    with families[i] the build_plan family of node names[i] and plan.served[i] whether it is served; None when no CLG node is.  The
    continuous columns of the served CLG nodes are of ONE float type, the first served node's: they share a pbn_table.  Their chunk
    records together stay within MAX_RECORD_BYTES of device memory: a node that would pass it keeps the loop (which needs no such
    buffer), the later ones are still tried."""
    from .factors import CLinearGaussianCPD, DiscreteFactor

    families, names, cards = [], [], {}
    ftype, taken = None, 0

    def categorical(columns):
        for name in columns:
            if name not in cards:
                col = _dictionary(rb, name)
                if col is None:
                    return False
                cards[name] = len(col.dictionary)
        return True

    for n in todo:
        f = model._cpds[n]
        if type(f) is CLinearGaussianCPD:
            fam = _clg_family(f, rb)
            if fam is None or (ftype is not None and fam[3] != ftype):
                continue
            categorical(fam[1])   # (dictionary columns: _clg_family saw them)
            if not within_caps(fam[:3], cards):
                continue
            need = record_bytes(_cells(fam[1], cards), 1 + len(fam[2]), rb.num_rows)
            if taken + need > MAX_RECORD_BYTES:
                continue
            ftype, taken = fam[3], taken + need
            families.append(fam[:3])
            names.append(n)
        elif type(f) is DiscreteFactor:
            family = [f.variable()] + list(f.evidence())
            if categorical(family):
                families.append((f.variable(), list(f.evidence()), None))
                names.append(n)
    plan = build_plan(families, cards)
    if not plan.nodes:
        return None
    return plan, families, names


def _pass(plan, rb):
    """The device side of one call: (code arrays, rows, params, status) of the plan's CLG cells and the family counts of its discrete
    nodes; None when the upload at hand does not hold the plan's continuous columns row for row."""
    from .dataset import DeviceTable, default_context

    ctx = default_context()
    table, mask = DeviceTable.from_dataframe(ctx, rb, plan.ccolumns)   # inside BayesianNetwork.fit: the shared upload
    if mask is not None or table.num_rows != rb.num_rows:
        return None
    cidx = table.index(plan.ccolumns)
    code_arrays = [codes(_dictionary(rb, name)) for name in plan.dcolumns]
    n_cells = plan.cell_off[-1]
    i64 = lambda values: np.ascontiguousarray(values, dtype=np.int64)
    i64p = C.POINTER(C.c_int64)
    cell_off, param_off = i64(plan.cell_off), i64(plan.param_off)
    rows = np.zeros(max(n_cells, 1), dtype=np.int64)
    params = np.zeros(max(plan.param_off[-1], 1), dtype=np.float64)
    status = np.zeros(max(n_cells, 1), dtype=np.uint8)
    launches = C.c_int64(0)
    with CodeTable(ctx, code_arrays, plan.cardinality, rb.num_rows) as ctable:
        _lib.check(_lib.load().pbn_clg_fit(
            ctx.handle, ctable.handle, table.handle, len(plan.var), _lib.int_array([cidx[v] for v in plan.var]), _lib.int_array(plan.dpar_off),
            _lib.int_array(plan.dparents), _lib.int_array(plan.cpar_off), _lib.int_array([cidx[v] for v in plan.cparents] or [0]),
            cell_off.ctypes.data_as(i64p), param_off.ctypes.data_as(i64p), rows.ctypes.data_as(i64p), _lib.dptr(params),
            status.ctypes.data_as(C.POINTER(C.c_ubyte)), None, None, C.byref(launches)))   # (the raw shifts and moments are the tests')
        counts = ctable.family_counts(plan.discrete) if plan.discrete.nodes else None
    counters["launches"] += launches.value
    return code_arrays, rows, params, status, counts


def fit_nodes(model, rb, todo):
    """Fit those of the nodes `todo` - their factors built and unfitted - that one pass serves; the others are left as they are, for the
    per-factor loop.  Returns the names of the nodes fitted here.

    A served CLinearGaussianCPD ends as _DiscreteAdaptator.fit leaves it: `_disc`, `_cont`, `_categories`, and per configuration a
    LinearGaussianCPD, or None for a configuration without rows or whose variance is below 1.49e-8 or infinite.  A configuration the
    C side marks suspect (nearly collinear parents, a nearly exact fit) is refitted the loop's way - take the rows, LinearGaussianCPD.fit
    - and is then the loop's bit for bit.  A DiscreteFactor ends bit-identical to DiscreteFactor.fit."""
    import pyarrow as pa

    from .factors import LinearGaussianCPD, _logprob_from_counts

    if not enabled() or not todo:
        return []
    planned = plan_nodes(model, rb, todo)
    if planned is None:
        return []
    plan, families, names = planned
    out = _pass(plan, rb)
    if out is None:
        return []
    code_arrays, rows, params, status, counts = out
    counters["calls"] += 1
    column_of = {name: k for k, name in enumerate(plan.dcolumns)}
    categories = {}

    def cats(name):
        if name not in categories:
            categories[name] = _dictionary(rb, name).dictionary.to_pylist()
        return categories[name]

    fitted = []
    for k, i in enumerate(plan.nodes):
        variable, disc, cont = families[i]
        f = model._cpds[names[i]]
        f._fitted = False
        f._disc, f._cont = list(disc), list(cont)
        f._categories = [list(cats(d)) for d in disc]
        f._factors = []
        w = len(cont) + 2
        key = valid = None
        for c in range(plan.configs[k]):
            cell = plan.cell_off[k] + c
            if status[cell] == 0:
                f._factors.append(None)
                continue
            if status[cell] == 1:
                rec = params[plan.param_off[k] + c * w: plan.param_off[k] + (c + 1) * w]
                sub = LinearGaussianCPD(variable, list(cont))
                sub.beta, sub.variance, sub._fitted = np.array(rec[:w - 1], dtype=np.float64), float(rec[w - 1]), True
                counters["cells_fitted"] += 1
                f._factors.append(None if (sub.variance < VARIANCE_TOL or np.isinf(sub.variance)) else sub)
                continue
            # suspect: the loop's own fit of this configuration (_DiscreteAdaptator.fit)
            if key is None:
                key = np.zeros(rb.num_rows, dtype=np.int64)
                valid = np.ones(rb.num_rows, dtype=bool)
                for d, stride in zip(disc, plan.strides[k]):
                    col = code_arrays[column_of[d]]
                    valid &= col >= 0
                    key += np.where(col >= 0, col, 0).astype(np.int64) * stride
            take = np.nonzero(valid & (key == c))[0]
            sub = f._base(f._cont)
            ok = f._fit_base(sub, rb.take(pa.array(take.astype(np.int32))))
            counters["cells_refitted"] += 1
            f._factors.append(sub if ok else None)
        f._fitted = True
        counters["nodes_served"] += 1
        fitted.append(names[i])
    dp = plan.discrete
    for k, i in enumerate(dp.nodes):
        variable, evidence, _ = families[i]
        f = model._cpds[names[i]]
        family = [variable] + list(evidence)
        f._fitted = False
        f._categories = [list(cats(n)) for n in family]
        f._cards = [len(cats(n)) for n in family]
        f._logprob = _logprob_from_counts(counts[dp.cpt_off[k]: dp.cpt_off[k + 1]], f._cards[0])
        f._fitted = True
        counters["discrete_nodes_fitted"] += 1
        fitted.append(names[i])
    return fitted
