"""Constraint-based structure learning: PC, MMPC and the Meek rules (learning/algorithms/pc.{hpp,cpp}, mmpc.cpp:996-1135,
constraint.hpp) over any IndependenceTest.  The searches run in the library (csrc/pc.hip, csrc/mmpc.hip); a test that has a batched
native callback is asked for all mutually independent p-values of a skeleton level, or of the v-structure phase, in one call.

Single process only: unlike `mmpc_cpcs`, PC does not shard its batches over the ranks of a process group."""
import ctypes as C

from . import _lib
from .graph import ConditionalPartiallyDirectedGraph, PartiallyDirectedGraph
from .independences import mmpc_cpcs, validate_restrictions


def _flat(pairs):
    return _lib.int_array([v for p in pairs for v in p] or [0])


def _name_rank(names):
    order = sorted(range(len(names)), key=lambda i: names[i].encode())
    rank = [0] * len(names)
    for pos, i in enumerate(order):
        rank[i] = pos
    return _lib.int_array(rank)


def _callbacks(test, names, batched):
    fn, user, keep, errors = test._ci_callback(list(names))
    batch = None
    if batched is None or batched is True:
        get = getattr(test, "_pc_batch_callback", None) or getattr(test, "_ci_batch_callback", None)
        batch = get() if get else None
    elif batched:
        batch = batched   # a pbn_ci_pvalue_batch_fn of the caller's
    return fn, batch, user, keep, errors


def _band(test, band):
    """The caller's band; left at -1, the test's own (`_pc_band`) when it has one - a batch whose rounding differs from the built-in
    band's measurement brings its own."""
    if band < 0:
        own = getattr(test, "_pc_band", None)
        if own is not None:
            return float(own())
    return float(band)


def _pairs(buf, count):
    return [(buf[2 * i], buf[2 * i + 1]) for i in range(count)]


def pc_estimate_indices(test, names, n_interface=0, alpha=0.05, arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(),
                        use_sepsets=False, ambiguous_threshold=0.5, allow_bidirected=True, batched=None, band=-1.0):
    """pbn_pc_estimate over `names` (the last n_interface are interface nodes) with index-pair restriction lists as validate_restrictions
    returns them.  batched: None = the test's own batch callback when it has one, False = the serial search, or a _lib.CI_BATCH_FN.
    Returns a dict: arcs, edges (index pairs), sepsets {(a, b): (sorted set, p-value)}, serial_tests, evaluated, band_redone."""
    n = len(names)
    fn, batch, user, keep, errors = _callbacks(test, names, batched)
    cap = max(1, n * (n - 1))
    arcs, edges = (C.c_int * (2 * cap))(), (C.c_int * (2 * cap))()
    n_arcs, n_edges, n_sep = C.c_int(0), C.c_int(0), C.c_int(0)
    sep_pair, sep_off = (C.c_int * (cap + 2))(), (C.c_int * (cap // 2 + 2))()
    sep_set, sep_p = (C.c_int * (n * (cap // 2) + 1))(), (C.c_double * (cap // 2 + 1))()
    tests = (C.c_int64 * 3)()
    rc = _lib.load().pbn_pc_estimate(n, int(n_interface), fn, batch, user, float(alpha), _band(test, band), len(arc_blacklist), _flat(arc_blacklist),
                                     len(arc_whitelist), _flat(arc_whitelist), len(edge_blacklist), _flat(edge_blacklist), len(edge_whitelist),
                                     _flat(edge_whitelist), int(bool(use_sepsets)), float(ambiguous_threshold), int(bool(allow_bidirected)),
                                     _name_rank(list(names)), C.byref(n_arcs), arcs, C.byref(n_edges), edges, C.byref(n_sep), sep_pair, sep_off,
                                     sep_set, sep_p, tests)
    if errors:
        raise errors[0]
    try:
        _lib.check(rc)
    except ValueError as ex:
        if "not found in sepset" in str(ex):   # std::out_of_range in the reference: use_sepsets with a pair the edge blacklist separated
            raise IndexError(str(ex)) from None
        raise
    del keep
    seps = {}
    for q in range(n_sep.value):
        seps[(sep_pair[2 * q], sep_pair[2 * q + 1])] = (sorted(sep_set[j] for j in range(sep_off[q], sep_off[q + 1])), sep_p[q])
    return {"arcs": _pairs(arcs, n_arcs.value), "edges": _pairs(edges, n_edges.value), "sepsets": seps, "serial_tests": tests[0],
            "evaluated": tests[1], "band_redone": tests[2]}


def pdag_orient_indices(test, names, n_interface, alpha, arcs, edges, arc_blacklist=(), arc_whitelist=(), allow_bidirected=True, batched=None,
                        band=-1.0):
    """pbn_pdag_orient: a given graph (index pairs) -> direct_arc_blacklist -> v-structures by the threshold-0 search -> Meek rules."""
    n = len(names)
    fn, batch, user, keep, errors = _callbacks(test, names, batched)
    cap = max(1, n * (n - 1))
    out_arcs, out_edges = (C.c_int * (2 * cap))(), (C.c_int * (2 * cap))()
    n_arcs, n_edges = C.c_int(0), C.c_int(0)
    tests = (C.c_int64 * 3)()
    rc = _lib.load().pbn_pdag_orient(n, int(n_interface), fn, batch, user, float(alpha), _band(test, band), len(arcs), _flat(arcs), len(edges), _flat(edges),
                                     len(arc_blacklist), _flat(arc_blacklist), len(arc_whitelist), _flat(arc_whitelist), int(bool(allow_bidirected)),
                                     _name_rank(list(names)), C.byref(n_arcs), out_arcs, C.byref(n_edges), out_edges, tests)
    if errors:
        raise errors[0]
    _lib.check(rc)
    del keep
    return {"arcs": _pairs(out_arcs, n_arcs.value), "edges": _pairs(out_edges, n_edges.value), "serial_tests": tests[0], "evaluated": tests[1],
            "band_redone": tests[2]}


def _graph(nodes, interface_nodes, res):
    names = list(nodes) + list(interface_nodes)
    arcs = [(names[a], names[b]) for a, b in res["arcs"]]
    edges = [(names[a], names[b]) for a, b in res["edges"]]
    if interface_nodes:
        return ConditionalPartiallyDirectedGraph(nodes, interface_nodes, arcs, edges)
    return PartiallyDirectedGraph(nodes, arcs, edges)


def _check_options(alpha, ambiguous_threshold):
    if alpha <= 0 or alpha >= 1:
        raise ValueError("alpha must be a number between 0 and 1.")
    if ambiguous_threshold < 0 or ambiguous_threshold > 1:
        raise ValueError("ambiguous_threshold must be a number between 0 and 1.")


class MeekRules:
    """MeekRules.rule1 / rule2 / rule3(pdag) (constraint.hpp:391-509): orient in place, return whether anything changed."""

    @staticmethod
    def _apply(rule, pdag):
        names = pdag.nodes() + pdag.interface_nodes()
        idx = {v: i for i, v in enumerate(names)}
        n = len(names)
        arcs = [(idx[s], idx[t]) for s, t in pdag.arcs()]
        edges = [(idx[a], idx[b]) for a, b in pdag.edges()]
        cap = max(1, n * (n - 1))
        out_arcs, out_edges = (C.c_int * (2 * cap))(), (C.c_int * (2 * cap))()
        n_arcs, n_edges, changed = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(_lib.load().pbn_meek_rule(rule, n, len(arcs), _flat(arcs), len(edges), _flat(edges), C.byref(n_arcs), out_arcs, C.byref(n_edges),
                                            out_edges, C.byref(changed)))
        have = set(arcs)
        for s, t in _pairs(out_arcs, n_arcs.value):
            if (s, t) not in have:
                pdag.direct(names[s], names[t])
        return bool(changed.value)

    @staticmethod
    def rule1(pdag):
        return MeekRules._apply(1, pdag)

    @staticmethod
    def rule2(pdag):
        return MeekRules._apply(2, pdag)

    @staticmethod
    def rule3(pdag):
        return MeekRules._apply(3, pdag)


class PC:
    """pbn.PC(): the PC-stable algorithm (learning/algorithms/pc.cpp) over any IndependenceTest."""

    def estimate(self, hypot_test, nodes=(), arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(), alpha=0.05, use_sepsets=False,
                 ambiguous_threshold=0.5, allow_bidirected=True, verbose=0):
        _check_options(alpha, ambiguous_threshold)
        nodes = list(nodes)
        if not nodes:
            nodes = list(hypot_test.variable_names())
        elif not hypot_test.has_variables(nodes):
            raise ValueError("IndependenceTest do not contain all the variables in nodes list.")
        return self._run(hypot_test, nodes, [], arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, use_sepsets, ambiguous_threshold,
                         allow_bidirected)

    def estimate_conditional(self, hypot_test, nodes, interface_nodes=(), arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(),
                             alpha=0.05, use_sepsets=False, ambiguous_threshold=0.5, allow_bidirected=True, verbose=0):
        _check_options(alpha, ambiguous_threshold)
        nodes, interface_nodes = list(nodes), list(interface_nodes)
        if not nodes:
            raise ValueError("Node list cannot be empty to train a Conditional graph.")
        if not interface_nodes:
            return self.estimate(hypot_test, nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, use_sepsets, ambiguous_threshold,
                                 allow_bidirected, verbose).conditional_graph()
        if not hypot_test.has_variables(nodes) or not hypot_test.has_variables(interface_nodes):
            raise ValueError("IndependenceTest do not contain all the variables in nodes/interface_nodes lists.")
        return self._run(hypot_test, nodes, interface_nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, use_sepsets,
                         ambiguous_threshold, allow_bidirected)

    def _run(self, test, nodes, interface_nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, use_sepsets, ambiguous_threshold,
             allow_bidirected):
        names = nodes + interface_nodes
        a_bl, a_wl, e_bl, e_wl = validate_restrictions(names, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist)
        res = pc_estimate_indices(test, names, len(interface_nodes), alpha, a_bl, a_wl, e_bl, e_wl, use_sepsets, ambiguous_threshold, allow_bidirected)
        self.last_search = {k: res[k] for k in ("sepsets", "serial_tests", "evaluated", "band_redone")}
        return _graph(nodes, interface_nodes, res)


class MMPC:
    """pbn.MMPC(): max-min parents and children of every node (mmpc.cpp:996-1135), an edge for every pair that chose each other, then
    v-structures and the Meek rules."""

    def estimate(self, hypot_test, nodes=(), arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(), alpha=0.05,
                 ambiguous_threshold=0.5, allow_bidirected=True, verbose=0):
        """`ambiguous_threshold` is accepted and checked but, as in the reference, has no effect: MMPC keeps no separating sets, and the
        v-structure search it then runs is the one with threshold 0 (constraint.hpp:219-222)."""
        _check_options(alpha, ambiguous_threshold)
        nodes = list(nodes)
        if not nodes:
            nodes = list(hypot_test.variable_names())
        elif not hypot_test.has_variables(nodes):
            raise ValueError("IndependenceTest do not contain all the variables in nodes list.")
        return self._run(hypot_test, nodes, [], arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, allow_bidirected)

    def estimate_conditional(self, hypot_test, nodes, interface_nodes=(), arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(),
                             alpha=0.05, ambiguous_threshold=0.5, allow_bidirected=True, verbose=0):
        """See `estimate` for `ambiguous_threshold`."""
        _check_options(alpha, ambiguous_threshold)
        nodes, interface_nodes = list(nodes), list(interface_nodes)
        if not nodes:
            raise ValueError("Node list cannot be empty to train a Conditional graph.")
        if not interface_nodes:
            return self.estimate(hypot_test, nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, ambiguous_threshold,
                                 allow_bidirected, verbose).conditional_graph()
        if not hypot_test.has_variables(nodes) or not hypot_test.has_variables(interface_nodes):
            raise ValueError("IndependenceTest do not contain all the variables in nodes/interface_nodes lists.")
        return self._run(hypot_test, nodes, interface_nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, allow_bidirected)

    def _run(self, test, nodes, interface_nodes, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist, alpha, allow_bidirected):
        names = nodes + interface_nodes
        idx = {v: i for i, v in enumerate(names)}
        a_bl, a_wl, e_bl, e_wl = validate_restrictions(names, arc_blacklist, arc_whitelist, edge_blacklist, edge_whitelist)
        cpcs, _ = mmpc_cpcs(test, nodes, alpha, a_wl, e_bl, e_wl, symmetric=False, interface_nodes=interface_nodes)
        cpcs = [[idx[v] for v in c] for c in cpcs]
        arcs, edges = skeleton_from_cpcs(cpcs, len(nodes), a_wl)
        res = pdag_orient_indices(test, names, len(interface_nodes), alpha, arcs, edges, a_bl, a_wl, allow_bidirected)
        return _graph(nodes, interface_nodes, res)


def skeleton_from_cpcs(cpcs, n_nodes, arc_whitelist):
    """mmpc.cpp:1009-1040: the whitelisted arcs, then an edge for every pair of variables that hold each other as candidates and carry no
    arc - an arc out of the interface node when one end is one.  Index pairs; variables n_nodes ... are interface nodes."""
    arcs = dict.fromkeys((a, b) for a, b in arc_whitelist)
    edges = []
    for i in range(n_nodes):
        for p in cpcs[i]:
            if i < p and i in cpcs[p] and (i, p) not in arcs and (p, i) not in arcs:
                if p >= n_nodes:
                    arcs[(p, i)] = None
                else:
                    edges.append((i, p))
    return list(arcs), edges
