"""TEST INFRASTRUCTURE ONLY.  Python restatement of the reference's PC algorithm, function by function, written from the text of
learning/algorithms/pc.cpp (:25-336), learning/algorithms/constraint.hpp (:16-509) and util/combinations.hpp - in the manner of
tests/kmi_restatement.py and oracle/mmpc_oracle.py.  It shares nothing with csrc/pc.hip.

Adjacency sets (neighbours, parents, children) are real libstdc++ std::unordered_set<int> objects (mmpc_oracle.USet), filled and erased in
the reference's order, because the first separating set found - and with it the recorded set, its p-value and the number of tests -
depends on their iteration order, as does the order of the v-structures, which decides the graph when allow_bidirected is false.  The
short-lived sets the reference builds from RANGES (`u`, `possible_sepset`, `remaining_neighbors`) are built the same way through
tests/c/uset_range.cpp: the range constructor sizes the bucket array from the range, which changes the iteration order.

The reference's hash containers of edges, arcs and restriction pairs are not restated: every loop over them collects and then applies,
and the applications commute.  The one exception is the arc whitelist (two whitelisted arcs into one node: the order of
`skeleton.direct` is the insertion order of that node's parents); the restatement, like the engine, applies it in list order.

Nodes are indices 0 ... n-1 with names; interface nodes are the last n_interface of them.  The test is `pvalue(a, b, cond)` over
indices, called in the reference's argument order."""
import ctypes as C
import os
import subprocess
import tempfile

from oracle.mmpc_oracle import USet

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def _rlib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="uset_range_"), "libuset_range.so")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, os.path.join(_HERE, "c", "uset_range.cpp")],
                       check=True, capture_output=True, timeout=300)
        _lib = C.CDLL(out)
        _lib.uset_new.restype = C.c_void_p
        _lib.uset_from_range.restype = C.c_void_p
    return _lib


def _arr(values):
    values = list(values)
    return (C.c_int * max(1, len(values)))(*values), len(values)


class RangeSet:
    """std::unordered_set<int>: RangeSet() is the default constructor, RangeSet(items) the range constructor."""

    def __init__(self, items=None):
        lib = _rlib()
        if items is None:
            self._h = C.c_void_p(lib.uset_new())
        else:
            a, n = _arr(items)
            self._h = C.c_void_p(lib.uset_from_range(a, n))

    def insert(self, v):
        _rlib().uset_insert(self._h, C.c_int(int(v)))

    def insert_range(self, items):
        a, n = _arr(items)
        _rlib().uset_insert_range(self._h, a, n)

    def erase(self, v):
        _rlib().uset_erase(self._h, C.c_int(int(v)))

    def __contains__(self, v):
        return _rlib().uset_count(self._h, C.c_int(int(v))) > 0

    def __len__(self):
        return _rlib().uset_size(self._h)

    def items(self):
        n = len(self)
        buf = (C.c_int * max(1, n))()
        _rlib().uset_items(self._h, buf)
        return [buf[i] for i in range(n)]

    def __iter__(self):
        return iter(self.items())

    def __del__(self):
        try:
            _rlib().uset_free(self._h)
        except Exception:
            pass


# ---- util/combinations.hpp ---------------------------------------------------------------------------------------------------------
def _binomial(n, k):
    import math

    return math.comb(n, k) if 0 <= k <= n else 0


class Combinations:   # :11-156, without a fixed part
    def __init__(self, elements, k):
        self.elements, self.k = list(elements), k
        self.num_combinations = _binomial(len(self.elements), k)

    def iterate(self, count=None):
        count = self.num_combinations if count is None else count
        p = self.k
        indices = list(range(p))
        subset = [self.elements[i] for i in indices] if count > 0 else []
        for idx in range(count):
            yield list(subset)
            # next_subset
            for i in range(p - 1, -1, -1):
                max_index = len(self.elements) - p + i
                if indices[i] < max_index:
                    indices[i] += 1
                    subset[i] = self.elements[indices[i]]
                    for j in range(i + 1, p):
                        indices[j] = indices[j - 1] + 1
                        subset[j] = self.elements[indices[j]]
                    break

    def __iter__(self):
        return self.iterate()


class Combinations2Sets:   # :167-276
    def __init__(self, v1, v2, k):
        v1, v2 = sorted(v1), sorted(v2)
        common = [x for x in v1 if x in v2]   # set_intersection of the sorted vectors
        self.comb1 = Combinations(v1, k)
        if len(common) < k:
            self.comb2 = Combinations(v2, k)
            self.valid2 = self.comb2.num_combinations
        else:
            common_start = len(v2) - len(common)
            for i in range(common_start):
                if v2[i] in common:
                    for j in range(len(v2) - 1, common_start - 1, -1):
                        if v2[j] not in common:
                            v2[i], v2[j] = v2[j], v2[i]
            self.comb2 = Combinations(v2, k)
            self.valid2 = self.comb2.num_combinations - _binomial(len(common), k)
        self.num_combinations = self.comb1.num_combinations + self.valid2

    def __iter__(self):
        yield from self.comb1.iterate()
        if self.valid2 > 0:
            yield from self.comb2.iterate(self.valid2)


# ---- the graph (graph/generic_graph.hpp, the part PC uses) --------------------------------------------------------------------------
class Graph:
    def __init__(self, names, n_interface=0):
        self.names = list(names)
        self.n = len(self.names)
        self.n_interface = n_interface
        self.index = {v: i for i, v in enumerate(self.names)}
        self.nbr = [USet() for _ in range(self.n)]
        self.pa = [USet() for _ in range(self.n)]
        self.ch = [USet() for _ in range(self.n)]
        self.edge_list = {}   # Edge as stored: (first, second)

    @classmethod
    def complete_undirected(cls, names, n_interface=0):   # generic_graph.cpp:6-39
        g = cls(names, n_interface)
        nn = g.n - n_interface
        for i in range(nn - 1):
            for j in range(i + 1, nn):
                g.add_edge(i, j)
        for i in range(nn):
            for j in range(nn, g.n):
                g.add_edge(i, j)
        return g

    def nodes(self):
        return range(self.n - self.n_interface)

    def interface_nodes(self):
        return range(self.n - self.n_interface, self.n)

    def num_edges(self):
        return len(self.edge_list)

    def has_edge(self, a, b):
        return a in self.nbr[b]

    def has_arc(self, s, t):
        return s in self.pa[t]

    def has_connection(self, a, b):
        return self.has_edge(a, b) or self.has_arc(a, b) or self.has_arc(b, a)

    def add_edge(self, a, b):
        self.edge_list[(a, b)] = None
        self.nbr[a].insert(b)
        self.nbr[b].insert(a)

    def remove_edge(self, a, b):
        if self.has_edge(a, b):
            self.edge_list.pop((a, b), None)
            self.edge_list.pop((b, a), None)
            self.nbr[a].erase(b)
            self.nbr[b].erase(a)

    def add_arc(self, s, t):
        self.ch[s].insert(t)
        self.pa[t].insert(s)

    def remove_arc(self, s, t):
        self.ch[s].erase(t)
        self.pa[t].erase(s)

    def direct(self, s, t):   # generic_graph.hpp:2243-2250
        if self.has_edge(s, t):
            self.remove_edge(s, t)
            self.add_arc(s, t)
        elif self.has_arc(t, s):
            self.add_arc(s, t)

    def arcs(self):
        return [(s, t) for s in range(self.n) for t in self.ch[s]]

    def edges(self):
        return list(self.edge_list)

    def direct_interface_edges(self):   # generic_graph.cpp:41-51
        for i in self.interface_nodes():
            for nbr in self.nbr[i].items():
                self.direct(i, nbr)

    def to_dag_check(self):   # generic_graph.hpp:2276-2341, the two ways it fails
        arcs = self.arcs()
        nbr = [set(s) for s in self.nbr]
        pa = [set(s) for s in self.pa]
        ch = [set(s) for s in self.ch]
        for i in self.interface_nodes():
            for v in list(nbr[i]):
                arcs.append((i, v))
                nbr[i].discard(v)
                nbr[v].discard(i)
        indeg = [0] * self.n
        for _, t in arcs:
            indeg[t] += 1
        stack, seen = [v for v in range(self.n) if not indeg[v]], 0
        while stack:
            v = stack.pop()
            seen += 1
            for s, t in arcs:
                if s == v:
                    indeg[t] -= 1
                    if not indeg[t]:
                        stack.append(t)
        if seen != self.n:
            raise ValueError("PDAG contains directed cycles.")
        alive = set(range(self.n))
        connected = lambda a, b: b in nbr[a] or b in pa[a] or b in ch[a]
        while any(nbr[v] for v in alive):
            for x in sorted(alive):
                if ch[x]:
                    continue
                if all(y == z or connected(y, z) for y in nbr[x] for z in nbr[x] | pa[x]):
                    for y in nbr[x]:
                        nbr[y].discard(x)
                    for p in pa[x]:
                        ch[p].discard(x)
                    alive.discard(x)
                    break
            else:
                raise ValueError("PDAG do not allow a valid DAG extension.")


# ---- constraint.hpp:16-41 ---------------------------------------------------------------------------------------------------------
class SepSet:
    def __init__(self):
        self.m_sep = {}

    def insert(self, edge, s, pvalue):
        self.m_sep.setdefault((min(edge), max(edge)), (list(s), pvalue))

    def sepset(self, edge):
        key = (min(edge), max(edge))
        if key not in self.m_sep:
            raise IndexError(f"Edge ({edge[0]}, {edge[1]}) not found in sepset.")
        return self.m_sep[key]


class Counter:
    def __init__(self, pvalue):
        self.pvalue, self.calls = pvalue, 0

    def __call__(self, a, b, cond=()):
        self.calls += 1
        return self.pvalue(a, b, list(cond))


# ---- pc.cpp ---------------------------------------------------------------------------------------------------------------------
def max_cardinality(g, limit):   # :17-23
    return all(len(g.nbr[i]) + len(g.pa[i]) <= limit for i in range(g.n))


def in_whitelist(edge_whitelist, a, b):
    return (a, b) in edge_whitelist or (b, a) in edge_whitelist


def filter_marginal_skeleton(g, test, sepset, alpha, edge_whitelist):   # :32-89
    nodes = list(g.nodes())
    for i in range(len(nodes) - 1):
        for j in range(i + 1, len(nodes)):
            a, b = nodes[i], nodes[j]
            if g.has_edge(a, b) and not in_whitelist(edge_whitelist, a, b):
                p = test(a, b)
                if p > alpha:
                    g.remove_edge(a, b)
                    sepset.insert((a, b), [], p)
    for a in nodes:
        for b in g.interface_nodes():
            if g.has_edge(a, b) and not in_whitelist(edge_whitelist, a, b):
                p = test(a, b)
                if p > alpha:
                    g.remove_edge(a, b)
                    sepset.insert((a, b), [], p)


def find_univariate_sepset(g, edge, alpha, test):   # :91-118
    u = RangeSet()
    u.insert_range(g.nbr[edge[0]].items())
    u.insert_range(g.pa[edge[0]].items())
    u.insert_range(g.nbr[edge[1]].items())
    u.insert_range(g.pa[edge[1]].items())
    u.erase(edge[0])
    u.erase(edge[1])
    for cond in u:
        p = test(edge[0], edge[1], [cond])
        if p > alpha:
            return cond, p
    return None


def filter_univariate_skeleton(g, test, sepset, alpha, edge_whitelist):   # :120-145
    edges_to_remove = []
    for edge in g.edges():
        if not in_whitelist(edge_whitelist, *edge):
            indep = find_univariate_sepset(g, edge, alpha, test)
            if indep:
                edges_to_remove.append(edge)
                sepset.insert(edge, [indep[0]], indep[1])
    for e in edges_to_remove:
        g.remove_edge(*e)


def evaluate_multivariate_sepset(g, edge, comb, test, alpha):   # :147-167
    for names in comb:
        cond = [g.index[v] for v in names]
        p = test(edge[0], edge[1], cond)
        if p > alpha:
            return cond, p
    return None


def find_multivariate_sepset(g, edge, sep_size, test, alpha):   # :169-220
    nbr1, pa1, nbr2, pa2 = g.nbr[edge[0]], g.pa[edge[0]], g.nbr[edge[1]], g.pa[edge[1]]
    set1_valid = len(nbr1) + len(pa1) > sep_size
    set2_valid = len(nbr2) + len(pa2) > sep_size
    if not set1_valid and not set2_valid:
        return None
    u1, u2 = [], []
    if set1_valid:
        u1 = [g.names[v] for v in nbr1 if v != edge[1]] + [g.names[v] for v in pa1]
    if set2_valid:
        u2 = [g.names[v] for v in nbr2 if v != edge[0]] + [g.names[v] for v in pa2]
    if set1_valid:
        if set2_valid:
            return evaluate_multivariate_sepset(g, edge, Combinations2Sets(u1, u2, sep_size), test, alpha)
        return evaluate_multivariate_sepset(g, edge, Combinations(u1, sep_size), test, alpha)
    return evaluate_multivariate_sepset(g, edge, Combinations(u2, sep_size), test, alpha)


def find_skeleton(g, test, alpha, edge_whitelist):   # :222-263
    if g.num_edges() == len(edge_whitelist):
        return SepSet()
    sepset = SepSet()
    filter_marginal_skeleton(g, test, sepset, alpha, edge_whitelist)
    if g.num_edges() == len(edge_whitelist) or max_cardinality(g, 1):
        return sepset
    filter_univariate_skeleton(g, test, sepset, alpha, edge_whitelist)
    limit = 2
    while g.num_edges() > len(edge_whitelist) and not max_cardinality(g, limit):
        edges_to_remove = []
        for edge in g.edges():
            if not in_whitelist(edge_whitelist, *edge):
                indep = find_multivariate_sepset(g, edge, limit, test, alpha)
                if indep:
                    edges_to_remove.append(edge)
                    sepset.insert(edge, indep[0], indep[1])
        for e in edges_to_remove:
            g.remove_edge(*e)
        limit += 1
    return sepset


# ---- constraint.hpp:43-353 --------------------------------------------------------------------------------------------------------
def direct_arc_blacklist(g, arc_blacklist):
    for a, b in arc_blacklist:
        if g.has_edge(a, b):
            g.direct(b, a)


def remove_interface_arcs_blacklist(g, arc_blacklist):
    for a, b in arc_blacklist:
        if g.has_arc(a, b):
            g.remove_arc(a, b)


def count_univariate_sepsets(g, vs, test, alpha):   # :67-100
    p1, p2, children = vs
    indep_sepsets = children_in_sepsets = 0
    if test(p1, p2, [children]) > alpha:
        indep_sepsets += 1
        children_in_sepsets += 1
    possible_sepset = RangeSet()
    possible_sepset.insert_range(g.nbr[p1].items())
    possible_sepset.insert_range(g.pa[p1].items())
    possible_sepset.insert_range(g.nbr[p2].items())
    possible_sepset.insert_range(g.pa[p2].items())
    possible_sepset.erase(children)
    for sp in possible_sepset:
        if test(p1, p2, [sp]) > alpha:
            indep_sepsets += 1
    return indep_sepsets, children_in_sepsets


def count_multivariate_sepsets(g, vs, comb, test, alpha):   # :102-122
    p1, p2, children = vs
    indep_sepsets = children_in_sepsets = 0
    for names in comb:
        if test(p1, p2, [g.index[v] for v in names]) > alpha:
            indep_sepsets += 1
            if g.names[children] in names:
                children_in_sepsets += 1
    return indep_sepsets, children_in_sepsets


def is_unambiguous_vstructure(g, vs, test, alpha, ambiguous_threshold):   # :124-195
    p1, p2, children = vs
    max_sepset = max(len(g.nbr[p1]) + len(g.pa[p1]), len(g.nbr[p2]) + len(g.pa[p2]))
    marg_pvalue = test(p1, p2)
    indep_sepsets = children_in_sepsets = 0
    if marg_pvalue > alpha:
        indep_sepsets += 1
    a, b = count_univariate_sepsets(g, vs, test, alpha)
    indep_sepsets += a
    children_in_sepsets += b
    if ambiguous_threshold == 0 and children_in_sepsets > 0:
        return False
    if max_sepset >= 2:
        nbr1, pa1, nbr2, pa2 = g.nbr[p1], g.pa[p1], g.nbr[p2], g.pa[p2]
        u1, u2 = [], []
        if len(nbr1) + len(pa1) >= 2:
            u1 = [g.names[v] for v in nbr1] + [g.names[v] for v in pa1]
        if len(nbr2) + len(pa2) >= 2:
            u2 = [g.names[v] for v in nbr2] + [g.names[v] for v in pa2]
        for i in range(2, max_sepset + 1):
            set1_valid, set2_valid = len(u1) >= i, len(u2) >= i
            if set1_valid:
                comb = Combinations2Sets(u1, u2, i) if set2_valid else Combinations(u1, i)
            else:
                comb = Combinations(u2, i)
            a, b = count_multivariate_sepsets(g, vs, comb, test, alpha)
            indep_sepsets += a
            children_in_sepsets += b
    if indep_sepsets > 0:
        ratio = children_in_sepsets / indep_sepsets
        return ratio < ambiguous_threshold or ratio == 0
    return False


def is_vstructure(g, vs, test, alpha, sepset, use_sepsets, ambiguous_threshold):   # :206-229
    if not g.has_connection(vs[0], vs[1]):
        if use_sepsets:
            if sepset is not None:
                return vs[2] not in sepset.sepset((vs[0], vs[1]))[0]
            return is_unambiguous_vstructure(g, vs, test, alpha, 0)
        return is_unambiguous_vstructure(g, vs, test, alpha, ambiguous_threshold)
    return False


def evaluate_vstructures_at_node(g, node, test, alpha, sepset, use_sepsets, ambiguous_threshold):   # :231-293
    nbr = g.nbr[node]
    v = nbr.items()
    res = []
    if len(v) > 1:   # (the reference spells sizes 2 and 3 out; Combinations(v, 2) gives the same pairs in the same order)
        for parents in Combinations(v, 2):
            vs = (parents[0], parents[1], node)
            if is_vstructure(g, vs, test, alpha, sepset, use_sepsets, ambiguous_threshold):
                res.append(vs)
    parents = g.pa[node]
    if len(parents) > 0:
        remaining_neighbors = RangeSet(nbr.items())
        for found in res:
            remaining_neighbors.erase(found[0])
            remaining_neighbors.erase(found[1])
        for neighbor in remaining_neighbors:
            for parent in parents:
                vs = (neighbor, parent, node)
                if is_vstructure(g, vs, test, alpha, sepset, use_sepsets, ambiguous_threshold):
                    res.append(vs)
    return res


def direct_unshielded_triples(g, test, arc_blacklist, arc_whitelist, alpha, sepset, use_sepsets, ambiguous_threshold, allow_bidirected):   # :295-353
    vs = []
    for node in range(g.n):
        if len(g.nbr[node]) >= 1 and len(g.pa[node]) + len(g.nbr[node]) >= 2:
            vs += evaluate_vstructures_at_node(g, node, test, alpha, sepset, use_sepsets, ambiguous_threshold)
    for p1, p2, children in vs:
        if (p1, children) in arc_blacklist or (p2, children) in arc_blacklist:
            continue
        if allow_bidirected:
            g.direct(p1, children)
            g.direct(p2, children)
        else:
            if (g.has_arc(children, p1) and (children, p1) in arc_whitelist) or (g.has_arc(children, p2) and (children, p2) in arc_whitelist):
                continue
            g.direct(p1, children)
            g.direct(p2, children)
            if g.has_arc(children, p1):
                g.remove_arc(children, p1)
            if g.has_arc(children, p2):
                g.remove_arc(children, p2)


# ---- MeekRules (constraint.hpp:391-509) -----------------------------------------------------------------------------------------------
def rule1_find_new_arcs(g, to_check, new_arcs):
    for first, children in to_check:
        for neigh in g.nbr[children]:
            if not g.has_connection(first, neigh):
                new_arcs.append((children, neigh))


def direct_new_arcs(g, new_arcs):
    for s, t in new_arcs:
        g.direct(s, t)


def rule1(g):
    new_arcs = []
    rule1_find_new_arcs(g, g.arcs(), new_arcs)
    direct_new_arcs(g, new_arcs)
    changed = bool(new_arcs)
    to_check = new_arcs
    while to_check:
        new_arcs = []
        rule1_find_new_arcs(g, to_check, new_arcs)
        direct_new_arcs(g, new_arcs)
        to_check = new_arcs
    return changed


def any_intersect(s1, s2):
    small, great = (s1, s2) if len(s1) <= len(s2) else (s2, s1)
    return any(el in great for el in small)


def rule2(g):
    new_arcs = []
    for first, second in g.edges():
        if any_intersect(g.pa[second], g.ch[first]):
            new_arcs.append((first, second))
            continue
        if any_intersect(g.pa[first], g.ch[second]):
            new_arcs.append((second, first))
    direct_new_arcs(g, new_arcs)
    return bool(new_arcs)


def rule3_at_node(g, n):
    new_arcs = []
    for neigh in g.nbr[n]:
        small, great = (g.nbr[neigh], g.pa[n]) if len(g.nbr[neigh]) <= len(g.pa[n]) else (g.pa[n], g.nbr[neigh])
        intersection = [el for el in small if el in great]
        if len(intersection) >= 2:
            for p in Combinations(intersection, 2):
                if not g.has_connection(p[0], p[1]):
                    new_arcs.append((neigh, n))
    direct_new_arcs(g, new_arcs)
    return bool(new_arcs)


def rule3(g):
    changed = False
    for node in range(g.n):
        if len(g.pa[node]) >= 2 and len(g.nbr[node]) >= 1:
            changed |= rule3_at_node(g, node)
    return changed


def meek(g):
    changed = True
    while changed:
        changed = False
        changed |= rule1(g)
        changed |= rule2(g)
        changed |= rule3(g)


# ---- pc.cpp:265-336 and mmpc.cpp:1042-1068 ----------------------------------------------------------------------------------------------
def result(g, sepset, test):
    return {"arcs": sorted(g.arcs()), "edges": sorted((min(e), max(e)) for e in g.edges()),
            "sepsets": {k: (sorted(s), p) for k, (s, p) in (sepset.m_sep if sepset is not None else {}).items()}, "serial_tests": test.calls}


def estimate(pvalue, names, n_interface=0, alpha=0.05, arc_blacklist=(), arc_whitelist=(), edge_blacklist=(), edge_whitelist=(), use_sepsets=False,
             ambiguous_threshold=0.5, allow_bidirected=True):
    """learning::algorithms::estimate of pc.cpp over a complete undirected graph; restriction lists as validate_restrictions returns them."""
    test = Counter(pvalue)
    g = Graph.complete_undirected(names, n_interface)
    for a, b in edge_blacklist:
        g.remove_edge(a, b)
    for a, b in arc_whitelist:
        g.direct(a, b)
    if len(arc_whitelist) > 2:
        try:
            g.to_dag_check()
        except ValueError:
            raise ValueError("The selected blacklist/whitelist configuration does not allow an acyclic graph.")
    edge_whitelist = {(a, b): None for a, b in edge_whitelist}
    sepset = find_skeleton(g, test, alpha, edge_whitelist)
    if n_interface:
        g.direct_interface_edges()
        remove_interface_arcs_blacklist(g, arc_blacklist)
    direct_arc_blacklist(g, arc_blacklist)
    direct_unshielded_triples(g, test, set(arc_blacklist), set(arc_whitelist), alpha, sepset, use_sepsets, ambiguous_threshold, allow_bidirected)
    meek(g)
    return result(g, sepset, test)


def orient(pvalue, names, n_interface, alpha, arcs, edges, arc_blacklist=(), arc_whitelist=(), allow_bidirected=True):
    """The second half of MMPC's estimate (mmpc.cpp:1042-1068) on a given graph: no separating sets, use_sepsets = true."""
    test = Counter(pvalue)
    g = Graph(names, n_interface)
    for a, b in edges:
        g.add_edge(a, b)
    for s, t in arcs:
        g.add_arc(s, t)
    direct_arc_blacklist(g, arc_blacklist)
    direct_unshielded_triples(g, test, set(arc_blacklist), set(arc_whitelist), alpha, None, True, 0.0, allow_bidirected)
    meek(g)
    return result(g, None, test)
