"""Partially directed graphs (graph/generic_graph.hpp PartiallyDirectedGraph / ConditionalPartiallyDirectedGraph): what the
constraint-based learners return.  Plain host values - node, arc and edge containers keep insertion order."""
from .models import Dag


class PartiallyDirectedGraph:
    """PartiallyDirectedGraph(nodes) | (arcs, edges) | (nodes, arcs, edges).  An arc is (source, target), an edge an unordered pair; a
    pair of nodes may carry an arc in each direction (a bidirected connection, which `direct` creates when both orientations are asked
    for)."""

    def __init__(self, *args):
        if len(args) > 3:
            raise TypeError("PartiallyDirectedGraph(nodes) | (arcs, edges) | (nodes, arcs, edges)")
        if len(args) == 2:
            arcs, edges = args
            nodes = list(dict.fromkeys(v for pr in list(arcs) + list(edges) for v in pr))
        else:
            nodes = list(args[0]) if args else []
            arcs, edges = (args[1], args[2]) if len(args) == 3 else ((), ())
        self._init(nodes, [], arcs, edges)

    def _init(self, nodes, interface_nodes, arcs, edges):
        if len(set(nodes) | set(interface_nodes)) != len(nodes) + len(interface_nodes):
            raise ValueError("Graph cannot be created with repeated names.")
        self._nodes, self._interface = list(nodes), list(interface_nodes)
        self._nbr = {v: {} for v in self._nodes + self._interface}
        self._pa = {v: {} for v in self._nbr}
        self._ch = {v: {} for v in self._nbr}
        self._edges = {}   # (a, b) as added
        for s, t in arcs:
            self.add_arc(s, t)
        for a, b in edges:
            self.add_edge(a, b)

    @classmethod
    def CompleteUndirected(cls, nodes):
        nodes = list(nodes)
        g = cls(nodes)
        for i in range(len(nodes) - 1):
            for j in range(i + 1, len(nodes)):
                g.add_edge(nodes[i], nodes[j])
        return g

    # ---- nodes ----------------------------------------------------------------------------------------------------------------
    def nodes(self):
        return list(self._nodes)

    def num_nodes(self):
        return len(self._nodes)

    def contains_node(self, node):
        return node in self._nbr and node not in self._interface

    def _check(self, *names):
        for v in names:
            if v not in self._nbr:
                raise ValueError(f"Node {v} not present in the graph.")

    # ---- arcs and edges ---------------------------------------------------------------------------------------------------------
    def arcs(self):
        return [(s, t) for s in self._ch for t in self._ch[s]]

    def edges(self):
        return list(self._edges)

    def num_arcs(self):
        return sum(len(c) for c in self._ch.values())

    def num_edges(self):
        return len(self._edges)

    def has_arc(self, source, target):
        self._check(source, target)
        return source in self._pa[target]

    def has_edge(self, n1, n2):
        self._check(n1, n2)
        return n1 in self._nbr[n2]

    def has_connection(self, n1, n2):
        return self.has_edge(n1, n2) or self.has_arc(n1, n2) or self.has_arc(n2, n1)

    def parents(self, node):
        self._check(node)
        return list(self._pa[node])

    def children(self, node):
        self._check(node)
        return list(self._ch[node])

    def neighbors(self, node):
        self._check(node)
        return list(self._nbr[node])

    def num_parents(self, node):
        return len(self.parents(node))

    def num_children(self, node):
        return len(self.children(node))

    def num_neighbors(self, node):
        return len(self.neighbors(node))

    # ---- mutators -------------------------------------------------------------------------------------------------------------
    def _can_have(self, a, b):
        if a == b:
            raise ValueError(f"A connection {a} - {b} of a node with itself is not allowed.")
        if a in self._interface and b in self._interface:
            raise ValueError(f"Interface nodes {a} and {b} cannot be connected.")

    def add_arc(self, source, target):
        self._check(source, target)
        if not self.has_arc(source, target):
            self._can_have(source, target)
            if target in self._interface:
                raise ValueError(f"Interface node {target} cannot have parents.")
            self._ch[source][target] = None
            self._pa[target][source] = None

    def remove_arc(self, source, target):
        if self.has_arc(source, target):
            del self._ch[source][target]
            del self._pa[target][source]

    def flip_arc(self, source, target):
        if self.has_arc(source, target):
            self.remove_arc(source, target)
            self.add_arc(target, source)

    def add_edge(self, n1, n2):
        self._check(n1, n2)
        if not self.has_edge(n1, n2):
            self._can_have(n1, n2)
            self._nbr[n1][n2] = None
            self._nbr[n2][n1] = None
            self._edges[(n1, n2)] = None

    def remove_edge(self, n1, n2):
        if self.has_edge(n1, n2):
            del self._nbr[n1][n2]
            del self._nbr[n2][n1]
            self._edges.pop((n1, n2), None)
            self._edges.pop((n2, n1), None)

    def direct(self, source, target):
        """generic_graph.hpp:2243-2250: an edge becomes the arc; an arc target -> source gains its reverse (a bidirected pair); anything
        else is left alone."""
        self._check(source, target)
        if self.has_edge(source, target):
            self.remove_edge(source, target)
            self.add_arc(source, target)
        elif self.has_arc(target, source):
            self.add_arc(source, target)

    def undirect(self, source, target):
        """generic_graph.hpp:2252-2257: the arc source -> target goes; the edge appears unless target -> source is an arc."""
        self._check(source, target)
        if self.has_arc(source, target):
            self.remove_arc(source, target)
        if not self.has_arc(target, source):
            self.add_edge(source, target)

    # ---- conversions ----------------------------------------------------------------------------------------------------------
    def interface_nodes(self):
        return list(self._interface)

    def _interface_edges(self):   # as arcs out of the interface node
        return [(a, b) if a in self._interface else (b, a) for a, b in self._edges if a in self._interface or b in self._interface]

    @staticmethod
    def _acyclic(nodes, arcs):
        indeg = {v: 0 for v in nodes}
        out = {v: [] for v in nodes}
        for s, t in arcs:
            out[s].append(t)
            indeg[t] += 1
        stack = [v for v in nodes if not indeg[v]]
        seen = 0
        while stack:
            v = stack.pop()
            seen += 1
            for c in out[v]:
                indeg[c] -= 1
                if not indeg[c]:
                    stack.append(c)
        return seen == len(nodes)

    def to_dag(self):
        """A consistent extension (Dor & Tarsi 1992, generic_graph.hpp to_dag): every edge directed so that the result is acyclic and
        has no v-structure the PDAG lacks.  ValueError when the arcs hold a cycle or no extension exists.  Which of several extensions
        comes back is not pinned."""
        arcs = self.arcs() + self._interface_edges()
        everyone = self._nodes + self._interface
        if not self._acyclic(everyone, arcs):
            raise ValueError("PDAG contains directed cycles.")
        nbr = {v: dict(self._nbr[v]) for v in everyone}
        pa = {v: dict(self._pa[v]) for v in everyone}
        ch = {v: dict(self._ch[v]) for v in everyone}
        for s, t in self._interface_edges():
            del nbr[s][t], nbr[t][s]
        connected = lambda a, b: b in nbr[a] or b in pa[a] or b in ch[a]
        alive = dict.fromkeys(everyone)
        while any(nbr[v] for v in alive):
            for x in alive:
                if ch[x]:
                    continue
                adj = list(nbr[x]) + list(pa[x])
                if all(y == z or connected(y, z) for y in nbr[x] for z in adj):
                    arcs += [(y, x) for y in nbr[x]]
                    for y in list(nbr[x]):
                        del nbr[y][x]
                    for p in list(pa[x]):
                        del ch[p][x]
                    del alive[x]
                    break
            else:
                raise ValueError("PDAG do not allow a valid DAG extension.")
        return Dag(self._nodes, arcs, self._interface)

    def to_approximate_dag(self):
        """generic_graph.hpp to_approximate_dag: always answers.  The arcs give a pseudo topological order (an arc that closes a cycle
        is flipped), and every edge is directed along that order."""
        everyone = self._nodes + self._interface
        arcs = dict.fromkeys(self.arcs() + self._interface_edges())
        dpa = {v: {} for v in everyone}
        dch = {v: {} for v in everyone}
        for s, t in arcs:
            dch[s][t] = None
            dpa[t][s] = None
        incoming = {v: sum(1 for p in self._pa[v] if p not in self._interface) for v in self._nodes}
        order, placed = [], set()
        stack = [v for v in self._nodes if not self._pa[v]]
        while len(order) != len(self._nodes):
            if not stack:
                best = None
                for explored in order:
                    for c in dch[explored]:
                        if c not in placed and (best is None or len(dpa[c]) < len(dpa[best])):
                            best = c
                if best is None:
                    for v in self._nodes:
                        if v not in placed and (best is None or len(dpa[v]) < len(dpa[best])):
                            best = v
                stack.append(best)
            v = stack.pop()
            if v in placed:
                continue
            order.append(v)
            placed.add(v)
            for c in self._ch[v]:
                incoming[c] -= 1
                if c in placed:
                    if c in dch[v]:
                        del dch[v][c], dpa[c][v]
                        dch[c][v] = None
                        dpa[v][c] = None
                elif incoming[c] == 0:
                    stack.append(c)
        pos = {v: i for i, v in enumerate(order)}
        out = [(s, t) for s in everyone for t in dch[s]]
        for a, b in self._edges:
            if a in self._interface or b in self._interface:
                continue
            out.append((a, b) if pos[a] < pos[b] else (b, a))
        return Dag(self._nodes, out, self._interface)

    def conditional_graph(self, nodes=None, interface_nodes=None):
        """The same connections over (nodes, interface_nodes); without arguments every node stays a node."""
        nodes = self._nodes if nodes is None else list(nodes)
        interface_nodes = [] if interface_nodes is None else list(interface_nodes)
        g = ConditionalPartiallyDirectedGraph(nodes, interface_nodes)
        keep = set(nodes) | set(interface_nodes)
        both_interface = lambda a, b: a in interface_nodes and b in interface_nodes
        for s, t in self.arcs():
            if s in keep and t in keep and not both_interface(s, t) and t not in interface_nodes:
                g.add_arc(s, t)
        for a, b in self._edges:
            if a in keep and b in keep and not both_interface(a, b):
                g.add_edge(a, b)
        return g

    def unconditional_graph(self):
        return PartiallyDirectedGraph(self._nodes + self._interface, self.arcs(), self.edges())

    # ---- value semantics ------------------------------------------------------------------------------------------------------
    def _value(self):
        return (type(self).__name__, self._nodes, self._interface, sorted(self.arcs()), sorted(tuple(sorted(e)) for e in self._edges))

    def __eq__(self, other):
        return isinstance(other, PartiallyDirectedGraph) and self._value() == other._value()

    __hash__ = None

    def __getstate__(self):
        return {"nodes": self._nodes, "interface_nodes": self._interface, "arcs": self.arcs(), "edges": self.edges()}

    def __setstate__(self, state):
        self._init(state["nodes"], state["interface_nodes"], state["arcs"], state["edges"])

    def __repr__(self):
        return f"{type(self).__name__}(nodes={self._nodes}, arcs={self.arcs()}, edges={self.edges()})"


class ConditionalPartiallyDirectedGraph(PartiallyDirectedGraph):
    """ConditionalPartiallyDirectedGraph(nodes, interface_nodes[, arcs, edges]): interface nodes have no parents and no connections
    among themselves."""

    def __init__(self, nodes, interface_nodes, arcs=(), edges=()):
        self._init(list(nodes), list(interface_nodes), arcs, edges)

    @classmethod
    def CompleteUndirected(cls, nodes, interface_nodes):
        nodes, interface_nodes = list(nodes), list(interface_nodes)
        g = cls(nodes, interface_nodes)
        for i in range(len(nodes) - 1):
            for j in range(i + 1, len(nodes)):
                g.add_edge(nodes[i], nodes[j])
        for v in nodes:
            for w in interface_nodes:
                g.add_edge(v, w)
        return g

    def num_interface_nodes(self):
        return len(self._interface)

    def contains_interface_node(self, node):
        return node in self._interface

    def interface_edges(self):
        return self._interface_edges()

    def interface_arcs(self):
        return [(s, t) for s in self._interface for t in self._ch[s]]


def dag_to_pdag(dag):
    """Dag.to_pdag(): the CPDAG of the DAG's equivalence class.  The reference orders the arcs (Chickering; generic_graph.hpp:2776-2850);
    the class is unique, so the skeleton with the DAG's v-structures closed under Meek's rules 1-3 is the same graph."""
    from .constraint import MeekRules

    nodes, interface = dag.nodes(), dag.interface_nodes()
    arcs = dag.arcs()
    g = ConditionalPartiallyDirectedGraph(nodes, interface) if interface else PartiallyDirectedGraph(nodes)
    parents = {v: [s for s, t in arcs if t == v] for v in nodes + interface}
    adjacent = {frozenset(a) for a in arcs}
    compelled = dict.fromkeys((s, t) for s, t in arcs if s in interface)
    for v in nodes:
        ps = parents[v]
        for i in range(len(ps)):
            for j in range(i + 1, len(ps)):
                if frozenset((ps[i], ps[j])) not in adjacent:
                    compelled[(ps[i], v)] = None
                    compelled[(ps[j], v)] = None
    for s, t in arcs:
        if (s, t) in compelled:
            g.add_arc(s, t)
        else:
            g.add_edge(s, t)
    changed = True
    while changed and g.num_edges():
        changed = MeekRules.rule1(g)
        changed |= MeekRules.rule2(g)
        changed |= MeekRules.rule3(g)
    return g

