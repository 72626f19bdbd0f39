"""CPU tier: PartiallyDirectedGraph / ConditionalPartiallyDirectedGraph, MeekRules and Dag.to_pdag (no device work).  The Meek cases are
the figures the reference's own tests use (Koller & Friedman, figures 3.12 and 3.13)."""
import itertools
import pickle

import numpy as np
import pytest

import pybnesian_amd as pbn
from pybnesian_amd import MeekRules, PartiallyDirectedGraph


def und(edges):
    return {frozenset(e) for e in edges}


MEEK = [
    # rule, nodes, arcs, edges -> arcs, edges afterwards
    (1, ["X", "Y", "Z"], [("X", "Y")], [("Y", "Z")], [("X", "Y"), ("Y", "Z")], []),
    (2, ["X", "Y", "Z"], [("X", "Y"), ("Y", "Z")], [("X", "Z")], [("X", "Y"), ("Y", "Z"), ("X", "Z")], []),
    (3, ["X", "Y1", "Y2", "Z"], [("Y1", "Z"), ("Y2", "Z")], [("X", "Y1"), ("X", "Y2"), ("X", "Z")], [("X", "Z"), ("Y1", "Z"), ("Y2", "Z")],
     [("X", "Y1"), ("X", "Y2")]),
]


@pytest.mark.parametrize("rule,nodes,arcs,edges,arcs_after,edges_after", MEEK)
def test_meek_rules_one_by_one(ensure_built, rule, nodes, arcs, edges, arcs_after, edges_after):
    g = PartiallyDirectedGraph(nodes, arcs, edges)
    apply = getattr(MeekRules, f"rule{rule}")
    assert apply(g) is True
    assert set(g.arcs()) == set(arcs_after) and set(g.edges()) == set(edges_after) and g.num_edges() == len(edges_after)
    assert apply(g) is False
    for other in {1, 2, 3} - {rule}:   # each figure is the pattern of its own rule only
        h = PartiallyDirectedGraph(nodes, arcs, edges)
        assert getattr(MeekRules, f"rule{other}")(h) is False and h == PartiallyDirectedGraph(nodes, arcs, edges)


def test_meek_rules_in_sequence(ensure_built):
    g = PartiallyDirectedGraph(list("ABCDEFG"), [("B", "E"), ("C", "E")], [("A", "B"), ("B", "D"), ("C", "F"), ("E", "F"), ("F", "G")])
    changed = True
    while changed:
        changed = MeekRules.rule1(g) or MeekRules.rule2(g) or MeekRules.rule3(g)
    assert set(g.edges()) == {("A", "B"), ("B", "D")}
    assert set(g.arcs()) == {("B", "E"), ("C", "E"), ("E", "F"), ("C", "F"), ("F", "G")}


def test_constructors_and_queries():
    g = PartiallyDirectedGraph(["a", "b", "c", "d"])
    assert g.nodes() == ["a", "b", "c", "d"] and g.num_nodes() == 4 and g.num_arcs() == g.num_edges() == 0
    assert g.contains_node("a") and not g.contains_node("z")
    g = PartiallyDirectedGraph([("a", "b")], [("b", "c"), ("d", "c")])
    assert g.nodes() == ["a", "b", "c", "d"]
    assert g.arcs() == [("a", "b")] and g.edges() == [("b", "c"), ("d", "c")]
    assert g.has_arc("a", "b") and not g.has_arc("b", "a") and g.has_edge("c", "b") and g.has_edge("c", "d")
    assert g.has_connection("b", "a") and not g.has_connection("a", "c")
    assert g.parents("b") == ["a"] and g.children("a") == ["b"] and sorted(g.neighbors("c")) == ["b", "d"]
    assert (g.num_parents("b"), g.num_children("a"), g.num_neighbors("c")) == (1, 1, 2)
    c = PartiallyDirectedGraph.CompleteUndirected(["x", "y", "z"])
    assert c.edges() == [("x", "y"), ("x", "z"), ("y", "z")] and c.num_arcs() == 0
    with pytest.raises(ValueError, match="not present"):
        g.has_arc("a", "zz")
    with pytest.raises(ValueError):
        PartiallyDirectedGraph(["a", "a"])
    g.flip_arc("a", "b")
    assert g.arcs() == [("b", "a")]
    g.remove_arc("b", "a")
    g.remove_edge("c", "b")
    assert g.num_arcs() == 0 and g.edges() == [("d", "c")]


def test_direct_and_undirect():
    g = PartiallyDirectedGraph(["a", "b", "c"], [], [("a", "b")])
    g.direct("a", "b")                      # an edge becomes the arc
    assert g.arcs() == [("a", "b")] and g.num_edges() == 0
    g.direct("a", "b")                      # already there: nothing
    assert g.arcs() == [("a", "b")]
    g.direct("b", "a")                      # the reverse of an arc: both stay - a bidirected pair
    assert set(g.arcs()) == {("a", "b"), ("b", "a")} and g.num_edges() == 0
    g.direct("a", "c")                      # no connection: nothing
    assert not g.has_connection("a", "c")
    g.undirect("a", "b")                    # one half of a bidirected pair goes, the other is still an arc: no edge
    assert g.arcs() == [("b", "a")] and g.num_edges() == 0
    g.undirect("b", "a")                    # the last arc goes and the edge comes back
    assert g.num_arcs() == 0 and g.has_edge("a", "b")
    g.undirect("a", "c")                    # as the reference: no arc either way, so the edge appears
    assert g.has_edge("a", "c")


def v_structures(nodes, arcs):
    adj = und(arcs)
    out = set()
    for v in nodes:
        ps = [s for s, t in arcs if t == v]
        for a, b in itertools.combinations(sorted(ps), 2):
            if frozenset((a, b)) not in adj:
                out.add((a, b, v))
    return out


def is_acyclic(nodes, arcs):
    return PartiallyDirectedGraph._acyclic(list(nodes), list(arcs))


def test_to_dag_with_and_without_an_extension():
    g = PartiallyDirectedGraph(list("abcdef"), [("a", "c"), ("b", "c")], [("c", "d"), ("d", "e"), ("e", "f"), ("d", "f")])
    # c - d and then d - e, d - f must point away from c (a new unshielded collider otherwise); e - f is free
    d = g.to_dag()
    assert isinstance(d, pbn.Dag) and d.nodes() == list("abcdef")
    assert {("c", "d"), ("d", "e"), ("d", "f")} <= set(d.arcs())
    assert is_acyclic(d.nodes(), d.arcs()) and und(d.arcs()) == und(g.arcs() + g.edges())
    assert ("a", "c") in d.arcs() and ("b", "c") in d.arcs()
    assert v_structures(d.nodes(), d.arcs()) == v_structures(g.nodes(), g.arcs())
    # an undirected four-cycle has no extension: whatever the orientation, an unshielded collider appears or a cycle closes
    square = PartiallyDirectedGraph(list("abcd"), [], [("a", "b"), ("b", "c"), ("c", "d"), ("d", "a")])
    with pytest.raises(ValueError, match="PDAG do not allow a valid DAG extension."):
        square.to_dag()
    cyc = PartiallyDirectedGraph(list("abc"), [("a", "b"), ("b", "c"), ("c", "a")], [])
    with pytest.raises(ValueError, match="PDAG contains directed cycles."):
        cyc.to_dag()
    # the approximate conversion always answers, with the same adjacencies and no cycle
    for h in (square, cyc, g):
        a = h.to_approximate_dag()
        assert is_acyclic(a.nodes(), a.arcs()) and und(a.arcs()) == und(h.arcs() + h.edges())


def random_dag(n, seed, p=0.3):
    rng = np.random.default_rng(seed)
    order = list(rng.permutation(n))
    names = [f"n{i}" for i in range(n)]
    arcs = [(names[order[i]], names[order[j]]) for i in range(n) for j in range(i + 1, n) if rng.random() < p]
    return names, arcs


def cpdag_by_enumeration(names, arcs):
    """The CPDAG from its definition: an arc is compelled when every DAG with the same skeleton and v-structures has it (brute force)."""
    skeleton = [tuple(a) for a in arcs]
    want = v_structures(names, arcs)
    always = None
    for flips in itertools.product((False, True), repeat=len(skeleton)):
        cand = [(t, s) if f else (s, t) for (s, t), f in zip(skeleton, flips)]
        if is_acyclic(names, cand) and v_structures(names, cand) == want:
            always = set(cand) if always is None else always & set(cand)
    return always


@pytest.mark.parametrize("n,seed", [(5, 0), (6, 1), (6, 2), (7, 3), (7, 4), (6, 5)])
def test_dag_to_pdag_is_the_cpdag(ensure_built, n, seed):
    names, arcs = random_dag(n, seed)
    assert len(arcs) <= 14
    g = pbn.Dag(names, arcs).to_pdag()
    compelled = cpdag_by_enumeration(names, arcs)
    assert set(g.arcs()) == compelled
    assert und(g.edges()) == und(a for a in arcs if a not in compelled)


@pytest.mark.parametrize("n,seed", [(8, 0), (12, 1), (20, 2), (30, 3)])
def test_dag_to_pdag_to_dag_keeps_the_class(ensure_built, n, seed):
    names, arcs = random_dag(n, seed, 0.2)
    g = pbn.Dag(names, arcs).to_pdag()
    assert und(g.arcs() + g.edges()) == und(arcs) and all(a in arcs for a in g.arcs())
    d = g.to_dag()
    assert is_acyclic(d.nodes(), d.arcs()) and und(d.arcs()) == und(arcs)
    assert v_structures(names, d.arcs()) == v_structures(names, arcs)
    assert all(a in d.arcs() for a in g.arcs())
    assert d.to_pdag() == g


def test_conditional_graph():
    C = pbn.ConditionalPartiallyDirectedGraph
    g = C.CompleteUndirected(["a", "b", "c"], ["i", "j"])
    assert g.nodes() == ["a", "b", "c"] and g.interface_nodes() == ["i", "j"] and g.num_nodes() == 3
    assert g.num_edges() == 3 + 3 * 2 and not g.has_connection("i", "j")
    assert sorted(g.interface_edges()) == [(i, v) for i in "ij" for v in "abc"]
    assert g.contains_interface_node("i") and not g.contains_node("i") and g.contains_node("a")
    with pytest.raises(ValueError):
        g.add_edge("i", "j")
    with pytest.raises(ValueError):
        g.add_arc("a", "i")
    g.direct("i", "a")
    assert g.interface_arcs() == [("i", "a")] and ("i", "a") not in g.interface_edges()
    u = g.unconditional_graph()
    assert type(u) is PartiallyDirectedGraph and u.nodes() == ["a", "b", "c", "i", "j"] and u.has_arc("i", "a") and u.num_edges() == g.num_edges()
    back = u.conditional_graph(["a", "b", "c"], ["i", "j"])
    assert back == g and back != u
    d = g.to_dag()
    assert d.interface_nodes() == ["i", "j"] and all((i, v) in d.arcs() for i in "ij" for v in "abc")
    plain = PartiallyDirectedGraph(["a", "b"], [], [("a", "b")]).conditional_graph()
    assert type(plain) is C and plain.interface_nodes() == [] and plain.has_edge("a", "b")


def test_equality_and_pickle():
    g = PartiallyDirectedGraph(list("abcd"), [("a", "b"), ("c", "b")], [("c", "d")])
    g.direct("b", "c")   # bidirected
    same = PartiallyDirectedGraph(list("abcd"), [("c", "b"), ("b", "c"), ("a", "b")], [("d", "c")])
    assert g == same and not (g != same)
    assert g != PartiallyDirectedGraph(list("abcd"), [("a", "b"), ("c", "b")], [("c", "d")])
    assert g != PartiallyDirectedGraph(list("abdc"), g.arcs(), g.edges())
    h = pickle.loads(pickle.dumps(g))
    assert h == g and h.arcs() == g.arcs() and h.edges() == g.edges() and h.neighbors("c") == ["d"]
    c = pbn.ConditionalPartiallyDirectedGraph(["a", "b"], ["i"], [("i", "a")], [("a", "b")])
    k = pickle.loads(pickle.dumps(c))
    assert type(k) is pbn.ConditionalPartiallyDirectedGraph and k == c and k.interface_nodes() == ["i"]
