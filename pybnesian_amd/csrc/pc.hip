// Constraint-based structure learning behind the C ABI: the PC algorithm (learning/algorithms/pc.cpp:25-336, PC-stable), the
// v-structure search and its application (learning/algorithms/constraint.hpp:16-353) and the Meek rules (:391-509).  Host logic: the
// arithmetic is in the independence test, which the engine asks for MANY p-values at a time wherever the reference's tests are
// mutually independent - all tests of a skeleton level (removals are collected and applied after the level) and all tests of the
// v-structure phase (the graph is not touched until every triple is judged).
//
// Batched = serial.  With batch_fn == NULL the engine is the serial search.  With a batch function a level gathers, per edge, the
// candidate separating sets in the reference's enumeration order and evaluates them in rounds of a bounded number of sets per
// still-unseparated edge; every edge then takes the first set in order with p > alpha.  The graph, the separating sets, their p-values
// and the count of tests the serial search would have run are those of the serial search; only "tests actually evaluated" is larger.
// A batched p-value within BAND * alpha of alpha is evaluated again through the scalar fn, and that value is used and reported: no
// decision rests on how a batch function rounds.
//
// Order.  Neighbour / parent / children sets are libstdc++ std::unordered_set<int> with the reference's insertion history, because
// the first separating set found and the order of v-structures (allow_bidirected = false) depend on their iteration order.  The
// reference's hash containers of edges and arcs are NOT restated: each loop over them collects and then applies, and application
// commutes - with one exception, the arc whitelist, whose iteration order decides the insertion order of a node's parents when two
// whitelisted arcs share their target; here the whitelist is applied in the order it is given.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <unordered_set>

#include "common.hpp"

using namespace pbn;

namespace {

// |p - alpha| <= PC_BAND * alpha is re-evaluated through the scalar callback.  Measured on an MI355X (tests/test_lincor_batch_gpu.py,
// 1.2 million tests of 0 ... 8 conditioning variables): the device batch of LinearCorrelation differs from its host routine by at most
// 4.28e-12 relative over host p-values in [alpha / 4, 4 alpha], alpha in {0.01, 0.05, 0.1}; times 64, rounded up
constexpr double PC_BAND = 3e-10;

using IntSet = std::unordered_set<int>;
using Pair = std::pair<int, int>;

struct Graph {   // PartiallyDirectedGraph / ConditionalPartiallyDirectedGraph over indices: nodes first, then ni interface nodes
    int n = 0, ni = 0;
    std::vector<IntSet> nbr, pa, ch;
    int num_edges = 0;
    Graph(int n_, int ni_) : n(n_), ni(ni_), nbr(n_), pa(n_), ch(n_) {}
    bool is_interface(int v) const { return v >= n - ni; }
    bool has_edge(int a, int b) const { return nbr[b].count(a) > 0; }
    bool has_arc(int s, int t) const { return pa[t].count(s) > 0; }
    bool has_connection(int a, int b) const { return has_edge(a, b) || has_arc(a, b) || has_arc(b, a); }
    std::set<Pair> stored_reversed;   // edges added as (larger, smaller): Meek's rule 2 tries the first end of an edge as the tail first
    void add_edge(int a, int b) {
        if (has_edge(a, b)) return;
        nbr[a].insert(b); nbr[b].insert(a); ++num_edges;
        if (a > b) stored_reversed.insert({b, a});
    }
    void remove_edge(int a, int b) {
        if (!has_edge(a, b)) return;
        nbr[a].erase(b); nbr[b].erase(a); --num_edges;
        stored_reversed.erase(a < b ? Pair{a, b} : Pair{b, a});
    }
    void add_arc(int s, int t) { ch[s].insert(t); pa[t].insert(s); }
    void remove_arc(int s, int t) { ch[s].erase(t); pa[t].erase(s); }
    void direct(int s, int t) {   // generic_graph.hpp:2243-2250
        if (has_edge(s, t)) { remove_edge(s, t); add_arc(s, t); }
        else if (has_arc(t, s)) add_arc(s, t);
    }
    std::vector<Pair> arcs() const {
        std::vector<Pair> r;
        for (int s = 0; s < n; ++s) for (int t : ch[s]) r.push_back({s, t});
        return r;
    }
    std::vector<Pair> edges() const {   // as (smaller, larger), sorted
        std::vector<Pair> r;
        for (int a = 0; a < n; ++a) for (int b : nbr[a]) if (a < b) r.push_back({a, b});
        std::sort(r.begin(), r.end());
        return r;
    }
    std::vector<Pair> stored_edges() const {   // in the orientation they were added with
        std::vector<Pair> r = edges();
        for (Pair& e : r) if (stored_reversed.count(e)) std::swap(e.first, e.second);
        return r;
    }
};

bool arcs_acyclic(int n, const std::vector<Pair>& arcs) {
    std::vector<std::vector<int>> out(n);
    std::vector<int> indeg(n, 0), stack;
    for (auto& a : arcs) { out[a.first].push_back(a.second); ++indeg[a.second]; }
    for (int i = 0; i < n; ++i) if (!indeg[i]) stack.push_back(i);
    int seen = 0;
    while (!stack.empty()) {
        const int v = stack.back(); stack.pop_back(); ++seen;
        for (int c : out[v]) if (--indeg[c] == 0) stack.push_back(c);
    }
    return seen == n;
}

// does the PDAG have a consistent DAG extension (Dor & Tarsi 1992; generic_graph.hpp to_dag)?  0 yes, 1 directed cycle, 2 none
int dag_extension_status(Graph g) {
    std::vector<Pair> arcs = g.arcs();
    if (g.ni) {   // interface edges count as arcs out of the interface node and leave the copy
        for (int i = g.n - g.ni; i < g.n; ++i) {
            std::vector<int> nb(g.nbr[i].begin(), g.nbr[i].end());
            for (int v : nb) { arcs.push_back({i, v}); g.remove_edge(i, v); }
        }
    }
    if (!arcs_acyclic(g.n, arcs)) return 1;
    std::vector<char> gone(g.n, 0);
    while (g.num_edges > 0) {
        bool ok = false;
        for (int x = 0; x < g.n && !ok; ++x) {
            if (gone[x] || !g.ch[x].empty()) continue;   // leaves
            bool adj = true;
            for (int y : g.nbr[x]) {
                for (int z : g.nbr[x]) if (y != z && !g.has_connection(y, z)) adj = false;
                for (int z : g.pa[x]) if (y != z && !g.has_connection(y, z)) adj = false;
            }
            if (!adj) continue;
            std::vector<int> nb(g.nbr[x].begin(), g.nbr[x].end()), ps(g.pa[x].begin(), g.pa[x].end());
            for (int v : nb) g.remove_edge(x, v);
            for (int v : ps) g.remove_arc(v, x);
            gone[x] = 1;
            ok = true;
        }
        if (!ok) return 2;
    }
    return 0;
}

int64_t binomial(int n, int k) {
    if (k < 0 || k > n) return 0;
    double r = 1;
    for (int i = 1; i <= k; ++i) r = r * (n - k + i) / i;
    return (int64_t)std::llround(std::min(r, 9e18));
}

// util::Combinations (util/combinations.hpp:11-156) without a fixed part: the first `limit` k-subsets in lexicographic index order
struct Subsets {
    std::vector<int> el;
    int k = 0;
    int64_t limit = 0, pos = 0;
    std::vector<int> ix;
    Subsets() = default;
    Subsets(std::vector<int> e, int k_) : el(std::move(e)), k(k_), limit(binomial((int)el.size(), k_)), ix(k_) { for (int i = 0; i < k; ++i) ix[i] = i; }
    bool next(std::vector<int>& out) {
        if (pos >= limit) return false;
        if (pos > 0) {
            const int m = (int)el.size();
            for (int i = k - 1; i >= 0; --i)
                if (ix[i] < m - k + i) {
                    ++ix[i];
                    for (int j = i + 1; j < k; ++j) ix[j] = ix[j - 1] + 1;
                    break;
                }
        }
        ++pos;
        out.clear();
        for (int i : ix) out.push_back(el[i]);
        return true;
    }
};

// the candidate conditioning sets of one search, in the reference's order
struct Candidates {
    std::vector<std::vector<int>> listed;   // explicit sets first ...
    size_t at = 0;
    std::vector<Subsets> seqs;              // ... then the enumerations, one after the other
    size_t seq = 0;
    bool next(std::vector<int>& out) {
        if (at < listed.size()) { out = listed[at++]; return true; }
        while (seq < seqs.size()) {
            if (seqs[seq].next(out)) return true;
            ++seq;
        }
        return false;
    }
};

struct Engine {
    Graph g;
    double alpha, band;
    pbn_ci_pvalue_fn fn;
    pbn_ci_pvalue_batch_fn batch_fn;
    void* user;
    std::vector<int> rank;   // position of a node's NAME among the sorted names: Combinations2Sets sorts its elements (strings)
    int64_t serial_tests = 0, evaluated = 0, band_redone = 0;
    std::map<Pair, std::pair<std::vector<int>, double>> sepset;
    std::vector<Pair> sep_order;

    Engine(int n, int ni) : g(n, ni) {}

    static Pair key(int a, int b) { return a < b ? Pair{a, b} : Pair{b, a}; }

    double scalar(int a, int b, const std::vector<int>& cond) {
        ++evaluated;
        const double p = fn(user, a, b, (int)cond.size(), cond.data());
        if (std::isnan(p)) throw invalid_error("PC: the independence test failed");
        return p;
    }
    struct Req { int a, b; std::vector<int> cond; };
    std::vector<double> pvalues(const std::vector<Req>& reqs) {
        std::vector<double> out(reqs.size());
        if (!batch_fn || reqs.size() < 2) {
            for (size_t i = 0; i < reqs.size(); ++i) out[i] = scalar(reqs[i].a, reqs[i].b, reqs[i].cond);
            return out;
        }
        std::vector<int> v1, v2, off{0}, cond;
        for (const Req& r : reqs) {
            v1.push_back(r.a); v2.push_back(r.b);
            cond.insert(cond.end(), r.cond.begin(), r.cond.end());
            off.push_back((int)cond.size());
        }
        if (cond.empty()) cond.push_back(0);
        batch_fn(user, (int)reqs.size(), v1.data(), v2.data(), off.data(), cond.data(), out.data());
        evaluated += (int64_t)reqs.size();
        for (size_t i = 0; i < reqs.size(); ++i) {
            if (std::isnan(out[i])) throw invalid_error("PC: the independence test failed");
            if (std::fabs(out[i] - alpha) <= band * alpha) { out[i] = scalar(reqs[i].a, reqs[i].b, reqs[i].cond); ++band_redone; }
        }
        return out;
    }

    // ---- skeleton -----------------------------------------------------------------------------------------------------------
    struct Search { int a, b; Candidates cand; bool open = true, separated = false; std::vector<int> sep; double p = 0; };

    // every search takes the first of its candidates with p > alpha (evaluate_multivariate_sepset, find_univariate_sepset)
    void run(std::vector<Search>& searches) {
        std::vector<int> cond;
        if (!batch_fn) {
            for (Search& s : searches)
                while (s.cand.next(cond)) {
                    ++serial_tests;
                    const double p = scalar(s.a, s.b, cond);
                    if (p > alpha) { s.separated = true; s.sep = cond; s.p = p; break; }
                }
            return;
        }
        // rounds: per open search the next `per` candidates (4, 8, ... 4096), all searches in one call of the batch function
        std::vector<Req> reqs;
        std::vector<int> owner;
        for (int per = 4;; per = std::min(per * 2, 4096)) {
            reqs.clear(); owner.clear();
            for (size_t si = 0; si < searches.size(); ++si) {
                Search& s = searches[si];
                if (!s.open) continue;
                int got = 0;
                while (got < per && s.cand.next(cond)) { reqs.push_back({s.a, s.b, cond}); owner.push_back((int)si); ++got; }
                if (got < per) s.open = false;   // exhausted: this round is its last
            }
            if (reqs.empty()) return;
            const std::vector<double> p = pvalues(reqs);
            for (size_t i = 0; i < reqs.size(); ++i) {
                Search& s = searches[owner[i]];
                if (s.separated) continue;   // what lies behind the separating set was evaluated for nothing
                ++serial_tests;
                if (p[i] > alpha) {
                    // the recorded p-value is the scalar function's, whatever the batch function's rounding (one test per removed edge)
                    s.separated = true; s.open = false; s.sep = reqs[i].cond; s.p = scalar(s.a, s.b, s.sep);
                }
            }
        }
    }

    void record(const Search& s) {
        sepset[key(s.a, s.b)] = {s.sep, s.p};
        sep_order.push_back(key(s.a, s.b));
    }

    bool max_cardinality(int limit) const {
        for (int i = 0; i < g.n; ++i)
            if ((int)(g.nbr[i].size() + g.pa[i].size()) > limit) return false;
        return true;
    }

    std::vector<int> by_rank(std::vector<int> v) const {
        std::sort(v.begin(), v.end(), [&](int x, int y) { return rank[x] < rank[y]; });
        return v;
    }

    // util::Combinations2Sets (util/combinations.hpp:167-276): the k-subsets of v1, then those of v2 that are not subsets of v1
    void two_sets(std::vector<int> v1, std::vector<int> v2, int k, Candidates& c) const {
        v1 = by_rank(std::move(v1));
        v2 = by_rank(std::move(v2));
        IntSet common;
        for (int x : v1) if (std::find(v2.begin(), v2.end(), x) != v2.end()) common.insert(x);
        c.seqs.emplace_back(v1, k);
        if ((int)common.size() < k) {
            c.seqs.emplace_back(v2, k);
            return;
        }
        for (size_t i = 0, common_start = v2.size() - common.size(); i < common_start; ++i)
            if (common.count(v2[i]) > 0)
                for (size_t j = v2.size() - 1; j >= common_start; --j)
                    if (common.count(v2[j]) == 0) std::swap(v2[i], v2[j]);
        Subsets s2(v2, k);
        s2.limit -= binomial((int)common.size(), k);
        c.seqs.push_back(std::move(s2));
    }

    void find_skeleton(const std::set<Pair>& edge_wl) {
        auto open_edges = [&] {
            std::vector<Pair> r;
            for (const Pair& e : g.edges()) if (!edge_wl.count(e)) r.push_back(e);
            return r;
        };
        if ((size_t)g.num_edges == edge_wl.size()) return;
        // filter_marginal_skeleton: node pairs, then node x interface pairs
        {
            std::vector<Search> ss;
            const int nn = g.n - g.ni;
            auto add = [&](int i, int j) {
                if (g.has_edge(i, j) && !edge_wl.count(key(i, j))) { Search s{i, j}; s.cand.listed.push_back({}); ss.push_back(std::move(s)); }
            };
            for (int i = 0; i + 1 < nn; ++i) for (int j = i + 1; j < nn; ++j) add(i, j);
            for (int i = 0; i < nn; ++i) for (int j = nn; j < g.n; ++j) add(i, j);
            run(ss);
            for (const Search& s : ss) if (s.separated) { g.remove_edge(s.a, s.b); record(s); }
        }
        if ((size_t)g.num_edges == edge_wl.size() || max_cardinality(1)) return;
        // filter_univariate_skeleton
        {
            std::vector<Search> ss;
            for (const Pair& e : open_edges()) {
                IntSet u;
                u.insert(g.nbr[e.first].begin(), g.nbr[e.first].end());
                u.insert(g.pa[e.first].begin(), g.pa[e.first].end());
                u.insert(g.nbr[e.second].begin(), g.nbr[e.second].end());
                u.insert(g.pa[e.second].begin(), g.pa[e.second].end());
                u.erase(e.first);
                u.erase(e.second);
                Search s{e.first, e.second};
                for (int c : u) s.cand.listed.push_back({c});
                ss.push_back(std::move(s));
            }
            run(ss);
            for (const Search& s : ss) if (s.separated) { g.remove_edge(s.a, s.b); record(s); }
        }
        for (int limit = 2; (size_t)g.num_edges > edge_wl.size() && !max_cardinality(limit); ++limit) {
            std::vector<Search> ss;
            for (const Pair& e : open_edges()) {   // find_multivariate_sepset
                const IntSet &nbr1 = g.nbr[e.first], &pa1 = g.pa[e.first], &nbr2 = g.nbr[e.second], &pa2 = g.pa[e.second];
                const bool valid1 = (int)(nbr1.size() + pa1.size()) > limit, valid2 = (int)(nbr2.size() + pa2.size()) > limit;
                if (!valid1 && !valid2) continue;
                std::vector<int> u1, u2;
                if (valid1) {
                    for (int v : nbr1) if (v != e.second) u1.push_back(v);
                    for (int v : pa1) u1.push_back(v);
                }
                if (valid2) {
                    for (int v : nbr2) if (v != e.first) u2.push_back(v);
                    for (int v : pa2) u2.push_back(v);
                }
                Search s{e.first, e.second};
                if (valid1 && valid2) two_sets(u1, u2, limit, s.cand);
                else s.cand.seqs.emplace_back(valid1 ? u1 : u2, limit);
                ss.push_back(std::move(s));
            }
            run(ss);
            for (const Search& s : ss) if (s.separated) { g.remove_edge(s.a, s.b); record(s); }
        }
    }

    // ---- v-structures (constraint.hpp:61-353) ---------------------------------------------------------------------------------
    struct Triple { int p1, p2, child; };
    struct Judge {   // is_unambiguous_vstructure of one unshielded triple, in two stages of mutually independent tests
        Triple t; double threshold; int indep = 0, child_in = 0; bool decided = false, result = false;
        std::vector<Req> reqs; std::vector<char> has_child;
    };

    void stage1(Judge& j) {
        const Triple& t = j.t;
        j.reqs.clear(); j.has_child.clear();
        j.reqs.push_back({t.p1, t.p2, {}}); j.has_child.push_back(0);
        j.reqs.push_back({t.p1, t.p2, {t.child}}); j.has_child.push_back(1);
        IntSet possible;
        possible.insert(g.nbr[t.p1].begin(), g.nbr[t.p1].end());
        possible.insert(g.pa[t.p1].begin(), g.pa[t.p1].end());
        possible.insert(g.nbr[t.p2].begin(), g.nbr[t.p2].end());
        possible.insert(g.pa[t.p2].begin(), g.pa[t.p2].end());
        possible.erase(t.child);
        for (int sp : possible) { j.reqs.push_back({t.p1, t.p2, {sp}}); j.has_child.push_back(0); }
    }
    void stage2(Judge& j) {
        const Triple& t = j.t;
        j.reqs.clear(); j.has_child.clear();
        const IntSet &nbr1 = g.nbr[t.p1], &pa1 = g.pa[t.p1], &nbr2 = g.nbr[t.p2], &pa2 = g.pa[t.p2];
        const size_t max_sepset = std::max(nbr1.size() + pa1.size(), nbr2.size() + pa2.size());
        if (max_sepset < 2) return;
        std::vector<int> u1, u2;
        if (nbr1.size() + pa1.size() >= 2) { for (int v : nbr1) u1.push_back(v); for (int v : pa1) u1.push_back(v); }
        if (nbr2.size() + pa2.size() >= 2) { for (int v : nbr2) u2.push_back(v); for (int v : pa2) u2.push_back(v); }
        std::vector<int> cond;
        for (size_t i = 2; i <= max_sepset; ++i) {
            const bool valid1 = u1.size() >= i, valid2 = u2.size() >= i;
            Candidates c;
            if (valid1 && valid2) two_sets(u1, u2, (int)i, c);
            else c.seqs.emplace_back(valid1 ? u1 : u2, (int)i);
            while (c.next(cond)) {
                j.reqs.push_back({t.p1, t.p2, cond});
                j.has_child.push_back(std::find(cond.begin(), cond.end(), t.child) != cond.end());
            }
        }
    }
    void tally(std::vector<Judge*>& js) {
        std::vector<Req> all;
        for (Judge* j : js) all.insert(all.end(), j->reqs.begin(), j->reqs.end());
        serial_tests += (int64_t)all.size();   // the reference evaluates every one of them: no early exit inside a stage
        const std::vector<double> p = pvalues(all);
        size_t at = 0;
        for (Judge* j : js)
            for (size_t i = 0; i < j->reqs.size(); ++i, ++at)
                if (p[at] > alpha) { ++j->indep; j->child_in += j->has_child[i]; }
    }
    void judge(std::vector<Judge>& js) {
        std::vector<Judge*> live;
        for (Judge& j : js) { stage1(j); live.push_back(&j); }
        tally(live);
        std::vector<Judge*> second;
        for (Judge* j : live) {
            if (j->threshold == 0 && j->child_in > 0) { j->decided = true; j->result = false; continue; }
            stage2(*j);
            second.push_back(j);
        }
        tally(second);
        for (Judge* j : second) {
            j->decided = true;
            if (j->indep > 0) {
                const double ratio = (double)j->child_in / j->indep;
                j->result = ratio < j->threshold || ratio == 0;
            }
        }
    }

    // is_vstructure for a list of triples of the unchanged graph; answers in order
    std::vector<char> are_vstructures(const std::vector<Triple>& ts, bool have_sepset, bool use_sepsets, double ambiguous_threshold) {
        std::vector<char> res(ts.size(), 0);
        std::vector<Judge> js;
        std::vector<size_t> where;
        for (size_t i = 0; i < ts.size(); ++i) {
            const Triple& t = ts[i];
            if (g.has_connection(t.p1, t.p2)) continue;   // shielded
            if (use_sepsets && have_sepset) {
                auto f = sepset.find(key(t.p1, t.p2));
                if (f == sepset.end())
                    throw invalid_error("Edge (" + std::to_string(t.p1) + ", " + std::to_string(t.p2) + ") not found in sepset.");
                const std::vector<int>& s = f->second.first;
                res[i] = std::find(s.begin(), s.end(), t.child) == s.end();
            } else {
                Judge j; j.t = t; j.threshold = use_sepsets ? 0.0 : ambiguous_threshold;
                js.push_back(std::move(j));
                where.push_back(i);
            }
        }
        judge(js);
        for (size_t q = 0; q < js.size(); ++q) res[where[q]] = js[q].result;
        return res;
    }

    void direct_unshielded_triples(const std::set<Pair>& arc_bl, const std::set<Pair>& arc_wl, bool have_sepset, bool use_sepsets,
                                   double ambiguous_threshold, bool allow_bidirected) {
        // evaluate_vstructures_at_node, all nodes at once: first the pairs of neighbours ...
        std::vector<int> at_nodes;
        for (int v = 0; v < g.n; ++v)
            if (g.nbr[v].size() >= 1 && g.pa[v].size() + g.nbr[v].size() >= 2) at_nodes.push_back(v);
        std::vector<Triple> ts;
        std::vector<std::vector<Triple>> found(g.n);
        for (int v : at_nodes) {
            std::vector<int> nb(g.nbr[v].begin(), g.nbr[v].end());
            for (size_t i = 0; i + 1 < nb.size(); ++i)
                for (size_t j = i + 1; j < nb.size(); ++j) ts.push_back({nb[i], nb[j], v});
        }
        std::vector<char> is = are_vstructures(ts, have_sepset, use_sepsets, ambiguous_threshold);
        for (size_t i = 0; i < ts.size(); ++i) if (is[i]) found[ts[i].child].push_back(ts[i]);
        // ... then a neighbour not yet directed by one of those with a parent
        ts.clear();
        for (int v : at_nodes) {
            if (g.pa[v].empty()) continue;
            IntSet remaining{g.nbr[v].begin(), g.nbr[v].end()};
            for (const Triple& t : found[v]) { remaining.erase(t.p1); remaining.erase(t.p2); }
            for (int neighbor : remaining)
                for (int parent : g.pa[v]) ts.push_back({neighbor, parent, v});
        }
        is = are_vstructures(ts, have_sepset, use_sepsets, ambiguous_threshold);
        for (size_t i = 0; i < ts.size(); ++i) if (is[i]) found[ts[i].child].push_back(ts[i]);

        for (int v : at_nodes)
            for (const Triple& t : found[v]) {
                if (arc_bl.count({t.p1, t.child}) || arc_bl.count({t.p2, t.child})) continue;
                if (allow_bidirected) {
                    g.direct(t.p1, t.child);
                    g.direct(t.p2, t.child);
                    continue;
                }
                if ((g.has_arc(t.child, t.p1) && arc_wl.count({t.child, t.p1})) || (g.has_arc(t.child, t.p2) && arc_wl.count({t.child, t.p2})))
                    continue;
                g.direct(t.p1, t.child);
                g.direct(t.p2, t.child);
                if (g.has_arc(t.child, t.p1)) g.remove_arc(t.child, t.p1);
                if (g.has_arc(t.child, t.p2)) g.remove_arc(t.child, t.p2);
            }
    }

    void orient(const std::set<Pair>& arc_bl, const std::set<Pair>& arc_wl, bool have_sepset, bool use_sepsets, double ambiguous_threshold,
                bool allow_bidirected);
};

// ---- Meek rules (constraint.hpp:391-509) ----------------------------------------------------------------------------------------
void direct_new_arcs(Graph& g, const std::vector<Pair>& arcs) { for (const Pair& a : arcs) g.direct(a.first, a.second); }

void rule1_find(const Graph& g, const std::vector<Pair>& to_check, std::vector<Pair>& out) {
    for (const Pair& arc : to_check)
        for (int neigh : g.nbr[arc.second])
            if (!g.has_connection(arc.first, neigh)) out.push_back({arc.second, neigh});
}
bool meek_rule1(Graph& g) {
    std::vector<Pair> fresh;
    rule1_find(g, g.arcs(), fresh);
    direct_new_arcs(g, fresh);
    const bool changed = !fresh.empty();
    std::vector<Pair> to_check = std::move(fresh);
    while (!to_check.empty()) {
        fresh.clear();
        rule1_find(g, to_check, fresh);
        direct_new_arcs(g, fresh);
        to_check = fresh;
    }
    return changed;
}
bool any_intersect(const IntSet& a, const IntSet& b) {
    const IntSet &s = a.size() <= b.size() ? a : b, &l = a.size() <= b.size() ? b : a;
    for (int v : s) if (l.count(v)) return true;
    return false;
}
// `edges` in their stored orientation: the first end is tried as the tail first
bool meek_rule2(Graph& g, const std::vector<Pair>& edges) {
    std::vector<Pair> fresh;
    for (const Pair& e : edges) {
        if (any_intersect(g.pa[e.second], g.ch[e.first])) { fresh.push_back({e.first, e.second}); continue; }
        if (any_intersect(g.pa[e.first], g.ch[e.second])) fresh.push_back({e.second, e.first});
    }
    direct_new_arcs(g, fresh);
    return !fresh.empty();
}
bool meek_rule3(Graph& g) {
    bool changed = false;
    for (int n = 0; n < g.n; ++n) {
        if (!(g.pa[n].size() >= 2 && g.nbr[n].size() >= 1)) continue;
        std::vector<Pair> fresh;
        for (int neigh : g.nbr[n]) {
            std::vector<int> inter;
            for (int v : g.nbr[neigh]) if (g.pa[n].count(v)) inter.push_back(v);
            for (size_t i = 0; i + 1 < inter.size(); ++i)
                for (size_t j = i + 1; j < inter.size(); ++j)
                    if (!g.has_connection(inter[i], inter[j])) fresh.push_back({neigh, n});
        }
        direct_new_arcs(g, fresh);
        changed |= !fresh.empty();
    }
    return changed;
}

void Engine::orient(const std::set<Pair>& arc_bl, const std::set<Pair>& arc_wl, bool have_sepset, bool use_sepsets, double ambiguous_threshold,
                    bool allow_bidirected) {
    for (const Pair& a : arc_bl)   // direct_arc_blacklist
        if (g.has_edge(a.first, a.second)) g.direct(a.second, a.first);
    direct_unshielded_triples(arc_bl, arc_wl, have_sepset, use_sepsets, ambiguous_threshold, allow_bidirected);
    for (bool changed = true; changed;) {
        changed = false;
        changed |= meek_rule1(g);
        changed |= meek_rule2(g, g.stored_edges());
        changed |= meek_rule3(g);
    }
}

std::set<Pair> pair_set(int n, int count, const int* prs, bool undirected, std::vector<Pair>* list = nullptr) {
    std::set<Pair> s;
    if (count < 0 || (count > 0 && !prs)) throw invalid_error("pbn_pc: bad restriction list");
    for (int i = 0; i < count; ++i) {
        const int a = prs[2 * i], b = prs[2 * i + 1];
        if (a < 0 || b < 0 || a >= n || b >= n || a == b) throw invalid_error("pbn_pc: node index out of range");
        s.insert(undirected ? Engine::key(a, b) : Pair{a, b});
        if (list) list->push_back({a, b});
    }
    return s;
}

void write_graph(const Graph& g, int* n_arcs, int* arcs, int* n_edges, int* edges) {
    std::vector<Pair> a = g.arcs(), e = g.edges();
    std::sort(a.begin(), a.end());
    *n_arcs = (int)a.size();
    for (size_t i = 0; i < a.size(); ++i) { arcs[2 * i] = a[i].first; arcs[2 * i + 1] = a[i].second; }
    *n_edges = (int)e.size();
    for (size_t i = 0; i < e.size(); ++i) { edges[2 * i] = e[i].first; edges[2 * i + 1] = e[i].second; }
}

void load_graph(Graph& g, int n_arcs, const int* arcs, int n_edges, const int* edges) {
    if (n_arcs < 0 || n_edges < 0 || (n_arcs && !arcs) || (n_edges && !edges)) throw invalid_error("pbn_pdag: bad graph lists");
    auto chk = [&](int v) { if (v < 0 || v >= g.n) throw invalid_error("pbn_pdag: node index out of range"); };
    for (int i = 0; i < n_edges; ++i) {
        chk(edges[2 * i]); chk(edges[2 * i + 1]);
        g.add_edge(edges[2 * i], edges[2 * i + 1]);
    }
    for (int i = 0; i < n_arcs; ++i) { chk(arcs[2 * i]); chk(arcs[2 * i + 1]); g.add_arc(arcs[2 * i], arcs[2 * i + 1]); }
}

void set_rank(Engine& e, const int* name_rank) {
    e.rank.resize(e.g.n);
    for (int i = 0; i < e.g.n; ++i) e.rank[i] = name_rank ? name_rank[i] : i;
}

}  // namespace

extern "C" {

double pbn_pc_band(void) { return PC_BAND; }

// PC::estimate / estimate_conditional over node indices (the last n_interface of the n variables are interface nodes).  Restriction
// lists are index pairs as util::validate_restrictions leaves them.  name_rank[i]: position of node i's name among the sorted names
// (NULL: the index).  band < 0: the built-in one.  arcs / edges: capacity n (n - 1) pairs each (a bidirected pair is two arcs).
// sep_pair: the removed edges (2 per edge), sep_off: n_sep + 1 offsets into sep_set (capacity n (n - 1) / 2 + 1 and n (n - 1) / 2 * n),
// sep_pvalue: their p-values.  tests[0]: what the reference's serial search evaluates, tests[1]: what was evaluated, tests[2]: how
// many of those were batched p-values inside the band, evaluated again through fn.
int pbn_pc_estimate(int n, int n_interface, pbn_ci_pvalue_fn fn, pbn_ci_pvalue_batch_fn batch_fn, void* user, double alpha, double band,
                    int n_arc_blacklist, const int* arc_blacklist, int n_arc_whitelist, const int* arc_whitelist, int n_edge_blacklist,
                    const int* edge_blacklist, int n_edge_whitelist, const int* edge_whitelist, int use_sepsets, double ambiguous_threshold,
                    int allow_bidirected, const int* name_rank, int* n_arcs, int* arcs, int* n_edges, int* edges, int* n_sep, int* sep_pair,
                    int* sep_off, int* sep_set, double* sep_pvalue, int64_t* tests) {
    std::recursive_mutex own;   // host-only search; the independence-test callbacks lock the contexts they use
    return guarded(own, [&] {
        if (n <= 0 || n_interface < 0 || n_interface >= n || !fn || !n_arcs || !arcs || !n_edges || !edges) throw invalid_error("pbn_pc_estimate: bad argument");
        if (!(alpha > 0 && alpha < 1)) throw invalid_error("alpha must be a number between 0 and 1.");
        if (!(ambiguous_threshold >= 0 && ambiguous_threshold <= 1)) throw invalid_error("ambiguous_threshold must be a number between 0 and 1.");
        Engine e(n, n_interface);
        e.alpha = alpha; e.band = band < 0 ? PC_BAND : band; e.fn = fn; e.batch_fn = batch_fn; e.user = user;
        set_rank(e, name_rank);
        std::vector<Pair> wl_list;
        const std::set<Pair> arc_bl = pair_set(n, n_arc_blacklist, arc_blacklist, false), arc_wl = pair_set(n, n_arc_whitelist, arc_whitelist, false, &wl_list),
                             edge_bl = pair_set(n, n_edge_blacklist, edge_blacklist, true), edge_wl = pair_set(n, n_edge_whitelist, edge_whitelist, true);
        Graph& g = e.g;
        const int nn = n - n_interface;
        for (int i = 0; i + 1 < nn; ++i) for (int j = i + 1; j < nn; ++j) g.add_edge(i, j);   // CompleteUndirected
        for (int i = 0; i < nn; ++i) for (int j = nn; j < n; ++j) g.add_edge(i, j);
        for (const Pair& b : edge_bl) g.remove_edge(b.first, b.second);
        for (const Pair& a : wl_list) g.direct(a.first, a.second);
        if (wl_list.size() > 2 && dag_extension_status(g) != 0)   // a cycle cannot be generated with less than 2 arcs (pc.cpp:288-297)
            throw invalid_error("The selected blacklist/whitelist configuration does not allow an acyclic graph.");
        e.find_skeleton(edge_wl);
        if (n_interface) {
            for (int i = nn; i < n; ++i) {   // direct_interface_edges
                IntSet copy = g.nbr[i];
                for (int v : copy) g.direct(i, v);
            }
            for (const Pair& a : arc_bl) if (g.has_arc(a.first, a.second)) g.remove_arc(a.first, a.second);
        }
        e.orient(arc_bl, arc_wl, true, use_sepsets != 0, ambiguous_threshold, allow_bidirected != 0);
        write_graph(g, n_arcs, arcs, n_edges, edges);
        if (n_sep && sep_pair && sep_off && sep_set && sep_pvalue) {
            int pos = 0, q = 0;
            for (auto& kv : e.sepset) {
                sep_pair[2 * q] = kv.first.first; sep_pair[2 * q + 1] = kv.first.second;
                sep_off[q] = pos;
                for (int v : kv.second.first) sep_set[pos++] = v;
                sep_pvalue[q] = kv.second.second;
                ++q;
            }
            sep_off[q] = pos;
            *n_sep = q;
        }
        if (tests) { tests[0] = e.serial_tests; tests[1] = e.evaluated; tests[2] = e.band_redone; }
    });
}

// The second half alone, for MMPC::estimate (mmpc.cpp:1042-1068): a given graph -> direct_arc_blacklist -> direct_unshielded_triples
// with no separating sets and use_sepsets = true (the threshold-0 search of constraint.hpp:219-222) -> Meek rules.
int pbn_pdag_orient(int n, int n_interface, pbn_ci_pvalue_fn fn, pbn_ci_pvalue_batch_fn batch_fn, void* user, double alpha, double band,
                    int n_in_arcs, const int* in_arcs, int n_in_edges, const int* in_edges, int n_arc_blacklist, const int* arc_blacklist,
                    int n_arc_whitelist, const int* arc_whitelist, int allow_bidirected, const int* name_rank, int* n_arcs, int* arcs,
                    int* n_edges, int* edges, int64_t* tests) {
    std::recursive_mutex own;
    return guarded(own, [&] {
        if (n <= 0 || n_interface < 0 || n_interface >= n || !fn || !n_arcs || !arcs || !n_edges || !edges) throw invalid_error("pbn_pdag_orient: bad argument");
        if (!(alpha > 0 && alpha < 1)) throw invalid_error("alpha must be a number between 0 and 1.");
        Engine e(n, n_interface);
        e.alpha = alpha; e.band = band < 0 ? PC_BAND : band; e.fn = fn; e.batch_fn = batch_fn; e.user = user;
        set_rank(e, name_rank);
        load_graph(e.g, n_in_arcs, in_arcs, n_in_edges, in_edges);
        const std::set<Pair> arc_bl = pair_set(n, n_arc_blacklist, arc_blacklist, false), arc_wl = pair_set(n, n_arc_whitelist, arc_whitelist, false);
        e.orient(arc_bl, arc_wl, false, true, 0.0, allow_bidirected != 0);
        write_graph(e.g, n_arcs, arcs, n_edges, edges);
        if (tests) { tests[0] = e.serial_tests; tests[1] = e.evaluated; tests[2] = e.band_redone; }
    });
}

// MeekRules::rule1 / rule2 / rule3 on a graph given as lists (edges in their stored orientation); *changed as the reference returns it.
int pbn_meek_rule(int rule, int n, int n_in_arcs, const int* in_arcs, int n_in_edges, const int* in_edges, int* n_arcs, int* arcs,
                  int* n_edges, int* edges, int* changed) {
    return guarded([&] {
        if (n <= 0 || rule < 1 || rule > 3 || !n_arcs || !arcs || !n_edges || !edges || !changed) throw invalid_error("pbn_meek_rule: bad argument");
        Graph g(n, 0);
        load_graph(g, n_in_arcs, in_arcs, n_in_edges, in_edges);
        *changed = rule == 1 ? meek_rule1(g) : rule == 2 ? meek_rule2(g, g.stored_edges()) : meek_rule3(g);
        write_graph(g, n_arcs, arcs, n_edges, edges);
    });
}

}  // extern "C"
