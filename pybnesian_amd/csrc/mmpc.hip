// The restriction phase in front of the hill-climb: Max-Min Parents and Children over all variables
// (learning/algorithms/mmpc.cpp:356-966) on the p-values of an independence-test callback.  Host logic only.
//
// The CPC / to-be-checked sets are libstdc++ std::unordered_set<int>, as in the reference, because their iteration
// order decides ties: with 10^6 rows the p-values of strongly dependent pairs underflow to exactly 0, several
// candidates share the minimum, and the first one met in iteration order is the one added to the CPC.
#include <algorithm>
#include <cmath>
#include <unordered_set>

#include "common.hpp"

using namespace pbn;

namespace {

constexpr int STOP = -1, RECOMPUTE = -2;                // mmpc.cpp:16

using IntSet = std::unordered_set<int>;

struct PairSet {  // ArcSet / EdgeSet over node indices
    std::unordered_set<int64_t> s;
    int n = 0;
    bool symmetric = false;
    int64_t key(int a, int b) const { if (symmetric && a > b) std::swap(a, b); return (int64_t)a * n + b; }
    void add(int a, int b) { s.insert(key(a, b)); }
    bool has(int a, int b) const { return s.count(key(a, b)) > 0; }
};

// k-subsets of {0..m-1} in lexicographic order of their index vectors (util/combinations.hpp:87-104)
struct Lex {
    int m, k;
    std::vector<int> idx;
    bool live;
    Lex(int m_, int k_) : m(m_), k(k_), idx(k_), live(k_ <= m_) { for (int i = 0; i < k; ++i) idx[i] = i; }
    void next() {
        for (int i = k - 1; i >= 0; --i)
            if (idx[i] < m - k + i) {
                ++idx[i];
                for (int j = i + 1; j < k; ++j) idx[j] = idx[j - 1] + 1;
                return;
            }
        live = false;
    }
};

struct Mmpc {
    int n;        // all variables: nodes first, then ni interface nodes (ConditionalPartiallyDirectedGraph)
    double alpha;
    pbn_ci_pvalue_fn fn;
    void* user;
    pbn_ci_pvalue_batch_fn batch_fn = nullptr;   // optional: many independent tests per call (one device launch)
    int64_t tests = 0;
    std::vector<double> min_assoc;   // n x n, column = variable whose CPC is built
    std::vector<double> maxmin;
    std::vector<int> maxmin_idx;
    PairSet arc_wl, edge_bl, edge_wl;
    std::vector<std::pair<int, int>> arc_wl_list, edge_wl_list;
    int ni = 0;   // interface nodes: candidates of the nodes only, never of each other (mmpc.cpp:875-908)

    double pvalue(int a, int b, const std::vector<int>& cond) {
        ++tests;
        const double p = fn(user, a, b, (int)cond.size(), cond.data());
        if (std::isnan(p)) throw invalid_error("MMPC: the independence test failed");
        return p;
    }
    struct Req { int a, b; std::vector<int> cond; };
    // p-values of independent requests, in request order; one call of the batched callback when there is one
    std::vector<double> pvalues(const std::vector<Req>& reqs, bool count = true) {
        std::vector<double> out(reqs.size());
        if (!batch_fn || reqs.size() < 2) {
            for (size_t i = 0; i < reqs.size(); ++i) out[i] = pvalue(reqs[i].a, reqs[i].b, reqs[i].cond);
            if (!count) tests -= (int64_t)reqs.size();
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
        if (count) tests += (int64_t)reqs.size();
        for (double p : out)
            if (std::isnan(p)) throw invalid_error("MMPC: the independence test failed");
        return out;
    }
    double pvalue(int a, int b) { static const std::vector<int> none; return pvalue(a, b, none); }
    double pvalue(int a, int b, int c) { return pvalue(a, b, std::vector<int>{c}); }

    double& cell(int row, int col) { return min_assoc[row + (size_t)col * n]; }
    void reset(int col) { maxmin[col] = alpha; maxmin_idx[col] = STOP; }
    void init_assoc(int row, int col, double p) {
        cell(row, col) = p;
        if (p < maxmin[col]) { maxmin[col] = p; maxmin_idx[col] = row; }
    }
    void update_assoc(int row, int col, double p) {
        const double nm = cell(row, col) = std::max(cell(row, col), p);
        if (nm < maxmin[col]) { maxmin[col] = nm; maxmin_idx[col] = row; }
    }

    void drop_independent(int var, IntSet& tbc) {  // update_to_be_checked
        for (auto it = tbc.begin(); it != tbc.end();)
            if (cell(*it, var) > alpha) it = tbc.erase(it); else ++it;
    }

    // association of every remaining candidate given every subset of the CPC that contains the variable added last
    void extend_assoc(int var, const IntSet& tbc, const IntSet& cpc, int last) {
        reset(var);
        // the tests of one extension step are independent of each other: requested together, applied in the
        // reference's order
        std::vector<Req> reqs;
        if (cpc.empty()) {
            for (int v : tbc) reqs.push_back({var, v, {}});
            const std::vector<double> p = pvalues(reqs);
            for (size_t i = 0; i < reqs.size(); ++i) init_assoc(reqs[i].b, var, p[i]);
            return;
        }
        std::vector<int> old;
        for (int pc : cpc) if (pc != last) old.push_back(pc);
        std::vector<int> cond;
        for (int v : tbc)
            for (int sz = 0; sz <= (int)old.size(); ++sz)   // {last}, {pc, last}, ..., the whole CPC
                for (Lex c((int)old.size(), sz); c.live; c.next()) {
                    cond.clear();
                    for (int i : c.idx) cond.push_back(old[i]);
                    cond.push_back(last);
                    reqs.push_back({var, v, cond});
                }
        const std::vector<double> p = pvalues(reqs);
        for (size_t i = 0; i < reqs.size(); ++i) update_assoc(reqs[i].b, var, p[i]);
    }

    void forward(int var, IntSet& cpc, IntSet& tbc, int last) {
        bool changed = true;
        if (cpc.empty()) {
            std::fill(min_assoc.begin() + (size_t)var * n, min_assoc.begin() + (size_t)(var + 1) * n, 0.0);
        } else if (last == RECOMPUTE) {
            // whitelisted CPC: association given the whole CPC (mmpc.cpp:357-382; the reference's loop never advances
            // its iterator there, so with a non-empty whitelist it does not terminate - here it does)
            std::vector<int> cond(cpc.begin(), cpc.end());
            reset(var);
            for (int v : tbc) init_assoc(v, var, pvalue(var, v, cond));
            const int add = maxmin_idx[var];
            if (add != STOP) { cpc.insert(add); tbc.erase(add); last = add; drop_independent(var, tbc); }
            else changed = false;
        }
        while (changed && !tbc.empty()) {
            extend_assoc(var, tbc, cpc, last);
            const int add = maxmin_idx[var];
            if (add != STOP) { cpc.insert(add); tbc.erase(add); last = add; drop_independent(var, tbc); }
            else changed = false;
        }
    }

    bool whitelisted(int var, int c) const { return edge_wl.has(var, c) || arc_wl.has(var, c) || arc_wl.has(c, var); }

    void backward(int var, IntSet& cpc) {
        if (cpc.size() <= 1) return;
        std::vector<int> rest(cpc.begin(), cpc.end());
        for (auto it = cpc.begin(); it != cpc.end();) {
            const int x = *it;
            if (whitelisted(var, x)) { ++it; continue; }
            auto pos = std::find(rest.begin(), rest.end(), x);   // swap_remove_v
            *pos = rest.back();
            rest.pop_back();
            bool separated = pvalue(var, x) > alpha;
            if (!separated && !batch_fn) {
                std::vector<int> cond;
                // subsets by increasing size, lexicographic inside a size, as the reference visits them
                for (int sz = 1; sz <= (int)rest.size() && !separated; ++sz)
                    for (Lex c((int)rest.size(), sz); c.live && !separated; c.next()) {
                        cond.clear();
                        for (int i : c.idx) cond.push_back(rest[i]);
                        separated = pvalue(var, x, cond) > alpha;
                    }
            } else if (!separated) {
                // batched callback: the subsets of one size are requested together and read in the reference's order up
                // to the first separating one - same decisions, same number of tests counted; what lies behind the
                // separating subset was evaluated for nothing, which costs less than one launch per subset
                std::vector<Req> reqs;
                std::vector<int> cond;
                for (int sz = 1; sz <= (int)rest.size() && !separated; ++sz) {
                    reqs.clear();
                    for (Lex c((int)rest.size(), sz); c.live; c.next()) {
                        cond.clear();
                        for (int i : c.idx) cond.push_back(rest[i]);
                        reqs.push_back({var, x, cond});
                    }
                    const std::vector<double> p = pvalues(reqs, false);
                    size_t used = reqs.size();
                    for (size_t i = 0; i < p.size(); ++i)
                        if (p[i] > alpha) { separated = true; used = i + 1; break; }
                    tests += (int64_t)used;
                }
            }
            if (separated) it = cpc.erase(it);
            else { rest.push_back(x); ++it; }
        }
    }

    std::vector<IntSet> run() {
        std::vector<IntSet> cpcs(n), tbc(n);
        for (auto& e : edge_wl_list) { cpcs[e.first].insert(e.second); cpcs[e.second].insert(e.first); }
        for (auto& a : arc_wl_list) { cpcs[a.first].insert(a.second); cpcs[a.second].insert(a.first); }
        const int nn = n - ni;   // nodes
        if (ni == 0) {
            for (int i = 0; i + 1 < n; ++i)
                for (int j = i + 1; j < n; ++j)
                    if (!edge_bl.has(i, j)) {
                        if (!cpcs[i].count(j)) tbc[i].insert(j);
                        if (!cpcs[j].count(i)) tbc[j].insert(i);
                    }
        } else {   // generate_cpcs of the conditional graph: every node against every other joint node
            for (int i = 0; i < nn; ++i)
                for (int j = 0; j < n; ++j)
                    if (i != j && !edge_bl.has(i, j)) {
                        if (!cpcs[i].count(j)) tbc[i].insert(j);
                        if (!cpcs[j].count(i)) tbc[j].insert(i);
                    }
        }
        min_assoc.assign((size_t)n * n, 0.0);
        maxmin.assign(n, alpha);
        maxmin_idx.assign(n, STOP);
        // marginal associations of all pairs at once (mmpc.cpp:698-738; node x interface pairs :740-784)
        // (the CPCs do not change during this pass, so the pairs can be requested together)
        std::vector<Req> mreq;
        auto marginal_pair = [&](int i, int j) {
            if ((cpcs[i].empty() || cpcs[j].empty()) && !edge_bl.has(i, j)) mreq.push_back({i, j, {}});
        };
        for (int i = 0; i + 1 < nn; ++i)
            for (int j = i + 1; j < nn; ++j) marginal_pair(i, j);
        for (int i = 0; i < nn; ++i)
            for (int j = nn; j < n; ++j) marginal_pair(i, j);
        {
            const std::vector<double> mp = pvalues(mreq);
            for (size_t q = 0; q < mreq.size(); ++q) {
                const int i = mreq[q].a, j = mreq[q].b;
                const double p = mp[q];
                if (p < alpha) {
                    if (cpcs[i].empty()) init_assoc(j, i, p);
                    if (cpcs[j].empty()) init_assoc(i, j, p);
                } else {
                    tbc[i].erase(j);
                    tbc[j].erase(i);
                }
            }
        }
        bool all_finished = true;
        for (int i = 0; i < n; ++i) {
            if (maxmin_idx[i] != STOP) {
                all_finished = false;
                cpcs[i].insert(maxmin_idx[i]);
                tbc[i].erase(maxmin_idx[i]);
            }
            if (cpcs[i].size() == 1) reset(i);
        }
        if (all_finished) return cpcs;
        // order-1 associations for the variables whose CPC holds one node; a test shared by both ends is run once
        // (mmpc.cpp:786-831)
        for (int i = 0; i < n; ++i) {
            if (cpcs[i].size() != 1) continue;
            const int c = *cpcs[i].begin();
            for (auto it = tbc[i].begin(); it != tbc[i].end();) {
                const int p = *it;
                const bool repeated = cpcs[p].size() == 1 && c == *cpcs[p].begin() && tbc[p].count(i) > 0;
                if (!repeated || i < p) {
                    const double pv = pvalue(i, p, c);
                    update_assoc(p, i, pv);
                    if (cell(p, i) > alpha) it = tbc[i].erase(it); else ++it;
                    if (repeated) {
                        update_assoc(i, p, pv);
                        if (cell(i, p) > alpha) tbc[p].erase(i);
                    }
                } else {
                    ++it;
                }
            }
        }
        for (int i = 0; i < n; ++i) {
            if (cpcs[i].size() > 1) {
                forward(i, cpcs[i], tbc[i], RECOMPUTE);
            } else if (maxmin_idx[i] != STOP) {
                const int add = maxmin_idx[i];
                cpcs[i].insert(add);
                tbc[i].erase(add);
                forward(i, cpcs[i], tbc[i], add);
            }
            backward(i, cpcs[i]);
        }
        return cpcs;
    }
};

}  // namespace

extern "C" {

static int mmpc_cpcs_impl(int n, int n_interface, pbn_ci_pvalue_fn fn, pbn_ci_pvalue_batch_fn batch_fn, void* user, double alpha, int n_arc_whitelist,
                          const int* arc_whitelist, int n_edge_blacklist, const int* edge_blacklist, int n_edge_whitelist,
                          const int* edge_whitelist, int symmetric, int* cpc_off, int* cpc, int64_t* n_tests) {
    std::recursive_mutex own;   // host-only search; the independence-test callbacks lock the contexts they use
    return guarded(own, [&] {
        if (n <= 0 || n_interface < 0 || n_interface >= n || !fn || !cpc_off || !cpc) throw invalid_error("pbn_mmpc_cpcs: bad argument");
        if (!(alpha > 0 && alpha < 1)) throw invalid_error("alpha must be a number between 0 and 1.");
        Mmpc m{n, alpha, fn, user};
        m.batch_fn = batch_fn;
        m.ni = n_interface;
        m.arc_wl.n = m.edge_bl.n = m.edge_wl.n = n;
        m.edge_bl.symmetric = m.edge_wl.symmetric = true;
        auto chk = [&](int v) { if (v < 0 || v >= n) throw invalid_error("pbn_mmpc_cpcs: node index out of range"); };
        for (int i = 0; i < n_arc_whitelist; ++i) {
            chk(arc_whitelist[2 * i]); chk(arc_whitelist[2 * i + 1]);
            m.arc_wl.add(arc_whitelist[2 * i], arc_whitelist[2 * i + 1]);
            m.arc_wl_list.push_back({arc_whitelist[2 * i], arc_whitelist[2 * i + 1]});
        }
        for (int i = 0; i < n_edge_blacklist; ++i) {
            chk(edge_blacklist[2 * i]); chk(edge_blacklist[2 * i + 1]);
            m.edge_bl.add(edge_blacklist[2 * i], edge_blacklist[2 * i + 1]);
        }
        for (int i = 0; i < n_edge_whitelist; ++i) {
            chk(edge_whitelist[2 * i]); chk(edge_whitelist[2 * i + 1]);
            m.edge_wl.add(edge_whitelist[2 * i], edge_whitelist[2 * i + 1]);
            m.edge_wl_list.push_back({edge_whitelist[2 * i], edge_whitelist[2 * i + 1]});
        }
        std::vector<IntSet> cpcs = m.run();
        if (symmetric) {  // remove_asymmetries (mmhc.cpp:12-22)
            for (int i = 0; i < n; ++i) {
                for (auto it = cpcs[i].begin(); it != cpcs[i].end();) {
                    if (!cpcs[*it].count(i)) it = cpcs[i].erase(it);
                    else ++it;
                }
            }
        }
        int pos = 0;
        for (int i = 0; i < n; ++i) {
            cpc_off[i] = pos;
            for (int v : cpcs[i]) cpc[pos++] = v;   // iteration order of the set, as the reference would walk it
        }
        cpc_off[n] = pos;
        if (n_tests) *n_tests = m.tests;
    });
}

int pbn_mmpc_cpcs(int n, pbn_ci_pvalue_fn fn, void* user, double alpha, int n_arc_whitelist, const int* arc_whitelist,
                  int n_edge_blacklist, const int* edge_blacklist, int n_edge_whitelist, const int* edge_whitelist,
                  int symmetric, int* cpc_off, int* cpc, int64_t* n_tests) {
    return mmpc_cpcs_impl(n, 0, fn, nullptr, user, alpha, n_arc_whitelist, arc_whitelist, n_edge_blacklist, edge_blacklist, n_edge_whitelist,
                          edge_whitelist, symmetric, cpc_off, cpc, n_tests);
}

// mmpc_all_variables over a ConditionalPartiallyDirectedGraph (mmpc.cpp:875-908, 740-784, 984-993): the last
// n_interface of the n variables are interface nodes.
int pbn_mmpc_cpcs_conditional(int n, int n_interface, pbn_ci_pvalue_fn fn, void* user, double alpha, int n_arc_whitelist,
                              const int* arc_whitelist, int n_edge_blacklist, const int* edge_blacklist, int n_edge_whitelist,
                              const int* edge_whitelist, int symmetric, int* cpc_off, int* cpc, int64_t* n_tests) {
    return mmpc_cpcs_impl(n, n_interface, fn, nullptr, user, alpha, n_arc_whitelist, arc_whitelist, n_edge_blacklist, edge_blacklist,
                          n_edge_whitelist, edge_whitelist, symmetric, cpc_off, cpc, n_tests);
}

// The same with a batched test callback for the steps whose tests are independent of each other (the marginal pass and
// every extension of the forward phase); fn still serves the sequential steps.  batch_fn may be NULL.
int pbn_mmpc_cpcs_batched(int n, int n_interface, pbn_ci_pvalue_fn fn, pbn_ci_pvalue_batch_fn batch_fn, void* user, double alpha,
                          int n_arc_whitelist, const int* arc_whitelist, int n_edge_blacklist, const int* edge_blacklist,
                          int n_edge_whitelist, const int* edge_whitelist, int symmetric, int* cpc_off, int* cpc, int64_t* n_tests) {
    return mmpc_cpcs_impl(n, n_interface, fn, batch_fn, user, alpha, n_arc_whitelist, arc_whitelist, n_edge_blacklist, edge_blacklist,
                          n_edge_whitelist, edge_whitelist, symmetric, cpc_off, cpc, n_tests);
}

}  // extern "C"
