// Score engine, CKDE likelihood terms: the plain (all-continuous) CKDE candidates of one batch through the set-function cache, the
// term entry points of the C ABI (pbn_score_terms ...), and the steps the hybrid engine (hybrid.hip: HybridBatch) shares with it.
// Host code only: the kernels are behind kde_model.hpp / kde_group.hpp.
//
// slogl of a CKDE on a test region = A(vars, d) - A(parents, d), with A(S, m) = sum_q log KDE(S) under the bandwidth rule evaluated
// for m dimensions on the region's training rows: the marginal of the reference (CKDE.hpp:186-199) is the KDE of the parents with
// H[1:,1:], and H = k(N, d) cov, so both terms are functions of a variable SET (and m, and the region) only.  A({s,t}, 2) serves
// s -> t and t -> s, A({s}, 2) serves every child of s: each is swept once and remembered for the life of the score data.
// Neither term known: two plain sweeps (joint, marginal), each pruned on its own box.  (The fused joint + marginal sweep costs exactly
// two sweeps' worth of exponentials anyway - they, not the MFMAs, are the cost - and under tile pruning it can only prune on the
// marginal box: C3 16-21 ms fused against 2 x 7 ms plain per fold.  The engine dropped it in round 2; the stand-alone CKDE handles
// keep the fused kernel.)
#include <algorithm>
#include <cmath>
#include <map>
#include <string>

#include "common.hpp"
#include "hostmath.hpp"
#include "kde_group.hpp"
#include "kde_model.hpp"
#include "scoring_internal.hpp"

using namespace pbn;
using namespace pbn::score;

namespace pbn {
namespace score {

bool f32_check_after() {
    static const bool v = PBN_TUNE(F32_CHECK, 1) != 0;
    return v;
}

std::vector<int> set_key(int x, int m, const int* v, int nv) {
    std::vector<int> k(v, v + nv);
    std::sort(k.begin(), k.end());
    k.insert(k.begin(), {x, m});
    return k;
}

GUnit group_unit(bool cv, int R, int region, const KdeModel& m, int nv, int64_t ntrain, int64_t ntest, int slot) {
    GUnit U{};
    U.test_region = cv ? region : 1;
    U.train_mask = cv ? (((R >= 64) ? ~0ull : ((1ull << R) - 1ull)) & ~(1ull << region)) : 1ull;
    U.N = (int32_t)ntrain; U.nq = (int32_t)ntest;
    U.lognorm = m.lognorm;
    for (int i = 0; i < nv * nv; ++i) U.W[i] = m.W[i];
    for (int i = 0; i < nv; ++i) U.mu[i] = m.mu[i];
    U.sum_slot = slot;
    return U;
}

void pool_standardise(GPool& P, const double* cov, const double* means, int nv) {
    double L[PBN_GROUP_MAX_D * PBN_GROUP_MAX_D] = {}, Li[PBN_GROUP_MAX_D * PBN_GROUP_MAX_D] = {};
    if (!hm::cholesky(cov, nv, L)) {
        std::fill(L, L + nv * nv, 0.0);
        for (int i = 0; i < nv; ++i) L[i + (size_t)i * nv] = std::sqrt(std::max(cov[i + (size_t)i * nv], 1e-300));
    }
    hm::lower_inverse(L, nv, Li);
    for (int i = 0; i < nv; ++i) {
        P.mug[i] = means[i];
        for (int j = 0; j < nv; ++j) P.Wg[i * nv + j] = j <= i ? Li[i + (size_t)j * nv] : 0.0;
    }
}

void enqueue_term_chain(pbn_ctx* ctx, KdeModel& m, const pbn_table* t, const int* cols, const TermRows& r, const int32_t* dev_rows, double* dev_sum,
                        double* dev_max, bool precise) {
    const KdePackBytes pb = kde_pack_bytes(m.fdtype(), m.dm, false, m.N);   // (every engine term is a plain KDE: no conditional pack)
    ctx->scratch_train.reserve(align256(pb.apack) + align256(pb.nxpack) + 256);
    m.Apack = ctx->scratch_train.p;
    m.nxpack = ctx->scratch_train.p + align256(pb.apack);
    m.Axpack = nullptr;
    kde_pack_train(ctx, m, t, cols, r.row0, r.n0, r.row1, dev_rows, /*prune=*/true, dev_max);
    kde_eval_enqueue(ctx, m, t, cols, r.te0, r.te_n, nullptr, dev_sum, dev_rows, nullptr, precise);
}

void append_pools(GroupBatch& dst, const std::vector<GPool>& pools, const std::vector<std::vector<GUnit>>& pool_units, size_t* bytes) {
    for (size_t pi = 0; pi < pools.size(); ++pi) {
        dst.pools.push_back(pools[pi]);
        dst.pools.back().unit0 = (int32_t)dst.units.size();
        dst.pools.back().nunits = (int32_t)pool_units[pi].size();
        dst.units.insert(dst.units.end(), pool_units[pi].begin(), pool_units[pi].end());
        if (bytes) *bytes += kde_group_pool_bytes(dst, dst.pools.back());
    }
}

namespace {

struct Unit { int cand; Term joint, marg; bool has_marg; int want; };   // one (candidate, region)
struct Work { int cand, f, mode, slot_j, slot_m; };                      // one evaluation: mode 1 joint term, 2 marginal term
inline int slot_of(const Work& w) { return w.mode == 2 ? w.slot_m : w.slot_j; }
// host side of one evaluation: columns, training moments of the region, bandwidth, whitening (KdeModel without packs)
struct Prep { KdeModel m; std::vector<int> use; TermRows rows; int64_t ntrain; };

// The plain CKDE candidates of one call, like HybridBatch for the hybrid ones: result slots numbered across the batch, `scheduled` lets a
// later candidate share a term an earlier one enqueued.  plan -> collect_pools -> run_singles -> redo (twice) -> assemble.
struct TermBatch {
    pbn_scoredata* const sd;
    const BatchArgs& a;
    ScoreScratch& s;
    pbn_ctx* const ctx = sd->ctx;
    const pbn_table* const t = sd->table();
    const bool cv = a.kind == PBN_SCORE_CVLIK;
    const bool precise_all = sd->force_precise && sd->dtype == PBN_F64;
    // fp32 tables: behind the sums, one slot per sum for |z|^2 of the evaluation's farthest whitened training row (the pack kernels report
    // it): an evaluation that kde_wants_widening() flags is redone on fp64 fragments (KdeModel::widen) before its value is used.  The
    // choice is a function of that evaluation alone - nothing is remembered per variable set, so the double a (term, region) gets does
    // not depend on what this process evaluated before or on how a job dealt its terms
    const bool f32 = sd->dtype == PBN_F32 && f32_check_after();
    std::map<std::vector<int>, int> scheduled;   // key -> slot (this batch)
    std::vector<std::vector<int>> slot_key;      // [slot] -> set-function cache key
    std::vector<Unit> units;
    std::vector<Work> work;
    std::vector<char> grouped;                   // [work]: evaluated by the grouped chain
    GroupBatch gb;
    double* dsums = nullptr;                     // [slots] sums, then (fp32) [slots] max-norms at dmax
    double* dmax = nullptr;
    std::vector<double> hs;                      // the same on the host

    TermBatch(pbn_scoredata* sd_, const BatchArgs& a_, ScoreScratch& s_) : sd(sd_), a(a_), s(s_) {}

    bool own_term(const Work& w) const { return w.mode == 2 && a.want_of(w.cand) == 3; }   // marginal term over all p + 1 columns, rule for p + 2

    bool lookup(const std::vector<int>& key, Term& term) const {
        auto it = sd->kde_cache.find(key);
        if (!precise_all && it != sd->kde_cache.end()) { term.value = it->second; return true; }
        auto is = scheduled.find(key);
        if (is != scheduled.end()) { term.slot = is->second; return true; }
        return false;
    }
    // a term whose total over the regions was installed (pbn_score_terms_put): the total stands for region 0, the others add 0
    bool lookup_total(int m, const int* v, int nv, int region_index, Term& term) const {
        if (sd->term_total.empty() || a.only_region || precise_all) return false;   // (one region of a term: never its total)
        auto it = sd->term_total.find(set_key(a.kind, m, v, nv));   // (by kind: a validated score asks one handle for both kinds)
        if (it == sd->term_total.end()) return false;
        term.value = region_index == 0 ? it->second : 0.0;
        return true;
    }
    int new_slot(const std::vector<int>& key) {
        const int slot = (int)slot_key.size();
        slot_key.push_back(key);
        scheduled[key] = slot;
        return slot;
    }

    // every (candidate, region) looked up in term_total, kde_cache and this batch's schedule; what is missing gets a slot and a Work item.
    // Then the slots on the device, zeroed.
    void plan(const std::vector<int>& pending) {
        std::vector<int>& cols = s.cols;
        for (const int c : pending) {
            candidate_cols(a, c, cols);
            const int d = (int)cols.size(), p = d - 1;
            for (int f = 0; f < (cv ? sd->k : 1); ++f) {
                if (a.only_region && a.only_region[c] >= 0 && f != a.only_region[c]) continue;
                const int region = cv ? f : sd->k;                    // fold index, or the hold-out region
                const int wnt = a.want_of(c);
                Unit u{c, {}, {}, wnt == 3 || (p > 0 && wnt != 1), wnt};
                const std::vector<int> kj = set_key(region, d, cols.data(), d);
                const bool have_j = wnt >= 2 || lookup_total(d, cols.data(), d, f, u.joint) || lookup(kj, u.joint);
                bool have_m = true;
                std::vector<int> km;
                if (wnt == 3) {   // a marginal TERM (pbn_score_terms): all d columns of the pseudo-candidate under the rule for d + 1 dimensions, no child
                    km = set_key(region, d + 1, cols.data(), d);
                    have_m = lookup_total(d + 1, cols.data(), d, f, u.marg) || lookup(km, u.marg);
                } else if (u.has_marg) {
                    km = set_key(region, d, cols.data() + 1, p);
                    have_m = lookup_total(d, cols.data() + 1, p, f, u.marg) || lookup(km, u.marg);
                }
                if (!have_j) { u.joint.slot = new_slot(kj); work.push_back({c, f, 1, u.joint.slot, -1}); }
                if (!have_m) { u.marg.slot = new_slot(km); work.push_back({c, f, 2, -1, u.marg.slot}); }
                units.push_back(u);
            }
        }
        const size_t nslots = slot_key.size();
        ctx->scratch_sums.reserve(std::max<size_t>(1, 2 * nslots));   // (grow-only: no hipMalloc / hipFree per batch)
        dsums = ctx->scratch_sums.p;
        HIP_CHECK(hipMemsetAsync(dsums, 0, std::max<size_t>(1, 2 * nslots) * sizeof(double), ctx->stream));
        dmax = f32 ? dsums + nslots : nullptr;
    }

    void prepare(const Work& w, Prep& pr) {
        std::vector<int>& cols = s.cols;
        candidate_cols(a, w.cand, cols);
        const int d = (int)cols.size(), p = d - 1;
        s.mu.resize(d); s.sse.resize((size_t)d * d); s.H.resize((size_t)d * d);
        const Stats* tr = &sd->all;
        pr.rows = TermRows{0, sd->n_cv, 0, sd->n_cv, sd->n_hold};
        if (cv) {
            stats_minus(sd->all, sd->fold[w.f], s.train);
            tr = &s.train;
            pr.rows = TermRows{0, sd->limits[w.f], sd->limits[w.f + 1], sd->limits[w.f], sd->limits[w.f + 1] - sd->limits[w.f]};
        }
        pr.ntrain = tr->N;
        // The plain terms are evaluated over their columns in ASCENDING order, whatever the candidate's orientation and the order
        // of its parents: A(S, m) is then a function of the set alone down to the last bit - the value a term gets does not
        // depend on which candidate asked for it first, and a job that evaluates the terms on other ranks (pbn_score_terms)
        // computes the very same doubles.  (H = k(N, d) cov: the bandwidth of a subset is the sub-block of the set's.)
        const int var0 = cols[0];
        std::sort(cols.begin(), cols.end());
        subset_moments(sd, *tr, cols.data(), d, s.mu.data(), s.sse.data());
        const double inv = 1.0 / (double)(tr->N - 1);
        for (auto& x : s.sse) x *= inv;  // covariance
        if (own_term(w)) {
            // a marginal term evaluated for itself (a job that deals the terms to its ranks): KDE of these d columns with
            // H = k(N, d + 1) cov - the block the joint bandwidth of ANY child over them would have (H = k(N, dims) cov for the
            // library selectors), bit for bit, without a child whose own degeneracy (a constant column ...) has nothing to do
            // with the term.  The pre-checks of the selector stand on the term's own columns; the real candidate's set is
            // checked by its joint term.
            bandwidth_full_block(sd->selector, s.sse.data(), d, d + 1, tr->N, sd->dtype, s.H.data());
            kde_prepare(pr.m, sd->dtype, d, tr->N, s.H.data(), PBN_BW_FULL, false, s.mu.data());
            pr.use = cols;
            return;
        }
        bandwidth_from_cov(sd->selector, PBN_BW_FULL, s.sse.data(), d, tr->N, sd->dtype, s.H.data());
        if (w.mode == 2) {            // KDE of the parents with the bandwidth block of the parents
            const int vp = (int)(std::find(cols.begin(), cols.end(), var0) - cols.begin());
            std::vector<double> Hm((size_t)p * p), mum((size_t)p);
            pr.use.clear();
            for (int j = 0, jj = 0; j < d; ++j) {
                if (j == vp) continue;
                for (int i = 0, ii = 0; i < d; ++i) {
                    if (i == vp) continue;
                    Hm[ii + (size_t)jj * p] = s.H[i + (size_t)j * d];
                    ++ii;
                }
                mum[jj] = s.mu[j];
                pr.use.push_back(cols[j]);
                ++jj;
            }
            kde_prepare(pr.m, sd->dtype, p, tr->N, Hm.data(), PBN_BW_FULL, false, mum.data());
        } else {
            kde_prepare(pr.m, sd->dtype, d, tr->N, s.H.data(), PBN_BW_FULL, false, s.mu.data());
            pr.use = cols;
        }
    }

    // a new pool over the columns `use`: all rows of the CV region (its folds the regions), or the hold-out training + test rows
    GPool new_pool(const std::vector<int>& use, int R) const {
        const int dims = (int)use.size();
        GPool P{};
        P.rows = nullptr; P.row_base = 0;
        P.n = (int32_t)(cv ? sd->n_cv : sd->n_cv + sd->n_hold);
        P.R = R; P.d = dims; P.kd = std::min(dims, 4);
        if (cv) for (int f = 0; f <= sd->k; ++f) P.rb[f] = sd->limits[f];
        else { P.rb[0] = 0; P.rb[1] = (int32_t)sd->n_cv; P.rb[2] = (int32_t)(sd->n_cv + sd->n_hold); }
        for (int r = 0; r < PBN_GROUP_MAX_R; ++r) P.test_unit[r] = -1;
        for (int i = 0; i < dims; ++i) P.cols[i] = use[i];
        // pool-level standardisation for the Morton keys: from the covariance of the whole CV / training region
        std::vector<double> gm(dims), gs((size_t)dims * dims);
        subset_moments(sd, sd->all, use.data(), dims, gm.data(), gs.data());
        for (auto& x : gs) x /= (double)std::max<int64_t>(1, sd->all.N - 1);
        pool_standardise(P, gs.data(), gm.data(), dims);
        return P;
    }

    // grouped evaluation (kde_group.hip): the terms whose shape qualifies are collected into pools - one per variable set and rule, its
    // units the regions asked for - for ONE launch chain per batch
    void collect_pools() {
        std::vector<GPool> pools;
        std::vector<std::vector<GUnit>> pool_units;
        std::map<std::vector<int>, int> pool_of;   // [m, sorted columns...] -> pool
        grouped.assign(work.size(), 0);
        const int R = cv ? sd->k : 2;
        const int64_t min_train = cv ? sd->n_cv - (sd->limits[1] - sd->limits[0]) : sd->n_cv;
        for (size_t wi = 0; wi < work.size(); ++wi) {
            const Work& w = work[wi];
            const int p = a.n_parents(w.cand);
            const int dims = own_term(w) ? p + 1 : (w.mode == 2 ? p : p + 1);
            if (precise_all || !kde_group_applies(sd->dtype, dims, min_train, R)) continue;   // (precise: one chain per term, per-row accuracy)
            Prep pr;
            prepare(w, pr);
            std::vector<int> key(pr.use);
            std::sort(key.begin(), key.end());
            key.insert(key.begin(), own_term(w) ? p + 2 : p + 1);
            auto it = pool_of.find(key);
            if (it == pool_of.end()) {
                it = pool_of.emplace(key, (int)pools.size()).first;
                pools.push_back(new_pool(pr.use, R));
                pool_units.emplace_back();
            }
            const int pi = it->second;
            const GUnit U = group_unit(cv, R, w.f, pr.m, dims, pr.ntrain, pr.rows.te_n, slot_of(w));
            pools[pi].test_unit[U.test_region] = (int32_t)pool_units[pi].size();
            pool_units[pi].push_back(U);
            grouped[wi] = 1;
        }
        append_pools(gb, pools, pool_units, nullptr);
    }

    // one evaluation through its own launch chain (shapes the grouped path does not take; the redo of a flagged evaluation)
    void run_single(const Work& w, bool force64, bool precise) {
        Prep pr;
        prepare(w, pr);
        const int slot = slot_of(w);
        if (f32 && force64) kde_widen(pr.m);
        enqueue_term_chain(ctx, pr.m, t, pr.use.data(), pr.rows, nullptr, dsums + slot, dmax ? dmax + slot : nullptr, precise);
    }

    // the grouped chain, then every other evaluation on a chain of its own, alternating between the context's issue lanes (common.hpp);
    // one wait, one copy-back of all sums
    void run_singles() {
        const size_t nslots = slot_key.size();
        size_t n_single = 0;
        for (char gflag : grouped) n_single += gflag ? 0 : 1;
        const int lanes = (n_single > 1 && !ctx->profiling) ? score_lanes(t->n_rows) : 1;
        if (lanes > 1) { ctx->ensure_lanes(lanes - 1); ctx->lanes_wait_for_stream(lanes - 1); }
        if (!gb.pools.empty()) kde_group_run(ctx, t, gb, dsums, dmax, false);
        size_t li = 0;
        for (size_t wi = 0; wi < work.size(); ++wi) {
            if (grouped[wi]) continue;
            LaneSwitch lane(ctx, (int)(li++ % (size_t)lanes));
            run_single(work[wi], false, precise_all);
        }
        hs.resize(std::max<size_t>(1, 2 * nslots));
        if (lanes > 1) ctx->sync_lanes(lanes - 1);
        if (nslots) HIP_CHECK(hipMemcpyAsync(hs.data(), dsums, (f32 ? 2 : 1) * nslots * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }

    // check-after: the evaluations `flagged` picks from the sums on the host are evaluated once more, each through a chain of its own,
    // and the sums copied back again -> how many
    template <typename Pred>
    int64_t redo(Pred flagged, bool force64, bool precise) {
        int64_t n = 0;
        for (const Work& w : work) {
            if (!flagged(w)) continue;
            HIP_CHECK(hipMemsetAsync(dsums + slot_of(w), 0, sizeof(double), ctx->stream));
            run_single(w, force64, precise);
            ++n;
        }
        if (n == 0) return 0;
        HIP_CHECK(hipMemcpyAsync(hs.data(), dsums, slot_key.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        sd->kde_sweeps += n;
        return n;
    }

    // the sums into the cache; a candidate = (its joint terms added in region order) - (its marginal terms added in region order): the two
    // sums are what pbn_score_terms hands out, so a job that computes the terms on different ranks assembles the same doubles
    void assemble(const std::vector<int>& pending) {
        ctx->drop_staged();
        for (size_t i = 0; i < slot_key.size(); ++i) sd->kde_cache[slot_key[i]] = hs[i];
        sd->kde_sweeps += (int64_t)work.size();
        std::vector<double> jsum((size_t)a.n_cand, 0.0), msum((size_t)a.n_cand, 0.0);
        for (const Unit& u : units) {
            if (u.want < 2) jsum[u.cand] += u.joint.slot >= 0 ? hs[u.joint.slot] : u.joint.value;
            if (u.has_marg) msum[u.cand] += u.marg.slot >= 0 ? hs[u.marg.slot] : u.marg.value;
        }
        for (const int c : pending) {
            const int wnt = a.want_of(c);
            a.out[c] = wnt >= 2 ? msum[c] : (wnt == 1 ? jsum[c] : jsum[c] - msum[c]);
        }
    }
};

}  // namespace

void score_ckde_terms(pbn_scoredata* sd, const BatchArgs& a, const std::vector<int>& pending, ScoreScratch& s) {
    TermBatch b(sd, a, s);
    b.plan(pending);
    b.collect_pools();
    b.run_singles();
    const size_t nslots = b.slot_key.size();
    if (b.f32 && nslots) {
        // evaluations whose training rows reach beyond what fp32 fragments hold (2^-24 max|z|^2 above the threshold of kde_wants_widening)
        // are redone on fp64 fragments.  The criterion follows the fragments' layout, i.e. the number of variables of the term: p + 1 for
        // a joint term, p or (a marginal TERM of pbn_score_terms) p + 1 for a marginal one - the stricter of the two there
        b.redo([&](const Work& w) {
            const int pw = a.n_parents(w.cand);
            const double far2 = b.hs[nslots + (size_t)slot_of(w)];
            return kde_wants_widening(far2, pw + 1) || (w.mode == 2 && kde_wants_widening(far2, pw));
        }, /*force64=*/true, /*precise=*/false);
    }
    if (sd->dtype == PBN_F64 && nslots) {
        // fp64 tables: a term whose sum over its test rows is a cancellation to ~0 (kde_sum_needs_precision: the sum-only sweeps'
        // absolute error budget would exceed 5e-7 of it) is evaluated once more at the accuracy of the per-row path
        sd->precise_redos += b.redo([&](const Work& w) {
            const int64_t nq = b.cv ? sd->limits[w.f + 1] - sd->limits[w.f] : sd->n_hold;
            return kde_sum_needs_precision(b.hs[(size_t)slot_of(w)], nq);
        }, /*force64=*/false, /*precise=*/true);
    }
    b.assemble(pending);
}

namespace {

// term i = columns vars[off[i] .. off[i + 1]) under the bandwidth rule for m[i] dimensions: m = the number of columns for a joint term,
// one more for the marginal term of a candidate with those parents
void check_terms(const pbn_scoredata* sd, int kind, int n_terms, const int* off, const int* vars, const int* m, const char* who) {
    if (!sd || (n_terms > 0 && (!off || !vars || !m))) throw invalid_error(std::string(who) + ": null argument");
    if (kind != PBN_SCORE_CVLIK && kind != PBN_SCORE_HOLDOUT) throw invalid_error(std::string(who) + ": likelihood scores only");
    for (int i = 0; i < n_terms; ++i) {
        const int nv = off[i + 1] - off[i];
        if (nv < 1 || (m[i] != nv && m[i] != nv + 1)) throw invalid_error(std::string(who) + ": a term has m = its columns (joint) or one more (marginal)");
        for (int j = off[i]; j < off[i + 1]; ++j)
            if (vars[j] < 0 || vars[j] >= sd->n) throw invalid_error(std::string(who) + ": continuous columns only");
    }
}

// Every term as a pseudo-candidate of the batch engine over the term's OWN columns (first column | the others): a joint term asks for
// the joint half only (want 1), a marginal term for "the KDE of all my columns under the rule for one more dimension" (want 3) - no
// pseudo-child: the bandwidth block of the parents does not depend on the child (H = k(N, d) cov for the library selectors), and a
// degenerate unrelated column must not fail a term no real candidate pairs with it.
// An exception of the engine goes out with its own class: a SingularCovarianceData of a term is one on every rank, not a device error.
void score_terms_as_candidates(pbn_scoredata* sd, int kind, int n_terms, const int* off, const int* vars, const int* m, const int* region, double* out) {
    if (n_terms <= 0) return;
    std::vector<int> var((size_t)n_terms), nt((size_t)n_terms, PBN_NODE_CKDE), po{0}, par, want((size_t)n_terms);
    for (int i = 0; i < n_terms; ++i) {
        const int nv = off[i + 1] - off[i];
        const int* v = vars + off[i];
        var[i] = v[0];
        want[i] = m[i] == nv ? 1 : 3;
        par.insert(par.end(), v + 1, v + nv);
        po.push_back((int)par.size());
    }
    BatchArgs a;
    a.kind = kind; a.n_cand = n_terms; a.var = var.data(); a.node_type = nt.data(); a.par_off = po.data(); a.parents = par.data();
    a.out = out; a.want = want.data(); a.only_region = region;
    score_batch_body(sd, a);
}

}  // namespace
}  // namespace score
}  // namespace pbn

extern "C" {

int pbn_score_terms(pbn_scoredata* sd, int kind, int n_terms, const int* off, const int* vars, const int* m, double* out) {
    return guarded(mu_of(sd), [&] {
        check_terms(sd, kind, n_terms, off, vars, m, "pbn_score_terms");
        if (n_terms > 0 && !out) throw invalid_error("pbn_score_terms: null output");
        score_terms_as_candidates(sd, kind, n_terms, off, vars, m, nullptr, out);
    });
}

int pbn_score_term_regions(pbn_scoredata* sd, int kind, int n_items, const int* off, const int* vars, const int* m, const int* region, double* out) {
    return guarded(mu_of(sd), [&] {
        check_terms(sd, kind, n_items, off, vars, m, "pbn_score_term_regions");
        if (n_items > 0 && (!out || !region)) throw invalid_error("pbn_score_term_regions: null argument");
        const int regions = kind == PBN_SCORE_CVLIK ? sd->k : 1;
        for (int i = 0; i < n_items; ++i)
            if (region[i] < 0 || region[i] >= regions) throw invalid_error("pbn_score_term_regions: region out of range (CV folds; 0 for the hold-out score)");
        score_terms_as_candidates(sd, kind, n_items, off, vars, m, region, out);
    });
}

int pbn_score_terms_put(pbn_scoredata* sd, int kind, int n_terms, const int* off, const int* vars, const int* m, const double* values) {
    return guarded(mu_of(sd), [&] {
        check_terms(sd, kind, n_terms, off, vars, m, "pbn_score_terms_put");
        if (n_terms > 0 && !values) throw invalid_error("pbn_score_terms_put: null values");
        if (sd->term_total.size() > score_cache_budget()) { sd->term_total.clear(); ++sd->cache_resets; }   // before the new terms go in: the batch being assembled keeps its own
        for (int i = 0; i < n_terms; ++i) sd->term_total[set_key(kind, m[i], vars + off[i], off[i + 1] - off[i])] = values[i];
    });
}

int pbn_score_terms_missing(pbn_scoredata* sd, int kind, int n_terms, const int* off, const int* vars, const int* m, int* missing) {
    return guarded(mu_of(sd), [&] {
        check_terms(sd, kind, n_terms, off, vars, m, "pbn_score_terms_missing");
        if (n_terms > 0 && !missing) throw invalid_error("pbn_score_terms_missing: null output");
        for (int i = 0; i < n_terms; ++i)
            missing[i] = (sd->force_precise && sd->dtype == PBN_F64) ||   // (precise mode: every term is evaluated again, by the rank it is dealt to)
                         sd->term_total.find(set_key(kind, m[i], vars + off[i], off[i + 1] - off[i])) == sd->term_total.end() ? 1 : 0;
    });
}

int pbn_score_batch_parts(pbn_scoredata* sd, int kind, int n_cand, const int* var, const int* node_type, const int* par_off,
                          const int* parents, int part, int n_parts, double* out) {
    return guarded(mu_of(sd), [&] {
        if (!sd || !var || !node_type || !par_off || !out) throw invalid_error("pbn_score_batch_parts: null argument");
        if (n_parts < 1 || n_parts > PBN_HYBRID_PARTS || part < 0 || part >= n_parts) throw invalid_error("pbn_score_batch_parts: part / n_parts out of range (at most 64 parts)");
        for (int c = 0; c < n_cand; ++c) {
            bool disc = false;
            for (int j = par_off[c]; j < par_off[c + 1]; ++j) disc = disc || parents[j] >= sd->n;
            if (!disc || node_type[c] != PBN_NODE_CKDE) throw invalid_error("pbn_score_batch_parts: CKDE candidates with discrete parents only");
        }
        std::vector<double> whole((size_t)std::max(n_cand, 1));
        std::fill(out, out + (size_t)n_cand * PBN_HYBRID_PARTS, 0.0);
        if (n_cand <= 0) return;
        BatchArgs a;
        a.kind = kind; a.n_cand = n_cand; a.var = var; a.node_type = node_type; a.par_off = par_off; a.parents = parents;
        a.out = whole.data(); a.parts_rank = part; a.parts_world = n_parts; a.parts_out = out;
        score_batch_body(sd, a);
    });
}

}  // extern "C"
