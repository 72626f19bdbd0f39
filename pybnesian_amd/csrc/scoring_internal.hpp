// Internal declarations shared by the units of the score engine (scoring.hip, score_terms.hip, hybrid.hip and the passes they call).
#pragma once
#include <cstdint>
#include <functional>
#include <limits>
#include <map>
#include <set>
#include <memory>
#include <vector>

#include "common.hpp"
#include "joint_counts.hpp"

namespace pbn {
struct KdeModel;     // kde_model.hpp
struct GPool;        // kde_group.hpp
struct GUnit;
struct GroupBatch;
namespace score {

constexpr double MACHINE_TOL = 1.4901161193847656e-08;  // util/math_constants.hpp:30, sqrt(eps(double))
constexpr double LOG_2PI = 1.8378770664093454835606594728112;
constexpr double LOG_PI = 1.1447298858494001741434273513531;
const double INF = std::numeric_limits<double>::infinity();

struct Stats {  // pilot-shifted moments of a row set over all n columns (or a column subset, see users)
    int64_t N = 0;
    std::vector<double> S;  // n   : sum_r (x_rc - shift_c)
    std::vector<double> G;  // n*n : sum_r (x_ri - shift_i)(x_rj - shift_j), col-major symmetric
    void zero(int n) { N = 0; S.assign(n, 0.0); G.assign((size_t)n * n, 0.0); }
    void add(const Stats& o) {
        N += o.N;
        for (size_t i = 0; i < S.size(); ++i) S[i] += o.S[i];
        for (size_t i = 0; i < G.size(); ++i) G[i] += o.G[i];
    }
};

// What a family-count pass (family_counts.hip) keeps between calls: the scratch of a launch chunk (joint_counts.hpp) and the counters
// behind pbn_scoredata_discrete_stats.  Score data and a pbn_dtable (discrete_model.hip) each own one.
struct FamilyScratch {
    pbn::joint::Scratch fc;
    int64_t fc_device_units = 0, fc_host_units = 0, fc_launches = 0;
};

}  // namespace score
}  // namespace pbn

// Rows of the score regions grouped by (configuration of a set of discrete parents, region): see hybrid.hip
struct HybridGrouping {
    int nc = 1, nregions = 1;
    std::vector<int64_t> off;          // [nc * nregions + 1], cell = configuration * nregions + region
    pbn::dev_buf<int32_t> rows;        // device: permuted-table row ids, cell by cell
    pbn::dev_buf<int32_t> piece;       // device [npieces][3]: cell, first, last + 1 (pieces of <= 4096 rows)
    pbn::dev_buf<int32_t> piece_off;   // device [cells + 1]
    int npieces = 0;
    // moments of ALL continuous columns per cell (hybrid.hip group_moments): one gathered, segmented MFMA Gram per grouping - every
    // candidate over this grouping then takes its columns' entries on the host instead of a launch and a synchronisation of its own
    mutable std::vector<pbn::score::Stats> full;
    mutable int full_state = 0;        // 0 not tried, 1 ready, -1 not applicable (more than 64 continuous columns / too many cells)
    mutable int full_pieces = 0;       // pieces that launch took (read by the test aid pbn_debug_hybrid_moments only)
};

struct pbn_scoredata : pbn::score::FamilyScratch {
    pbn::ctx_ptr ctx;
    int dtype = PBN_F64;
    int n = 0;  // continuous columns
    int split = PBN_SPLIT_NONE;
    int k = 0;
    int selector = PBN_SEL_NORMAL_REFERENCE;  // bandwidth selector of the CKDEs fitted while scoring
    // A(S, m) of the CKDE likelihood scores, keyed by [region, m, sorted columns...] (see pbn_score_batch)
    std::map<std::vector<int>, double> kde_cache;
    // totals of A(S, m) over the test regions of a score kind, keyed by [kind, m, sorted columns...]: installed by pbn_score_terms_put (values another
    // rank computed) and preferred over kde_cache, so that every rank of a job assembles a candidate from the very same doubles
    std::map<std::vector<int>, double> term_total;
    int64_t kde_sweeps = 0;
    int64_t precise_redos = 0;   // fp64 terms evaluated a second time at per-row accuracy (kde_sum_needs_precision)
    // pbn_scoredata_set_precise: CKDE terms of fp64 tables are evaluated at the accuracy of the per-row path (polynomial 2^f, per-row pruning
    // margin, no fp32 tail, no moment pass), whatever the caches hold - their results replace the cached ones.  What the search's near-tie
    // check asks for (hc.hip); never on by default.
    bool force_precise = false;
    // hybrid likelihood local scores by [kind, node type, variable, sorted parents...] (see pbn_score_batch)
    std::map<std::vector<int>, double> score_memo;
    int64_t memo_hits = 0;
    int64_t cache_resets = 0;   // times kde_cache / score_memo started over (PBN_SCORE_CACHE_ENTRIES)
    bool partial = false;  // moments hold only this rank's row share (pbn_scoredata_create_sharded)
    // one process per GPU (pbn_scoredata_set_comm): pbn_score_batch evaluates this rank's share and completes the batch through the
    // host's all-gather (shard.hip)
    bool has_comm = false;
    pbn_comm comm{};
    const pbn_table* src = nullptr;  // caller's table (borrowed)
    pbn_table* perm_table = nullptr; // owned permuted copy (null for PBN_SPLIT_NONE)
    const pbn_table* table() const { return perm_table ? perm_table : src; }
    std::vector<int32_t> perm;    // permuted row -> source row
    std::vector<int32_t> limits;  // k+1 fold limits inside the CV region
    int64_t n_cv = 0;             // rows of the CV / training region [0, n_cv)
    int64_t n_hold = 0;           // hold-out test rows [n_cv, n_cv + n_hold)
    std::vector<double> shift;    // n pilot shifts
    pbn::dev_buf<double> shift_dev;
    pbn::score::Stats all;               // CV / training region
    std::vector<pbn::score::Stats> fold; // k
    pbn::score::Stats hold;              // hold-out test region
    // World-size-invariant summation (pbn_scoredata_create_sharded): every region is cut into a FIXED number of super-blocks
    // (boundaries a function of the region's length only); a super-block's moments come from one segment of one segmented Gram
    // launch - a function of the segment's rows only - and a region's moments are the sum of its segments in segment order,
    // whichever rank computed which segment.
    std::vector<pbn::score::Stats> seg;  // per segment
    std::vector<int> seg_region;         // 0 .. k-1 folds (or 0 = the CV / training region when k == 0), then the hold-out region
    std::vector<int64_t> seg_r0, seg_r1; // row range of the segment
    // discrete (dictionary) columns, addressed as column ids n .. n + n_disc - 1, in permuted row order
    int n_disc = 0;
    std::vector<std::vector<int32_t>> codes;
    std::vector<int> card;
    pbn::dev_buf<int32_t> rows_dev;  // gather lists (valid rows of BIC / BGe candidates on tables with nulls)
    // by [kind, sorted discrete parents...]; shared: a HybridBatch keeps the groupings its enqueued work reads alive until it has flushed
    std::map<std::vector<int>, std::shared_ptr<HybridGrouping>> groupings;
    // the codes once more on the device, and the family-count pass over them (family_counts.hip): int32 [n_disc][rows] in permuted row
    // order, and a byte mirror [n_disc][ld8] (0xFF past the last row, ld8 a multiple of 16) when every cardinality is <= 255
    pbn::dev_buf<int32_t> codes_dev;
    pbn::dev_buf<uint8_t> codes8;
    int64_t ld8 = 0;                 // 0: no byte mirror
    // (the pass's buffers and the counters of pbn_scoredata_discrete_stats: FamilyScratch)
    // pbn_scoredata_create_discrete: no table, n = 0, the discrete columns are ids 0 .. n_disc - 1
    bool discrete_only = false;
    // validity of the continuous columns (BIC / BGe on tables with nulls): byte masks, empty = no nulls
    std::vector<std::vector<uint8_t>> valid;
    bool has_nulls = false;
    // the same validity once more on the device (masked_moments.hip): valid_nw = ceil(n / 64) 64-bit words per row, bit c of a row's words
    // set when column c is valid there; empty without nulls.  mm_*: the masked pass's grow-only buffers and its counters.
    pbn::dev_buf<uint64_t> valid_words;
    int valid_nw = 0;
    pbn::dev_buf<char> mm_descs;
    pbn::dev_buf<int32_t> mm_owner;
    pbn::dev_buf<double> mm_partial;
    int64_t mm_launches = 0, mm_units = 0;
    // null codes (-1) of the discrete columns (BIC / BDe score data only): per column, and whether any column holds one
    std::vector<char> disc_null;
    bool has_disc_nulls = false;
};

namespace pbn {
namespace score {

// Shifted Gram of up to 64 columns over a contiguous row range or a device gather list -> raw S (d), G (d*d).
void gram_raw(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const int32_t* dev_rows,
              const double* shift_dev, double* S, double* G);
void subset_moments(const pbn_scoredata* sd, const Stats& st, const int* cols, int d, double* mu, double* sse);
void stats_minus(const Stats& a, const Stats& b, Stats& out);
// suspect (nullable, p >= 3 only): set when the normal equations cannot be trusted (see lg_fit) - refit with lg_fit_accurate
double lg_fit(int64_t N, int p, const double* mu, const double* S, double* beta, bool* suspect = nullptr);
// lg_accurate.hip: least-squares fit of cols[0] on cols[1..d-1] from double-double moments of the rows
// r < n0 ? row0 + r : row1 + (r - n0), r < n (through dev_rows when given).  d <= 16.  *rank (nullable): parents kept.
double lg_fit_accurate(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n0, int64_t row1, int64_t n,
                       const int32_t* dev_rows, double* beta, int* rank = nullptr);
bool lg_guard_on();   // PBN_LG_GUARD (default 1)
double bic_lg(int64_t N, int p, double variance);
double lg_slogl_from_rows(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const int32_t* dev_rows,
                          const double* beta, double variance);
double lg_slogl_from_moments(const pbn_scoredata* sd, const Stats& test, const int* cols, int p, const double* beta,
                             double variance);
// hybrid.hip: candidates with a discrete variable or discrete parents (synchronous)
// The CKDE slices (configuration c, region u) of a hybrid candidate fall into PBN_HYBRID_PARTS = 64 fixed PARTS, part = (c * regions + u) mod 64,
// and the candidate's score is the sum of its parts in part order - with one process as with many: a job with one process per GPU
// evaluates on rank r only the parts that rank owns and hands out the per-part sums (pbn_score_batch_parts).  Owners: the parts are dealt
// longest-processing-time first on their slices' training x test rows - every rank computes the same dealing from the same counts - so
// that the folds of a large configuration do not pile up on the ranks a fixed pattern would give them; which rank owns a part changes no
// bit of the result.
constexpr int PBN_HYBRID_PARTS = 64;
struct HybridParts {
    int rank, world;            // evaluate the parts dealt to `rank` of `world`
    double* out;                // [PBN_HYBRID_PARTS] per-part sums (0 for the parts not owned)
};
// CKDE candidates of one pbn_score_batch call evaluated together (hybrid.hip: HybridBatch): score_hybrid(..., hb, sink, &deferred) enqueues
// the candidate's sweeps and returns at once with *deferred = true; hybrid_batch_flush() runs the batch's one grouped chain, waits once and
// delivers every pending score through its sink (and its per-part sums through `parts->out`, which must stay valid until then).  Without a
// batch score_hybrid is synchronous.  hybrid_batch_end() frees the batch (waiting for whatever an exception left in flight).
struct HybridSink {
    double* out;                  // where the candidate's score goes
    std::vector<int> memo_key;    // non-empty: also remembered in pbn_scoredata::score_memo under this key
};
// One call of the batch engine (scoring.hip).  want (nullable, per candidate): 0 = the local score; 1 / 2 = only the joint / only the marginal
// CKDE term of the candidate, summed over the regions; 3 = a marginal TERM over all of the pseudo-candidate's columns (pbn_score_terms).
// only_region (nullable, per candidate; pbn_score_term_regions): >= 0 = that region's contribution alone (a CV fold; 0 for the hold-out score).
// parts_out (pbn_score_batch_parts): hybrid CKDE candidates evaluated on the parts of rank parts_rank of parts_world only, per-part sums to
// parts_out[c * PBN_HYBRID_PARTS ...].
struct BatchArgs {
    int kind = 0, n_cand = 0;
    const int *var = nullptr, *node_type = nullptr, *par_off = nullptr, *parents = nullptr;   // as pbn_score_batch takes them
    const double* params = nullptr;
    int n_params = 0;
    double* out = nullptr;
    const int* want = nullptr;
    int parts_rank = 0, parts_world = 0;
    double* parts_out = nullptr;
    const int* only_region = nullptr;
    int n_parents(int c) const { return par_off[c + 1] - par_off[c]; }
    int want_of(int c) const { return want ? want[c] : 0; }
};
// the engine itself: throws; the caller holds the handle's lock (guarded(mu_of(sd), ...))
void score_batch_body(pbn_scoredata* sd, const BatchArgs& a);
void candidate_cols(const BatchArgs& a, int c, std::vector<int>& cols);   // [variable, parents as given]
size_t score_cache_budget();   // PBN_SCORE_CACHE_ENTRIES (default 2^21): kde_cache / score_memo / term_total start over beyond it
// host buffers of one call, reused from candidate to candidate and from term to term (no allocation per candidate on the search's path)
struct ScoreScratch {
    Stats train;
    std::vector<int> cols;
    std::vector<double> mu, sse, beta, H;
};
// score_terms.hip: the plain CKDE candidates of a call (`pending`: their indices, in call order) through the set-function cache
void score_ckde_terms(pbn_scoredata* sd, const BatchArgs& a, const std::vector<int>& pending, ScoreScratch& s);

// ---- shared by the plain term engine (score_terms.hip) and the hybrid one (hybrid.hip) ----
struct Term { double value = 0; int slot = -1; };   // a term's cached value, or its slot in the device sums
bool f32_check_after();   // PBN_F32_CHECK (default 1; 0: measurement only): fp32 evaluations flagged by kde_wants_widening are redone on fp64 fragments
inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
// [x, m, sorted columns...]: the keys of kde_cache (x = region) and of term_total (x = score kind)
std::vector<int> set_key(int x, int m, const int* v, int nv);
// a unit of a grouped pool from a prepared model of nv columns: trained on every region but `region` (CV) or on region 0 (hold-out)
GUnit group_unit(bool cv, int R, int region, const KdeModel& m, int nv, int64_t ntrain, int64_t ntest, int slot);
// a pool's standardisation for the Morton keys (Wg, mug) from the covariance (nv x nv col-major) and means of its columns: L^-1 of the
// covariance; a singular one falls back to its diagonal - the keys only order the rows
void pool_standardise(GPool& P, const double* cov, const double* means, int nv);
// rows of one evaluation: training [row0, row0 + n0) ++ [row1, ...), test [te0, te0 + te_n) - of the table, or of a gather list
struct TermRows { int64_t row0, n0, row1, te0, te_n; };
// one term through a launch chain of its own, on the current lane: carves the lane's scratch_train, packs the training rows and enqueues the sweep
void enqueue_term_chain(pbn_ctx* ctx, KdeModel& m, const pbn_table* t, const int* cols, const TermRows& r, const int32_t* dev_rows, double* dev_sum,
                        double* dev_max, bool precise);
// closes collected pools - unit0 / nunits, their units behind dst's - and appends them to dst; bytes (nullable) grows by their arena bytes
void append_pools(GroupBatch& dst, const std::vector<GPool>& pools, const std::vector<std::vector<GUnit>>& pool_units, size_t* bytes);

// pbn_score_batch without / with the job's communicator (scoring.hip / shard.hip)
int score_batch_local(pbn_scoredata* sd, int kind, int n_cand, const int* var, const int* node_type, const int* par_off, const int* parents,
                      const double* params, int n_params, double* out);
void score_batch_sharded(pbn_scoredata* sd, int kind, int n_cand, const int* var, const int* node_type, const int* par_off, const int* parents,
                         const double* params, int n_params, double* out);
// Discrete candidates (variable and parents all discrete columns; hybrid.hip, family_counts.hip).  A region is a contiguous row range of
// the permuted table: a CV fold, the hold-out train or test part, or all of [0, n_cv).
struct Region { int64_t r0, r1; };
std::vector<Region> regions_of(const pbn_scoredata* sd, int kind);
// A family: the variable (fastest) and its parents in ascending column order, as indices into the DISCRETE columns; G = prod card.
constexpr int FAMILY_MAX_VARS = 8;                 // variable + 7 parents: the arrays of the device descriptor
constexpr int64_t FAMILY_MAX_CELLS = 1ll << 20;    // cells of one table counted on the device
constexpr int FAMILY_LDS_CELLS = 4096;             // up to here in LDS, above with global atomics
enum { FAMILY_HOST = 0, FAMILY_LDS_U8 = 1, FAMILY_LDS_I32 = 2, FAMILY_GLOBAL = 3 };   // what served a unit (pbn_debug_family_counts)
struct Family {
    std::vector<int> cols;
    int64_t G = 1;
};
// tables[ri][cell]: the family's counts in region ri
using FamilySink = std::function<void(size_t family, const std::vector<std::vector<int64_t>>& tables, int form)>;
// counts every family in every region - on the device where `device` allows it and the family fits (family_counts.hip), else with the
// host loop - and hands each family's tables to `sink`; the families are distinct
void count_families(pbn_scoredata* sd, const std::vector<Region>& regions, const std::vector<Family>& fams, bool device, const FamilySink& sink);
// The device pass by itself, over any table of codes: int32 [cols][ld32], and the byte mirror [cols][ld8] when ld8 > 0 (every cardinality
// <= 255; 0xFF in the rows past the last).  nulls: a code < 0 (0xFF in the mirror) is a null, and a row with a null in any column of a
// family is left out of that family's tables; without it no code may be negative.  `which` indexes the families to count - each must
// pass family_fits_device - and the regions are row ranges of the table.
struct FamilyCodes : pbn::joint::Codes {
    pbn_ctx* ctx = nullptr;
    FamilyScratch* scratch = nullptr;
    const int* card = nullptr;       // per column
    bool nulls = false;
};
bool family_fits_device(const Family& f);
void count_families_device(const FamilyCodes& src, const std::vector<Region>& regions, const std::vector<Family>& fams, const std::vector<size_t>& which,
                           const FamilySink& sink);
void family_counts_host(const pbn_scoredata* sd, const std::vector<Region>& regions, const Family& f, std::vector<std::vector<int64_t>>& tables);
void family_codes_upload(pbn_scoredata* sd);   // after pbn_scoredata_set_discrete filled sd->codes
Family make_family(const pbn_scoredata* sd, int var, const int* parents, int p);   // column ids of the score data; sorts the parents
// The discrete candidates of one pbn_score_batch call: checked as they come (check_discrete_candidate throws what the single-candidate
// path threw), counted together and finished on the host by score_discrete_batch, which writes *out and the memo.
struct DiscreteCand {
    int var;
    std::vector<int> parents;
    double* out;
    std::vector<int> memo_key;   // non-empty: also remembered in pbn_scoredata::score_memo
};
void check_discrete_candidate(const pbn_scoredata* sd, int kind, int node_type, const int* parents, int p);
void score_discrete_batch(pbn_scoredata* sd, int kind, double iss, std::vector<DiscreteCand>& cands);
// masked_moments.hip: (N, S, upper triangle of G) of up to 8 continuous columns over the rows valid in all of them, for a batch of units in
// one device pass.  rows == nullptr: the unit's rows are all rows of the table, one segment; else a device row list of n_list entries cut
// into the segments [seg_off[s], seg_off[s + 1]).  G row by row: (0,0) (0,1) ... (0,d-1) (1,1) ...
constexpr int MASKED_MAX_COLS = 8;
struct MaskedUnit {
    std::vector<int> cols;
    const int32_t* rows = nullptr;
    int64_t n_list = 0;
    std::vector<int64_t> seg_off;
};
struct MaskedMoments {
    int64_t N = 0;
    double S[MASKED_MAX_COLS] = {};
    double G[MASKED_MAX_COLS * (MASKED_MAX_COLS + 1) / 2] = {};
};
bool masked_moments_on();   // PBN_NULL_MOMENTS (default 1)
void masked_validity_upload(pbn_scoredata* sd);   // after pbn_scoredata_set_validity filled sd->valid
void masked_moments(pbn_scoredata* sd, const std::vector<MaskedUnit>& units, std::vector<std::vector<MaskedMoments>>& out);
// a unit's moments as Stats over all n columns (the unit's entries filled in, the rest zero)
void masked_to_stats(const pbn_scoredata* sd, const int* cols, int d, const MaskedMoments& m, Stats& st);
struct HybridBatch;
HybridBatch* hybrid_batch_begin(pbn_scoredata* sd);
void hybrid_batch_flush(HybridBatch* hb);
void hybrid_batch_end(HybridBatch* hb) noexcept;
double score_hybrid(pbn_scoredata* sd, int kind, int var, int node_type, const int* parents, int p, const HybridParts* parts = nullptr,
                    HybridBatch* hb = nullptr, const HybridSink* sink = nullptr, bool* deferred = nullptr);

}  // namespace score
}  // namespace pbn
