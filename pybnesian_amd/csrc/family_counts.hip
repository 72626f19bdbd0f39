// Joint counts of the discrete candidates of a score batch (factors/discrete/discrete_indices.cpp:134-150 joint_counts, as bic.cpp:66-96,
// mle_DiscreteFactor.cpp:5-41 and bde.cpp:5-47 use them): the tables of ALL families of one pbn_score_batch call in one device pass over
// the score data's codes, instead of one host loop over all rows per candidate.
//
// Unit of work = (family, region).  A family is the variable and its parents - variable fastest, parents in ascending column order, the
// order score_discrete_batch finishes them in; a region is a contiguous row range of the permuted table (a CV fold, the hold-out train or
// test part, or [0, n_cv)).  The unit's output is its table of prod(card) uint32 counts.
//
// The counting itself is the joint-count kernel of joint_counts.hip: its LDS form for tables of at most FAMILY_LDS_CELLS =
// 4 096 cells, its global-atomics form for tables of 4 097 ... 2^20 cells, on the byte mirror when every cardinality fits a byte, else on
// the int32 codes; regions start on any row.  Null-free score data runs its NONE policy; a pbn_dtable and score data with nulls run
// BY_CARD, which a null (-1, 0xFF in the mirror) fails - every other code lies in [0, card): pbn_scoredata_set_discrete and
// pbn_dtable_create refuse anything else.  What is kept here: the units per (family, region), the chunk budget, the sink and the form
// codes, the host fallback, the upload of the score data's codes and pbn_debug_family_counts.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "scoring_internal.hpp"

namespace pbn {
namespace score {

static_assert(joint::MAX_VARS >= FAMILY_MAX_VARS, "a family's columns fit the descriptor");

namespace {

constexpr int64_t CHUNK_CELLS = 1ll << 24; // cells of one launch chunk's count buffer: 64 MB of uint32 (PBN_DISCRETE_CHUNK_CELLS)

bool on_device(const pbn_scoredata* sd, const Family& f) {
    return sd->codes_dev.p && family_fits_device(f);
}

}  // namespace

bool family_fits_device(const Family& f) { return (int)f.cols.size() <= FAMILY_MAX_VARS && f.G <= FAMILY_MAX_CELLS; }

// The families `which` (all on_device), chunk by chunk through joint::run_chunk
void count_families_device(const FamilyCodes& src, const std::vector<Region>& regions, const std::vector<Family>& fams, const std::vector<size_t>& which,
                           const FamilySink& sink) {
    pbn_ctx* ctx = src.ctx;
    FamilyScratch* sd = src.scratch;
    HIP_CHECK(hipSetDevice(ctx->device));
    const bool bytes = src.ld8 > 0;
    const size_t R = regions.size();
    const int64_t budget = std::max<int64_t>(1, knob_ll("PBN_DISCRETE_CHUNK_CELLS", CHUNK_CELLS));   // (per call: the chunking test lowers it)
    std::vector<joint::Desc> descs[2];   // LDS form, global form
    std::vector<std::vector<int64_t>> tables(R);
    for (size_t base = 0; base < which.size();) {
        // a chunk: as many whole families as keep the count buffer within the budget (one family always fits: R tables of <= 2^20 cells)
        size_t end = base;
        int64_t cells = 0;
        while (end < which.size() && end - base < ((size_t)1 << 20) && (end == base || cells + fams[which[end]].G * (int64_t)R <= budget))
            cells += fams[which[end++]].G * (int64_t)R;
        const int64_t T = (int64_t)(end - base) * (int64_t)R;
        const int64_t want = std::max<int64_t>(1, ceil_div((int64_t)ctx->num_cus * 8, T));   // slices that fill the chip (plan_slices)
        descs[0].clear(); descs[1].clear();
        int64_t off = 0;
        for (size_t i = base; i < end; ++i) {
            const Family& f = fams[which[i]];
            const bool lds = f.G <= FAMILY_LDS_CELLS;
            for (size_t ri = 0; ri < R; ++ri) {
                joint::Desc d{};
                d.m = (int)f.cols.size(); d.G = (int)f.G;
                int stride = 1;
                for (int j = 0; j < d.m; ++j) { d.col[j] = f.cols[j]; d.card[j] = src.card[f.cols[j]]; d.stride[j] = stride; stride *= d.card[j]; }
                joint::plan_slices(d, regions[ri].r0, regions[ri].r1, bytes, lds, want, joint::MAX_COPIES);
                d.table_off = off;
                off += f.G;
                descs[lds ? 0 : 1].push_back(d);
            }
        }
        sd->fc_launches += joint::run_chunk(ctx, sd->fc, descs, (size_t)cells, src, src.nulls ? joint::BY_CARD : joint::NONE);
        const uint32_t* c = sd->fc.host.data();
        for (size_t i = base; i < end; ++i) {
            const Family& f = fams[which[i]];
            for (size_t ri = 0; ri < R; ++ri, c += f.G) tables[ri].assign(c, c + f.G);
            sink(which[i], tables, f.G <= FAMILY_LDS_CELLS ? (bytes ? FAMILY_LDS_U8 : FAMILY_LDS_I32) : FAMILY_GLOBAL);
        }
        sd->fc_device_units += T;
        base = end;
    }
}

// sd->codes (permuted row order) -> the device: int32 [n_disc][rows], and the byte mirror when every cardinality is <= 255 (a null code -1 is
// 0xFF there, the rule of a pbn_dtable's mirror: joint::byte_mirror keeps the low byte)
void family_codes_upload(pbn_scoredata* sd) {
    pbn_ctx* ctx = sd->ctx;
    const int64_t rows = (int64_t)sd->perm.size();
    sd->codes_dev.release();
    sd->codes8.release();
    sd->ld8 = 0;
    if (sd->n_disc <= 0 || rows <= 0) return;
    HIP_CHECK(hipSetDevice(ctx->device));
    sd->codes_dev.alloc((size_t)sd->n_disc * rows);
    for (int j = 0; j < sd->n_disc; ++j)
        HIP_CHECK(hipMemcpyAsync(sd->codes_dev.p + (size_t)j * rows, sd->codes[j].data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const int max_card = *std::max_element(sd->card.begin(), sd->card.end());
    if (max_card <= 255 && sd->n_disc <= 65535) {
        sd->ld8 = ceil_div(rows, joint::MIRROR_ALIGN) * joint::MIRROR_ALIGN;
        sd->codes8.alloc((size_t)sd->ld8 * sd->n_disc);
        joint::byte_mirror(ctx, sd->codes_dev.p, rows, sd->n_disc, sd->codes8.p, sd->ld8);
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void count_families(pbn_scoredata* sd, const std::vector<Region>& regions, const std::vector<Family>& fams, bool device, const FamilySink& sink) {
    std::vector<size_t> dev;
    if (device)
        for (size_t f = 0; f < fams.size(); ++f)
            if (on_device(sd, fams[f])) dev.push_back(f);
    if (!dev.empty()) {
        FamilyCodes src;
        src.ctx = sd->ctx; src.scratch = sd; src.card = sd->card.data();
        src.codes32 = sd->codes_dev.p; src.ld32 = (int64_t)sd->perm.size();
        src.codes8 = sd->codes8.p; src.ld8 = sd->ld8;
        // null codes (BIC / BDe score data, pbn_scoredata_set_discrete): the null-aware instantiations, when a column of the call's families holds one
        src.nulls = false;
        if (sd->has_disc_nulls)
            for (size_t f : dev)
                for (int c : fams[f].cols) src.nulls = src.nulls || sd->disc_null[c];
        count_families_device(src, regions, fams, dev, sink);
    }
    std::vector<std::vector<int64_t>> tables;
    for (size_t f = 0; f < fams.size(); ++f) {
        if (device && on_device(sd, fams[f])) continue;
        family_counts_host(sd, regions, fams[f], tables);
        sink(f, tables, FAMILY_HOST);
        sd->fc_host_units += (int64_t)regions.size();
    }
}

}  // namespace score
}  // namespace pbn

using namespace pbn;
using namespace pbn::score;

extern "C" {

int pbn_scoredata_discrete_stats(const pbn_scoredata* sd, int64_t* device_units, int64_t* host_units, int64_t* launches) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_discrete_stats: null argument");
        if (device_units) *device_units = sd->fc_device_units;
        if (host_units) *host_units = sd->fc_host_units;
        if (launches) *launches = sd->fc_launches;
    });
}

// pbn_debug_family_counts (test aid, not part of the C ABI header): the tables of a batch of families as the batch path of pbn_score_batch
// counts them - same deduplication, same chunking, same choice of form, PBN_DISCRETE_COUNTS honoured.  Family f = var[f] with parents
// parents[par_off[f] .. par_off[f + 1]) (column ids of the score data, any order); unit u = f * regions + region over the regions of `kind`
// (BIC / BDe: [0, n_cv); CV: the folds; hold-out: train, test).  out_off[u] .. out_off[u + 1] (n_fam * regions + 1 entries) is unit u's
// table in out_counts, the variable fastest, the parents in ascending column order; out_form[u] is what served it (0 host loop, 1 LDS on
// the byte mirror, 2 LDS on the int32 codes, 3 global atomics).  PBN_ERR_INVALID when the tables need more than `cap` entries.
int pbn_debug_family_counts(pbn_scoredata* sd, int kind, int n_fam, const int* var, const int* par_off, const int* parents, int64_t* out_off,
                            int64_t* out_counts, int64_t cap, int* out_form) {
    return guarded(mu_of(sd), [&] {
        if (!sd || n_fam < 0 || (n_fam > 0 && (!var || !par_off || !out_off || !out_counts || !out_form))) throw invalid_error("pbn_debug_family_counts: bad argument");
        if (kind == PBN_SCORE_CVLIK && sd->k <= 0) throw invalid_error("pbn_debug_family_counts: score data has no CV folds");
        if (kind == PBN_SCORE_HOLDOUT && sd->n_hold <= 0) throw invalid_error("pbn_debug_family_counts: score data has no hold-out split");
        const std::vector<Region> regions = regions_of(sd, kind);
        const size_t R = regions.size();
        std::map<std::vector<int>, size_t> seen;
        std::vector<Family> fams;
        std::vector<size_t> fam_of((size_t)n_fam);
        int64_t total = 0;
        for (int i = 0; i < n_fam; ++i) {
            const int p = par_off[i + 1] - par_off[i];
            if (p < 0 || (p > 0 && !parents)) throw invalid_error("pbn_debug_family_counts: bad parent offsets");
            for (int j = -1; j < p; ++j) {
                const int c = j < 0 ? var[i] : parents[par_off[i] + j];
                if (c < sd->n || c >= sd->n + sd->n_disc) throw invalid_error("pbn_debug_family_counts: discrete columns only");
            }
            Family f = make_family(sd, var[i], parents + par_off[i], p);
            auto it = seen.find(f.cols);
            if (it == seen.end()) { it = seen.emplace(f.cols, fams.size()).first; fams.push_back(std::move(f)); }
            fam_of[i] = it->second;
            for (size_t ri = 0; ri < R; ++ri) { out_off[(size_t)i * R + ri] = total; total += fams[it->second].G; }
        }
        out_off[(size_t)n_fam * R] = total;
        if (total > cap) throw invalid_error("pbn_debug_family_counts: the tables need more entries than cap");
        std::vector<std::vector<size_t>> askers(fams.size());
        for (int i = 0; i < n_fam; ++i) askers[fam_of[i]].push_back((size_t)i);
        count_families(sd, regions, fams, knob_int("PBN_DISCRETE_COUNTS", 1) != 0, [&](size_t f, const std::vector<std::vector<int64_t>>& tables, int form) {
            for (size_t i : askers[f])
                for (size_t ri = 0; ri < R; ++ri) {
                    std::memcpy(out_counts + out_off[i * R + ri], tables[ri].data(), tables[ri].size() * sizeof(int64_t));
                    out_form[i * R + ri] = form;
                }
        });
    });
}

}  // extern "C"
