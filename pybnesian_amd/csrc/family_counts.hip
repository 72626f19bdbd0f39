// Joint counts of the discrete candidates of a score batch (factors/discrete/discrete_indices.cpp:134-150 joint_counts, as bic.cpp:66-96,
// mle_DiscreteFactor.cpp:5-41 and bde.cpp:5-47 use them): the tables of ALL families of one pbn_score_batch call in one device pass over
// the score data's codes, instead of one host loop over all rows per candidate.
//
// Unit of work = (family, region).  A family is the variable and its parents - variable fastest, parents in ascending column order, the
// order score_discrete_batch finishes them in; a region is a contiguous row range of the permuted table (a CV fold, the hold-out train or
// test part, or [0, n_cv)).  The unit's output is its table of prod(card) uint32 counts.
//
// Two forms, one kernel text.  Tables of at most FAMILY_LDS_CELLS = 4 096 cells: one workgroup per (unit, row slice), lanes form the keys of
// their rows from the unit's code columns and add into replicated sub-tables in LDS (the replication and the one-bank stagger of the
// copies are chisq.hip's, DESIGN.md 3.11: LDS atomics on one address serialise), then the workgroup adds its table into the unit's table in
// global memory.  Tables of 4 097 ... 2^20 cells: every lane adds straight into the unit's zeroed table in global memory - at these sizes
// the rows of a wave spread over many cells, and one slice of a 2^20-cell table would otherwise flush 4 MB.  All sums are integer: no
// order of adds can change a count.
//
// Codes come from a byte mirror (8 consecutive rows of a column per 8-byte load) when every cardinality fits a byte, else from the int32
// codes (4 coalesced loads 256 rows apart).  Regions start on any row: a byte-form slice starts on the multiple of 8 at or below its
// region's first row and masks the rows outside [row0, row1) - the loads stay aligned and never leave the mirror's padded column.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "scoring_internal.hpp"

namespace pbn {
namespace score {

namespace {

constexpr int BLOCK = 256;
constexpr int LDS_WORDS = 8192;            // 32 KiB of counters per workgroup: five workgroups per CU of the 160 KiB
constexpr int MAX_COPIES = 32;             // replicated sub-tables of one workgroup
constexpr int ROWS_PER_LANE_U8 = 8;        // one 8-byte load per column and step
constexpr int ROWS_PER_LANE_I32 = 4;       // four coalesced 4-byte loads per column and step
constexpr int SLICE_ALIGN = BLOCK * ROWS_PER_LANE_U8;   // rows of a slice: a multiple of it
constexpr int MIRROR_ALIGN = FAMILY_MIRROR_ALIGN;   // the byte mirror's leading dimension is a multiple of it (rows past the last hold 0xFF)
constexpr int64_t CHUNK_CELLS = 1ll << 24; // cells of one launch chunk's count buffer: 64 MB of uint32 (PBN_DISCRETE_CHUNK_CELLS)

struct Desc {
    int m, G;
    int col[FAMILY_MAX_VARS];      // discrete column index, the variable first
    int stride[FAMILY_MAX_VARS];   // the variable fastest
    int copies, copy_stride;       // LDS form: R replicated sub-tables, copy c at c * copy_stride
    int slices;                    // workgroups of this unit: slice s takes rows [base + s * rows_per_slice, ...) within [row0, row1)
    int64_t table_off;             // first cell of its table in the launch's count buffer
    int64_t row0, row1, base, rows_per_slice;
};

// R = the largest power of two <= MAX_COPIES for which R padded tables fit LDS_WORDS; the copy stride is G rounded up to the 32 banks
// plus one, so that cell c of copy r lies on bank (r + c) mod 32 (chisq.hip, copies_for: the same rule)
void copies_for(int G, int* copies, int* copy_stride) {
    const int padded = ((G + 31) & ~31) + 1;
    int r = 1;
    while (2 * r <= MAX_COPIES && (int64_t)2 * r * padded <= LDS_WORDS) r *= 2;
    *copies = r;
    *copy_stride = r == 1 ? G : padded;
}

// grid = (units, slices).  LDS = true: cells[] holds the workgroup's copies; false: the lanes add into the unit's table in global memory.
// NULLS = true (the tables of a pbn_dtable, discrete_model.hip): a row with a null - byte 0xFF, int32 code < 0 - in ANY column of the
// unit is left out of the unit's table (the combined bitmap of discrete_indices.cpp:134-150); false compiles to the text it was before.
template <typename CodeT, bool LDS, bool NULLS>
__global__ __launch_bounds__(BLOCK) void family_count_kernel(const Desc* __restrict__ descs, const CodeT* __restrict__ codes, int64_t ld,
                                                              uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t cells[];   // [copies][copy_stride]
    const Desc& d = descs[blockIdx.x];
    const int slice = blockIdx.y;
    if (slice >= d.slices) return;
    const int tid = threadIdx.x, m = d.m, copies = d.copies, copy_stride = d.copy_stride;
    const uint32_t G = (uint32_t)d.G;
    uint32_t* out = counts + d.table_off;
    uint32_t* mine = out;
    if constexpr (LDS) {
        const int words = copies * copy_stride;
        for (int i = tid; i < words; i += BLOCK) cells[i] = 0u;
        __syncthreads();
        mine = cells + (tid & (copies - 1)) * copy_stride;
    }
    const int64_t row0 = d.row0, row1 = d.row1;
    const int64_t s0 = d.base + (int64_t)slice * d.rows_per_slice;
    const int64_t s1 = s0 + d.rows_per_slice < row1 ? s0 + d.rows_per_slice : row1;
    if constexpr (sizeof(CodeT) == 1) {
        constexpr int V = ROWS_PER_LANE_U8;
        for (int64_t r = s0 + (int64_t)tid * V; r < s1; r += (int64_t)BLOCK * V) {   // r is a multiple of 8 below ld: r + 7 < ld
            uint32_t key[V];
            uint32_t null_rows = 0u;   // NULLS: bit i = row r + i has a null in one of the unit's columns
#pragma unroll
            for (int i = 0; i < V; ++i) key[i] = 0u;
            for (int j = 0; j < m; ++j) {
                const uint2 v = *reinterpret_cast<const uint2*>(codes + (int64_t)d.col[j] * ld + r);
                const uint32_t stride = (uint32_t)d.stride[j];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t code = ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xFFu;
                    key[i] += code * stride;
                    if constexpr (NULLS) null_rows |= (code == 0xFFu ? 1u : 0u) << i;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (r + i >= row0 && r + i < s1 && key[i] < G && !(NULLS && ((null_rows >> i) & 1u))) atomicAdd(mine + key[i], 1u);
        }
    } else {
        constexpr int V = ROWS_PER_LANE_I32;
        for (int64_t r = (s0 < row0 ? row0 : s0) + tid; r < s1; r += (int64_t)BLOCK * V) {
            uint32_t key[V];
            uint32_t null_rows = 0u;
#pragma unroll
            for (int i = 0; i < V; ++i) key[i] = 0u;
            for (int j = 0; j < m; ++j) {
                const CodeT* col = codes + (int64_t)d.col[j] * ld + r;
                const uint32_t stride = (uint32_t)d.stride[j];
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (r + (int64_t)i * BLOCK < s1) {
                        const CodeT code = col[(int64_t)i * BLOCK];
                        key[i] += (uint32_t)code * stride;
                        if constexpr (NULLS) null_rows |= (code < 0 ? 1u : 0u) << i;
                    }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (r + (int64_t)i * BLOCK < s1 && key[i] < G && !(NULLS && ((null_rows >> i) & 1u))) atomicAdd(mine + key[i], 1u);
        }
    }
    if constexpr (LDS) {
        __syncthreads();
        // flush: the R copies of a cell, summed; a unit of one slice owns its table (plain stores over the zeroed buffer)
        const bool single = d.slices == 1;
        for (uint32_t cell = tid; cell < G; cell += BLOCK) {
            uint32_t s = 0u;
            for (int c = 0; c < copies; ++c) s += cells[c * copy_stride + cell];
            if (s == 0u) continue;
            if (single) out[cell] = s;
            else atomicAdd(out + cell, s);
        }
    }
}

// one thread packs four rows of one column; 0xFF in the padding rows n ... ld8 - 1
__global__ __launch_bounds__(BLOCK) void family_byte_mirror_kernel(const int32_t* __restrict__ codes, int64_t n, uint8_t* __restrict__ mirror,
                                                                    int64_t ld8) {
    const int64_t r = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (r >= ld8) return;
    const int32_t* col = codes + (int64_t)blockIdx.y * n;
    uint32_t packed = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) packed |= (r + i < n ? (uint32_t)col[r + i] & 0xFFu : 0xFFu) << (8 * i);
    *reinterpret_cast<uint32_t*>(mirror + (int64_t)blockIdx.y * ld8 + r) = packed;
}

// the codes are the byte mirror (codes8, leading dimension ld8) when ld8 > 0, else the int32 codes (codes32, ld32)
template <bool LDS, bool NULLS>
void launch_count(const Desc* descs, int n_units, int max_slices, int lds_words, const uint8_t* codes8, int64_t ld8, const int32_t* codes32, int64_t ld32,
                  uint32_t* counts, hipStream_t st) {
    if (n_units <= 0) return;
    if (lds_words < 0 || lds_words > LDS_WORDS || max_slices < 1 || max_slices > 65535) throw invalid_error("family counts: bad launch shape");
    const dim3 grid((unsigned)n_units, (unsigned)max_slices), block(BLOCK);
    const size_t lds = LDS ? (size_t)lds_words * sizeof(uint32_t) : 0;
    if (ld8 > 0) hipLaunchKernelGGL((family_count_kernel<uint8_t, LDS, NULLS>), grid, block, lds, st, descs, codes8, ld8, counts);
    else hipLaunchKernelGGL((family_count_kernel<int32_t, LDS, NULLS>), grid, block, lds, st, descs, codes32, ld32, counts);
    HIP_CHECK(hipGetLastError());
}

bool on_device(const pbn_scoredata* sd, const Family& f) {
    return sd->codes_dev.p && family_fits_device(f);
}

}  // namespace

bool family_fits_device(const Family& f) { return (int)f.cols.size() <= FAMILY_MAX_VARS && f.G <= FAMILY_MAX_CELLS; }

// The families `which` (all on_device), chunk by chunk: descriptors up, one memset, one launch per form present, the chunk's tables down.
void count_families_device(const FamilyCodes& src, const std::vector<Region>& regions, const std::vector<Family>& fams, const std::vector<size_t>& which,
                           const FamilySink& sink) {
    pbn_ctx* ctx = src.ctx;
    FamilyScratch* sd = src.scratch;
    HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const bool bytes = src.ld8 > 0;
    const size_t R = regions.size();
    const int64_t budget = std::max<int64_t>(1, knob_ll("PBN_DISCRETE_CHUNK_CELLS", CHUNK_CELLS));   // (per call: the chunking test lowers it)
    std::vector<Desc> descs[2];   // LDS form, global form
    std::vector<std::vector<int64_t>> tables(R);
    for (size_t base = 0; base < which.size();) {
        // a chunk: as many whole families as keep the count buffer within the budget (one family always fits: R tables of <= 2^20 cells)
        size_t end = base;
        int64_t cells = 0;
        while (end < which.size() && end - base < ((size_t)1 << 20) && (end == base || cells + fams[which[end]].G * (int64_t)R <= budget))
            cells += fams[which[end++]].G * (int64_t)R;
        const int64_t T = (int64_t)(end - base) * (int64_t)R;
        // slices: enough workgroups to fill the chip when the chunk has few units, while a slice's flush (G cells) stays small against
        // its row work: at least max(4096, 8 G) rows per LDS slice, 4096 per global one
        const int64_t want = std::max<int64_t>(1, ceil_div((int64_t)ctx->num_cus * 8, T));
        descs[0].clear(); descs[1].clear();
        int max_slices[2] = {1, 1}, lds_words = 1;
        int64_t off = 0;
        for (size_t i = base; i < end; ++i) {
            const Family& f = fams[which[i]];
            const bool lds = f.G <= FAMILY_LDS_CELLS;
            for (size_t ri = 0; ri < R; ++ri) {
                Desc d{};
                d.m = (int)f.cols.size(); d.G = (int)f.G;
                int stride = 1;
                for (int j = 0; j < d.m; ++j) { d.col[j] = f.cols[j]; d.stride[j] = stride; stride *= src.card[f.cols[j]]; }
                if (lds) copies_for(d.G, &d.copies, &d.copy_stride);
                d.row0 = regions[ri].r0; d.row1 = regions[ri].r1;
                d.base = bytes ? d.row0 / ROWS_PER_LANE_U8 * ROWS_PER_LANE_U8 : d.row0;
                const int64_t rows = std::max<int64_t>(1, d.row1 - d.base);
                const int64_t cap = std::max<int64_t>(1, rows / std::max<int64_t>(4096, lds ? 8 * f.G : 0));
                const int64_t s = std::min<int64_t>(std::min(want, cap), 65535);
                d.rows_per_slice = ceil_div(ceil_div(rows, s), SLICE_ALIGN) * SLICE_ALIGN;
                d.slices = (int)ceil_div(rows, d.rows_per_slice);
                d.table_off = off;
                off += f.G;
                max_slices[lds ? 0 : 1] = std::max(max_slices[lds ? 0 : 1], d.slices);
                if (lds) lds_words = std::max(lds_words, d.copies * d.copy_stride);
                descs[lds ? 0 : 1].push_back(d);
            }
        }
        const size_t n0 = descs[0].size(), n1 = descs[1].size();
        sd->fc_descs.reserve((n0 + n1) * sizeof(Desc));
        sd->fc_counts.reserve((size_t)cells);
        if (sd->fc_host.size() < (size_t)cells) sd->fc_host.resize((size_t)cells);
        Desc* dd = reinterpret_cast<Desc*>(sd->fc_descs.p);
        if (n0) HIP_CHECK(hipMemcpyAsync(dd, descs[0].data(), n0 * sizeof(Desc), hipMemcpyHostToDevice, st));
        if (n1) HIP_CHECK(hipMemcpyAsync(dd + n0, descs[1].data(), n1 * sizeof(Desc), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(sd->fc_counts.p, 0, (size_t)cells * sizeof(uint32_t), st));
        if (src.nulls) {
            launch_count<true, true>(dd, (int)n0, max_slices[0], lds_words, src.codes8, src.ld8, src.codes32, src.ld32, sd->fc_counts.p, st);
            launch_count<false, true>(dd + n0, (int)n1, max_slices[1], 0, src.codes8, src.ld8, src.codes32, src.ld32, sd->fc_counts.p, st);
        } else {
            launch_count<true, false>(dd, (int)n0, max_slices[0], lds_words, src.codes8, src.ld8, src.codes32, src.ld32, sd->fc_counts.p, st);
            launch_count<false, false>(dd + n0, (int)n1, max_slices[1], 0, src.codes8, src.ld8, src.codes32, src.ld32, sd->fc_counts.p, st);
        }
        sd->fc_launches += (n0 ? 1 : 0) + (n1 ? 1 : 0);
        HIP_CHECK(hipMemcpyAsync(sd->fc_host.data(), sd->fc_counts.p, (size_t)cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));   // (the descriptors are read by then as well)
        const uint32_t* c = sd->fc_host.data();
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
// 0xFF there, the rule of a pbn_dtable's mirror: family_byte_mirror_kernel keeps the low byte)
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
        sd->ld8 = ceil_div(rows, MIRROR_ALIGN) * MIRROR_ALIGN;
        sd->codes8.alloc((size_t)sd->ld8 * sd->n_disc);
        family_byte_mirror(ctx, sd->codes_dev.p, rows, sd->n_disc, sd->codes8.p, sd->ld8);
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

void family_byte_mirror(pbn_ctx* ctx, const int32_t* codes_dev, int64_t rows, int n_cols, uint8_t* mirror, int64_t ld8) {
    hipLaunchKernelGGL(family_byte_mirror_kernel, dim3((unsigned)ceil_div(ld8 / 4, BLOCK), (unsigned)n_cols), dim3(BLOCK), 0, ctx->stream, codes_dev, rows,
                       mirror, ld8);
    HIP_CHECK(hipGetLastError());
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
