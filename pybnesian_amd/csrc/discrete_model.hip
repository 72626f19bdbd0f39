// Fitting and evaluating a discrete network in one device pass (learning/parameters/mle_DiscreteFactor.cpp:5-41,
// factors/discrete/DiscreteFactor.cpp:34-76,133-171, factors/discrete/discrete_indices.cpp:134-150 joint_counts,
// models/BayesianNetwork.hpp:960-994 fit / logl / slogl of the network) - instead of one host pass over all rows per node.
//
// pbn_dtable: the dictionary codes of a table on the device, outside any score data and WITH nulls (code -1; 0xFF in the byte mirror,
// which exists when every cardinality is <= 255 - no valid code is 0xFF then).  Its family tables come from the joint-count kernel's
// null-aware instantiations (family_counts.hip): a row with a null in any variable of a family is left out of that family's table.
//
// pbn_dnet: the concatenated CPTs of a fitted network.  dnet_logl_kernel evaluates all nodes for a tile of rows: a lane owns 8 consecutive
// rows of the byte mirror (one 8-byte load per family column and node) or 4 rows 256 apart of the int32 codes, forms each node's key,
// checks it against the node's cell count, gathers logprob[cpt_off + key] and adds it to the row's running sum - fp64 adds only, the
// nodes in node order, the first node's value as the start: what `out = ll_0; out = out + ll_1; ...` computes on the host, bit for bit.
// Code columns are NOT staged in LDS: a network has any number of columns (a tile of all of them need not fit), a column is read once
// per family it belongs to - 1 + its children - and a workgroup's 2 KiB of it stay in the L1 / L2 between those reads; the CPTs are the
// random part of the traffic and are cache-resident as well (40 nodes x <= 625 cells x 8 B in the timing tool's networks).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "common.hpp"
#include "discrete_model.hpp"
#include "net_eval.hpp"
#include "scoring_internal.hpp"

using namespace pbn;
using namespace pbn::score;

namespace {

constexpr int BLOCK = 256;
constexpr int ROWS_U8 = 8, ROWS_I32 = 4;       // rows of a lane: the row tile of a workgroup is 2 048 (byte mirror) / 1 024 (int32 codes)
constexpr int64_t DNET_MAX_CELLS = 2147483647; // cells of one CPT: keys are formed in 32 bits

struct DNode {
    int m;                          // family variables
    uint32_t G;                     // cells of the CPT
    int64_t cpt_off;                // first cell in the concatenated CPTs
    int col[FAMILY_MAX_VARS];       // the variable first, then the parents as given
    uint32_t stride[FAMILY_MAX_VARS];
};

}  // namespace

struct pbn_dnet {
    pbn::ctx_ptr ctx;
    int n_cols = 0;
    std::vector<int> card;
    std::vector<DNode> nodes;
    std::vector<double> logprob;                // host copy (slogl)
    pbn::dev_buf<DNode> nodes_dev;
    pbn::dev_buf<double> logprob_dev;
    pbn::dev_buf<double> out_dev;               // grow-only: the rows' sums of one pbn_dnet_logl call
    int64_t logl_launches = 0, rows_evaluated = 0;
};

namespace {

// grid = row tiles.  VGPRs: 8 (4) running sums in fp64, as many keys, the null bits and two loaded words; no LDS, no scratch.
template <typename CodeT>
__global__ __launch_bounds__(BLOCK) void dnet_logl_kernel(const DNode* __restrict__ nodes, int n_nodes, const double* __restrict__ logprob,
                                                           const CodeT* __restrict__ codes, int64_t ld, int64_t n_rows, double* __restrict__ out) {
    constexpr bool BYTES = sizeof(CodeT) == 1;
    constexpr int V = BYTES ? ROWS_U8 : ROWS_I32;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    // row i of this lane: BYTES r + i (r a multiple of 8 below ld: r + 7 < ld), else r + i * BLOCK
    const int64_t r = BYTES ? ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * V : (int64_t)blockIdx.x * BLOCK * V + threadIdx.x;
    if (r >= n_rows) return;
    double acc[V];
    for (int n = 0; n < n_nodes; ++n) {
        const DNode& d = nodes[n];
        const int m = d.m;
        uint32_t key[V];
        uint32_t null_rows = 0u;   // bit i: row i has a null in one of the node's family columns
#pragma unroll
        for (int i = 0; i < V; ++i) key[i] = 0u;
        for (int j = 0; j < m; ++j) {
            const CodeT* col = codes + (int64_t)d.col[j] * ld + r;
            const uint32_t stride = d.stride[j];
            if constexpr (BYTES) {
                const uint2 v = *reinterpret_cast<const uint2*>(col);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t code = ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xFFu;
                    key[i] += code * stride;
                    null_rows |= (code == 0xFFu ? 1u : 0u) << i;
                }
            } else {
#pragma unroll
                for (int i = 0; i < V; ++i)
                    if (r + (int64_t)i * BLOCK < n_rows) {
                        const int32_t code = col[(int64_t)i * BLOCK];
                        key[i] += (uint32_t)code * stride;
                        null_rows |= (code < 0 ? 1u : 0u) << i;
                    }
            }
        }
        const double* cpt = logprob + d.cpt_off;
        const uint32_t G = d.G;
#pragma unroll
        for (int i = 0; i < V; ++i) {
            // the key is an address only when it is inside the CPT (G >= 1: cell 0 exists)
            const bool ok = key[i] < G && !((null_rows >> i) & 1u);
            const double lp = cpt[ok ? key[i] : 0u];
            const double v = ok ? lp : nan;
            acc[i] = n == 0 ? v : acc[i] + v;
        }
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int64_t row = BYTES ? r + i : r + (int64_t)i * BLOCK;
        if (row < n_rows) out[row] = acc[i];
    }
}

// ---- families of a call over a pbn_dtable ----------------------------------------------------------------------------------------------

struct AskedFamily {
    std::vector<int> cols;   // the variable, then the parents as given
    int64_t G = 1;
    size_t canon = 0;        // index into the distinct families (the variable, then the parents ascending)
};

// table in canonical order (the variable, then the parents ascending) -> the order of `cols`
void permute_table(const std::vector<int>& card, const std::vector<int>& canon_cols, const std::vector<int>& cols, const int64_t* src, int64_t* dst) {
    const size_t m = cols.size();
    if (canon_cols == cols) { std::memcpy(dst, src, (size_t)cells_of(card, cols, "") * sizeof(int64_t)); return; }
    std::vector<int64_t> stride_by_col(card.size(), 0);
    int64_t s = 1;
    for (size_t j = 0; j < m; ++j) { stride_by_col[cols[j]] = s; s *= card[cols[j]]; }
    std::vector<int64_t> dst_stride(m);
    std::vector<int> digit(m, 0), radix(m);
    for (size_t j = 0; j < m; ++j) { dst_stride[j] = stride_by_col[canon_cols[j]]; radix[j] = card[canon_cols[j]]; }
    int64_t to = 0;
    for (int64_t cell = 0; cell < s; ++cell) {
        dst[to] = src[cell];
        for (size_t j = 0; j < m; ++j) {   // the next canonical cell: a mixed-radix increment
            to += dst_stride[j];
            if (++digit[j] < radix[j]) break;
            to -= dst_stride[j] * radix[j];
            digit[j] = 0;
        }
    }
}

// the host loop (discrete_indices.cpp:134-150 with the combined bitmap): the table in the order of `cols`
void family_counts_host_nulls(const pbn_dtable* dt, const std::vector<int>& cols, int64_t G, std::vector<int64_t>& table) {
    table.assign((size_t)G, 0);
    const size_t m = cols.size();
    std::vector<int64_t> stride(m);
    int64_t s = 1;
    for (size_t j = 0; j < m; ++j) { stride[j] = s; s *= dt->card[cols[j]]; }
    for (int64_t r = 0; r < dt->n_rows; ++r) {
        int64_t key = 0;
        bool valid = true;
        for (size_t j = 0; j < m; ++j) {
            const int32_t c = dt->codes[cols[j]][r];
            if (c < 0) { valid = false; break; }
            key += c * stride[j];
        }
        if (valid) ++table[(size_t)key];
    }
}

// Every asked family's table in the order asked, through `sink(i, table, form)`: distinct families are counted once, on the device where
// they fit (at most 8 variables and 2^20 cells) and otherwise by the host loop inside the same call.
template <typename Sink>
void dtable_family_counts(pbn_dtable* dt, const std::vector<AskedFamily>& asked, size_t n_canon, const std::vector<Family>& fams, const Sink& sink) {
    std::vector<std::vector<size_t>> askers(n_canon);
    for (size_t i = 0; i < asked.size(); ++i) askers[asked[i].canon].push_back(i);
    std::vector<int64_t> permuted;
    auto deliver = [&](size_t f, const std::vector<int64_t>& table, int form) {
        for (size_t i : askers[f]) {
            if (asked[i].cols == fams[f].cols) { sink(i, table.data(), form); continue; }
            permuted.resize(table.size());
            permute_table(dt->card, fams[f].cols, asked[i].cols, table.data(), permuted.data());
            sink(i, permuted.data(), form);
        }
    };
    std::vector<size_t> dev;
    for (size_t f = 0; f < fams.size(); ++f)
        if (dt->codes_dev.p && family_fits_device(fams[f])) dev.push_back(f);
    if (!dev.empty()) {
        FamilyCodes src;
        src.ctx = dt->ctx; src.scratch = dt; src.card = dt->card.data();
        src.codes32 = dt->codes_dev.p; src.ld32 = dt->n_rows;
        src.codes8 = dt->codes8.p; src.ld8 = dt->ld8;
        src.nulls = true;
        const std::vector<Region> all{Region{0, dt->n_rows}};
        count_families_device(src, all, fams, dev, [&](size_t f, const std::vector<std::vector<int64_t>>& tables, int form) { deliver(f, tables[0], form); });
    }
    std::vector<int64_t> table;
    for (size_t f = 0; f < fams.size(); ++f) {
        if (dt->codes_dev.p && family_fits_device(fams[f])) continue;
        family_counts_host_nulls(dt, fams[f].cols, fams[f].G, table);
        deliver(f, table, FAMILY_HOST);
        dt->fc_host_units += 1;
    }
}

// (var, parents) lists of the C ABI -> asked families and their distinct canonical forms
void plan_families(const std::vector<int>& card, int n_fam, const int* var, const int* par_off, const int* parents, const char* who,
                   std::vector<AskedFamily>& asked, std::vector<Family>& fams) {
    std::map<std::vector<int>, size_t> seen;
    asked.resize((size_t)n_fam);
    for (int i = 0; i < n_fam; ++i) {
        const int p = par_off[i + 1] - par_off[i];
        if (p < 0 || (p > 0 && !parents)) throw invalid_error(std::string(who) + ": bad parent offsets");
        AskedFamily& a = asked[(size_t)i];
        a.cols.push_back(var[i]);
        for (int j = 0; j < p; ++j) a.cols.push_back(parents[par_off[i] + j]);
        check_family_cols((int)card.size(), a.cols, who);
        a.G = cells_of(card, a.cols, who);
        Family f;
        f.cols = a.cols;
        std::sort(f.cols.begin() + 1, f.cols.end());
        f.G = a.G;
        auto it = seen.find(f.cols);
        if (it == seen.end()) { it = seen.emplace(f.cols, fams.size()).first; fams.push_back(std::move(f)); }
        a.canon = it->second;
    }
}

}  // namespace

extern "C" {

int pbn_dtable_create(pbn_ctx* ctx, int64_t n_rows, int n_cols, const int32_t* const* codes, const int* cardinality, pbn_dtable** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !out || n_cols < 1 || !codes || !cardinality) throw invalid_error("pbn_dtable_create: bad argument");
        if (n_rows < 0 || n_rows > INT32_MAX) throw invalid_error("pbn_dtable_create: row count out of range");
        std::unique_ptr<pbn_dtable> dt(new pbn_dtable);
        dt->ctx = ctx;
        dt->n_rows = n_rows;
        dt->n_cols = n_cols;
        dt->card.assign(cardinality, cardinality + n_cols);
        dt->codes.resize((size_t)n_cols);
        for (int j = 0; j < n_cols; ++j) {
            if (dt->card[j] < 1) throw invalid_error("pbn_dtable_create: a cardinality below 1");
            if (n_rows > 0 && !codes[j]) throw invalid_error("pbn_dtable_create: null column");
            if (n_rows > 0) dt->codes[j].assign(codes[j], codes[j] + n_rows);
            for (int32_t c : dt->codes[j])
                if (c < -1 || c >= dt->card[j]) throw invalid_error("pbn_dtable_create: a code outside [-1, cardinality)");
        }
        if (n_rows > 0) {
            HIP_CHECK(hipSetDevice(ctx->device));
            dt->codes_dev.alloc((size_t)n_cols * n_rows);
            for (int j = 0; j < n_cols; ++j)
                HIP_CHECK(hipMemcpyAsync(dt->codes_dev.p + (size_t)j * n_rows, dt->codes[j].data(), (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice,
                                         ctx->stream));
            if (*std::max_element(dt->card.begin(), dt->card.end()) <= 255 && n_cols <= 65535) {
                dt->ld8 = ceil_div(n_rows, joint::MIRROR_ALIGN) * joint::MIRROR_ALIGN;
                dt->codes8.alloc((size_t)dt->ld8 * n_cols);
                joint::byte_mirror(ctx, dt->codes_dev.p, n_rows, n_cols, dt->codes8.p, dt->ld8);   // -1 & 0xFF = 0xFF: the null byte
            }
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        *out = dt.release();
    });
}

void pbn_dtable_destroy(pbn_dtable* dt) { destroy_handle(dt); }

int pbn_dtable_family_counts(pbn_dtable* dt, int n_fam, const int* var, const int* par_off, const int* parents, int64_t* out_off, int64_t* out_counts,
                             int64_t cap, int* out_form) {
    return guarded(mu_of(dt), [&] {
        if (!dt || n_fam < 0 || !out_off || (n_fam > 0 && (!var || !par_off || !out_counts || !out_form))) throw invalid_error("pbn_dtable_family_counts: bad argument");
        std::vector<AskedFamily> asked;
        std::vector<Family> fams;
        plan_families(dt->card, n_fam, var, par_off, parents, "pbn_dtable_family_counts", asked, fams);
        int64_t total = 0;
        for (int i = 0; i < n_fam; ++i) {
            out_off[i] = total;
            total += asked[(size_t)i].G;
            if (total > cap) throw invalid_error("pbn_dtable_family_counts: the tables need more entries than cap");
        }
        out_off[n_fam] = total;
        dtable_family_counts(dt, asked, fams.size(), fams, [&](size_t i, const int64_t* table, int form) {
            std::memcpy(out_counts + out_off[i], table, (size_t)asked[i].G * sizeof(int64_t));
            out_form[i] = form;
        });
    });
}

int pbn_dnet_create(pbn_ctx* ctx, int n_cols, const int* cardinality, int n_nodes, const int* var, const int* par_off, const int* parents,
                    const int64_t* cpt_off, const double* logprob, pbn_dnet** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !out || n_cols < 1 || !cardinality || n_nodes < 1 || !var || !par_off || !cpt_off || !logprob) throw invalid_error("pbn_dnet_create: bad argument");
        std::unique_ptr<pbn_dnet> dn(new pbn_dnet);
        dn->ctx = ctx;
        dn->n_cols = n_cols;
        dn->card.assign(cardinality, cardinality + n_cols);
        for (int c : dn->card)
            if (c < 1) throw invalid_error("pbn_dnet_create: a cardinality below 1");
        if (cpt_off[0] != 0) throw invalid_error("pbn_dnet_create: the CPT offsets do not start at 0");
        dn->nodes.resize((size_t)n_nodes);
        for (int n = 0; n < n_nodes; ++n) {
            const int p = par_off[n + 1] - par_off[n];
            if (p < 0 || (p > 0 && !parents)) throw invalid_error("pbn_dnet_create: bad parent offsets");
            if (1 + p > FAMILY_MAX_VARS) throw invalid_error("pbn_dnet_create: a node with more than 8 family variables");
            std::vector<int> cols{var[n]};
            for (int j = 0; j < p; ++j) cols.push_back(parents[par_off[n] + j]);
            check_family_cols(n_cols, cols, "pbn_dnet_create");
            const int64_t G = cells_of(dn->card, cols, "pbn_dnet_create");
            if (G > DNET_MAX_CELLS) throw invalid_error("pbn_dnet_create: a family with more than 2^31 - 1 cells");
            if (cpt_off[n + 1] - cpt_off[n] != G) throw invalid_error("pbn_dnet_create: the CPT offsets do not match the families' cells");
            DNode& d = dn->nodes[(size_t)n];
            d = DNode{};
            d.m = 1 + p;
            d.G = (uint32_t)G;
            d.cpt_off = cpt_off[n];
            std::copy(cols.begin(), cols.end(), d.col);
            family_strides(dn->card, cols, d.stride, DNET_MAX_CELLS);   // (the strides alone: G, checked above, is within the cap)
        }
        dn->logprob.assign(logprob, logprob + cpt_off[n_nodes]);
        HIP_CHECK(hipSetDevice(ctx->device));
        dn->nodes_dev.alloc((size_t)n_nodes);
        dn->logprob_dev.alloc(dn->logprob.size());
        HIP_CHECK(hipMemcpyAsync(dn->nodes_dev.p, dn->nodes.data(), (size_t)n_nodes * sizeof(DNode), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(dn->logprob_dev.p, dn->logprob.data(), dn->logprob.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = dn.release();
    });
}

void pbn_dnet_destroy(pbn_dnet* dn) { destroy_handle(dn); }

static void check_same_columns(const pbn_dnet* dn, const pbn_dtable* dt, const char* who) {
    if (dn->ctx.p != dt->ctx.p) throw invalid_error(std::string(who) + ": the network and the table belong to different contexts");
    if (dn->n_cols != dt->n_cols || dn->card != dt->card) throw invalid_error(std::string(who) + ": the table's cardinalities are not the network's");
}

int pbn_dnet_logl(pbn_dnet* dn, const pbn_dtable* dt, double* out) {
    return guarded(mu_of(dn), [&] {
        if (!dn || !dt) throw invalid_error("pbn_dnet_logl: null argument");
        check_same_columns(dn, dt, "pbn_dnet_logl");
        const int64_t n = dt->n_rows;
        if (n == 0) return;
        if (!out) throw invalid_error("pbn_dnet_logl: null output");
        pbn_ctx* ctx = dn->ctx;
        HIP_CHECK(hipSetDevice(ctx->device));
        dn->out_dev.reserve((size_t)n);
        const bool bytes = dt->ld8 > 0;
        const int64_t tile = (int64_t)BLOCK * (bytes ? ROWS_U8 : ROWS_I32);
        const dim3 grid((unsigned)ceil_div(n, tile)), block(BLOCK);
        if (bytes)
            hipLaunchKernelGGL(dnet_logl_kernel<uint8_t>, grid, block, 0, ctx->stream, dn->nodes_dev.p, (int)dn->nodes.size(), dn->logprob_dev.p,
                               (const uint8_t*)dt->codes8.p, dt->ld8, n, dn->out_dev.p);
        else
            hipLaunchKernelGGL(dnet_logl_kernel<int32_t>, grid, block, 0, ctx->stream, dn->nodes_dev.p, (int)dn->nodes.size(), dn->logprob_dev.p,
                               (const int32_t*)dt->codes_dev.p, n, n, dn->out_dev.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(out, dn->out_dev.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        dn->logl_launches += 1;
        dn->rows_evaluated += n;
    });
}

int pbn_dnet_slogl(pbn_dnet* dn, pbn_dtable* dt, double* out_total, double* out_per_node) {
    return guarded(mu_of(dn), [&] {
        if (!dn || !dt) throw invalid_error("pbn_dnet_slogl: null argument");
        check_same_columns(dn, dt, "pbn_dnet_slogl");
        const size_t N = dn->nodes.size();
        std::vector<int> var(N), par_off(N + 1, 0), parents;
        for (size_t n = 0; n < N; ++n) {
            const DNode& d = dn->nodes[n];
            var[n] = d.col[0];
            for (int j = 1; j < d.m; ++j) parents.push_back(d.col[j]);
            par_off[n + 1] = (int)parents.size();
        }
        std::vector<AskedFamily> asked;
        std::vector<Family> fams;
        plan_families(dt->card, (int)N, var.data(), par_off.data(), parents.data(), "pbn_dnet_slogl", asked, fams);
        // per node: count x logprob over the cells in cell order, cells without rows skipped (0 x -inf must not make a NaN)
        std::vector<double> per_node(N, 0.0);
        dtable_family_counts(dt, asked, fams.size(), fams, [&](size_t n, const int64_t* table, int) {
            const double* lp = dn->logprob.data() + dn->nodes[n].cpt_off;
            double s = 0.0;
            for (int64_t c = 0; c < asked[n].G; ++c)
                if (table[c] > 0) s += (double)table[c] * lp[c];
            per_node[n] = s;
        });
        double total = per_node[0];
        for (size_t n = 1; n < N; ++n) total += per_node[n];
        if (out_total) *out_total = total;
        if (out_per_node) std::memcpy(out_per_node, per_node.data(), N * sizeof(double));
    });
}

int pbn_dnet_stats(const pbn_dnet* dn, int64_t* logl_launches, int64_t* rows_evaluated) {
    return handle_stats(dn, "pbn_dnet_stats", &pbn_dnet::logl_launches, &pbn_dnet::rows_evaluated, logl_launches, rows_evaluated);
}

}  // extern "C"
