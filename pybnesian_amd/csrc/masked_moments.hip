// Masked moments: pilot-shifted (N, S, G) of small column sets over the rows that are valid in ALL of the set's columns - the
// statistics BIC / BGe need on tables with nulls (learning/scores/bic.cpp:12-64 work on valid_rows of the candidate's columns;
// dataset.cpp:208-235 combined_bitmap) - for a whole batch of sets in one device pass.
//
// A UNIT is an ordered list of d <= 8 continuous columns, optionally with a device row list cut into segments (the cells of a hybrid
// grouping); without a list its rows are [0, rows) as one segment.  For every (unit, segment) the pass returns N (exact), S[d] and the
// upper triangle of G[d][d] of x - shift_c, accumulated in fp64 for fp32 and fp64 tables alike, exactly as Stats holds them.
//
// Validity lives on the device once per score data (pbn_scoredata_set_validity): ceil(n / 64) 64-bit words per row, bit c set when column
// c is valid in that row.  A unit carries, per validity word it touches, the mask of its columns' bits; a row counts when
// (word & mask) == mask for each of them.  The value under a null slot is never used: the lanes SELECT 0 for the whole row of a unit
// when the row does not count, so whatever the table holds there (zeros as the package uploads them, NaN from another caller) stays out.
//
// Summation order.  A segment of L rows is cut into ceil(L / SLICE_ROWS) slices - a function of L alone.  One workgroup takes one slice of
// one (unit, segment): lane t adds rows t, t + 256, ... of the slice into 1 + d + d (d + 1) / 2 register accumulators, a fixed butterfly
// adds the lanes of a wave, the four waves are added in wave order: the slice's partial.  A second kernel adds a (unit, segment)'s
// partials in slice order.  No floating-point atomics, nothing that depends on the grid, on the number of CUs or on what else the call
// holds: a unit's numbers are a function of the table, the validity words, the shifts and the unit alone.
//
// The plain form: every unit reads its own columns and the validity words through L2 (DESIGN.md 3.14 on why no LDS staging).
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#include "common.hpp"
#include "scoring_internal.hpp"

namespace pbn {
namespace score {

namespace {

constexpr int BLOCK = 256;
constexpr int64_t SLICE_ROWS = 16384;            // rows of a slice: part of the summation order, never tuned per call
constexpr int64_t CHUNK_DOUBLES = 1ll << 23;     // partials of one launch: 64 MB

struct Desc {
    int cols[MASKED_MAX_COLS];
    double shift[MASKED_MAX_COLS];
    int n_words;                       // validity words the unit's columns touch
    int word[MASKED_MAX_COLS];         // their indices within a row's words
    uint64_t mask[MASKED_MAX_COLS];    // the unit's bits in each
    const int32_t* rows;               // device row list, or null: the segment is rows [r0, r1) of the table
    int64_t r0, r1;                    // the segment: positions in the list (or table rows)
    int64_t slot0;                     // its first partial in the launch
    int slices;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// grid = the launch's (unit, segment, slice) triples, one workgroup each; owner[block] = descriptor.  W = 1 + D + D (D + 1) / 2 doubles per
// partial: N first (a count <= SLICE_ROWS, exact in a double), then S, then the upper triangle of G row by row.
template <typename T, int D>
__global__ __launch_bounds__(BLOCK) void masked_moments_kernel(const Desc* __restrict__ descs, const int32_t* __restrict__ owner, const void* __restrict__ base,
                                                                int64_t ld, const uint64_t* __restrict__ valid, int nw, double* __restrict__ partial) {
    constexpr int S = D + D * (D + 1) / 2;
    constexpr int W = S + 1;
    __shared__ double red[4][W];
    const Desc& de = descs[owner[blockIdx.x]];
    const int64_t slice = (int64_t)blockIdx.x - de.slot0;
    const int64_t s0 = de.r0 + slice * SLICE_ROWS;
    const int64_t s1 = s0 + SLICE_ROWS < de.r1 ? s0 + SLICE_ROWS : de.r1;
    const int32_t* __restrict__ rows = de.rows;
    const int n_words = de.n_words;
    const T* col[D];
    double shift[D];
#pragma unroll
    for (int i = 0; i < D; ++i) { col[i] = (const T*)base + (int64_t)de.cols[i] * ld; shift[i] = de.shift[i]; }
    double acc[S];
#pragma unroll
    for (int i = 0; i < S; ++i) acc[i] = 0.0;
    uint32_t count = 0u;
    for (int64_t r = s0 + (int64_t)threadIdx.x; r < s1; r += BLOCK) {
        const int64_t row = rows ? (int64_t)rows[r] : r;
        bool ok = true;
        for (int k = 0; k < n_words; ++k) {
            const uint64_t m = de.mask[k];
            ok = ok && (valid[row * nw + de.word[k]] & m) == m;
        }
        double x[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double v = (double)col[i][row] - shift[i];
            x[i] = ok ? v : 0.0;   // a select: a row that does not count adds +0.0 to every sum, whatever its slots hold
        }
        count += ok ? 1u : 0u;
        int pos = D;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            acc[i] += x[i];
#pragma unroll
            for (int j = i; j < D; ++j) { acc[pos] = __builtin_fma(x[i], x[j], acc[pos]); ++pos; }
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    {
        uint32_t c = count;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
        if (lane == 0) red[wave][0] = (double)c;
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) red[wave][1 + i] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < W)
        partial[(size_t)blockIdx.x * W + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// one thread per (descriptor, entry): the slices of a (unit, segment) in slice order; a segment without rows gives zeros
__global__ __launch_bounds__(BLOCK) void masked_reduce_kernel(const Desc* __restrict__ descs, int n_desc, int W, const double* __restrict__ partial,
                                                               double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (int64_t)n_desc * W) return;
    const int d = (int)(i / W), e = (int)(i - (int64_t)d * W);
    const double* p = partial + (size_t)descs[d].slot0 * W + e;
    const int slices = descs[d].slices;
    double v = 0.0;
    for (int s = 0; s < slices; ++s) v += p[(size_t)s * W];
    out[i] = v;
}

template <typename T>
void launch_masked(int d, int blocks, const Desc* descs, const int32_t* owner, const pbn_table* t, const uint64_t* valid, int nw, double* partial,
                   hipStream_t st) {
    const dim3 grid((unsigned)blocks), block(BLOCK);
#define PBN_MM_CASE(D) case D: hipLaunchKernelGGL((masked_moments_kernel<T, D>), grid, block, 0, st, descs, owner, t->data, t->ld, valid, nw, partial); break;
    switch (d) {
        PBN_MM_CASE(1) PBN_MM_CASE(2) PBN_MM_CASE(3) PBN_MM_CASE(4) PBN_MM_CASE(5) PBN_MM_CASE(6) PBN_MM_CASE(7) PBN_MM_CASE(8)
        default: throw invalid_error("masked moments: between 1 and 8 columns per unit");
    }
#undef PBN_MM_CASE
    HIP_CHECK(hipGetLastError());
}

}  // namespace

bool masked_moments_on() { return knob_int("PBN_NULL_MOMENTS", 1) != 0; }   // (per call: the tests switch it)

// Bits of the validity words from the byte masks of pbn_scoredata_set_validity (permuted row order = source order: split NONE only).
void masked_validity_upload(pbn_scoredata* sd) {
    sd->valid_words.release();
    sd->valid_nw = 0;
    if (!sd->has_nulls) return;
    const int64_t rows = (int64_t)sd->perm.size();
    const int nw = (sd->n + 63) / 64;
    std::vector<uint64_t> w((size_t)rows * nw, ~0ull);
    for (int c = 0; c < sd->n; ++c) {
        if (sd->valid[c].empty()) continue;
        const uint8_t* m = sd->valid[c].data();
        const uint64_t bit = 1ull << (c & 63);
        uint64_t* p = w.data() + (c >> 6);
        for (int64_t r = 0; r < rows; ++r)
            if (!m[r]) p[(size_t)r * nw] &= ~bit;
    }
    HIP_CHECK(hipSetDevice(sd->ctx->device));
    sd->valid_words.alloc(w.size());
    HIP_CHECK(hipMemcpyAsync(sd->valid_words.p, w.data(), w.size() * sizeof(uint64_t), hipMemcpyHostToDevice, sd->ctx->stream));
    HIP_CHECK(hipStreamSynchronize(sd->ctx->stream));
    sd->valid_nw = nw;
}

void masked_moments(pbn_scoredata* sd, const std::vector<MaskedUnit>& units, std::vector<std::vector<MaskedMoments>>& out) {
    out.assign(units.size(), {});
    if (units.empty()) return;
    if (!sd->valid_words.p) throw invalid_error("masked moments: the score data holds no validity words (pbn_scoredata_set_validity)");
    const pbn_table* t = sd->table();
    pbn_ctx* ctx = sd->ctx;
    const int nw = sd->valid_nw;
    const int64_t rows = t->n_rows;
    HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    // the (unit, segment) descriptors, by the unit's width: one kernel instantiation and one partial width per launch
    struct Item { size_t unit; int seg; Desc d; };
    std::vector<Item> by_d[MASKED_MAX_COLS + 1];
    for (size_t u = 0; u < units.size(); ++u) {
        const MaskedUnit& mu = units[u];
        const int d = (int)mu.cols.size();
        if (d < 1 || d > MASKED_MAX_COLS) throw invalid_error("masked moments: between 1 and 8 columns per unit");
        Desc base{};
        for (int i = 0; i < d; ++i) {
            const int c = mu.cols[i];
            if (c < 0 || c >= sd->n) throw invalid_error("masked moments: column out of range");
            base.cols[i] = c;
            base.shift[i] = sd->shift[c];
            int k = 0;
            while (k < base.n_words && base.word[k] != (c >> 6)) ++k;
            if (k == base.n_words) { base.word[k] = c >> 6; base.mask[k] = 0; ++base.n_words; }
            base.mask[k] |= 1ull << (c & 63);
        }
        base.rows = mu.rows;
        const int nseg = mu.rows ? (int)mu.seg_off.size() - 1 : 1;
        if (nseg < 0) throw invalid_error("masked moments: a row list needs segment offsets");
        out[u].assign((size_t)nseg, MaskedMoments{});
        for (int s = 0; s < nseg; ++s) {
            Item it{u, s, base};
            it.d.r0 = mu.rows ? mu.seg_off[s] : 0;
            it.d.r1 = mu.rows ? mu.seg_off[s + 1] : rows;
            if (it.d.r0 < 0 || it.d.r1 < it.d.r0 || (mu.rows ? it.d.r1 > mu.n_list : it.d.r1 > rows)) throw invalid_error("masked moments: segment out of range");
            it.d.slices = (int)ceil_div(it.d.r1 - it.d.r0, SLICE_ROWS);
            by_d[d].push_back(it);
        }
    }
    std::vector<Desc> descs;
    std::vector<int32_t> owner;
    std::vector<double> host;
    for (int d = 1; d <= MASKED_MAX_COLS; ++d) {
        const std::vector<Item>& items = by_d[d];
        const int W = 1 + d + d * (d + 1) / 2;
        for (size_t base = 0; base < items.size();) {
            // a chunk: as many descriptors as keep the partials within the budget (one always fits: <= 2^31 / 16384 slices of 46 doubles)
            size_t end = base;
            int64_t slots = 0;
            descs.clear(); owner.clear();
            while (end < items.size() && (end == base || (slots + items[end].d.slices) * W <= CHUNK_DOUBLES)) {
                Desc de = items[end].d;
                de.slot0 = slots;
                for (int s = 0; s < de.slices; ++s) owner.push_back((int32_t)(end - base));
                slots += de.slices;
                descs.push_back(de);
                ++end;
            }
            const size_t nd = end - base;
            sd->mm_descs.reserve(nd * sizeof(Desc));
            sd->mm_owner.reserve(std::max<size_t>(1, owner.size()));
            sd->mm_partial.reserve((size_t)std::max<int64_t>(1, slots) * W + nd * W);
            Desc* dd = reinterpret_cast<Desc*>(sd->mm_descs.p);
            double* partial = sd->mm_partial.p;
            double* outd = partial + (size_t)std::max<int64_t>(1, slots) * W;
            HIP_CHECK(hipMemcpyAsync(dd, descs.data(), nd * sizeof(Desc), hipMemcpyHostToDevice, st));
            if (slots > 0) {
                HIP_CHECK(hipMemcpyAsync(sd->mm_owner.p, owner.data(), owner.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
                KernelTimer kt(ctx, PBN_K_GRAM);
                if (t->dtype == PBN_F64) launch_masked<double>(d, (int)slots, dd, sd->mm_owner.p, t, sd->valid_words.p, nw, partial, st);
                else launch_masked<float>(d, (int)slots, dd, sd->mm_owner.p, t, sd->valid_words.p, nw, partial, st);
            }
            hipLaunchKernelGGL(masked_reduce_kernel, dim3((unsigned)ceil_div((int64_t)nd * W, BLOCK)), dim3(BLOCK), 0, st, dd, (int)nd, W, partial, outd);
            HIP_CHECK(hipGetLastError());
            host.resize(nd * W);
            HIP_CHECK(hipMemcpyAsync(host.data(), outd, host.size() * sizeof(double), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));   // (descs / owner are read by then as well)
            for (size_t i = 0; i < nd; ++i) {
                const Item& it = items[base + i];
                const double* w = host.data() + i * W;
                MaskedMoments& m = out[it.unit][(size_t)it.seg];
                m.N = (int64_t)w[0];
                std::memcpy(m.S, w + 1, d * sizeof(double));
                std::memcpy(m.G, w + 1 + d, (size_t)(d * (d + 1) / 2) * sizeof(double));
            }
            ++sd->mm_launches;
            sd->mm_units += (int64_t)nd;
            base = end;
        }
    }
}

// (N, S, G of the unit's columns) -> Stats over ALL n columns with the unit's entries filled in, as the consumers of sd->all read them
void masked_to_stats(const pbn_scoredata* sd, const int* cols, int d, const MaskedMoments& m, Stats& st) {
    const int n = sd->n;
    st.zero(n);
    st.N = m.N;
    int pos = 0;
    for (int i = 0; i < d; ++i) {
        st.S[cols[i]] = m.S[i];
        for (int j = i; j < d; ++j, ++pos) {
            st.G[cols[i] + (size_t)cols[j] * n] = m.G[pos];
            st.G[cols[j] + (size_t)cols[i] * n] = m.G[pos];
        }
    }
}

}  // namespace score
}  // namespace pbn

using namespace pbn;
using namespace pbn::score;

extern "C" {

// pbn_debug_masked_moments (test aid, not part of the C ABI header): the masked pass for units given by the caller on a score handle that
// holds validity words.  Unit u = columns cols[col_off[u] .. col_off[u + 1]) (1 ... 8, in this order).  list_off == NULL: every unit is the
// plain form, one segment of all rows.  Otherwise unit u's row list is rows[list_off[u] .. list_off[u + 1]) (table row ids, any order, repeats
// allowed), cut into the segments seg_off[seg_ptr[u] .. seg_ptr[u + 1]) - offsets into the unit's own list, the first 0, the last its length;
// a unit with an empty offset range (seg_ptr[u] == seg_ptr[u + 1]) is the plain form.  Outputs per (unit, segment), units in order,
// segments in order: out_N[k], out_S[8 k ..], out_G[36 k ..] (upper triangle row by row: (0,0) (0,1) ... (0,d-1) (1,1) ...), for at most
// `cap` pairs; out_shift[j] = the shift of column cols[j].
int pbn_debug_masked_moments(pbn_scoredata* sd, int n_units, const int* col_off, const int* cols, const int64_t* list_off, const int32_t* rows,
                             const int* seg_ptr, const int64_t* seg_off, int64_t cap, int64_t* out_N, double* out_S, double* out_G, double* out_shift) {
    return guarded(mu_of(sd), [&] {
        if (!sd || n_units < 0 || (n_units > 0 && (!col_off || !cols || !out_N || !out_S || !out_G))) throw invalid_error("pbn_debug_masked_moments: bad argument");
        if (sd->discrete_only) throw invalid_error("pbn_debug_masked_moments: discrete-only score data has no continuous columns");
        if (list_off && (!rows || !seg_ptr || !seg_off)) throw invalid_error("pbn_debug_masked_moments: a row list needs rows, seg_ptr and seg_off");
        const int64_t n_rows = sd->table()->n_rows;
        std::vector<MaskedUnit> units((size_t)n_units);
        dev_buf<int32_t> drows;
        if (list_off && n_units > 0) {
            const int64_t total = list_off[n_units];
            if (list_off[0] != 0 || total < 0) throw invalid_error("pbn_debug_masked_moments: bad list offsets");
            for (int64_t i = 0; i < total; ++i)
                if (rows[i] < 0 || rows[i] >= n_rows) throw invalid_error("pbn_debug_masked_moments: row out of range");
            drows.alloc((size_t)total + 1);
            if (total > 0) HIP_CHECK(hipMemcpyAsync(drows.p, rows, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, sd->ctx->stream));
        }
        int64_t pairs = 0;
        for (int u = 0; u < n_units; ++u) {
            if (col_off[u + 1] < col_off[u]) throw invalid_error("pbn_debug_masked_moments: bad column offsets");
            units[u].cols.assign(cols + col_off[u], cols + col_off[u + 1]);
            if (list_off && seg_ptr[u + 1] > seg_ptr[u]) {
                const int64_t len = list_off[u + 1] - list_off[u];
                if (len < 0) throw invalid_error("pbn_debug_masked_moments: bad list offsets");
                units[u].rows = drows.p + list_off[u];
                units[u].n_list = len;
                units[u].seg_off.assign(seg_off + seg_ptr[u], seg_off + seg_ptr[u + 1]);
                if (units[u].seg_off.front() != 0 || units[u].seg_off.back() != len) throw invalid_error("pbn_debug_masked_moments: segment offsets must span the unit's list");
                pairs += (int64_t)units[u].seg_off.size() - 1;
            } else {
                pairs += 1;
            }
        }
        if (pairs > cap) throw invalid_error("pbn_debug_masked_moments: more (unit, segment) pairs than cap");
        std::vector<std::vector<MaskedMoments>> res;
        masked_moments(sd, units, res);
        HIP_CHECK(hipStreamSynchronize(sd->ctx->stream));   // drows goes out of scope
        int64_t k = 0;
        for (int u = 0; u < n_units; ++u)
            for (const MaskedMoments& m : res[u]) {
                out_N[k] = m.N;
                std::memcpy(out_S + 8 * k, m.S, sizeof(m.S));
                std::memcpy(out_G + 36 * k, m.G, sizeof(m.G));
                ++k;
            }
        if (out_shift)
            for (int j = 0; j < col_off[n_units]; ++j) out_shift[j] = sd->shift[cols[j]];
    });
}

}  // extern "C"
