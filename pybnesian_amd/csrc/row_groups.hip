// Grouping the rows of a table by configuration of discrete columns on the device, for the factors that keep one base factor per
// configuration of their discrete evidence (factors/discrete/DiscreteAdaptator.hpp:201-348 fit / logl / slogl over the indices of
// factors/discrete/discrete_indices.cpp:93-204) - instead of, per configuration, a scan of all rows on the host, an arrow take of the
// whole frame and an upload of the slice.
//
// pbn_rowgroups: the row numbers of a pbn_dtable ordered by configuration - a STABLE partition, the rows of one configuration in
// source order - and the G + 1 offsets of the configurations in that list.  Three launches, no sort and no library:
//   count    at most RG_MAX_BLOCKS workgroups of 256 threads; workgroup b owns the rows [b * chunk, (b + 1) * chunk), chunk a multiple
//            of the row tile (RG_TILE = 256 rows, one a lane).  A lane forms its row's key from the int32 codes as clgnet_logl_kernel
//            does (sum code_j * stride_j in 32 bits, the codes or-ed for the sign of a -1), reads the row's validity bit, and adds 1 to
//            its key's counter in LDS; after the chunk the workgroup writes counts[key][b] for every key below G.
//   scan     ONE workgroup of 1 024 threads scans counts in place, configuration-major and workgroup-minor: counts[key][b] becomes the
//            first slot of workgroup b's rows of that configuration, and offsets[key] = counts[key][0], offsets[G] = the total.
//   scatter  the grid of `count`.  A workgroup loads its row of the scanned counts into LDS as running counters and walks its chunk
//            again in row order: tile after tile, and inside a tile wave after wave (the four waves take turns between barriers).  A
//            wave loops over its distinct keys: the first pending lane's key is broadcast, a ballot marks the lanes that hold it, such a
//            lane's slot is the key's counter plus the number of marked lanes below it, and the first lane then advances the counter by
//            the number of marked lanes.  LDS operations of one wave complete in program order, so the lanes' reads of the counter
//            come before that write.  The lane writes its row number at its slot with an ordinary (vector) store.
// The integer atomics of `count` commute, the scan and the scatter have one order each: the list is THE stable order whatever the
// hardware did, and two calls give the same bytes.
//
// PBN_ROWGROUPS_MAX_CONFIGS = 8 192: one 32-bit counter a configuration in a workgroup's LDS is 32 KiB, which lets five workgroups (20
// of the 32 waves a CU holds) share a CU's 160 KiB, and keeps counts (G x workgroups x 4 bytes) at 8 MiB at the most.  A 64 KiB array
// (16 384) would leave two workgroups a CU for configuration counts no factor here comes near: a base factor per configuration needs
// rows of its own, and 8 192 configurations of even 100 rows are most of a million-row table.
//
// pbn_table_take_group gathers one configuration's rows of selected columns into a NEW owned table with pbn_table_take's allocation and
// launch_take, reading the row list where it lies on the device.
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "discrete_model.hpp"
#include "net_eval.hpp"
#include "stats_kernels.hpp"

using namespace pbn;

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_TILE = RG_BLOCK;             // rows of a workgroup's step: one a lane
constexpr int RG_WAVES = RG_BLOCK / 64;
constexpr int RG_MAX_BLOCKS = 256;
constexpr int RG_MAX_KEY_COLS = 7;            // the adaptator's discrete parents (clg_model.hip: CLG_MAX_DISCRETE_PARENTS)
constexpr int RG_SCAN_THREADS = 1024;
constexpr uint32_t RG_NO_KEY = 0xFFFFFFFFu;   // a row in no group
constexpr int64_t RG_MAX_CONFIGS = PBN_ROWGROUPS_MAX_CONFIGS;

static_assert(RG_MAX_CONFIGS * 4 <= 64 * 1024, "the counters of a workgroup are static LDS");

struct RgKey {
    int m;
    uint32_t G;
    int col[RG_MAX_KEY_COLS];
    uint32_t stride[RG_MAX_KEY_COLS];
};

// the key of row r (r < n_rows), RG_NO_KEY when a code is -1, the validity bit is 0 or the key is no configuration
__device__ __forceinline__ uint32_t rg_key(const RgKey& k, const int32_t* __restrict__ codes, const uint8_t* __restrict__ valid, int64_t n_rows,
                                           uint32_t r) {
    uint32_t key = 0u;
    int32_t any = 0;
    for (int j = 0; j < k.m; ++j) {
        const int32_t code = codes[(int64_t)k.col[j] * n_rows + r];
        key += (uint32_t)code * k.stride[j];
        any |= code;
    }
    bool ok = (any >= 0) & (key < k.G);
    if (valid) ok = ok & (((valid[r >> 3] >> (r & 7u)) & 1u) != 0u);
    return ok ? key : RG_NO_KEY;
}

// counts: [G][gridDim.x]
__global__ __launch_bounds__(RG_BLOCK) void rg_count_kernel(RgKey k, const int32_t* __restrict__ codes, const uint8_t* __restrict__ valid,
                                                            int64_t n_rows, uint32_t chunk, uint32_t* __restrict__ counts) {
    __shared__ uint32_t cnt[RG_MAX_CONFIGS];
    const uint32_t t = threadIdx.x, G = k.G;
    for (uint32_t c = t; c < G; c += RG_BLOCK) cnt[c] = 0u;
    __syncthreads();
    const uint32_t n32 = (uint32_t)n_rows, lo = blockIdx.x * chunk, hi = min(lo + chunk, n32);   // (lo < n32: the grid covers no more)
    for (uint32_t r = lo + t; r < hi; r += RG_TILE) {
        const uint32_t key = rg_key(k, codes, valid, n_rows, r);
        if (key != RG_NO_KEY) atomicAdd(&cnt[key], 1u);
    }
    __syncthreads();
    for (uint32_t c = t; c < G; c += RG_BLOCK) counts[(size_t)c * gridDim.x + blockIdx.x] = cnt[c];
}

// Exclusive scan of v[0 .. len) in place, one workgroup: a thread owns `seg` consecutive entries.  offsets[c] = v[c * nb] after the scan
// (c < G), offsets[G] = the total.
__global__ __launch_bounds__(RG_SCAN_THREADS) void rg_scan_kernel(uint32_t* __restrict__ v, uint32_t len, uint32_t seg, uint32_t G, uint32_t nb,
                                                                  uint32_t* __restrict__ offsets) {
    __shared__ uint32_t part[RG_SCAN_THREADS];
    const uint32_t t = threadIdx.x;
    const uint32_t lo = min(t * seg, len), hi = min(lo + seg, len);
    uint32_t s = 0u;
    for (uint32_t i = lo; i < hi; ++i) s += v[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0u;
        for (int i = 0; i < RG_SCAN_THREADS; ++i) {
            const uint32_t x = part[i];
            part[i] = run;
            run += x;
        }
        offsets[G] = run;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t x = v[i];
        v[i] = run;
        run += x;
    }
    __syncthreads();   // (one workgroup: the stores above are visible to its threads behind the barrier)
    for (uint32_t c = t; c < G; c += RG_SCAN_THREADS) offsets[c] = v[(size_t)c * nb];
}

// starts: the scanned counts [G][gridDim.x]; rows_out: as many entries as offsets[G]
__global__ __launch_bounds__(RG_BLOCK) void rg_scatter_kernel(RgKey k, const int32_t* __restrict__ codes, const uint8_t* __restrict__ valid,
                                                              int64_t n_rows, uint32_t chunk, const uint32_t* __restrict__ starts,
                                                              int32_t* __restrict__ rows_out) {
    __shared__ uint32_t run[RG_MAX_CONFIGS];
    const uint32_t t = threadIdx.x, G = k.G;
    for (uint32_t c = t; c < G; c += RG_BLOCK) run[c] = starts[(size_t)c * gridDim.x + blockIdx.x];
    __syncthreads();
    const uint32_t n32 = (uint32_t)n_rows, lo = blockIdx.x * chunk, hi = min(lo + chunk, n32);
    const int wave = (int)(t >> 6);
    const unsigned long long below = (1ull << (t & 63u)) - 1ull;   // the lanes of the wave before this one
    for (uint32_t base = lo; base < hi; base += RG_TILE) {          // the same trip count for every thread: barriers inside
        const uint32_t r = base + t;
        const uint32_t key = r < hi ? rg_key(k, codes, valid, n_rows, r) : RG_NO_KEY;
        for (int w = 0; w < RG_WAVES; ++w) {
            if (wave == w) {
                unsigned long long todo = __ballot(key != RG_NO_KEY);
                while (todo) {   // wave-uniform: todo is a ballot
                    const int first = __ffsll((long long)todo) - 1;
                    const uint32_t kf = (uint32_t)__shfl((int)key, first);
                    const bool mine = key == kf;   // (kf is a configuration, never RG_NO_KEY)
                    const unsigned long long same = __ballot(mine);
                    if (mine) rows_out[run[kf] + (uint32_t)__popcll(same & below)] = (int32_t)r;
                    if ((int)(t & 63u) == first) run[kf] += (uint32_t)__popcll(same);
                    todo &= ~same;
                }
            }
            __syncthreads();
        }
    }
}

}  // namespace

struct pbn_rowgroups {
    pbn::ctx_ptr ctx;
    int64_t n_rows = 0;              // of the table that was grouped: the rows a gather may address
    std::vector<int64_t> offsets;    // G + 1
    pbn::dev_buf<int32_t> rows_dev;  // offsets[G] source rows, grouped order
};

extern "C" {

int pbn_dtable_group_rows(const pbn_dtable* dt, int m, const int* cols, const unsigned char* valid_bitmap, pbn_rowgroups** out) {
    return guarded(mu_of(dt), [&] {
        const char* who = "pbn_dtable_group_rows";
        if (!dt || !cols || !out) throw invalid_error(std::string(who) + ": null argument");
        if (m < 1 || m > RG_MAX_KEY_COLS) throw invalid_error(std::string(who) + ": between 1 and 7 key columns are supported");
        const std::vector<int> keys(cols, cols + m);
        check_family_cols(dt->n_cols, keys, who);
        RgKey k{};
        k.m = m;
        std::copy(keys.begin(), keys.end(), k.col);
        const int64_t G = family_strides(dt->card, keys, k.stride, RG_MAX_CONFIGS);
        if (G > RG_MAX_CONFIGS) throw invalid_error(std::string(who) + ": more than PBN_ROWGROUPS_MAX_CONFIGS configurations");
        k.G = (uint32_t)G;
        pbn_ctx* ctx = dt->ctx;
        std::unique_ptr<pbn_rowgroups> g(new pbn_rowgroups);
        g->ctx = ctx;
        g->n_rows = dt->n_rows;
        g->offsets.assign((size_t)G + 1, 0);
        const int64_t n = dt->n_rows;   // at most 2^31 - 1: pbn_dtable_create
        if (n > 0) {
            HIP_CHECK(hipSetDevice(ctx->device));
            hipStream_t st = ctx->stream;
            int nb = (int)std::min<int64_t>(RG_MAX_BLOCKS, ceil_div(n, RG_TILE));
            const int64_t chunk = ceil_div(ceil_div(n, nb), RG_TILE) * RG_TILE;
            nb = (int)ceil_div(n, chunk);
            const size_t len = (size_t)G * nb;   // at most 2^21
            dev_buf<uint32_t> counts(len), offsets_dev((size_t)G + 1);
            dev_buf<uint8_t> valid_dev;
            g->rows_dev.alloc((size_t)n);
            if (valid_bitmap) {
                valid_dev.alloc((size_t)ceil_div(n, 8));
                HIP_CHECK(hipMemcpyAsync(valid_dev.p, valid_bitmap, (size_t)ceil_div(n, 8), hipMemcpyHostToDevice, st));
            }
            hipLaunchKernelGGL(rg_count_kernel, dim3((unsigned)nb), dim3(RG_BLOCK), 0, st, k, dt->codes_dev.p, valid_dev.p, n, (uint32_t)chunk, counts.p);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(rg_scan_kernel, dim3(1), dim3(RG_SCAN_THREADS), 0, st, counts.p, (uint32_t)len, (uint32_t)ceil_div((int64_t)len, RG_SCAN_THREADS),
                               (uint32_t)G, (uint32_t)nb, offsets_dev.p);
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(rg_scatter_kernel, dim3((unsigned)nb), dim3(RG_BLOCK), 0, st, k, dt->codes_dev.p, valid_dev.p, n, (uint32_t)chunk, counts.p,
                               g->rows_dev.p);
            HIP_CHECK(hipGetLastError());
            std::vector<uint32_t> off((size_t)G + 1);
            HIP_CHECK(hipMemcpyAsync(off.data(), offsets_dev.p, off.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));   // (the bitmap's host buffer and the scratch are free to go)
            for (size_t c = 0; c <= (size_t)G; ++c) g->offsets[c] = off[c];
        }
        *out = g.release();
    });
}

int pbn_rowgroups_offsets(const pbn_rowgroups* g, int64_t* n_configs, int64_t* offsets) {
    return guarded(mu_of(g), [&] {
        if (!g || !n_configs) throw invalid_error("pbn_rowgroups_offsets: null argument");
        *n_configs = (int64_t)g->offsets.size() - 1;
        if (offsets) std::copy(g->offsets.begin(), g->offsets.end(), offsets);
    });
}

int pbn_rowgroups_rows(const pbn_rowgroups* g, int32_t* rows) {
    return guarded(mu_of(g), [&] {
        if (!g) throw invalid_error("pbn_rowgroups_rows: null argument");
        const int64_t total = g->offsets.back();
        if (total == 0) return;
        if (!rows) throw invalid_error("pbn_rowgroups_rows: null argument");
        HIP_CHECK(hipSetDevice(g->ctx->device));
        HIP_CHECK(hipMemcpyAsync(rows, g->rows_dev.p, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, g->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
    });
}

int pbn_table_take_group(const pbn_table* t, const int* cols, int n_cols, const pbn_rowgroups* g, int64_t c, pbn_table** out) {
    return guarded(mu_of(t), [&] {
        const char* who = "pbn_table_take_group";
        if (!t || !g || !out || !cols) throw invalid_error(std::string(who) + ": null argument");
        if (t->ctx.p != g->ctx.p) throw invalid_error(std::string(who) + ": the table and the groups belong to different contexts");
        if (t->n_rows != g->n_rows) throw invalid_error(std::string(who) + ": the table has other rows than the grouped one");
        if (n_cols < 1) throw invalid_error(std::string(who) + ": no column");
        for (int j = 0; j < n_cols; ++j)
            if (cols[j] < 0 || cols[j] >= t->n_cols) throw invalid_error(std::string(who) + ": column out of range");
        if (c < 0 || c >= (int64_t)g->offsets.size() - 1) throw invalid_error(std::string(who) + ": configuration out of range");
        const int64_t first = g->offsets[(size_t)c], n = g->offsets[(size_t)c + 1] - first;
        pbn_ctx* ctx = t->ctx;
        HIP_CHECK(hipSetDevice(ctx->device));
        // pbn_table_take's allocation: the table is what an upload of these rows and columns gives
        auto o = std::make_unique<pbn_table>();
        o->ctx = ctx; o->dtype = t->dtype; o->n_cols = n_cols; o->n_rows = n;
        o->ld = std::max<int64_t>(64, (n + 63) / 64 * 64);
        o->owns = true;
        const size_t es = dtype_size(t->dtype);
        void* data = nullptr;
        HIP_CHECK(hipMalloc(&data, (size_t)o->ld * n_cols * es));
        o->data = data;
        try {
            // one column a launch: the columns asked for lie anywhere in the source.  Everything is in stream order with what reads the
            // table next (pbn_table_read and the destroy calls wait for the stream).
            for (int j = 0; j < n_cols; ++j)
                launch_take(t->col(cols[j]), 0, (char*)o->data + (size_t)j * o->ld * es, 0, g->rows_dev.p + first, n, 1, t->dtype, ctx->stream);
        } catch (...) {
            (void)hipFree(data);
            throw;
        }
        *out = o.release();
    });
}

void pbn_rowgroups_destroy(pbn_rowgroups* g) {
    if (!g) return;
    ctx_pin pin(g->ctx);
    std::lock_guard<std::recursive_mutex> lock(mu_of(g));
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);   // gathers that read the row list may still be in flight
    delete g;
}

}  // extern "C"
