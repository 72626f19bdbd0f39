// The joint-count kernel (joint_counts.hpp): one workgroup counts one (unit, row slice).  Every lane forms the keys of its
// rows from the unit's code columns and adds 1 into the unit's table; no sort, no permutation, one launch per chunk of units and form.
//
// LDS form (tables that fit LDS_WORDS): the adds go to a table in LDS, which the workgroup then adds into the unit's table in global
// memory.  LDS atomics on one address serialise: a 2 x 2 table takes the 64 lanes of a wave to 4 addresses, a constant column to 1.  The
// table is therefore replicated R times (copies_for): a lane adds into copy (lane mod R), and the copies are staggered by one bank, so
// that the lanes of a 32-lane group that meet in one cell are spread over R banks.  Global form (larger tables): every lane adds straight
// into the unit's zeroed table in global memory - at these sizes the rows of a wave spread over many cells, and one slice of a 2^20-cell
// table would otherwise flush 4 MB.  All sums are integer: no order of adds can change a count.
//
// Codes come from a byte mirror (8 consecutive rows of a column per 8-byte load) or from the int32 codes (4 coalesced loads 256 rows
// apart; their columns are ld elements apart, which aligns nothing wider).  Units start on any row: a byte-form slice starts on the
// multiple of 8 at or below row0 and masks the rows outside [row0, row1) - the loads stay aligned and never leave the mirror's padded
// column.  The row bounds are tested by themselves, never through a code's value: the byte that pads a mirror, 0xFF, is a valid code of a
// 256-category column.
#include "joint_counts.hpp"

namespace pbn {
namespace joint {

namespace {

// grid = (units, slices).  LDS = true: cells[] holds the workgroup's copies; false: the lanes add into the unit's table in global memory.
// POLICY is compile-time: NONE loads no cardinality and tests no code.
template <typename CodeT, bool LDS, Policy POLICY>
__global__ __launch_bounds__(BLOCK) void joint_count_kernel(const Desc* __restrict__ descs, const CodeT* __restrict__ codes, int64_t ld,
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
    // bit i of `drop` = row i of the lane's step is not counted: it lies outside [row0, s1) - tested by row number, never through a code's
    // value - or, BY_CARD, one of its codes failed.  Without a test per code a key is checked against G before it is used as an address.
    auto counted = [&](uint32_t key, uint32_t drop, int i) { return !((drop >> i) & 1u) && (POLICY == BY_CARD || key < G); };
    if constexpr (sizeof(CodeT) == 1) {
        constexpr int V = ROWS_PER_LANE_U8;
        for (int64_t r = s0 + (int64_t)tid * V; r < s1; r += (int64_t)BLOCK * V) {   // r is a multiple of 8 below ld: r + 7 < ld
            uint32_t key[V];
            uint32_t drop = (r < row0 ? (1u << (int)(row0 - r < V ? row0 - r : V)) - 1u : 0u) | (s1 - r < V ? ~0u << (int)(s1 - r) : 0u);
#pragma unroll
            for (int i = 0; i < V; ++i) key[i] = 0u;
            for (int j = 0; j < m; ++j) {
                const uint2 v = *reinterpret_cast<const uint2*>(codes + (int64_t)d.col[j] * ld + r);
                const uint32_t stride = (uint32_t)d.stride[j];
                [[maybe_unused]] uint32_t card = 0u;
                if constexpr (POLICY == BY_CARD) card = (uint32_t)d.card[j];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t code = ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xFFu;
                    key[i] += code * stride;
                    if constexpr (POLICY == BY_CARD) drop |= (code >= card ? 1u : 0u) << i;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (counted(key[i], drop, i)) atomicAdd(mine + key[i], 1u);
        }
    } else {
        constexpr int V = ROWS_PER_LANE_I32;
        for (int64_t r = (s0 < row0 ? row0 : s0) + tid; r < s1; r += (int64_t)BLOCK * V) {
            uint32_t key[V];
            uint32_t drop = 0u;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                key[i] = 0u;
                drop |= (r + (int64_t)i * BLOCK < s1 ? 0u : 1u) << i;
            }
            for (int j = 0; j < m; ++j) {
                const CodeT* col = codes + (int64_t)d.col[j] * ld + r;
                const uint32_t stride = (uint32_t)d.stride[j];
                [[maybe_unused]] uint32_t card = 0u;
                if constexpr (POLICY == BY_CARD) card = (uint32_t)d.card[j];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    // a guarded load without a branch: a lane past the slice reads row r once more, never past the slice - the V loads
                    // of a column are in flight together
                    const uint32_t code = (uint32_t)col[((drop >> i) & 1u) ? 0 : (int64_t)i * BLOCK];
                    key[i] += code * stride;
                    if constexpr (POLICY == BY_CARD) drop |= (code >= card ? 1u : 0u) << i;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (counted(key[i], drop, i)) atomicAdd(mine + key[i], 1u);
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

// one thread packs four rows of one column
__global__ __launch_bounds__(BLOCK) void byte_mirror_kernel(const int32_t* __restrict__ codes, int64_t n, uint8_t* __restrict__ mirror, int64_t ld8) {
    const int64_t r = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (r >= ld8) return;
    const int32_t* col = codes + (int64_t)blockIdx.y * n;
    uint32_t packed = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) packed |= (r + i < n ? (uint32_t)col[r + i] & 0xFFu : 0xFFu) << (8 * i);
    *reinterpret_cast<uint32_t*>(mirror + (int64_t)blockIdx.y * ld8 + r) = packed;
}

// the units of one form: descs in device memory; the count buffer must be zero where a unit has more than one slice or takes the global form
template <bool LDS, Policy POLICY>
void launch_count(const Desc* dev, const std::vector<Desc>& descs, const Codes& c, uint32_t* counts, hipStream_t st) {
    if (descs.empty()) return;
    int max_slices = 1, lds_words = LDS ? 1 : 0;
    for (const Desc& d : descs) {
        max_slices = std::max(max_slices, d.slices);
        if (LDS) lds_words = std::max(lds_words, d.copies * d.copy_stride);
    }
    if (lds_words > LDS_WORDS || max_slices > MAX_SLICES) throw invalid_error("joint counts: bad launch shape");
    const dim3 grid((unsigned)descs.size(), (unsigned)max_slices), block(BLOCK);
    const size_t lds = (size_t)lds_words * sizeof(uint32_t);
    if (c.ld8 > 0) hipLaunchKernelGGL((joint_count_kernel<uint8_t, LDS, POLICY>), grid, block, lds, st, dev, c.codes8, c.ld8, counts);
    else hipLaunchKernelGGL((joint_count_kernel<int32_t, LDS, POLICY>), grid, block, lds, st, dev, c.codes32, c.ld32, counts);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

int run_chunk(pbn_ctx* ctx, Scratch& s, const std::vector<Desc> (&descs)[2], size_t cells, const Codes& codes, Policy policy,
              const std::function<void(int)>& after_step) {
    hipStream_t st = ctx->stream;
    const size_t n0 = descs[0].size(), n1 = descs[1].size();
    s.descs.reserve(n0 + n1);
    s.counts.reserve(cells);
    if (s.host.size() < cells) s.host.resize(cells);
    if (n0) HIP_CHECK(hipMemcpyAsync(s.descs.p, descs[0].data(), n0 * sizeof(Desc), hipMemcpyHostToDevice, st));
    if (n1) HIP_CHECK(hipMemcpyAsync(s.descs.p + n0, descs[1].data(), n1 * sizeof(Desc), hipMemcpyHostToDevice, st));
    if (after_step) after_step(0);
    HIP_CHECK(hipMemsetAsync(s.counts.p, 0, cells * sizeof(uint32_t), st));
    if (after_step) after_step(1);
    if (policy == BY_CARD) {
        launch_count<true, BY_CARD>(s.descs.p, descs[0], codes, s.counts.p, st);
        launch_count<false, BY_CARD>(s.descs.p + n0, descs[1], codes, s.counts.p, st);
    } else {
        launch_count<true, NONE>(s.descs.p, descs[0], codes, s.counts.p, st);
        launch_count<false, NONE>(s.descs.p + n0, descs[1], codes, s.counts.p, st);
    }
    if (after_step) after_step(2);
    HIP_CHECK(hipMemcpyAsync(s.host.data(), s.counts.p, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));   // (the descriptors are read by then as well)
    if (after_step) after_step(3);
    return (n0 ? 1 : 0) + (n1 ? 1 : 0);
}

void byte_mirror(pbn_ctx* ctx, const int32_t* codes, int64_t n, int n_cols, uint8_t* mirror, int64_t ld8) {
    if (n_cols <= 0 || ld8 <= 0) return;
    if (ld8 % MIRROR_ALIGN != 0 || ld8 < n) throw invalid_error("joint counts: bad mirror shape");
    hipLaunchKernelGGL(byte_mirror_kernel, dim3((unsigned)ceil_div(ld8 / 4, BLOCK), (unsigned)n_cols), dim3(BLOCK), 0, ctx->stream, codes, n, mirror, ld8);
    HIP_CHECK(hipGetLastError());
}

}  // namespace joint
}  // namespace pbn
