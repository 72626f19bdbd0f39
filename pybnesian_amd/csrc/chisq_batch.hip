// ChiSquare, many tests per call: the contingency tables of a whole skeleton level counted in one device pass.
//
// A purely discrete test needs the cell counts of ONE contingency table and nothing else.  The scalar routine gets them as the segment
// lengths of a row grouping (mi.hip, Engine::group_for: a key kernel, a radix sort of all N rows, a segment kernel, two synchronisations
// and an N-entry permutation kept in the grouping cache) - built for the continuous moments of hybrid tests, and one of it per variable
// set.  A PC or MMPC level asks for 10^3 ... 10^6 tables over nearly as many distinct variable sets.  Here one workgroup counts one
// (test, row slice): every lane forms the keys of its rows from the code columns of the test and adds 1 into a table in LDS; the
// workgroup then adds its table into the test's table in global memory.  No sort, no permutation, one launch per chunk of tests.
//
// LDS atomics on one address serialise: a 2 x 2 table takes the 64 lanes of a wave to 4 addresses, a constant column to 1.  The table is
// therefore replicated R times (chisq_batch.hpp, copies_for): a lane adds into copy (lane mod R), and the copies are staggered by one
// bank, so that the lanes of a 32-lane group that meet in one cell are spread over R banks.  All sums are integer: neither the order of the LDS adds nor
// the order in which the slices of a test reach global memory can change a count.
#include "chisq_batch.hpp"

#include "common.hpp"

namespace pbn {
namespace chisq {

namespace {

// CodeT = uint8_t: the byte mirror, ROWS_PER_LANE_U8 consecutive rows per lane and step from one 8-byte load per column.
// CodeT = int32_t: the handle's codes as they are, ROWS_PER_LANE_I32 rows per lane and step, BLOCK rows apart (coalesced 4-byte loads;
// the columns of codes_dev are N elements apart, which aligns nothing wider).
template <typename CodeT>
__global__ __launch_bounds__(BLOCK) void chisq_count_kernel(const Desc* __restrict__ descs, const CodeT* __restrict__ codes, int64_t ld,
                                                             uint32_t* __restrict__ counts) {
    extern __shared__ uint32_t cells[];   // [copies][copy_stride]
    const Desc& d = descs[blockIdx.x];
    const int slice = blockIdx.y;
    if (slice >= d.slices) return;
    const int tid = threadIdx.x, m = d.m, G = d.G, copies = d.copies, copy_stride = d.copy_stride;
    const int words = copies * copy_stride;
    for (int i = tid; i < words; i += BLOCK) cells[i] = 0u;
    __syncthreads();
    uint32_t* mine = cells + (tid & (copies - 1)) * copy_stride;
    const int64_t r0 = d.row0 + (int64_t)slice * d.rows_per_slice;
    const int64_t r1 = r0 + d.rows_per_slice < d.row1 ? r0 + d.rows_per_slice : d.row1;
    if constexpr (sizeof(CodeT) == 1) {
        constexpr int V = ROWS_PER_LANE_U8;
        for (int64_t r = r0 + (int64_t)tid * V; r < r1; r += (int64_t)BLOCK * V) {
            uint32_t key[V];
#pragma unroll
            for (int i = 0; i < V; ++i) key[i] = 0u;
            uint32_t bad = 0u;
            for (int j = 0; j < m; ++j) {
                const uint2 v = *reinterpret_cast<const uint2*>(codes + (int64_t)d.col[j] * ld + r);
                const uint32_t stride = (uint32_t)d.stride[j], card = (uint32_t)d.card[j];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t c = ((i < 4 ? v.x : v.y) >> (8 * (i & 3))) & 0xFFu;
                    key[i] += c * stride;
                    bad |= (c >= card ? 1u : 0u) << i;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (!((bad >> i) & 1u) && r + i < r1) atomicAdd(mine + key[i], 1u);
        }
    } else {
        constexpr int V = ROWS_PER_LANE_I32;
        for (int64_t r = r0 + tid; r < r1; r += (int64_t)BLOCK * V) {
            uint32_t key[V];
#pragma unroll
            for (int i = 0; i < V; ++i) key[i] = 0u;
            uint32_t bad = 0u;
#pragma unroll
            for (int i = 0; i < V; ++i) bad |= (r + (int64_t)i * BLOCK < r1 ? 0u : 1u) << i;
            for (int j = 0; j < m; ++j) {
                const CodeT* col = codes + (int64_t)d.col[j] * ld + r;
                const uint32_t stride = (uint32_t)d.stride[j], card = (uint32_t)d.card[j];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const uint32_t c = ((bad >> i) & 1u) ? card : (uint32_t)col[(int64_t)i * BLOCK];
                    key[i] += c * stride;
                    bad |= (c >= card ? 1u : 0u) << i;
                }
            }
#pragma unroll
            for (int i = 0; i < V; ++i)
                if (!((bad >> i) & 1u)) atomicAdd(mine + key[i], 1u);
        }
    }
    __syncthreads();
    // flush: the R copies of a cell, summed; a test of one slice owns its table (plain stores over the zeroed buffer)
    uint32_t* out = counts + d.table_off;
    const bool single = d.slices == 1;
    for (int cell = tid; cell < G; cell += BLOCK) {
        uint32_t s = 0u;
        for (int c = 0; c < copies; ++c) s += cells[c * copy_stride + cell];
        if (s == 0u) continue;
        if (single) out[cell] = s;
        else atomicAdd(out + cell, s);
    }
}

// one thread packs four rows of one column
__global__ __launch_bounds__(BLOCK) void chisq_byte_mirror_kernel(const int32_t* __restrict__ codes, int64_t n, uint8_t* __restrict__ mirror,
                                                                   int64_t ld8) {
    const int64_t r = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (r >= ld8) return;
    const int32_t* col = codes + (int64_t)blockIdx.y * n;
    uint32_t packed = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) packed |= (r + i < n ? (uint32_t)col[r + i] & 0xFFu : 0xFFu) << (8 * i);
    *reinterpret_cast<uint32_t*>(mirror + (int64_t)blockIdx.y * ld8 + r) = packed;
}

}  // namespace

void launch_count(const Desc* descs, int n_tests, int max_slices, int lds_words, bool bytes, const void* codes, int64_t ld, uint32_t* counts,
                  hipStream_t stream) {
    if (n_tests <= 0) return;
    if (lds_words < 1 || lds_words > LDS_WORDS || max_slices < 1 || max_slices > 65535) throw invalid_error("ChiSquare batch: bad launch shape");
    const dim3 grid((unsigned)n_tests, (unsigned)max_slices), block(BLOCK);
    const size_t lds = (size_t)lds_words * sizeof(uint32_t);
    if (bytes) hipLaunchKernelGGL(chisq_count_kernel<uint8_t>, grid, block, lds, stream, descs, (const uint8_t*)codes, ld, counts);
    else hipLaunchKernelGGL(chisq_count_kernel<int32_t>, grid, block, lds, stream, descs, (const int32_t*)codes, ld, counts);
    HIP_CHECK(hipGetLastError());
}

void launch_byte_mirror(const int32_t* codes, int64_t n, int n_disc, uint8_t* mirror, int64_t ld8, hipStream_t stream) {
    if (n_disc <= 0 || ld8 <= 0) return;
    if (ld8 % MIRROR_ALIGN != 0 || ld8 < n) throw invalid_error("ChiSquare batch: bad mirror shape");
    hipLaunchKernelGGL(chisq_byte_mirror_kernel, dim3((unsigned)ceil_div(ld8 / 4, BLOCK), (unsigned)n_disc), dim3(BLOCK), 0, stream, codes, n, mirror,
                       ld8);
    HIP_CHECK(hipGetLastError());
}

}  // namespace chisq
}  // namespace pbn
