// Batched joint counts for ChiSquare (chisq_batch.hip): what the kernels and the batch function of mi.hip share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbn {
namespace chisq {

constexpr int MAX_CELLS = 4096;            // cells of one contingency table counted on the device (pbn_chisq_batch_max_cells)
constexpr int MAX_COND = 6;                // conditioning variables of a device test (pbn_chisq_batch_max_cond); fixes the descriptor's arrays
constexpr int MAX_VARS = MAX_COND + 2;
constexpr int BLOCK = 256;
constexpr int LDS_WORDS = 8192;            // 32 KiB of counters per workgroup: five workgroups per CU of the 160 KiB
constexpr int MAX_COPIES = 32;             // replicated sub-tables of one workgroup
constexpr int ROWS_PER_LANE_U8 = 8;        // one 8-byte load per column and step
constexpr int ROWS_PER_LANE_I32 = 4;       // four coalesced 4-byte loads per column and step
constexpr int SLICE_ALIGN = BLOCK * ROWS_PER_LANE_U8;   // a slice starts on a multiple of it: the 8-byte loads stay aligned
constexpr int MIRROR_ALIGN = 16;           // the byte mirror's leading dimension is a multiple of it (rows past N hold 0xFF)

// One test = one contingency table.  key of a row = sum_j code[col[j]][row] * stride[j]; the row counts when code_j < card[j] for all j.
struct Desc {
    int m;                    // 2 + k variables: x, y, Z in the order given
    int col[MAX_VARS];        // discrete column index
    int stride[MAX_VARS];     // x fastest
    int card[MAX_VARS];
    int G;                    // prod card
    int copies, copy_stride;  // R replicated sub-tables in LDS, copy c at c * copy_stride (copies_for)
    int slices;               // workgroups of this test: slice s counts rows [row0 + s * rows_per_slice, ...) up to row1
    int64_t table_off;        // first cell of its table in the launch's count buffer
    int64_t row0, row1, rows_per_slice;
};

// R = the largest power of two <= r_max for which R padded tables fit LDS_WORDS.  The copy stride is G rounded up to the 32 banks a
// 4-byte LDS atomic sees, plus one: cell c of copy r lies on bank (r + c) mod 32, so the lanes of a 32-lane group that hit one cell -
// every lane, for a constant column - go to R different banks.  (Per 32-lane group: lanes l and l + 32 of a wave share a copy and are
// served in different LDS passes, so more than 32 copies would buy nothing.)  One copy needs no padding.
inline void copies_for(int G, int r_max, int* copies, int* copy_stride) {
    const int padded = ((G + 31) & ~31) + 1;
    int r = 1;
    while (2 * r <= r_max && 2 * r <= MAX_COPIES && (int64_t)2 * r * padded <= LDS_WORDS) r *= 2;
    *copies = r;
    *copy_stride = r == 1 ? G : padded;
}

// descs: n_tests descriptors in device memory; codes: the byte mirror ([n_disc][ld], bytes = true) or the handle's int32 codes; the
// count buffer must be zero where a test has more than one slice.  lds_words = max over the tests of copies * copy_stride.
void launch_count(const Desc* descs, int n_tests, int max_slices, int lds_words, bool bytes, const void* codes, int64_t ld, uint32_t* counts,
                  hipStream_t stream);
// mirror[j * ld8 + r] = (uint8_t)codes[j * n + r], 0xFF in the padding rows n ... ld8 - 1 (ld8 a multiple of MIRROR_ALIGN)
void launch_byte_mirror(const int32_t* codes, int64_t n, int n_disc, uint8_t* mirror, int64_t ld8, hipStream_t stream);

}  // namespace chisq
}  // namespace pbn
