// Joint counts of discrete columns on the device (joint_counts.hip): the contingency tables of a ChiSquare level (chisq.hip) and the family
// tables of the score engine and of a pbn_dtable (family_counts.hip, discrete_model.hip) come from one kernel.  This part - the constants,
// the descriptor of a unit of work and how a unit's rows are cut into slices - is plain C++ without a device type: a host-only program
// (tests/c/joint_counts_host_main.cpp) includes the header alone and stops at the #ifdef below.
#pragma once
#include <algorithm>
#include <cstdint>

namespace pbn {
namespace joint {

constexpr int MAX_VARS = 8;                // columns of one unit: the descriptor's arrays
constexpr int BLOCK = 256;
constexpr int LDS_WORDS = 8192;            // 32 KiB of counters per workgroup: five workgroups per CU of the 160 KiB
constexpr int MAX_COPIES = 32;             // replicated sub-tables of one workgroup
constexpr int ROWS_PER_LANE_U8 = 8;        // one 8-byte load per column and step
constexpr int ROWS_PER_LANE_I32 = 4;       // four coalesced 4-byte loads per column and step
constexpr int SLICE_ALIGN = BLOCK * ROWS_PER_LANE_U8;   // rows of a slice: a multiple of it, so that the 8-byte loads stay aligned
constexpr int MIRROR_ALIGN = 16;           // the byte mirror's leading dimension is a multiple of it (rows past the last hold 0xFF)
constexpr int MAX_SLICES = 65535;          // grid.y

// One unit = one table.  key of a row = sum_j code[col[j]][row] * stride[j], counted over the rows [row0, row1) that the kernel's validity
// policy lets through.
struct Desc {
    int m, G;                 // columns; prod card = cells
    int col[MAX_VARS];        // column index into the codes
    int stride[MAX_VARS];     // the first column fastest
    int card[MAX_VARS];       // BY_CARD: a code counts when (uint32_t)code < card
    int copies, copy_stride;  // LDS form: R replicated sub-tables, copy c at c * copy_stride (copies_for)
    int slices;               // workgroups of this unit: slice s takes rows [base + s * rows_per_slice, ...) within [row0, row1)
    int64_t table_off;        // first cell of its table in the launch's count buffer
    int64_t row0, row1, base, rows_per_slice;
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

// Rows [row0, row1) of unit d (d.G set) cut into slices, and the copies of the LDS form.  `want` slices fill the chip when a launch has
// few units; a slice's flush (G cells) stays small against its row work: at least max(4096, 8 G) rows per LDS slice, 4096 per global one.
// A byte-form unit starts on the multiple of 8 at or below row0 - its loads stay aligned and the kernel masks the rows below row0.
inline void plan_slices(Desc& d, int64_t row0, int64_t row1, bool bytes, bool lds, int64_t want, int r_max) {
    if (lds) copies_for(d.G, r_max, &d.copies, &d.copy_stride);
    d.row0 = row0; d.row1 = row1;
    d.base = bytes ? row0 / ROWS_PER_LANE_U8 * ROWS_PER_LANE_U8 : row0;
    const int64_t rows = std::max<int64_t>(1, row1 - d.base);
    const int64_t cap = std::max<int64_t>(1, rows / std::max<int64_t>(4096, lds ? 8 * (int64_t)d.G : 0));
    const int64_t s = std::min<int64_t>(std::min(std::max<int64_t>(1, want), cap), MAX_SLICES);
    d.rows_per_slice = (rows + s - 1) / s;
    d.rows_per_slice = (d.rows_per_slice + SLICE_ALIGN - 1) / SLICE_ALIGN * SLICE_ALIGN;
    d.slices = (int)((rows + d.rows_per_slice - 1) / d.rows_per_slice);
}

}  // namespace joint
}  // namespace pbn

#ifdef __HIPCC__   // the device half, for the units of the library
#include <functional>
#include <vector>

#include "common.hpp"

namespace pbn {
namespace joint {

// which rows of [row0, row1) a unit counts.  NONE: all of them (no code may lie outside its column's cardinality; the kernel only keeps
// key < G).  BY_CARD: those with (uint32_t)code < card[j] in every column of the unit - a null is any code that fails it: the null bucket
// code == card of a pbn_mi handle, -1 of score data and of a pbn_dtable, 0xFF in their byte mirrors (which exist when max card <= 255).
enum Policy { NONE = 0, BY_CARD = 1 };

// int32 codes [cols][ld32] on the device, and their byte mirror [cols][ld8] when ld8 > 0: the kernels then read the mirror
struct Codes {
    const int32_t* codes32 = nullptr;
    int64_t ld32 = 0;
    const uint8_t* codes8 = nullptr;
    int64_t ld8 = 0;
};

// what a caller keeps between chunks, grow-only: a launch chunk's descriptors, its count buffer and the host copy of the counts
struct Scratch {
    dev_buf<Desc> descs;
    dev_buf<uint32_t> counts;
    std::vector<uint32_t> host;
};

// One launch chunk: descs[0] (LDS form) and descs[1] (global-atomics form) up, the `cells` of the count buffer zeroed, one launch per form
// present (the return value), the counts down into s.host, the stream synchronised.  after_step, when set, is called with 0 after the
// descriptors are enqueued, 1 after the memset, 2 after the launches and 3 after the download and the synchronisation.
int run_chunk(pbn_ctx* ctx, Scratch& s, const std::vector<Desc> (&descs)[2], size_t cells, const Codes& codes, Policy policy,
              const std::function<void(int)>& after_step = nullptr);

// mirror[j * ld8 + r] = (uint8_t)codes[j * n + r], 0xFF in the padding rows n ... ld8 - 1 (ld8 a multiple of MIRROR_ALIGN); enqueued on
// the context's stream
void byte_mirror(pbn_ctx* ctx, const int32_t* codes, int64_t n, int n_cols, uint8_t* mirror, int64_t ld8);

}  // namespace joint
}  // namespace pbn
#endif
