// The host half of LinearCorrelation's batch over tables with nulls (lincor_null_batch.hip) that is plain C++: the shape constants,
// the split of the rows into clean and dirty ones, the cut of the dirty rows into slices, and the grouping of a batch's tests by
// conditioning-set size.  No device type in here: tests/c/lincor_null_host_main.cpp compiles this file alone under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pbn {
namespace lincor_null {

constexpr int CHUNK = 256;        // tests of one workgroup, one per lane
constexpr int TILE = 16;          // dirty rows staged in LDS at a time, all columns of them
// The most continuous columns a handle may have for the device pass; wider tables loop over the scalar routine.  A tile is TILE rows of
// all columns: 32 KiB of doubles at this cap, so that four workgroups still share a CU's 160 KiB of LDS (a cap of 1 280 columns would
// fit one tile into the LDS of a CU and leave one workgroup per CU).
constexpr int NC_MAX = 256;
constexpr int SLICES_MAX = 32;    // slices of the dirty rows: workgroups per chunk of tests, partial records per test
constexpr int SLICE_MIN = 256;    // rows; fewer dirty rows are one slice
// default of pbn_mi_lincor_set_batch_threshold: the smallest measured batch from which the device wins for every k.  The loop it
// replaces costs a launch, a wait and a copy per TEST (34 - 51 us at 1e5 rows), so the device wins far earlier than on a null-free
// handle, whose loop is host arithmetic: at 20 tests 1.3 x (k = 6) to 3.7 x (k = 0); at 10 tests k = 6 loses (0.8 x) and k = 3, 5 tie
// (1e5 rows, 30 % of them dirty; profiles/lincor_null/lincor_null_timing.json)
constexpr int64_t LINCOR_NULL_BATCH_MIN_TESTS = 20;

// Rows of a slice: a function of the number of dirty rows ALONE (it is part of the order of additions), a multiple of TILE.
inline int64_t slice_rows(int64_t n_dirty) {
    const int64_t per = (n_dirty + SLICES_MAX - 1) / SLICES_MAX;
    return std::max<int64_t>(SLICE_MIN, (per + TILE - 1) / TILE * TILE);
}
inline int num_slices(int64_t n_dirty) { return (int)((n_dirty + slice_rows(n_dirty) - 1) / slice_rows(n_dirty)); }

// mask[r] != 0: row r holds a NaN in some continuous column.  Both lists ascending.
inline void partition_rows(const unsigned char* mask, int64_t n, std::vector<int32_t>& clean, std::vector<int32_t>& dirty) {
    clean.clear();
    dirty.clear();
    int64_t nd = 0;
    for (int64_t r = 0; r < n; ++r) nd += mask[r] != 0;
    dirty.reserve((size_t)nd);
    clean.reserve((size_t)(n - nd));
    for (int64_t r = 0; r < n; ++r) (mask[r] ? dirty : clean).push_back((int32_t)r);
}

// The tests of a batch by conditioning-set size: by_k[k] lists, in batch order, the tests with ok[t] != 0 and k = cond_off[t + 1] -
// cond_off[t] <= k_dev; every other test goes to `rest` (the scalar routine answers it, or refuses it in its own words).
inline void group_tests(int n_tests, const int* cond_off, const unsigned char* ok, int k_dev, std::vector<std::vector<int>>& by_k,
                        std::vector<int>& rest) {
    by_k.assign((size_t)k_dev + 1, {});
    rest.clear();
    for (int t = 0; t < n_tests; ++t) {
        const int k = cond_off[t + 1] - cond_off[t];
        if (ok[t] && k >= 0 && k <= k_dev) by_k[(size_t)k].push_back(t);
        else rest.push_back(t);
    }
}

// Tests of one launch: as many whole chunks as keep the slices' partial records (n_slices x acc doubles per test) within `budget` bytes.
inline int64_t tests_per_launch(int n_slices, int acc, int64_t budget) {
    const int64_t per_test = (int64_t)std::max(1, n_slices) * acc * (int64_t)sizeof(double);
    return std::max<int64_t>(CHUNK, budget / per_test / CHUNK * CHUNK);
}

}  // namespace lincor_null
}  // namespace pbn
