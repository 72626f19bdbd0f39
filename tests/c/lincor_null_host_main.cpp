// The plain-C++ half of LinearCorrelation's batch over tables with nulls (csrc/lincor_null_host.hpp) - the split of the rows into
// clean and dirty ones, the cut of the dirty rows into slices, the grouping of a batch by conditioning-set size, the launch chunking -
// as a stand-alone program, so that it can run under the host sanitizers without a device:
//   hipcc -O1 -g -std=c++17 -x c++ -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -Ipybnesian_amd/csrc tests/c/lincor_null_host_main.cpp -o lincor_null_host_main && ./lincor_null_host_main
// (any C++17 compiler does: the header uses no device type).  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "lincor_null_host.hpp"

using namespace pbn::lincor_null;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int check_partition(const std::vector<unsigned char>& mask) {
    const int64_t n = (int64_t)mask.size();
    std::vector<int32_t> clean{7, 7}, dirty{9};   // stale contents must go
    partition_rows(mask.data(), n, clean, dirty);
    CHECK((int64_t)(clean.size() + dirty.size()) == n);
    size_t ic = 0, id = 0;
    for (int64_t r = 0; r < n; ++r) {
        if (mask[(size_t)r]) { CHECK(id < dirty.size() && dirty[id] == r); ++id; }
        else { CHECK(ic < clean.size() && clean[ic] == r); ++ic; }
    }
    // the slices cover the dirty rows exactly once, every one but the last full, all starting on a tile boundary
    const int64_t nd = (int64_t)dirty.size();
    const int64_t len = slice_rows(nd);
    CHECK(len >= SLICE_MIN && len % TILE == 0);
    if (nd > 0) {
        const int ns = num_slices(nd);
        CHECK(ns >= 1 && ns <= SLICES_MAX);
        CHECK((int64_t)(ns - 1) * len < nd && (int64_t)ns * len >= nd);
    }
    return 0;
}

int main() {
    std::mt19937 rng(11);
    // N_dirty = 0, 1 (first, last, middle row), all rows, and random fractions; an empty table
    for (int64_t n : {0, 1, 2, 255, 256, 257, 5000, 100003}) {
        std::vector<unsigned char> mask((size_t)n, 0);
        if (check_partition(mask)) return 1;
        if (n > 0) {
            for (int64_t at : {(int64_t)0, n / 2, n - 1}) {
                std::fill(mask.begin(), mask.end(), 0);
                mask[(size_t)at] = 1;
                if (check_partition(mask)) return 1;
            }
            std::fill(mask.begin(), mask.end(), 1);
            if (check_partition(mask)) return 1;
            for (double frac : {0.001, 0.3, 0.9}) {
                std::bernoulli_distribution d(frac);
                for (auto& m : mask) m = d(rng) ? 255 : 0;
                if (check_partition(mask)) return 1;
            }
        }
    }
    // slice length: a function of n_dirty alone, never more than SLICES_MAX slices
    for (int64_t nd : {(int64_t)1, (int64_t)SLICE_MIN - 1, (int64_t)SLICE_MIN, (int64_t)SLICE_MIN + 1, (int64_t)SLICE_MIN * SLICES_MAX,
                       (int64_t)SLICE_MIN * SLICES_MAX + 1, (int64_t)1000000, ((int64_t)1 << 31) - 1}) {
        const int64_t len = slice_rows(nd);
        CHECK(len % TILE == 0 && len >= SLICE_MIN);
        CHECK(num_slices(nd) >= 1 && num_slices(nd) <= SLICES_MAX);
        CHECK((int64_t)num_slices(nd) * len >= nd);
    }
    // grouping: every test lands in exactly one list, in batch order; refused tests and large sets go to `rest`
    for (int n_tests : {0, 1, 63, 64, 65, 1000}) {
        std::vector<int> off((size_t)n_tests + 1, 0);
        std::vector<unsigned char> ok((size_t)std::max(1, n_tests), 1);
        for (int t = 0; t < n_tests; ++t) {
            off[(size_t)t + 1] = off[(size_t)t] + (int)(rng() % 9);   // k = 0 ... 8
            ok[(size_t)t] = rng() % 7 != 0;
        }
        std::vector<std::vector<int>> by_k{{1, 2, 3}};
        std::vector<int> rest{5};
        const int k_dev = 6;
        group_tests(n_tests, off.data(), ok.data(), k_dev, by_k, rest);
        CHECK((int)by_k.size() == k_dev + 1);
        std::vector<int> seen((size_t)std::max(1, n_tests), 0);
        for (int k = 0; k <= k_dev; ++k)
            for (size_t i = 0; i < by_k[(size_t)k].size(); ++i) {
                const int t = by_k[(size_t)k][i];
                CHECK(t >= 0 && t < n_tests && ok[(size_t)t] && off[(size_t)t + 1] - off[(size_t)t] == k);
                CHECK(i == 0 || by_k[(size_t)k][i - 1] < t);
                ++seen[(size_t)t];
            }
        for (int t : rest) {
            CHECK(t >= 0 && t < n_tests && (!ok[(size_t)t] || off[(size_t)t + 1] - off[(size_t)t] > k_dev));
            ++seen[(size_t)t];
        }
        for (int t = 0; t < n_tests; ++t) CHECK(seen[(size_t)t] == 1);
    }
    // launch chunking: whole chunks, at least one, the partials within the budget whenever more than one chunk is taken
    for (int ns : {0, 1, SLICES_MAX})
        for (int acc : {6, 45}) {
            const int64_t per = tests_per_launch(ns, acc, (int64_t)256 << 20);
            CHECK(per >= CHUNK && per % CHUNK == 0);
            CHECK(per == CHUNK || per * std::max(1, ns) * acc * 8 <= ((int64_t)256 << 20));
        }
    std::puts("ok");
    return 0;
}
