// The plain-C++ half of the joint-count unit (csrc/joint_counts.hpp) - how a unit's rows are cut into slices and how many replicated
// sub-tables fit LDS - as a stand-alone program, so that it can run under the host sanitizers without a device:
//   hipcc -O1 -g -std=c++17 -x c++ -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//         -Ipybnesian_amd/csrc tests/c/joint_counts_host_main.cpp -o joint_counts_host_main && ./joint_counts_host_main
// (any C++17 compiler does: the header alone uses no device type).  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <initializer_list>

#include "joint_counts.hpp"

using namespace pbn::joint;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

static int64_t up(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the rule as tests/test_chisq_batch_gpu.py::slicing transcribes it, with the slices the chip asks for (`want`) and the global form
// (no 8 G term) added
static int check_rule(int64_t row0, int64_t row1, int G, bool bytes, bool lds, int64_t want) {
    Desc d{};
    d.G = G;
    d.copies = -1; d.copy_stride = -1;
    plan_slices(d, row0, row1, bytes, lds, want, MAX_COPIES);
    CHECK(d.row0 == row0 && d.row1 == row1);
    if (bytes) CHECK(d.base % 8 == 0 && d.base <= row0 && row0 - d.base < 8);
    else CHECK(d.base == row0);
    const int64_t rows = row1 - d.base;
    int64_t s = rows / (lds ? (4096 > 8 * (int64_t)G ? 4096 : 8 * (int64_t)G) : 4096);
    if (s < 1) s = 1;
    if (s > want) s = want;
    if (s > 65535) s = 65535;
    const int64_t per = up(up(rows, s), 2048) * 2048;
    CHECK(d.rows_per_slice == per && d.slices == up(rows, per));
    // the slices cover [base, row1) exactly once: all but the last full, the last not empty
    CHECK(d.slices >= 1 && d.slices <= MAX_SLICES && d.rows_per_slice % SLICE_ALIGN == 0);
    CHECK((int64_t)(d.slices - 1) * d.rows_per_slice < rows && (int64_t)d.slices * d.rows_per_slice >= rows);
    if (lds) {
        int r = 0, stride = 0;
        copies_for(G, MAX_COPIES, &r, &stride);
        CHECK(d.copies == r && d.copy_stride == stride);
    } else {
        CHECK(d.copies == -1 && d.copy_stride == -1);   // the global form has none: left alone
    }
    return 0;
}

int main() {
    for (int64_t rows : {(int64_t)1, (int64_t)4095, (int64_t)4096, (int64_t)4097, (int64_t)8193, (int64_t)12289, (int64_t)1000000})
        for (int G : {1, 6, 512, 4096, 4097, 1 << 20})
            for (bool lds : {true, false})
                for (int64_t want : {(int64_t)1, (int64_t)3, (int64_t)65535 + 1})
                    for (bool bytes : {true, false}) {
                        if (check_rule(0, rows, G, bytes, lds, want)) return 1;
                        // a family region on any first row
                        for (int64_t row0 : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)8, (int64_t)2049})
                            if (check_rule(row0, row0 + rows, G, bytes, lds, want)) return 1;
                    }
    // the figures tests/test_chisq_batch_gpu.py names: 12 289 rows of a 6-cell table are three slices (4 097 rows each, rounded up to
    // 6 144: two full ones and one row), 8 193 rows are two (6 144 + 2 049)
    {
        Desc d{};
        d.G = 6;
        plan_slices(d, 0, 12289, true, true, 1 << 20, MAX_COPIES);
        CHECK(d.slices == 3 && d.rows_per_slice == 6144 && d.copies == 32 && d.copy_stride == 33);
        plan_slices(d, 0, 8193, true, true, 1 << 20, MAX_COPIES);
        CHECK(d.slices == 2 && d.rows_per_slice == 6144);
    }
    for (int G : {1, 4, 31, 32, 33, 255, 256, 4096})
        for (int r_max : {1, 8, 32}) {
            int r = 0, stride = 0;
            copies_for(G, r_max, &r, &stride);
            CHECK(r >= 1 && r <= r_max && r <= MAX_COPIES && (r & (r - 1)) == 0);
            CHECK((int64_t)r * stride <= LDS_WORDS);
            CHECK(stride == (r == 1 ? G : ((G + 31) & ~31) + 1));
            // the largest such power of two: the next one is over r_max or does not fit
            CHECK(2 * r > r_max || 2 * r > MAX_COPIES || (int64_t)2 * r * (((G + 31) & ~31) + 1) > LDS_WORDS);
        }
    std::puts("ok");
    return 0;
}
