// ChiSquare (learning/independences/discrete/chi_square.{hpp,cpp}) over the discrete columns of a pbn_mi handle (mi_internal.hpp): the
// scalar test on the counts of the handle's row groupings, and many tests per call - the contingency tables of a whole skeleton level
// counted in one device pass.
//
// A purely discrete test needs the cell counts of ONE contingency table and nothing else.  The scalar routine gets them as the segment
// lengths of a row grouping (mi.hip, Engine::group_for: a key kernel, a radix sort of all N rows, a segment kernel, two synchronisations
// and an N-entry permutation kept in the grouping cache) - built for the continuous moments of hybrid tests, and one of it per variable
// set.  A PC or MMPC level asks for 10^3 ... 10^6 tables over nearly as many distinct variable sets.  Here one workgroup counts one
// (test, row slice): every lane forms the keys of its rows from the code columns of the test and adds 1 into a table in LDS; the
// workgroup then adds its table into the test's table in global memory.  No sort, no permutation, one launch per chunk of tests.
//
// The counting itself is the joint-count kernel of joint_counts.hip in its LDS form under the BY_CARD policy: the null
// bucket of a column, code == card, fails it.  What is kept here: decoding and eligibility of the requests, chisq_from_counts, the
// capture / phase test aid, the scalar routine - and mi::count_tables, the chunk runner (byte mirror, a descriptor per test, slices,
// launch chunks) that the count-only tests of pbn_mi_pvalue_batch (mi.hip) share.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <functional>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "specfun.hpp"
#include "hostmath.hpp"
#include "mi_internal.hpp"

namespace pbn {
namespace chisq {

constexpr int MAX_CELLS = 4096;            // cells of one contingency table counted on the device (pbn_chisq_batch_max_cells)
constexpr int MAX_COND = 6;                // conditioning variables of a device test (pbn_chisq_batch_max_cond)
constexpr int MAX_VARS = MAX_COND + 2;
static_assert(joint::MAX_VARS >= MAX_VARS, "x, y and the conditioning set fit the descriptor");
static_assert(MAX_CELLS <= mi::COUNT_LDS_MAX_CELLS && mi::COUNT_LDS_MAX_CELLS <= joint::LDS_WORDS, "a table fits the LDS form");

}  // namespace chisq
}  // namespace pbn

using namespace pbn;

// pbn_chisq_pvalue_batch: a call with fewer device-eligible tests loops over the scalar routine.  The crossover that tools/chisq_timing.py
// measured on an MI355X (profiles/chisq/chisq_timing.json): a batch of ONE test already beats the scalar routine - 1.9x at
// 5e3 rows, 2.8x at 1e5, 5-10x at 1e6, k = 0 ... 4 (a scalar test: 77-460 us around its sort; a batch of one: 40-50 us) - so every non-empty
// call goes to the device.  Results are bit-identical either way, so this value can only cost time.
#define CHISQ_BATCH_MIN_TESTS 1
#define CHISQ_CHUNK_CELLS ((size_t)1 << 26)   // cells of one launch chunk's count buffer: 256 MB of uint32

namespace {

// ChiSquare's p-value from the cell counts of one contingency table (chi_square.cpp:8-139): c[i + j * cx + k * cx * cy] rows with
// x = i, y = j and configuration k of the conditioning set.  The ONE text behind pbn_chisq_pvalue and pbn_chisq_pvalue_batch - never
// inlined, so that both callers run the same instructions: equal counts give the same bits.
__attribute__((noinline)) double chisq_from_counts(const double* counts, int cx, int cy, int zc, int n_cond) {
    const int vc = cx * cy;
    double statistic = 0;
    for (int k = 0; k < zc; ++k) {
        const double* c = counts + (size_t)k * vc;
        std::vector<double> mx(cx, 0.0), my(cy, 0.0);
        double tot = 0;
        for (int i = 0; i < cx; ++i)
            for (int j = 0; j < cy; ++j) { mx[i] += c[i + j * cx]; my[j] += c[i + j * cx]; tot += c[i + j * cx]; }
        if (tot == 0) continue;
        const double inv = 1.0 / tot;
        for (int i = 0; i < cx; ++i)
            for (int j = 0; j < cy; ++j) {
                const double expected = mx[i] * my[j] * inv;
                if (expected != 0) { const double dd = c[i + j * cx] - expected; statistic += dd * dd / expected; }
            }
    }
    if (n_cond > 1 && statistic < 1.4901161193847656e-08) return 1.0;   // chi_square.cpp:130-134
    const double df = (cx - 1.0) * (cy - 1.0) * zc;
    return gamma_q(0.5 * df, 0.5 * statistic);
}

// pbn_debug_chisq (test aid, not part of the C ABI header; see its definition)
std::atomic<int> g_chisq_capture{0};   // bit 0: record every batch call, bit 1: time its phases
std::mutex g_chisq_mu;
std::vector<int64_t> g_chisq_rec;
double g_chisq_phase[5] = {0, 0, 0, 0, 0};   // seconds: request and descriptors, memset, kernel, download, host finish

using ChisqTest = mi::CountTest;   // one slot of a batch call; where: 1 device, 0 host, -1 refused (NaN)

// The device part of pbn_chisq_pvalue_batch: the tests `which` (all eligible) counted by mi::count_tables, then chisq_from_counts on the
// host threads, chunk by chunk.  `tables` (capture only) receives every test's integer table.
void chisq_batch_device(pbn_mi* h, std::vector<ChisqTest>& tests, const std::vector<int>& which, const int* cond_off, double* out, int* width,
                        std::vector<std::vector<uint32_t>>* tables) {
    hipStream_t st = h->ctx->stream;
    const bool timing = (g_chisq_capture.load() & 2) != 0;
    double tp = mi_now();
    std::function<void(int)> phase;   // the phase clock: request and descriptors, memset, kernel, download
    if (timing) phase = [&](int i) {
        HIP_CHECK(hipStreamSynchronize(st));
        const double t = mi_now();
        g_chisq_phase[i] += t - tp;
        tp = t;
    };
    *width = mi::count_tables(h, tests, which, phase, [&](size_t base, int T, const std::vector<joint::Desc>& descs, const uint32_t* all) {
        host_finish(T, [&](int i) {
            const int slot = which[base + i];
            const ChisqTest& t = tests[slot];
            const uint32_t* c = all + descs[i].table_off;
            std::vector<double> cnt((size_t)t.G);
            for (int g = 0; g < t.G; ++g) cnt[g] = (double)c[g];
            const int cx = descs[i].card[0], cy = descs[i].card[1];
            out[slot] = chisq_from_counts(cnt.data(), cx, cy, t.G / (cx * cy), cond_off[slot + 1] - cond_off[slot]);
            if (tables) (*tables)[slot].assign(c, c + t.G);
        });
        if (timing) { const double t = mi_now(); g_chisq_phase[4] += t - tp; tp = t; }
        h->cs.device_tests += T;
    });
}

}  // namespace

// mi_internal.hpp: the one chunk runner behind pbn_chisq_pvalue_batch and the count-only tests of pbn_mi_pvalue_batch
int pbn::mi::count_tables(pbn_mi* h, std::vector<CountTest>& tests, const std::vector<int>& which, const std::function<void(int)>& phase,
                          const std::function<void(size_t, int, const std::vector<joint::Desc>&, const uint32_t*)>& finish) {
    pbn_ctx* ctx = h->ctx;
    HIP_CHECK(hipSetDevice(ctx->device));
    const int64_t N = h->N;
    if (h->cs.codes8_state == 0) {   // the byte mirror: a quarter of the bytes of every later pass
        // built when every CODE fits a byte: card - 1, or card where the column has a null bucket, <= 255.  256 categories without a null
        // still fit; their code 255 is also the byte that pads the mirror past N, which the kernel's row bound keeps out, not its value.
        int max_code = 0;
        for (int j = 0; j < h->n_disc; ++j) max_code = std::max(max_code, h->card[j] - 1 + (int)h->disc_null[j]);
        h->cs.codes8_state = -1;
        static const bool allow = PBN_TUNE(CHISQ_BYTES, 1) != 0;
        if (allow && max_code <= 255 && h->n_disc <= 65535) {
            h->cs.ld8 = ceil_div(N, joint::MIRROR_ALIGN) * joint::MIRROR_ALIGN;
            h->cs.codes8.alloc((size_t)h->cs.ld8 * h->n_disc);
            joint::byte_mirror(ctx, h->codes_dev.p, N, h->n_disc, h->cs.codes8.p, h->cs.ld8);
            h->cs.codes8_state = 1;
        }
    }
    const bool bytes = h->cs.codes8_state == 1;
    joint::Codes codes;
    codes.codes32 = h->codes_dev.p; codes.ld32 = N;
    if (bytes) { codes.codes8 = h->cs.codes8.p; codes.ld8 = h->cs.ld8; }
    static const int r_max = PBN_TUNE(CHISQ_COPIES, joint::MAX_COPIES);
    static const int blocks_per_cu = PBN_TUNE(CHISQ_BLOCKS_PER_CU, 8);
    std::vector<joint::Desc> both[2];   // LDS form, global form: what run_chunk launches
    std::vector<joint::Desc> descs;     // the chunk's tests in call order
    for (size_t base = 0; base < which.size();) {
        // a chunk: as many tests as keep the count buffer within CHISQ_CHUNK_CELLS
        size_t end = base, cells = 0;
        while (end < which.size() && end - base < ((size_t)1 << 18) && cells + (size_t)tests[which[end]].G <= CHISQ_CHUNK_CELLS) cells += (size_t)tests[which[end++]].G;
        if (end == base) throw invalid_error("joint counts: a table larger than a launch chunk");
        const int T = (int)(end - base);
        const int64_t want = std::max<int64_t>(1, ceil_div((int64_t)ctx->num_cus * blocks_per_cu, T));   // slices that fill the chip (plan_slices)
        descs.assign((size_t)T, joint::Desc{});
        both[0].clear(); both[1].clear();
        size_t off = 0;
        int n_global = 0;
        for (int i = 0; i < T; ++i) {
            CountTest& t = tests[which[base + i]];
            joint::Desc& d = descs[i];
            d.m = t.m; d.G = t.G;
            int stride = 1;
            for (int j = 0; j < t.m; ++j) {
                d.col[j] = t.vars[j] - h->n_cont;
                d.card[j] = h->card[d.col[j]];
                d.stride[j] = stride;
                stride *= d.card[j];
            }
            const bool lds = t.G <= COUNT_LDS_MAX_CELLS;
            joint::plan_slices(d, 0, N, bytes, lds, want, r_max);
            d.table_off = (int64_t)off;
            off += (size_t)t.G;
            t.slices = d.slices; t.copies = lds ? d.copies : 0;
            n_global += lds ? 0 : 1;
        }
        if (n_global == 0) {   // every ChiSquare chunk: the descriptors as they stand, no copy
            both[0].swap(descs);
        } else {
            for (const joint::Desc& d : descs) both[d.G <= COUNT_LDS_MAX_CELLS ? 0 : 1].push_back(d);
        }
        joint::run_chunk(ctx, h->cs.scratch, both, cells, codes, joint::BY_CARD, phase);
        if (n_global == 0) both[0].swap(descs);
        finish(base, T, descs, h->cs.scratch.host.data());
        base = end;
    }
    return bytes ? 1 : 4;
}

extern "C" {

// ChiSquare::pvalue (learning/independences/discrete/chi_square.cpp:8-139) over the discrete columns of a pbn_mi handle:
// Pearson's statistic summed over the configurations of the conditioning set, df = (|X|-1)(|Y|-1) prod |Z|.  Counts come
// from the same device pass as the mutual information (no continuous statistics).  Expected counts are formed in
// double; the reference multiplies two int marginals (chi_square.cpp:21,62,116), which overflows beyond ~46 000 rows
// per cell pair.  pbn_ci_pvalue_fn signature, indices mapped through pbn_mi_set_order when set.
double pbn_chisq_pvalue(void* user, int v1, int v2, int n_cond, const int* cond) {
    pbn_mi* h = (pbn_mi*)user;
    double result = std::nan("");
    const int rc = guarded([&] {
        if (!h || (n_cond > 0 && !cond)) throw invalid_error("pbn_chisq_pvalue: null argument");
        std::vector<int> vars;
        if (!mi::map_request(h, v1, v2, n_cond, cond, vars)) throw invalid_error("ChiSquare: variable index out of range");
        int64_t G = 1;
        for (int v : vars) {
            if (v < h->n_cont || v >= h->n_cont + h->n_disc) throw invalid_error("ChiSquare: variable is not categorical");
            G *= h->card[v - h->n_cont];
            if (G > (1 << 24)) throw invalid_error("ChiSquare: too many discrete configurations");
        }
        std::vector<double> st;
        mi::group_stats(h, {}, vars, st);
        const int cx = h->card[vars[0] - h->n_cont], cy = h->card[vars[1] - h->n_cont];
        result = chisq_from_counts(st.data(), cx, cy, (int)(G / (cx * cy)), n_cond);
    });
    return rc == PBN_OK ? result : std::nan("");
}

// ChiSquare::pvalue for many tests per call (chi_square.cpp:8-139 on the joint_counts layout of discrete_indices.cpp:134-150;
// pbn_ci_pvalue_batch_fn, user = the pbn_mi handle, indices mapped through pbn_mi_set_order when set).  Tests of at most
// chisq::MAX_CELLS cells and chisq::MAX_COND conditioning variables are counted by the kernels above - no DiscGroup, no sort, no
// permutation - and finished by chisq_from_counts, the scalar routine's own arithmetic on the same integers: out[i] is bit-identical to
// pbn_chisq_pvalue of test i, wherever it ran.  Every other test, and every test of a call with fewer eligible tests than the handle's
// threshold, goes through pbn_chisq_pvalue here; so does a test with a bad index or a non-categorical variable, which that routine
// refuses with NaN and pbn_last_error.  One NaN comes WITHOUT pbn_last_error, from the scalar routine and from here alike: a test of zero
// degrees of freedom (a one-category x or y), where chisq_from_counts answers 1 when its statistic is exactly 0 and NaN when rounding
// left it a few ulps above (gamma_q(0, tiny)).
void pbn_chisq_pvalue_batch(void* user, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out) {
    pbn_mi* h = (pbn_mi*)user;
    if (!out || n_tests <= 0) return;
    for (int i = 0; i < n_tests; ++i) out[i] = std::nan("");
    if (!h || !v1 || !v2 || !cond_off) { set_last_error("pbn_chisq_pvalue_batch: null argument"); return; }
    (void)guarded(mu_of(h), [&] {
        const int64_t groups0 = h->groups_built;
        const int nv = h->n_cont + h->n_disc;
        std::vector<ChisqTest> tests((size_t)n_tests);
        std::vector<int> device, vars;
        for (int i = 0; i < n_tests; ++i) {
            ChisqTest& t = tests[i];
            const int k = cond_off[i + 1] - cond_off[i];
            if (k < 0 || (k > 0 && !cond)) continue;   // refused by the scalar routine below
            t.where = 0;
            if (k > chisq::MAX_COND || h->N <= 0) continue;
            t.m = 2 + k;
            if (!mi::map_request(h, v1[i], v2[i], k, k > 0 ? cond + cond_off[i] : nullptr, vars)) continue;
            bool ok = true;
            int64_t G = 1;
            for (int j = 0; j < t.m && ok; ++j) {
                const int v = vars[j];
                if (v < h->n_cont || v >= nv) { ok = false; break; }
                for (int q = 0; q < j; ++q) ok = ok && t.vars[q] != v;   // a repeated variable: the scalar routine's own reading of it
                t.vars[j] = v;
                G *= h->card[v - h->n_cont];
                ok = ok && G >= 1 && G <= chisq::MAX_CELLS;
            }
            if (!ok) continue;
            t.G = (int)G;
            device.push_back(i);
        }
        if ((int64_t)device.size() < (h->cs.threshold < 0 ? CHISQ_BATCH_MIN_TESTS : h->cs.threshold)) device.clear();
        const bool capture = (g_chisq_capture.load() & 1) != 0;
        std::vector<std::vector<uint32_t>> tables;
        if (capture) tables.resize((size_t)n_tests);
        int width = 0;
        if (!device.empty()) {
            chisq_batch_device(h, tests, device, cond_off, out, &width, capture ? &tables : nullptr);
            for (int i : device) tests[i].where = 1;
        }
        const bool timing = (g_chisq_capture.load() & 2) != 0;
        const double th0 = mi_now();
        int64_t looped = 0;
        for (int i = 0; i < n_tests; ++i) {
            if (tests[i].where == 1) continue;
            const int k = cond_off[i + 1] - cond_off[i];
            out[i] = pbn_chisq_pvalue(user, v1[i], v2[i], k, (cond && k > 0) ? cond + cond_off[i] : nullptr);
            if (out[i] == out[i]) ++looped; else tests[i].where = -1;
        }
        if (timing) g_chisq_phase[4] += mi_now() - th0;
        h->cs.host_tests += looped;
        if (capture) {
            std::vector<int64_t> r{3, n_tests, groups0, h->groups_built};
            for (int i = 0; i < n_tests; ++i) {
                const ChisqTest& t = tests[i];
                const bool dev = t.where == 1;
                r.insert(r.end(), {(int64_t)t.where, dev ? width : 0, dev ? t.slices : 0, dev ? t.copies : 0, (int64_t)t.G, (int64_t)tables[i].size()});
                r.insert(r.end(), tables[i].begin(), tables[i].end());
            }
            std::lock_guard<std::mutex> lk(g_chisq_mu);
            g_chisq_rec.insert(g_chisq_rec.end(), r.begin(), r.end());
        }
    });
}

int pbn_chisq_batch_stats(const pbn_mi* h, int64_t* device_tests, int64_t* host_tests) {
    return guarded(mu_of(h), [&] {
        if (!h) throw invalid_error("pbn_chisq_batch_stats: null argument");
        if (device_tests) *device_tests = h->cs.device_tests;
        if (host_tests) *host_tests = h->cs.host_tests;
    });
}

int pbn_chisq_set_batch_threshold(pbn_mi* h, int64_t min_tests) {
    return guarded(mu_of(h), [&] {
        if (!h || min_tests < 0) throw invalid_error("pbn_chisq_set_batch_threshold: bad argument");
        h->cs.threshold = min_tests;
    });
}

int pbn_chisq_batch_max_cells(void) { return chisq::MAX_CELLS; }
int pbn_chisq_batch_max_cond(void) { return chisq::MAX_COND; }

// pbn_debug_chisq (test aid, not part of the C ABI header).  op 1 arms the capture and clears it, op 0 disarms everything and clears,
// op 2 copies up to `cap` int64 of the records into out and returns how many are held.  While armed, every pbn_chisq_pvalue_batch call
// appends one record:
//   3, n_tests, the handle's count of row groupings built before the call and after it, then per test in call order
//      where (1 = counted on the device, 0 = looped on the host, -1 = refused with NaN), code width in bytes (1 = the byte mirror, 4 =
//      int32; 0 off the device), slices, R (the replicated LDS sub-tables; both 0 off the device), G (cells; 0 when the test was not
//      sized for the device), n (G on the device, else 0), and the n cell counts as copied back from the device, x fastest.
// op 3 arms the phase clock and clears it, op 4 copies the 5 accumulated phase times in nanoseconds into out (request and descriptors,
// memset, kernel, download, host finish): while it runs a batch call synchronises the stream after every phase.
// Unarmed, a call pays two flag tests; no kernel and no result depends on any of it.
int64_t pbn_debug_chisq(int op, int64_t* out, int64_t cap) {
    std::lock_guard<std::mutex> lk(g_chisq_mu);
    if (op == 0 || op == 1) {
        g_chisq_rec.clear();
        g_chisq_capture.store(op == 1 ? (g_chisq_capture.load() | 1) : 0);
        return 0;
    }
    if (op == 2) {
        for (int64_t i = 0; out && i < (int64_t)g_chisq_rec.size() && i < cap; ++i) out[i] = g_chisq_rec[(size_t)i];
        return (int64_t)g_chisq_rec.size();
    }
    if (op == 3) {
        for (double& p : g_chisq_phase) p = 0;
        g_chisq_capture.store(g_chisq_capture.load() | 2);
        return 0;
    }
    if (op == 4) {
        for (int i = 0; out && i < 5 && i < cap; ++i) out[i] = (int64_t)(g_chisq_phase[i] * 1e9);
        return 5;
    }
    return -1;
}

}  // extern "C"
