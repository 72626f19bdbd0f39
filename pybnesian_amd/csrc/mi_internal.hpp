// The pbn_mi handle (mi.hip) as the other independence tests over it see it - ChiSquare (chisq.hip) and the null-aware
// LinearCorrelation (lincor.hip): the handle, its row groupings, and the two services of mi.hip they build on.
#pragma once
#include <functional>
#include <map>
#include <memory>
#include <vector>

#include "common.hpp"
#include "joint_counts.hpp"

// Rows grouped by the configuration of one set of discrete variables (sorted ids, first id fastest): `perm` lists the
// rows configuration by configuration, ascending inside a configuration (stable radix sort), `off` are the segment
// bounds = the counts, `blk` cuts every segment into pieces of at most MI_SORTED_ROWS rows.  Built once per set and
// reused by every test over it; the set of no variables is the identity (perm empty).
struct DiscGroup {
    std::vector<int> vars;
    int G = 1;
    pbn::dev_buf<int32_t> perm;     // [N]
    std::vector<int64_t> off;       // [G + 1]
    pbn::dev_buf<int32_t> blk;      // [nblk][4]: configuration, first position, end position, unused
    std::vector<int> blk_off;       // [G + 1] first block of every configuration
    int nblk = 0;
    uint64_t stamp = 0;
    // configuration id in this grouping's order -> id in a test's own (x, y, z...) order, per variable order seen
    std::map<std::vector<int>, std::vector<int>> order_maps;
    // per configuration, the pilot-shifted sums and products of ALL continuous columns (Engine::ensure_full): every test over
    // this set of discrete variables reads its moments out of them
    bool full_ready = false;
    std::vector<double> fullS, fullP;   // [G][nc], [G][nc][nc]
    // how ensure_full launched the pass (read by the test aid pbn_debug_mi_moments only): the kernel family - 0 gram_gring_kernel gathering
    // from the columns, 1 the same through the row-major mirror, 2 the contiguous gram_glds kernels -, the blocks launched (padding
    // included) and the order of the pieces - 0 stripe-major, 1 stripe-major aligned in groups of 8, 2 the partial slots' own
    int full_form = -1, full_launched = 0, full_order = -1;
};

struct pbn_mi {
    pbn::ctx_ptr ctx;
    const pbn_table* table = nullptr;  // continuous columns (borrowed), null when there are none
    int n_cont = 0, n_disc = 0;
    int64_t N = 0;
    bool asymptotic = true;
    std::vector<int> card;
    std::vector<char> disc_null, cont_null;   // columns holding nulls: code == card[j] / NaN; such rows drop out of a test
    bool any_null = false;
    pbn::dev_buf<int32_t> codes_dev;          // [n_disc][N]
    std::vector<double> shift;                // pilot mean of every continuous column
    int64_t device_passes = 0, host_passes = 0, device_launches = 0;
    std::vector<int> order;  // external index -> variable id for the callback form (empty = identity)
    std::map<std::vector<int>, std::unique_ptr<DiscGroup>> groups;
    uint64_t clock = 0;
    int64_t groups_built = 0, count_only = 0;
    pbn::dev_buf<int32_t> iota;       // [N] 0..N-1, the values the radix sort permutes
    pbn::dev_buf<uint32_t> keys[2];   // [N] configuration ids, unsorted / sorted
    pbn::dev_buf<int32_t> first;      // [G] first sorted position of every configuration
    pbn::dev_buf<char> sort_tmp;
    pbn::dev_buf<double> shift_dev;   // the pilot means on the device, indexed by table column (Engine::ensure_full)
    pbn::dev_buf<char> rowmajor;      // row-major mirror of the continuous columns for the gathered Gram of the groupings (Engine::ensure_full)
    bool rowmajor_tried = false;
    int64_t full_grams = 0;      // groupings whose full per-configuration moments were taken
    size_t full_bytes_held = 0;  // host bytes of the cached full moments
    // PBN_MI_TIMING=1: wall seconds per phase, printed when the handle is destroyed
    double t_group = 0, t_device = 0, t_host = 0, t_prep = 0;
    int64_t batches = 0;
    // test aid (pbn_debug_mi_moments, mi.hip): non-null only inside its call - one record per plan of the batch, filled by group_stats_many
    std::vector<int64_t>* dbg = nullptr;
    // pbn_chisq_pvalue_batch (chisq.hip): the byte mirror of the codes ([n_disc][ld8], built by the first batch when every code fits a
    // byte) and the scratch of a launch chunk (joint_counts.hpp)
    struct ChisqState {
        pbn::dev_buf<uint8_t> codes8;
        int64_t ld8 = 0;
        int codes8_state = 0;        // 0 not tried yet, 1 built, -1 the codes need int32
        pbn::joint::Scratch scratch;
        int64_t device_tests = 0, host_tests = 0;
        int64_t threshold = -1;      // pbn_chisq_set_batch_threshold; negative: not set, chisq.hip's CHISQ_BATCH_MIN_TESTS
    } cs;
    // the count-only tests of pbn_mi_pvalue_batch (mi.hip): counted through the same mirror and scratch (cs above, under the context's
    // lock); the counters of pbn_mi_discrete_batch_stats
    struct DiscreteBatchState {
        int64_t device_tests = 0, cached_tests = 0, grouped_tests = 0;
        int64_t threshold = -1;      // pbn_mi_discrete_set_batch_threshold; negative: not set, mi.hip's MI_DISCRETE_BATCH_MIN_TESTS
    } db;
    // pbn_mi_lincor_pvalue_batch (lincor_null_batch.hip): the split of the table's rows into clean ones (no NaN in any continuous
    // column: one Gram of all columns serves every test) and dirty ones (kept as a compact row-major copy that the per-test kernel
    // walks), built by the first batch; the grow-only buffers of a launch chunk; the counters of pbn_mi_lincor_batch_stats
    struct LincorNullState {
        bool ready = false;
        int64_t n_clean = 0, n_dirty = 0;
        pbn::dev_buf<char> dirty;        // [n_dirty][n_cont] in the table's dtype
        pbn::dev_buf<double> clean;      // count, n_cont sums, n_cont x n_cont products of x - shift over the clean rows
        pbn::dev_buf<double> shift;      // [n_cont]: h->shift as the state was built with it
        pbn::dev_buf<int> idx;
        pbn::dev_buf<double> part, out, rec;
        pbn::dev_buf<unsigned char> flag;
        int64_t device_tests = 0, host_tests = 0, host_redone = 0;
        int64_t threshold = -1;          // pbn_mi_lincor_set_batch_threshold; negative: not set, LINCOR_NULL_BATCH_MIN_TESTS
    } ln;
};

namespace pbn {
namespace mi {

// Per-configuration statistics of one test over the continuous variables `cont` and the discrete variables `disc` (variable ids; the
// first discrete variable fastest): per configuration the count, the sums and the upper-triangle products of the pilot-shifted
// continuous variables.  With nulls the count is that of the rows valid in every variable of the test.
void group_stats(pbn_mi* h, const std::vector<int>& cont, const std::vector<int>& disc, std::vector<double>& out);

// vars = [v1, v2, cond...] as variable ids: through the handle's order (pbn_mi_set_order) when one is set, else as given.  false when
// an index lies outside the order.  No kind check and no message: every entry point refuses in its own words.
bool map_request(const pbn_mi* h, int v1, int v2, int n_cond, const int* cond, std::vector<int>& vars);

// One table of a batch call that counts on the device: ChiSquare's contingency tables (chisq.hip) and the count-only tests of
// pbn_mi_pvalue_batch (mi.hip).
struct CountTest {
    int m = 0;
    int vars[joint::MAX_VARS];   // variable ids, x, y, Z: the first fastest
    int G = 0;                   // prod card
    int where = -1;              // the caller's: where the test ran
    int slices = 0, copies = 0;  // as launched (copies 0: the global form)
};

constexpr int COUNT_LDS_MAX_CELLS = 4096;   // larger tables take the kernel's global-atomics form

// The tables of the tests `which` (indices into `tests`; m, vars and G set, every variable categorical and named once) under the
// BY_CARD policy, launch chunk by launch chunk: the byte mirror of the handle built on first use, a descriptor per test (its columns in
// the test's own order, strides of card), plan_slices, joint::run_chunk.  After every chunk `finish(base, T, descs, counts)` gets the
// tests which[base .. base + T), their descriptors and the count buffer on the host: the table of test i starts at
// counts[descs[i].table_off].  `phase`, when set, is run_chunk's after_step.  Returns the code width in bytes (1 the mirror, 4 int32).
// The caller holds the context's lock: the mirror and the scratch are the handle's (pbn_mi::cs).
int count_tables(pbn_mi* h, std::vector<CountTest>& tests, const std::vector<int>& which, const std::function<void(int)>& phase,
                 const std::function<void(size_t base, int T, const std::vector<joint::Desc>& descs, const uint32_t* counts)>& finish);

}  // namespace mi
}  // namespace pbn
