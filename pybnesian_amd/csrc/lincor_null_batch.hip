// LinearCorrelation on a table with nulls, many tests per call (pbn_ci_pvalue_batch_fn over a pbn_mi handle whose variables are all
// continuous; continuous/linearcorrelation.cpp:20-122, the pvalue_impl branch).
//
// Every test takes the covariance of ITS variables over the rows valid in all of them.  The rows split in two.  A CLEAN row - no NaN in
// any continuous column of the handle - is valid for every test: its share of a test's moments is an entry of one pilot-shifted Gram
// of all columns over the clean rows, taken once per handle on the f64 matrix-unit Gram kernels (score::gram_raw through the list of
// clean rows).  Only the DIRTY rows need work per test, and they are kept as a compact row-major copy [n_dirty][n_cont].
//
// lincor_null_moments_kernel<T, M>: a workgroup owns CHUNK tests, one per lane, and one slice of the dirty rows.  It stages TILE rows
// of ALL columns in LDS and every lane reads its M = k + 2 columns of a row from there - a wave reads one row at a time, so lanes on
// the same column share a broadcast and the row stride cannot make two lanes collide (only columns 32 doubles apart do, in any
// layout).  The 1 + M + M (M + 1) / 2 accumulators - count, sums, upper triangle of products of x - shift - are fp64 registers indexed
// by compile-time constants.  A row is valid when x == x for all M values; an invalid row's values are replaced by the shifts with a
// select before any arithmetic, so it adds +0.0 to everything.  Order of additions: a lane adds the rows of its slice in row order;
// lincor_null_finish_kernel<M> adds a test's slices in slice order, then the clean part.  The slice length depends on n_dirty alone
// (lincor_null_host.hpp), there are no atomics: a test's numbers do not depend on the batch, its place in it, or the launch chunking.
//
// The finish kernel forms the covariance as the scalar routine does, (G_ij - S_i S_j / n) / (n - 1), and runs block_pvalue
// (lincor_device.hpp), the per-lane eigenproblem and Student-t tail lincor_batch_kernel runs, with the test's own valid count.  Tests
// that rounding could decide (flag 1) and tests the device tail does not cover - fewer than LGAMMA_SERIES_MIN half degrees of freedom,
// not more valid rows than variables (flag 2) - go through pbn_mi_lincor_pvalue before the call returns.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "lincor.hpp"
#include "lincor_device.hpp"
#include "lincor_null_host.hpp"
#include "mi_internal.hpp"
#include "scoring_internal.hpp"

using namespace pbn;
using namespace pbn::lincor;
using namespace pbn::lincor_null;

extern "C" double pbn_mi_lincor_pvalue(void* user, int v1, int v2, int n_cond, const int* cond);

namespace {

// 64 x the largest relative difference between this batch and the scalar routine over p-values in [alpha / 4, 4 alpha], alpha in
// {0.01, 0.05, 0.1}: measured 2.96e-12 on the float64 table and 5.21e-12 on the float32 one of tests/test_lincor_null_batch_gpu.py
constexpr double LINCOR_NULL_BAND = 3.4e-10;
constexpr int64_t PART_BUDGET = 256ll << 20;   // bytes of slice partials per launch
constexpr int64_t LAUNCH_MAX = 1 << 22;        // tests per launch

template <int M>
constexpr int acc_size() { return 1 + M + Tri<M>::SIZE; }

template <typename T>
__global__ __launch_bounds__(256) void dirty_mask_kernel(const T* __restrict__ base, int64_t ld, int nc, int64_t n, unsigned char* __restrict__ mask) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    bool bad = false;
    for (int c = 0; c < nc; ++c) { const T x = base[(int64_t)c * ld + r]; bad = bad || !(x == x); }
    mask[r] = bad ? 1 : 0;
}

// out[i][c] = column c of row rows[i]
template <typename T>
__global__ __launch_bounds__(256) void take_rows_kernel(const T* __restrict__ base, int64_t ld, int nc, const int32_t* __restrict__ rows, int64_t n,
                                                        T* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i];
    for (int c = 0; c < nc; ++c) out[i * nc + c] = base[(int64_t)c * ld + r];
}

// idx: M rows of n_tests variable ids, test-fastest.  part: [slice][accumulator][test].  grid (chunks, slices); LDS TILE * nc * sizeof(T).
template <typename T, int M>
__global__ __launch_bounds__(CHUNK) void lincor_null_moments_kernel(const T* __restrict__ dirty, int n_dirty, int nc, int slice_len,
                                                                    const double* __restrict__ shift, int n_tests, const int* __restrict__ idx,
                                                                    double* __restrict__ part) {
    extern __shared__ double lds_raw[];
    T* tile = reinterpret_cast<T*>(lds_raw);
    const int t = blockIdx.x * CHUNK + threadIdx.x;
    const int tt = t < n_tests ? t : n_tests - 1;   // a lane past the batch shadows the last test: it takes part in the barriers, writes nothing
    int v[M];
    double sh[M];
#pragma unroll
    for (int i = 0; i < M; ++i) { v[i] = idx[(size_t)i * n_tests + tt]; sh[i] = shift[v[i]]; }
    double cnt = 0.0, s[M], p[Tri<M>::SIZE];
#pragma unroll
    for (int i = 0; i < M; ++i) s[i] = 0.0;
#pragma unroll
    for (int i = 0; i < Tri<M>::SIZE; ++i) p[i] = 0.0;
    const int r0 = blockIdx.y * slice_len, r1 = min(n_dirty, r0 + slice_len);
    for (int base = r0; base < r1; base += TILE) {
        const int rows = min(TILE, r1 - base), elems = rows * nc;
        const T* src = dirty + (size_t)base * nc;
        __syncthreads();   // the previous tile has been read by every lane
        for (int e = threadIdx.x; e < elems; e += CHUNK) tile[e] = src[e];
        __syncthreads();
        const T* row = tile;
        for (int r = 0; r < rows; ++r, row += nc) {
            double x[M];
            bool ok = true;
#pragma unroll
            for (int i = 0; i < M; ++i) { x[i] = (double)row[v[i]]; ok = ok && (x[i] == x[i]); }
            double d[M];
#pragma unroll
            for (int i = 0; i < M; ++i) d[i] = (ok ? x[i] : sh[i]) - sh[i];   // an invalid row: +0.0, no arithmetic on its values
            cnt += ok ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < M; ++i) s[i] += d[i];
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int j = i; j < M; ++j) p[Tri<M>::at(i, j)] += d[i] * d[j];
        }
    }
    if (t >= n_tests) return;
    constexpr int ACC = acc_size<M>();
    double* o = part + (size_t)blockIdx.y * ACC * n_tests + t;
    o[0] = cnt;
#pragma unroll
    for (int i = 0; i < M; ++i) o[(size_t)(1 + i) * n_tests] = s[i];
#pragma unroll
    for (int i = 0; i < Tri<M>::SIZE; ++i) o[(size_t)(1 + M + i) * n_tests] = p[i];
}

// clean: [1 + nc + nc * nc] count, sums, products (col-major) over the clean rows.  rec (nullable, test aid): per test the clean part, the
// dirty part and their sum, 3 x ACC doubles.  flag: 0 the p-value stands, 1 recompute on the host, 2 a test the device tail does not cover.
template <int M>
__global__ __launch_bounds__(CHUNK) void lincor_null_finish_kernel(const double* __restrict__ part, int n_slices, const double* __restrict__ clean,
                                                                   int nc, int n_tests, const int* __restrict__ idx, double* __restrict__ out,
                                                                   unsigned char* __restrict__ flag, double* __restrict__ rec) {
    const int t = blockIdx.x * CHUNK + threadIdx.x;
    if (t >= n_tests) return;
    constexpr int ACC = acc_size<M>();
    int v[M];
#pragma unroll
    for (int i = 0; i < M; ++i) v[i] = idx[(size_t)i * n_tests + t];
    double sum[ACC];   // the dirty part first: the slices in slice order
#pragma unroll
    for (int a = 0; a < ACC; ++a) sum[a] = 0.0;
    for (int sl = 0; sl < n_slices; ++sl) {
        const double* o = part + (size_t)sl * ACC * n_tests + t;
#pragma unroll
        for (int a = 0; a < ACC; ++a) sum[a] += o[(size_t)a * n_tests];
    }
    // sum = clean + dirty, in that order, in place (the test aid's records leave as they are formed)
    double* o = rec ? rec + (size_t)t * 3 * ACC : nullptr;
    auto add_clean = [&](int a, double c) {
        if (o) { o[a] = c; o[ACC + a] = sum[a]; }
        sum[a] = c + sum[a];
        if (o) o[2 * ACC + a] = sum[a];
    };
    add_clean(0, clean[0]);
#pragma unroll
    for (int i = 0; i < M; ++i) add_clean(1 + i, clean[1 + v[i]]);
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) add_clean(1 + M + Tri<M>::at(i, j), clean[1 + nc + v[i] + (size_t)v[j] * nc]);
    const double n = sum[0];
    if (!(n > (double)M) || 0.5 * (double)test_df((long long)n, M - 2) < LGAMMA_SERIES_MIN) {
        out[t] = __builtin_nan("");
        flag[t] = 2;
        return;
    }
    double a[Tri<M>::SIZE];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) a[Tri<M>::at(i, j)] = (sum[1 + M + Tri<M>::at(i, j)] - sum[1 + i] * sum[1 + j] / n) / (n - 1.0);
    bool redo;
    const double pv = block_pvalue<M>(a, (long long)n, redo);
    out[t] = pv;
    flag[t] = (redo || !(pv == pv)) ? 1 : 0;   // a NaN - a block holding one - is the scalar routine's to report
}

template <typename T, int M>
void launch_moments(pbn_mi* h, int cnt, int n_slices, int slice_len) {
    auto& ln = h->ln;
    const size_t lds = (size_t)TILE * h->n_cont * sizeof(T);
    hipLaunchKernelGGL((lincor_null_moments_kernel<T, M>), dim3((unsigned)ceil_div(cnt, CHUNK), (unsigned)n_slices), dim3(CHUNK), lds, h->ctx->stream,
                       (const T*)ln.dirty.p, (int)ln.n_dirty, h->n_cont, slice_len, ln.shift.p, cnt, ln.idx.p, ln.part.p);
}

template <int M>
void launch(pbn_mi* h, int cnt, int n_slices, int slice_len, double* rec) {
    auto& ln = h->ln;
    if (n_slices > 0) {
        if (h->table->dtype == PBN_F64) launch_moments<double, M>(h, cnt, n_slices, slice_len);
        else launch_moments<float, M>(h, cnt, n_slices, slice_len);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(lincor_null_finish_kernel<M>, dim3((unsigned)ceil_div(cnt, CHUNK)), dim3(CHUNK), 0, h->ctx->stream, ln.part.p, n_slices,
                       ln.clean.p, h->n_cont, cnt, ln.idx.p, ln.out.p, ln.flag.p, rec);
    HIP_CHECK(hipGetLastError());
}

bool device_applies(const pbn_mi* h) {
    return h->table && h->n_disc == 0 && h->n_cont >= 2 && h->n_cont <= NC_MAX && h->N > 0 && h->N < (int64_t)1 << 30;
}

// the row split, the compact dirty rows and the clean rows' moments, once per handle (and again after the shifts changed)
void ensure_state(pbn_mi* h) {
    auto& ln = h->ln;
    if (ln.ready) return;
    const pbn_table* t = h->table;
    pbn_ctx* ctx = h->ctx;
    hipStream_t st = ctx->stream;
    const int nc = h->n_cont;
    const int64_t N = h->N;
    const bool f64 = t->dtype == PBN_F64;
    dev_buf<unsigned char> dmask((size_t)N);
    const unsigned grid = (unsigned)ceil_div(N, 256);
    if (f64) hipLaunchKernelGGL(dirty_mask_kernel<double>, dim3(grid), dim3(256), 0, st, (const double*)t->data, t->ld, nc, N, dmask.p);
    else hipLaunchKernelGGL(dirty_mask_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)t->data, t->ld, nc, N, dmask.p);
    HIP_CHECK(hipGetLastError());
    std::vector<unsigned char> mask((size_t)N);
    HIP_CHECK(hipMemcpyAsync(mask.data(), dmask.p, (size_t)N, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    std::vector<int32_t> clean_rows, dirty_rows;
    partition_rows(mask.data(), N, clean_rows, dirty_rows);
    ln.n_clean = (int64_t)clean_rows.size();
    ln.n_dirty = (int64_t)dirty_rows.size();
    ln.shift.alloc((size_t)nc);
    HIP_CHECK(hipMemcpyAsync(ln.shift.p, h->shift.data(), (size_t)nc * sizeof(double), hipMemcpyHostToDevice, st));
    ln.dirty.alloc(std::max<size_t>(1, (size_t)ln.n_dirty * nc * dtype_size(t->dtype)));
    if (ln.n_dirty > 0) {
        dev_buf<int32_t> drows((size_t)ln.n_dirty);
        HIP_CHECK(hipMemcpyAsync(drows.p, dirty_rows.data(), (size_t)ln.n_dirty * sizeof(int32_t), hipMemcpyHostToDevice, st));
        const unsigned g = (unsigned)ceil_div(ln.n_dirty, 256);
        if (f64) hipLaunchKernelGGL(take_rows_kernel<double>, dim3(g), dim3(256), 0, st, (const double*)t->data, t->ld, nc, drows.p, ln.n_dirty, (double*)ln.dirty.p);
        else hipLaunchKernelGGL(take_rows_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)t->data, t->ld, nc, drows.p, ln.n_dirty, (float*)ln.dirty.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));   // drows goes out of scope
    }
    std::vector<double> cl((size_t)1 + nc + (size_t)nc * nc, 0.0);
    cl[0] = (double)ln.n_clean;
    if (ln.n_clean > 0) {
        dev_buf<int32_t> crows((size_t)ln.n_clean);
        HIP_CHECK(hipMemcpyAsync(crows.p, clean_rows.data(), (size_t)ln.n_clean * sizeof(int32_t), hipMemcpyHostToDevice, st));
        // 32-column blocks so that every pair of columns meets in one Gram launch (<= 64 columns per launch), as pbn_lincor_create does
        std::vector<int> cols;
        std::vector<double> S, G;
        const int nb = (nc + 31) / 32;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi + (nb > 1 ? 1 : 0); bj < nb; ++bj) {
                cols.clear();
                for (int c = bi * 32; c < std::min(nc, bi * 32 + 32); ++c) cols.push_back(c);
                if (bj != bi)
                    for (int c = bj * 32; c < std::min(nc, bj * 32 + 32); ++c) cols.push_back(c);
                const int d = (int)cols.size();
                S.assign((size_t)d, 0.0);
                G.assign((size_t)d * d, 0.0);
                score::gram_raw(t, cols.data(), d, 0, ln.n_clean, crows.p, ln.shift.p, S.data(), G.data());   // synchronises
                for (int i = 0; i < d; ++i) cl[(size_t)1 + cols[i]] = S[i];
                for (int j = 0; j < d; ++j)
                    for (int i = 0; i < d; ++i) cl[(size_t)1 + nc + cols[i] + (size_t)cols[j] * nc] = G[i + (size_t)j * d];
            }
    }
    ln.clean.alloc(cl.size());
    HIP_CHECK(hipMemcpyAsync(ln.clean.p, cl.data(), cl.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ln.ready = true;
}

// the tests `which` (all of k conditioning variables; vars: their variable ids, M per test) on the device.  out / flags per test of
// `which`; recs (nullable): the raw records of the test aid, 3 x ACC doubles per test.
void device_group(pbn_mi* h, int k, const std::vector<int>& which, const std::vector<int>& vars, const std::vector<int>& var_off, double* out,
                  unsigned char* flags, std::vector<std::vector<double>>* recs) {
    auto& ln = h->ln;
    const int m = k + 2, acc = 1 + m + m * (m + 1) / 2;
    const int n_slices = ln.n_dirty > 0 ? num_slices(ln.n_dirty) : 0;
    const int slice_len = (int)slice_rows(ln.n_dirty);
    const size_t per_launch = (size_t)std::min<int64_t>(LAUNCH_MAX, tests_per_launch(n_slices, acc, PART_BUDGET));
    hipStream_t st = h->ctx->stream;
    std::vector<int> idx;
    std::vector<double> res, rec;
    std::vector<unsigned char> flg;
    for (size_t base = 0; base < which.size(); base += per_launch) {
        const int cnt = (int)std::min(per_launch, which.size() - base);
        idx.resize((size_t)m * cnt);
        for (int j = 0; j < cnt; ++j) {
            const int* vv = vars.data() + var_off[which[base + j]];
            for (int i = 0; i < m; ++i) idx[(size_t)i * cnt + j] = vv[i];
        }
        ln.idx.reserve(idx.size());
        ln.out.reserve((size_t)cnt);
        ln.flag.reserve((size_t)cnt);
        ln.part.reserve(std::max<size_t>(1, (size_t)n_slices * acc * cnt));
        if (recs) ln.rec.reserve((size_t)3 * acc * cnt);
        HIP_CHECK(hipMemcpyAsync(ln.idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, st));
        double* drec = recs ? ln.rec.p : nullptr;
        switch (m) {
            case 2: launch<2>(h, cnt, n_slices, slice_len, drec); break;
            case 3: launch<3>(h, cnt, n_slices, slice_len, drec); break;
            case 4: launch<4>(h, cnt, n_slices, slice_len, drec); break;
            case 5: launch<5>(h, cnt, n_slices, slice_len, drec); break;
            case 6: launch<6>(h, cnt, n_slices, slice_len, drec); break;
            case 7: launch<7>(h, cnt, n_slices, slice_len, drec); break;
            case 8: launch<8>(h, cnt, n_slices, slice_len, drec); break;
            default: throw invalid_error("pbn_mi_lincor_pvalue_batch: no device kernel for this conditioning-set size");
        }
        static_assert(K_DEV + 2 == 8, "one specialisation per k = 0 ... K_DEV");
        res.resize((size_t)cnt);
        flg.resize((size_t)cnt);
        HIP_CHECK(hipMemcpyAsync(res.data(), ln.out.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(flg.data(), ln.flag.p, (size_t)cnt, hipMemcpyDeviceToHost, st));
        if (recs) {
            rec.resize((size_t)3 * acc * cnt);
            HIP_CHECK(hipMemcpyAsync(rec.data(), ln.rec.p, rec.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        }
        HIP_CHECK(hipStreamSynchronize(st));
        for (int j = 0; j < cnt; ++j) {
            const int t = which[base + j];
            out[t] = res[(size_t)j];
            flags[t] = flg[(size_t)j];
            if (recs) (*recs)[(size_t)t].assign(rec.begin() + (size_t)j * 3 * acc, rec.begin() + (size_t)(j + 1) * 3 * acc);
        }
    }
}

// The batch: out[t] for every test.  recs non-null (the test aid): every test must be one the device serves, whatever the threshold.
void run_batch(pbn_mi* h, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out,
               std::vector<std::vector<double>>* recs) {
    auto& ln = h->ln;
    // variable ids of every test through THE decoder of the handle's order; a test it refuses, or one over a variable that is not
    // continuous, is left to the scalar routine, which reports it in its own words
    std::vector<int> vars, var_off((size_t)n_tests + 1, 0), one;
    std::vector<unsigned char> ok((size_t)n_tests, 0);
    vars.reserve((size_t)n_tests * 2 + (size_t)cond_off[n_tests]);
    for (int t = 0; t < n_tests; ++t) {
        const int k = cond_off[t + 1] - cond_off[t];
        bool good = k >= 0 && (k == 0 || cond) && mi::map_request(h, v1[t], v2[t], k, k > 0 ? cond + cond_off[t] : nullptr, one);
        if (good)
            for (int v : one) good = good && v >= 0 && v < h->n_cont;
        if (good) { vars.insert(vars.end(), one.begin(), one.end()); ok[(size_t)t] = 1; }
        var_off[(size_t)t + 1] = (int)vars.size();
    }
    std::vector<std::vector<int>> by_k;
    std::vector<int> rest;
    const bool on = knob_int("PBN_LINCOR_NULL_BATCH", 1) != 0 && device_applies(h);   // read per call
    if (on) group_tests(n_tests, cond_off, ok.data(), K_DEV, by_k, rest);
    else { rest.resize((size_t)n_tests); for (int t = 0; t < n_tests; ++t) rest[(size_t)t] = t; }
    if (recs && !rest.empty()) throw invalid_error("pbn_debug_mi_lincor_moments: a test the device pass does not serve");
    std::vector<unsigned char> flags((size_t)n_tests, 0);
    if (on) {
        HIP_CHECK(hipSetDevice(h->ctx->device));
        const int64_t threshold = recs ? 0 : (ln.threshold < 0 ? LINCOR_NULL_BATCH_MIN_TESTS : ln.threshold);
        for (int k = 0; k <= K_DEV; ++k) {
            std::vector<int>& g = by_k[(size_t)k];
            if (g.empty()) continue;
            if ((int64_t)g.size() < threshold) { rest.insert(rest.end(), g.begin(), g.end()); continue; }
            ensure_state(h);
            device_group(h, k, g, vars, var_off, out, flags.data(), recs);
            int64_t host = 0, redo = 0;
            for (int t : g) {
                if (flags[(size_t)t] == 0) continue;
                (flags[(size_t)t] == 2 ? host : redo) += 1;
                out[t] = pbn_mi_lincor_pvalue(h, v1[t], v2[t], k, cond ? cond + cond_off[t] : nullptr);
            }
            ln.device_tests += (int64_t)g.size() - host;
            ln.host_tests += host;
            ln.host_redone += redo;
        }
    }
    for (int t : rest) {
        const int k = cond_off[t + 1] - cond_off[t];
        out[t] = pbn_mi_lincor_pvalue(h, v1[t], v2[t], k, cond ? cond + cond_off[t] : nullptr);
    }
    ln.host_tests += (int64_t)rest.size();
}

}  // namespace

extern "C" {

// pbn_ci_pvalue_batch_fn over a pbn_mi handle (user = the handle); indices go through pbn_mi_set_order's order.  NaN for a test the
// scalar routine refuses (pbn_last_error has the last reason).
void pbn_mi_lincor_pvalue_batch(void* user, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out) {
    pbn_mi* h = (pbn_mi*)user;
    if (!out || n_tests <= 0) return;
    for (int i = 0; i < n_tests; ++i) out[i] = std::nan("");
    (void)guarded([&] {
        if (!h || !v1 || !v2 || !cond_off) throw invalid_error("pbn_mi_lincor_pvalue_batch: null argument");
        run_batch(h, n_tests, v1, v2, cond_off, cond, out, nullptr);
    });
}

int pbn_mi_lincor_batch_stats(const pbn_mi* h, int64_t* device_tests, int64_t* host_tests, int64_t* host_redone, int64_t* clean_rows,
                              int64_t* dirty_rows) {
    return guarded([&] {
        if (!h) throw invalid_error("pbn_mi_lincor_batch_stats: null argument");
        if (device_tests) *device_tests = h->ln.device_tests;
        if (host_tests) *host_tests = h->ln.host_tests;
        if (host_redone) *host_redone = h->ln.host_redone;
        if (clean_rows) *clean_rows = h->ln.ready ? h->ln.n_clean : -1;
        if (dirty_rows) *dirty_rows = h->ln.ready ? h->ln.n_dirty : -1;
    });
}

int pbn_mi_lincor_set_batch_threshold(pbn_mi* h, int64_t min_tests) {
    return guarded([&] {
        if (!h || min_tests < 0) throw invalid_error("pbn_mi_lincor_set_batch_threshold: bad argument");
        h->ln.threshold = min_tests;
    });
}

double pbn_mi_lincor_band(void) { return LINCOR_NULL_BAND; }

// Test aid: the raw records of a batch, as pbn_mi_lincor_pvalue_batch takes it (same indices, same grouping and launches, but every
// group goes to the device whatever the threshold).  out receives up to `cap` doubles, per test in batch order three records of
// 1 + M + M (M + 1) / 2 doubles (M = its conditioning-set size + 2) - count, sums, upper triangle (i <= j, row-major) of the products of
// x - shift: over the clean rows, over the dirty rows valid in all of its variables, and their sum.  shape (nullable, 5 int64): the
// kernel's TILE, CHUNK and column cap, the handle's slice length and number of slices.  Returns the doubles all tests hold together, or -1
// after an error - a test the device pass does not serve among them (pbn_last_error).
int64_t pbn_debug_mi_lincor_moments(pbn_mi* h, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out,
                                    int64_t cap, int64_t* shape) {
    int64_t total = 0;
    const int rc = guarded([&] {
        if (!h || n_tests < 0 || !v1 || !v2 || !cond_off) throw invalid_error("pbn_debug_mi_lincor_moments: null argument");
        std::vector<std::vector<double>> recs((size_t)n_tests);
        std::vector<double> p((size_t)std::max(1, n_tests));
        if (n_tests > 0) run_batch(h, n_tests, v1, v2, cond_off, cond, p.data(), &recs);
        for (auto& r : recs)
            for (double v : r) { if (out && total < cap) out[total] = v; ++total; }
        if (shape) {
            shape[0] = TILE; shape[1] = CHUNK; shape[2] = NC_MAX;
            shape[3] = h->ln.ready ? slice_rows(h->ln.n_dirty) : -1;
            shape[4] = h->ln.ready ? (h->ln.n_dirty > 0 ? num_slices(h->ln.n_dirty) : 0) : -1;
        }
    });
    return rc == PBN_OK ? total : -1;
}

}  // extern "C"
