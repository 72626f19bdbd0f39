// LinearCorrelation, many tests per call (pbn_ci_pvalue_batch_fn over a pbn_lincor handle): one test per lane.
//
// A constraint-based search asks for 10^5 ... 10^6 partial correlations per level, each a symmetric eigenproblem of k + 2 <= 8
// variables taken out of the covariance the handle already keeps.  The kernel is specialised on M = k + 2: the upper triangle of the
// block and rows 0 and 1 of the eigenvector matrix (all that cor_svd reads) are M (M + 1) / 2 + 2 M doubles per lane, indexed by
// compile-time constants only - a dynamically indexed per-lane array would live in scratch memory - and every rotation of a cyclic
// Jacobi sweep is straight-line code.  Tests are grouped by k on the host, so that a wave runs one specialisation.
//
// The arithmetic restates lincor_pvalue (mmpc.hip) rule for rule - cor_0cond's variance guard, the sweep order and the convergence
// criterion of jacobi_eigh, the k d_max eps threshold of the pseudo-inverse, the clamp, the degrees of freedom - and calls the SAME
// Student-t tail (lincor.hpp).  It keeps one triangle where the host keeps both, sums the pseudo-inverse in index order where the host
// sorts the eigenvalues first, and is contracted to FMAs: p-values agree to rounding, not bit for bit.  Where rounding could decide
// - an eigenvalue within REDO_FACTOR of the threshold, which is every singular block - the lane flags its test and the batch function
// recomputes it with the host routine before it returns.  Everything is fp64 on the vector ALU; there is no matrix-unit work here.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "lincor.hpp"

using namespace pbn;
using namespace pbn::lincor;

namespace {

constexpr int BLOCK = 256;

template <int M>
struct Tri {   // upper triangle, row-major: (i, j) with i <= j
    static constexpr int SIZE = M * (M + 1) / 2;
    static constexpr __host__ __device__ int at(int i, int j) { return i <= j ? i * M - i * (i - 1) / 2 + (j - i) : j * M - j * (j - 1) / 2 + (i - j); }
};

// idx: M rows of n_tests variable indices (v1, v2, the conditioning set), test-fastest so that a wave's loads coalesce
template <int M>
__global__ __launch_bounds__(BLOCK) void lincor_batch_kernel(const double* __restrict__ cov, int n, long long rows, int n_tests,
                                                              const int* __restrict__ idx, double* __restrict__ out,
                                                              unsigned char* __restrict__ flag) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= n_tests) return;
    int v[M];
#pragma unroll
    for (int i = 0; i < M; ++i) v[i] = idx[(size_t)i * n_tests + t];
    double a[Tri<M>::SIZE];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = i; j < M; ++j) a[Tri<M>::at(i, j)] = cov[v[i] + (size_t)v[j] * n];
    if constexpr (M == 2) {   // cor_0cond
        double cor = 0;
        if (!(a[Tri<2>::at(0, 0)] < MACHINE_TOL || a[Tri<2>::at(1, 1)] < MACHINE_TOL))
            cor = fmin(1.0, fmax(-1.0, a[Tri<2>::at(0, 1)] / sqrt(a[Tri<2>::at(0, 0)] * a[Tri<2>::at(1, 1)])));
        out[t] = cor_pvalue(cor, test_df(rows, 0));
        flag[t] = 0;
        return;
    } else {
        double u0[M], u1[M];
#pragma unroll
        for (int i = 0; i < M; ++i) { u0[i] = i == 0 ? 1.0 : 0.0; u1[i] = i == 1 ? 1.0 : 0.0; }
        for (int sweep = 0; sweep < 64; ++sweep) {
            double off = 0.0, diag = 0.0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                diag += a[Tri<M>::at(i, i)] * a[Tri<M>::at(i, i)];
#pragma unroll
                for (int j = i + 1; j < M; ++j) off += a[Tri<M>::at(i, j)] * a[Tri<M>::at(i, j)];
            }
            if (off <= 1e-34 * diag || off == 0.0) break;
#pragma unroll
            for (int p = 0; p < M - 1; ++p)
#pragma unroll
                for (int q = p + 1; q < M; ++q) {
                    const double apq = a[Tri<M>::at(p, q)];
                    if (apq == 0.0) continue;
                    const double app = a[Tri<M>::at(p, p)], aqq = a[Tri<M>::at(q, q)];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
                    for (int r = 0; r < M; ++r) {
                        if (r == p || r == q) continue;
                        const double arp = a[Tri<M>::at(r, p)], arq = a[Tri<M>::at(r, q)];
                        a[Tri<M>::at(r, p)] = c * arp - s * arq;
                        a[Tri<M>::at(r, q)] = s * arp + c * arq;
                    }
                    // the 2 x 2 block: columns p, q first, then rows p, q, as the host's two passes do
                    const double app1 = c * app - s * apq, apq1 = s * app + c * apq;
                    const double aqp1 = c * apq - s * aqq, aqq1 = s * apq + c * aqq;
                    a[Tri<M>::at(p, p)] = c * app1 - s * aqp1;
                    a[Tri<M>::at(p, q)] = c * apq1 - s * aqq1;
                    a[Tri<M>::at(q, q)] = s * apq1 + c * aqq1;
                    const double u0p = u0[p], u0q = u0[q], u1p = u1[p], u1q = u1[q];
                    u0[p] = c * u0p - s * u0q; u0[q] = s * u0p + c * u0q;
                    u1[p] = c * u1p - s * u1q; u1[q] = s * u1p + c * u1q;
                }
        }
        // cor_svd (linearcorrelation.hpp:29-47): partial correlation of the first two variables from the pseudo-inverse
        double dmax = a[Tri<M>::at(0, 0)], dmin = dmax;
#pragma unroll
        for (int i = 1; i < M; ++i) { dmax = fmax(dmax, a[Tri<M>::at(i, i)]); dmin = fmin(dmin, a[Tri<M>::at(i, i)]); }
        const double tol = M * dmax * 2.220446049250313e-16;
        double p11 = 0, p12 = 0, p22 = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const double d = a[Tri<M>::at(i, i)];
            if (d > tol) {
                const double inv = 1.0 / d;
                p11 += u0[i] * u0[i] * inv;
                p12 += u0[i] * u1[i] * inv;
                p22 += u1[i] * u1[i] * inv;
            }
        }
        double cor = 0;
        if (!(p11 < MACHINE_TOL || p22 < MACHINE_TOL)) cor = fmin(1.0, fmax(-1.0, -p12 / sqrt(p11 * p22)));
        out[t] = cor_pvalue(cor, test_df(rows, M - 2));
        flag[t] = !(dmin >= REDO_FACTOR * tol);   // (a NaN block is flagged as well)
    }
}

template <int M>
void launch(pbn_lincor* h, int cnt) {
    hipLaunchKernelGGL(lincor_batch_kernel<M>, dim3((unsigned)ceil_div(cnt, BLOCK)), dim3(BLOCK), 0, h->ctx->stream, h->dcov.p, h->n,
                       (long long)h->rows, cnt, h->d_idx.p, h->d_out.p, h->d_flag.p);
}

bool valid(const pbn_lincor* h, int v1, int v2, int k, const int* cond) {
    if (v1 < 0 || v2 < 0 || v1 >= h->n || v2 >= h->n || k < 0) return false;
    for (int i = 0; i < k; ++i)
        if (cond[i] < 0 || cond[i] >= h->n) return false;
    return true;
}

constexpr int CHUNK = 1 << 22;   // tests per launch: 128 MB of indices at M = 8

// the tests `which` (all of k conditioning variables) on the device; flagged ones again on the host
void device_group(pbn_lincor* h, int k, const std::vector<int>& which, const int* v1, const int* v2, const int* cond_off, const int* cond,
                  double* out) {
    const int m = k + 2;
    std::vector<int> idx;
    std::vector<double> res;
    std::vector<unsigned char> flg;
    for (size_t base = 0; base < which.size(); base += CHUNK) {
        const int cnt = (int)std::min<size_t>(CHUNK, which.size() - base);
        idx.resize((size_t)m * cnt);
        for (int j = 0; j < cnt; ++j) {
            const int t = which[base + j];
            idx[j] = v1[t];
            idx[(size_t)cnt + j] = v2[t];
            for (int i = 0; i < k; ++i) idx[(size_t)(i + 2) * cnt + j] = cond[cond_off[t] + i];
        }
        h->d_idx.reserve(idx.size());
        h->d_out.reserve(cnt);
        h->d_flag.reserve(cnt);
        hipStream_t st = h->ctx->stream;
        HIP_CHECK(hipMemcpyAsync(h->d_idx.p, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice, st));
        switch (m) {
            case 2: launch<2>(h, cnt); break;
            case 3: launch<3>(h, cnt); break;
            case 4: launch<4>(h, cnt); break;
            case 5: launch<5>(h, cnt); break;
            case 6: launch<6>(h, cnt); break;
            case 7: launch<7>(h, cnt); break;
            case 8: launch<8>(h, cnt); break;
            default: throw invalid_error("pbn_lincor_pvalue_batch: no device kernel for this conditioning-set size");
        }
        static_assert(K_DEV + 2 == 8, "one specialisation per k = 0 ... K_DEV");
        HIP_CHECK(hipGetLastError());
        res.resize(cnt);
        flg.resize(cnt);
        HIP_CHECK(hipMemcpyAsync(res.data(), h->d_out.p, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(flg.data(), h->d_flag.p, (size_t)cnt, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        for (int j = 0; j < cnt; ++j) {
            const int t = which[base + j];
            if (flg[j]) {
                out[t] = lincor_pvalue(h, v1[t], v2[t], k, cond + cond_off[t]);
                ++h->host_redone;
            } else {
                out[t] = res[j];
            }
        }
        h->device_tests += cnt;
    }
}

}  // namespace

extern "C" {

// pbn_ci_pvalue_batch_fn over a pbn_lincor handle (user = the handle); NaN for a test with bad indices.
void pbn_lincor_pvalue_batch(void* user, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out) {
    pbn_lincor* h = (pbn_lincor*)user;
    if (!out || n_tests <= 0) return;
    for (int i = 0; i < n_tests; ++i) out[i] = std::nan("");
    if (!h || !v1 || !v2 || !cond_off) return;
    (void)guarded(mu_of(h), [&] {
        std::vector<std::vector<int>> by_k(K_DEV + 1);
        std::vector<int> host;
        for (int t = 0; t < n_tests; ++t) {
            const int k = cond_off[t + 1] - cond_off[t];
            if ((k > 0 && !cond) || !valid(h, v1[t], v2[t], k, cond ? cond + cond_off[t] : nullptr)) continue;   // stays NaN
            if (h->ctx && k <= K_DEV) by_k[k].push_back(t);
            else host.push_back(t);
        }
        if (h->ctx) HIP_CHECK(hipSetDevice(h->ctx->device));
        for (int k = 0; k <= K_DEV; ++k) {
            std::vector<int>& g = by_k[k];
            if (g.empty()) continue;
            // small groups are not worth a launch and two copies; few degrees of freedom need lgamma(), which the device has not
            const bool dev = (int64_t)g.size() >= h->batch_threshold && 0.5 * (double)test_df(h->rows, k) >= LGAMMA_SERIES_MIN;
            if (dev) device_group(h, k, g, v1, v2, cond_off, cond, out);
            else host.insert(host.end(), g.begin(), g.end());
        }
        for (int t : host) out[t] = lincor_pvalue(h, v1[t], v2[t], cond_off[t + 1] - cond_off[t], cond ? cond + cond_off[t] : nullptr);
        h->host_tests += (int64_t)host.size();
    });
}

int pbn_lincor_batch_stats(const pbn_lincor* h, int64_t* device_tests, int64_t* host_tests, int64_t* host_redone) {
    return guarded(mu_of(h), [&] {
        if (!h) throw invalid_error("pbn_lincor_batch_stats: null argument");
        if (device_tests) *device_tests = h->device_tests;
        if (host_tests) *host_tests = h->host_tests;
        if (host_redone) *host_redone = h->host_redone;
    });
}

int pbn_lincor_set_batch_threshold(pbn_lincor* h, int64_t min_tests) {
    return guarded(mu_of(h), [&] {
        if (!h || min_tests < 0) throw invalid_error("pbn_lincor_set_batch_threshold: bad argument");
        h->batch_threshold = min_tests;
    });
}

int pbn_lincor_batch_max_cond(void) { return K_DEV; }

}  // extern "C"
