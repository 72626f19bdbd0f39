// The LinearCorrelation independence test (learning/independences/continuous/linearcorrelation.{hpp,cpp}): the partial correlation of
// two variables given a conditioning set from a covariance matrix, and its t-test.  Host arithmetic; the only O(N) work - the covariance
// of all continuous columns, or on a table with nulls that of one test's variables over the rows valid in all of them - is a pass of
// the Gram / moments kernels on the device.  (struct pbn_lincor and the Student-t tail shared with the device batch: lincor.hpp; the
// device batch: lincor_batch.hip.)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>

#include "common.hpp"
#include "lincor.hpp"
#include "mi_internal.hpp"

using namespace pbn;
using namespace pbn::lincor;

namespace {

// Symmetric eigen-decomposition by cyclic Jacobi rotations (k is the conditioning-set size + 2: a handful).
// Eigenvalues ascending in d, eigenvectors in the columns of u.
void jacobi_eigh(std::vector<double>& a, int k, std::vector<double>& d, std::vector<double>& u) {
    u.assign((size_t)k * k, 0.0);
    for (int i = 0; i < k; ++i) u[i + (size_t)i * k] = 1.0;
    auto A = [&](int i, int j) -> double& { return a[i + (size_t)j * k]; };
    auto U = [&](int i, int j) -> double& { return u[i + (size_t)j * k]; };
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < k; ++i) {
            diag += A(i, i) * A(i, i);
            for (int j = i + 1; j < k; ++j) off += A(i, j) * A(i, j);
        }
        if (off <= 1e-34 * diag || off == 0.0) break;
        for (int p = 0; p < k - 1; ++p)
            for (int q = p + 1; q < k; ++q) {
                if (A(p, q) == 0.0) continue;
                const double theta = (A(q, q) - A(p, p)) / (2.0 * A(p, q));
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < k; ++r) {
                    const double arp = A(r, p), arq = A(r, q);
                    A(r, p) = c * arp - s * arq;
                    A(r, q) = s * arp + c * arq;
                }
                for (int r = 0; r < k; ++r) {
                    const double apr = A(p, r), aqr = A(q, r);
                    A(p, r) = c * apr - s * aqr;
                    A(q, r) = s * apr + c * aqr;
                }
                for (int r = 0; r < k; ++r) {
                    const double urp = U(r, p), urq = U(r, q);
                    U(r, p) = c * urp - s * urq;
                    U(r, q) = s * urp + c * urq;
                }
            }
    }
    std::vector<int> order(k);
    for (int i = 0; i < k; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return A(x, x) < A(y, y); });
    d.resize(k);
    std::vector<double> us((size_t)k * k);
    for (int j = 0; j < k; ++j) {
        d[j] = A(order[j], order[j]);
        for (int i = 0; i < k; ++i) us[i + (size_t)j * k] = U(i, order[j]);
    }
    u.swap(us);
}

// cor_svd (linearcorrelation.hpp:29-47): partial correlation of the first two variables from the pseudo-inverse
double cor_from_eigen(const std::vector<double>& d, const std::vector<double>& u, int k) {
    double p11 = 0, p12 = 0, p22 = 0;
    const double tol = k * d[k - 1] * std::numeric_limits<double>::epsilon();
    for (int i = 0; i < k; ++i)
        if (d[i] > tol) {
            const double inv = 1.0 / d[i], u0 = u[0 + (size_t)i * k], u1 = u[1 + (size_t)i * k];
            p11 += u0 * u0 * inv;
            p12 += u0 * u1 * inv;
            p22 += u1 * u1 * inv;
        }
    if (p11 < MACHINE_TOL || p22 < MACHINE_TOL) return 0;
    return std::min(1.0, std::max(-1.0, -p12 / std::sqrt(p11 * p22)));
}

}  // namespace

double pbn::lincor::lincor_pvalue(const pbn_lincor* h, int v1, int v2, int k, const int* cond) {
    const int n = h->n;
    auto C = [&](int i, int j) { return h->cov[i + (size_t)j * n]; };
    if (k == 0) {  // cor_0cond, df = N - 2
        double cor = 0;
        if (!(C(v1, v1) < MACHINE_TOL || C(v2, v2) < MACHINE_TOL))
            cor = std::min(1.0, std::max(-1.0, C(v1, v2) / std::sqrt(C(v1, v1) * C(v2, v2))));
        return cor_pvalue(cor, test_df(h->rows, 0));
    }
    const int m = k + 2;
    std::vector<int> idx(m);
    idx[0] = v1; idx[1] = v2;
    for (int i = 0; i < k; ++i) idx[i + 2] = cond[i];
    std::vector<double> a((size_t)m * m), d, u;
    for (int j = 0; j < m; ++j)
        for (int i = 0; i < m; ++i) a[i + (size_t)j * m] = C(idx[i], idx[j]);
    jacobi_eigh(a, m, d, u);
    const double cor = cor_from_eigen(d, u, m);
    return cor_pvalue(cor, test_df(h->rows, k));
}

extern "C" {

int pbn_lincor_create(pbn_ctx* ctx, const pbn_table* table, pbn_lincor** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !table || !out) throw invalid_error("pbn_lincor_create: null argument");
        const int n = table->n_cols;
        if (n < 2) throw invalid_error("DataFrame does not contain enough continuous columns.");
        auto h = std::make_unique<pbn_lincor>();
        h->n = n;
        h->rows = table->n_rows;
        h->cov.assign((size_t)n * n, 0.0);
        h->ctx = ctx;
        h->batch_threshold = LINCOR_BATCH_MIN_TESTS;
        std::vector<int> cols;
        std::vector<double> mu, sse;
        // 32-column blocks so that every pair of columns meets in one Gram launch (<= 64 columns per launch)
        const int nb = (n + 31) / 32;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi + (nb > 1 ? 1 : 0); bj < nb; ++bj) {
                cols.clear();
                for (int c = bi * 32; c < std::min(n, bi * 32 + 32); ++c) cols.push_back(c);
                if (bj != bi)
                    for (int c = bj * 32; c < std::min(n, bj * 32 + 32); ++c) cols.push_back(c);
                const int d = (int)cols.size();
                mu.assign(d, 0.0);
                sse.assign((size_t)d * d, 0.0);
                if (pbn_table_sse(table, cols.data(), d, 0, table->n_rows, mu.data(), sse.data()) != PBN_OK)
                    throw device_error(pbn_last_error());
                for (int j = 0; j < d; ++j)
                    for (int i = 0; i < d; ++i) h->cov[cols[i] + (size_t)cols[j] * n] = sse[i + (size_t)j * d] / (double)(table->n_rows - 1);
            }
        // the device batch (lincor_batch.hip) gathers its blocks from a device copy
        HIP_CHECK(hipSetDevice(ctx->device));
        h->dcov.alloc((size_t)n * n);
        HIP_CHECK(hipMemcpyAsync(h->dcov.p, h->cov.data(), (size_t)n * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = h.release();
    });
}

// Host-only construction from a covariance matrix already at hand (n x n, col-major) and the number of rows.
int pbn_lincor_from_cov(int n, int64_t rows, const double* cov, pbn_lincor** out) {
    return guarded([&] {
        if (n < 2 || !cov || !out) throw invalid_error("pbn_lincor_from_cov: bad argument");
        auto h = std::make_unique<pbn_lincor>();
        h->n = n;
        h->rows = rows;
        h->cov.assign(cov, cov + (size_t)n * n);
        *out = h.release();
    });
}

void pbn_lincor_destroy(pbn_lincor* h) {
    if (!h) return;
    if (!h->ctx) { PBN_API_LOCK; delete h; return; }
    pbn::ctx_pin pin_(h->ctx);
    std::lock_guard<std::recursive_mutex> lock_(mu_of(h));
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
}

int pbn_lincor_cov(const pbn_lincor* h, double* cov) {
    return guarded([&] {
        if (!h || !cov) throw invalid_error("pbn_lincor_cov: null argument");
        std::memcpy(cov, h->cov.data(), h->cov.size() * sizeof(double));
    });
}

// pbn_ci_pvalue_fn over a pbn_lincor handle (user = the handle); NaN on bad indices.
double pbn_lincor_pvalue(void* user, int v1, int v2, int n_cond, const int* cond) {
    const pbn_lincor* h = (const pbn_lincor*)user;
    if (!h || v1 < 0 || v2 < 0 || v1 >= h->n || v2 >= h->n || n_cond < 0 || (n_cond > 0 && !cond)) return std::nan("");
    for (int i = 0; i < n_cond; ++i)
        if (cond[i] < 0 || cond[i] >= h->n) return std::nan("");
    return lincor_pvalue(h, v1, v2, n_cond, cond);
}

// LinearCorrelation::pvalue on a table with nulls (continuous/linearcorrelation.cpp:20-122, the pvalue_impl branch): the
// covariance of [v1, v2, cond...] over the rows valid in all of them - one pass of the NaN-skipping moments kernel - then
// the same partial-correlation t-test as the cached form, with `valid rows - 2 - |cond|` degrees of freedom.
// pbn_ci_pvalue_fn signature over a pbn_mi handle whose variables are all continuous.
double pbn_mi_lincor_pvalue(void* user, int v1, int v2, int n_cond, const int* cond) {
    pbn_mi* h = (pbn_mi*)user;
    double result = std::nan("");
    (void)guarded([&] {
        if (!h || (n_cond > 0 && !cond)) throw invalid_error("pbn_mi_lincor_pvalue: null argument");
        std::vector<int> vars;
        if (!mi::map_request(h, v1, v2, n_cond, cond, vars)) throw invalid_error("LinearCorrelation: variable index out of range");
        for (int v : vars)
            if (v < 0 || v >= h->n_cont) throw invalid_error("LinearCorrelation: variable is not continuous");
        std::vector<double> st;
        mi::group_stats(h, vars, {}, st);
        const int c = (int)vars.size();
        const double n = st[0];
        if (!(n > c)) throw invalid_error("LinearCorrelation: not enough valid rows");
        std::vector<double> cov((size_t)c * c);
        int pos = 1 + c;
        for (int i = 0; i < c; ++i)
            for (int j = i; j < c; ++j) {
                const double v = (st[pos++] - st[1 + i] * st[1 + j] / n) / (n - 1.0);
                cov[i + (size_t)j * c] = cov[j + (size_t)i * c] = v;
            }
        pbn_lincor* lc = nullptr;
        if (pbn_lincor_from_cov(c, (int64_t)n, cov.data(), &lc) != PBN_OK) throw device_error(pbn_last_error());
        std::vector<int> zc(std::max(1, n_cond));
        for (int i = 0; i < n_cond; ++i) zc[i] = 2 + i;
        result = pbn_lincor_pvalue(lc, 0, 1, n_cond, zc.data());
        pbn_lincor_destroy(lc);
    });
    return result;
}

}  // extern "C"
