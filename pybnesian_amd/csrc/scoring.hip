// Score engine: BIC / BGe / CV-likelihood / hold-out likelihood local scores, batched.
//
// Reference (paths under /root/reference/pybnesian/): learning/scores/bic.cpp:12-27, bge.hpp:154-234,
// bge.cpp:106-144, cv_likelihood.cpp:11-25, holdout_likelihood.cpp:14-23, validated_likelihood.hpp:14-60,
// learning/parameters/mle_LinearGaussianCPD.hpp:11-221, factors/continuous/LinearGaussianCPD.cpp:92-149,
// dataset/crossvalidation_adaptator.hpp:15-58, dataset/holdout_adaptator.hpp:17-61.
//
// MI355X design (DESIGN.md "score engine"):
//  * The table is permuted ONCE on device into split order (libstdc++ std::shuffle of std::mt19937{seed},
//    exactly the reference's fold membership): CV fold f is the contiguous row range [limits[f],
//    limits[f+1]) and its training set the two ranges around it, so no per-call arrow::Take is needed.
//  * One f64-MFMA Gram pass per fold gives pilot-shifted moments (N, S, G) of every fold; moments are
//    additive, so the statistics of "all rows but fold f" are a subtraction.  Every LinearGaussian quantity
//    (MLE, BIC, BGe, and the Gaussian test log-likelihood of a fold, which is a quadratic form in the test
//    fold's moments) is then O(p^3) host arithmetic on <= (p+1)^2 numbers: the reference's O(N p^2) QR per
//    candidate disappears.  (Normal equations instead of column-pivoted QR: see DESIGN.md "numerics".)
//  * CKDE candidates: bandwidth from the training-fold moments (no extra pass), then per fold
//    pack(train) -> pack(test) -> fused joint+marginal sweep -> finish, all enqueued on the stream from
//    scratch arenas; one synchronisation and one D2H of all fold sums per batch.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <map>
#include <numeric>
#include <random>

#include "common.hpp"
#include "hostmath.hpp"
#include "kde_model.hpp"
#include "scoring_internal.hpp"
#include "stats_kernels.hpp"

using namespace pbn;
using namespace pbn::score;

namespace pbn {
namespace score {

// Shifted Gram of up to 64 columns over a contiguous row range -> raw S (d) and G (d*d col-major).
void gram_raw(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const int32_t* dev_rows,
              const double* shift_dev, double* S, double* G) {
    pbn_ctx* ctx = t->ctx;
    const int nct = (d + 15) / 16;
    const int WS = gram_ws(nct);
    int nblocks = (int)std::min<int64_t>(4 * ctx->num_cus, std::max<int64_t>(1, ceil_div(n, 256)));
    int64_t rpb = ceil_div(std::max<int64_t>(n, 1), nblocks);
    rpb = (rpb + 63) / 64 * 64;
    nblocks = (int)std::max<int64_t>(1, ceil_div(n, rpb));
    ctx->scratch_red.reserve((size_t)nblocks * WS + WS);
    double* partial = ctx->scratch_red.p;
    double* total = partial + (size_t)nblocks * WS;
    GramArgs a{};
    a.base = t->data; a.ld = t->ld; a.n_cols = d; a.row0 = row0; a.rows = dev_rows; a.n = n;
    for (int i = 0; i < d; ++i) a.gc.cols[i] = cols[i];
    a.rows_per_block = rpb; a.shift = shift_dev; a.partial = partial; a.num_cus = ctx->num_cus;
    { KernelTimer kt(ctx, PBN_K_GRAM); launch_gram(a, t->dtype, nblocks, total, ctx->stream); }
    std::vector<double> h((size_t)WS);
    HIP_CHECK(hipMemcpyAsync(h.data(), total, (size_t)WS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const double* Sx = h.data() + (WS - nct * 16);
    for (int i = 0; i < d; ++i) S[i] = Sx[i];
    int p = 0;
    for (int I = 0; I < nct; ++I)
        for (int J = I; J < nct; ++J, ++p) {
            const double* tile = h.data() + (size_t)p * 256;
            for (int e = 0; e < 256; ++e) {
                const int reg = e >> 6, lane = e & 63;
                const int r = I * 16 + (lane >> 4) + 4 * reg, c = J * 16 + (lane & 15);
                if (r >= d || c >= d) continue;
                if (I == J && r > c) continue;  // keep the upper triangle of diagonal tiles
                G[r + (size_t)c * d] = tile[e];
                G[c + (size_t)r * d] = tile[e];
            }
        }
}

// Moments of all n columns over each of the row ranges [r0[i], r1[i]), i in [s0, s1): ONE segmented Gram launch per block (pair)
// of <= 64 columns.  A range is cut into pieces of SEG_ROWS rows (one workgroup each) that are added in order: the result for a
// range depends on its rows only - not on the other ranges of the launch, not on who else computes what.
// PBN_MOMENT_SEG_ROWS (default 4096, a multiple of 128; 2M x 64 doubles: 231 / 212 / 196 / 203 us at 1024 / 2048 / 4096 / 8192 - pieces on
// 512 resident workgroup slots): the piece size is part of the summation order - like PBN_MOMENT_SUPERBLOCKS it must
// be the same on every rank of a job, and another value gives other last bits.
static int64_t seg_rows() {
    static const int64_t v = [] {
        const int64_t r = PBN_TUNE(MOMENT_SEG_ROWS, 4096);
        return std::max<int64_t>(128, r / 128 * 128);
    }();
    return v;
}
// rec (nullable, read by the test aid pbn_debug_scoredata_segments only): pieces launched, launches, element size, NCT of the last launch.
void compute_stats_segments(const pbn_scoredata* sd, const std::vector<int64_t>& r0, const std::vector<int64_t>& r1, size_t s0, size_t s1,
                            std::vector<Stats>& out, int64_t* rec = nullptr) {
    const int n = sd->n;
    const int64_t SEG_ROWS = seg_rows();
    for (size_t i = s0; i < s1; ++i) { out[i].zero(n); out[i].N = r1[i] - r0[i]; }
    if (rec) { rec[0] = rec[1] = rec[3] = 0; rec[2] = (int64_t)dtype_size(sd->dtype); }
    if (s1 <= s0) return;
    const pbn_table* t = sd->table();
    pbn_ctx* ctx = t->ctx;
    const int nseg = (int)(s1 - s0);
    std::vector<int32_t> blk, off(nseg + 1, 0);
    for (int g = 0; g < nseg; ++g) {
        for (int64_t r = r0[s0 + g]; r < r1[s0 + g]; r += SEG_ROWS) {
            const int32_t slot = (int32_t)(blk.size() / 4);   // the piece's partial: pieces of a segment are consecutive slots
            blk.push_back(g); blk.push_back((int32_t)r); blk.push_back((int32_t)std::min(r + SEG_ROWS, r1[s0 + g])); blk.push_back(slot);
        }
        off[g + 1] = (int32_t)(blk.size() / 4);
    }
    const int nblk = (int)(blk.size() / 4);
    if (nblk == 0) return;
    if (t->n_rows > 0x7fffffffll) throw invalid_error("score data: more than 2^31 rows");
    dev_buf<int32_t> dblk(blk.size() + off.size());
    HIP_CHECK(hipMemcpyAsync(dblk.p, blk.data(), blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(dblk.p + blk.size(), off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    auto run = [&](const std::vector<int>& cols) {
        const int d = (int)cols.size(), nct = (d + 15) / 16, WS = gram_ws(nct);
        ctx->scratch_red.reserve(((size_t)nblk + (size_t)nseg) * WS);
        double* partial = ctx->scratch_red.p;
        double* outd = partial + (size_t)nblk * WS;
        GramArgs a{};
        a.base = t->data; a.ld = t->ld; a.n_cols = d; a.row0 = 0; a.rows = nullptr; a.n = t->n_rows;
        for (int i = 0; i < d; ++i) a.gc.cols[i] = cols[i];
        a.rows_per_block = SEG_ROWS; a.blk = dblk.p; a.shift = sd->shift_dev.p; a.partial = partial; a.num_cus = ctx->num_cus;
        { KernelTimer kt(ctx, PBN_K_GRAM); launch_gram_segments(a, t->dtype, nblk, dblk.p + blk.size(), nseg, outd, ctx->stream); }
        if (rec) { rec[0] = nblk; rec[1] += 1; rec[3] = nct; }
        std::vector<double> h((size_t)nseg * WS);
        HIP_CHECK(hipMemcpyAsync(h.data(), outd, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int g = 0; g < nseg; ++g) {
            const double* w = h.data() + (size_t)g * WS;
            Stats& st = out[s0 + g];
            for (int i = 0; i < d; ++i) st.S[cols[i]] = w[WS - nct * 16 + i];
            int p = 0;
            for (int I = 0; I < nct; ++I)
                for (int J = I; J < nct; ++J, ++p) {
                    const double* tile = w + (size_t)p * 256;
                    for (int e = 0; e < 256; ++e) {
                        const int reg = e >> 6, lane = e & 63;
                        const int r = I * 16 + (lane >> 4) + 4 * reg, c = J * 16 + (lane & 15);
                        if (r >= d || c >= d || (I == J && r > c)) continue;
                        st.G[cols[r] + (size_t)cols[c] * n] = tile[e];
                        st.G[cols[c] + (size_t)cols[r] * n] = tile[e];
                    }
                }
        }
    };
    if (n <= 64) {
        std::vector<int> cols(n);
        std::iota(cols.begin(), cols.end(), 0);
        run(cols);
    } else {
        const int nb = (n + 31) / 32;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi + 1; bj < nb; ++bj) {
                std::vector<int> cols;
                for (int c = bi * 32; c < std::min(n, bi * 32 + 32); ++c) cols.push_back(c);
                for (int c = bj * 32; c < std::min(n, bj * 32 + 32); ++c) cols.push_back(c);
                run(cols);
            }
    }
    HIP_CHECK(hipStreamSynchronize(ctx->stream));   // dblk goes out of scope
}

// means / centred SSE of a column subset from moments.
void subset_moments(const pbn_scoredata* sd, const Stats& st, const int* cols, int d, double* mu, double* sse) {
    const int n = sd->n;
    const double N = (double)st.N;
    for (int i = 0; i < d; ++i) mu[i] = sd->shift[cols[i]] + (st.N > 0 ? st.S[cols[i]] / N : 0.0);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i)
            sse[i + (size_t)j * d] =
                st.G[cols[i] + (size_t)cols[j] * n] - (st.N > 0 ? st.S[cols[i]] * st.S[cols[j]] / N : 0.0);
}

void stats_minus(const Stats& a, const Stats& b, Stats& out) {
    out.N = a.N - b.N;
    out.S.resize(a.S.size());
    out.G.resize(a.G.size());
    for (size_t i = 0; i < a.S.size(); ++i) out.S[i] = a.S[i] - b.S[i];
    for (size_t i = 0; i < a.G.size(); ++i) out.G[i] = a.G[i] - b.G[i];
}

// ---- MLE<LinearGaussianCPD> from (N, means, SSE) of [y, x1..xp] (mle_LinearGaussianCPD.hpp:11-221) -----
// beta: p+1 (intercept first); returns the unbiased variance (inf when N <= p+1).
double lg_fit(int64_t N, int p, const double* mu, const double* S /* (p+1)^2 col-major */, double* beta, bool* suspect) {
    if (suspect) *suspect = false;
    const int d = p + 1;
    auto s = [&](int i, int j) { return S[i + (size_t)j * d]; };
    const double rows = (double)N;
    if (p == 0) {
        beta[0] = mu[0];
        if (N == 1) return INF;
        return s(0, 0) / (rows - 1);
    }
    if (p == 1) {
        const double var_x = s(1, 1) / (rows - 1);
        if (var_x < MACHINE_TOL) {
            beta[0] = mu[0]; beta[1] = 0;
            return N <= 2 ? INF : s(0, 0) / (rows - 2);
        }
        const double b = s(0, 1) / s(1, 1);
        beta[0] = mu[0] - b * mu[1]; beta[1] = b;
        if (N <= 2) return INF;
        const double rss = s(0, 0) - 2 * b * s(0, 1) + b * b * s(1, 1);
        return std::max(rss, 0.0) / (rows - 2);
    }
    if (p == 2) {
        const double v1 = s(1, 1) / (rows - 1), v2 = s(2, 2) / (rows - 1), c12 = s(1, 2) / (rows - 1);
        const bool singular1 = v1 < MACHINE_TOL;
        const bool singular2 = v2 < MACHINE_TOL || std::fabs(c12 / std::sqrt(v1 * v2)) > (1 - MACHINE_TOL);
        double b1 = 0, b2 = 0;
        if (singular1) {
            if (!singular2) b2 = s(0, 2) / s(2, 2);
        } else if (singular2) {
            b1 = s(0, 1) / s(1, 1);
        } else {
            const double cy1 = s(0, 1) / (rows - 1), cy2 = s(0, 2) / (rows - 1);
            const double den = v1 * v2 - c12 * c12;
            b1 = (v2 * cy1 - c12 * cy2) / den;
            b2 = (cy2 - b1 * c12) / v2;
        }
        beta[0] = mu[0] - b1 * mu[1] - b2 * mu[2]; beta[1] = b1; beta[2] = b2;
        if (N <= 3) return INF;
        const double rss = s(0, 0) - 2 * b1 * s(0, 1) - 2 * b2 * s(0, 2) + b1 * b1 * s(1, 1) + 2 * b1 * b2 * s(1, 2) +
                           b2 * b2 * s(2, 2);
        return std::max(rss, 0.0) / (rows - 3);
    }
    // p >= 3: normal equations on the centred moments by a diagonally pivoted Cholesky - the pivot order of
    // ColPivHouseholderQR (largest remaining column norm first, mle_LinearGaussianCPD.hpp:171) - a pivot that is not
    // positive relative to its column's scale marks a dependent column (coefficient 0, like the rank-deficient QR solve).
    // RSS is the Schur complement S_yy - |L^-1 b|^2 (error ~ eps S_yy, whatever the size of the coefficients), not the
    // quadratic form in beta.  What this cannot deliver is reported through `suspect`: nearly collinear parents (smallest
    // pivot ratio below 1e-6: coefficients good to ~1e-9 at best) or a nearly exact fit (RSS < 1e-8 S_yy): the callers
    // then refit from the rows in double-double (lg_accurate.hip).
    std::vector<double> A((size_t)p * p), L((size_t)p * p, 0.0), w(p, 0.0), z(p, 0.0), diag(p), scale(p);
    std::vector<int> piv(p);
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < p; ++i) A[i + (size_t)j * p] = s(i + 1, j + 1);
    std::iota(piv.begin(), piv.end(), 0);
    for (int i = 0; i < p; ++i) diag[i] = scale[i] = A[i + (size_t)i * p];
    int rank = 0;
    double min_ratio = 1.0;
    for (int k = 0; k < p; ++k) {
        int best = k;
        for (int j = k + 1; j < p; ++j)
            if (diag[piv[j]] > diag[piv[best]]) best = j;
        std::swap(piv[k], piv[best]);
        for (int c2 = 0; c2 < k; ++c2) std::swap(L[k + (size_t)c2 * p], L[best + (size_t)c2 * p]);
        const double pk = diag[piv[k]];
        if (!(pk > scale[piv[k]] * p * 2.220446049250313e-16) || !std::isfinite(pk)) break;  // the rest depends on the columns taken
        min_ratio = std::min(min_ratio, pk / scale[piv[k]]);
        const double lkk = std::sqrt(pk);
        L[k + (size_t)k * p] = lkk;
        for (int i = k + 1; i < p; ++i) {
            double t = A[piv[i] + (size_t)piv[k] * p];
            for (int c2 = 0; c2 < k; ++c2) t -= L[i + (size_t)c2 * p] * L[k + (size_t)c2 * p];
            t /= lkk;
            L[i + (size_t)k * p] = t;
            diag[piv[i]] -= t * t;
        }
        rank = k + 1;
    }
    double rss = s(0, 0);
    for (int i = 0; i < rank; ++i) {  // forward: w = L^-1 b
        double t = s(0, piv[i] + 1);
        for (int c2 = 0; c2 < i; ++c2) t -= L[i + (size_t)c2 * p] * w[c2];
        w[i] = t / L[i + (size_t)i * p];
        rss -= w[i] * w[i];
    }
    for (int i = rank - 1; i >= 0; --i) {  // backward
        double t = w[i];
        for (int c2 = i + 1; c2 < rank; ++c2) t -= L[c2 + (size_t)i * p] * z[c2];
        z[i] = t / L[i + (size_t)i * p];
    }
    for (int j = 0; j < p; ++j) beta[j + 1] = 0.0;
    for (int i = 0; i < rank; ++i) beta[piv[i] + 1] = z[i];
    double b0 = mu[0];
    for (int j = 0; j < p; ++j) b0 -= beta[j + 1] * mu[j + 1];
    beta[0] = b0;
    if (suspect) *suspect = rank < p || min_ratio < 1e-6 || !(rss > 1e-8 * s(0, 0));
    if (N <= p + 1) return INF;
    return std::max(rss, 0.0) / (rows - p - 1);
}

// BIC of a LinearGaussianCPD (bic.cpp:12-27)
double bic_lg(int64_t N, int p, double variance) {
    if (variance < MACHINE_TOL || std::isinf(variance)) return -INF;
    const double rows = (double)N;
    const double loglik = 0.5 * (1 + (double)p - rows) - 0.5 * rows * LOG_2PI - rows * 0.5 * std::log(variance);
    return loglik - std::log(rows) * 0.5 * (p + 2);
}

// Gaussian log-likelihood of the rows behind `test` moments under (beta, variance)
// (LinearGaussianCPD.cpp:92-149 summed): -1/2 n log(2 pi var) - RSS / (2 var), RSS as a quadratic form.
double lg_slogl_from_moments(const pbn_scoredata* sd, const Stats& test, const int* cols, int p, const double* beta,
                             double variance) {
    const int n = sd->n;
    const double Nt = (double)test.N;
    // residual r = (y - s_y) - sum_j beta_j (x_j - s_j) - c,  c = beta0 - s_y + sum_j beta_j s_j
    double c = beta[0] - sd->shift[cols[0]];
    for (int j = 1; j <= p; ++j) c += beta[j] * sd->shift[cols[j]];
    auto G = [&](int i, int j) { return test.G[cols[i] + (size_t)cols[j] * n]; };
    double rss = G(0, 0);
    double lin = test.S[cols[0]];
    for (int j = 1; j <= p; ++j) {
        rss -= 2 * beta[j] * G(0, j);
        lin -= beta[j] * test.S[cols[j]];
    }
    for (int i = 1; i <= p; ++i)
        for (int j = 1; j <= p; ++j) rss += beta[i] * beta[j] * G(i, j);
    rss += -2 * c * lin + Nt * c * c;
    rss = std::max(rss, 0.0);
    return -0.5 * Nt * (std::log(variance) + LOG_2PI) - 0.5 * rss / variance;
}

// The same sum from the ROWS (one streaming pass, lg_logl_kernel): for fits whose coefficients are huge (nearly collinear
// parents) the quadratic form above cancels - eps beta^2 G against a residual sum of squares that is tiny beside it.
double lg_slogl_from_rows(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const int32_t* dev_rows,
                          const double* beta, double variance) {
    if (n == 0) return 0.0;
    pbn_ctx* ctx = t->ctx;
    const int64_t nblocks = ceil_div(n, 256);
    ctx->scratch_misc.reserve((size_t)(nblocks + 1) * sizeof(double));
    double* bs = (double*)ctx->scratch_misc.p;
    LgArgs a{};
    a.base = t->data; a.ld = t->ld; a.p = d - 1; a.row0 = row0; a.n = n; a.rows = dev_rows;
    for (int i = 0; i < d; ++i) { a.gc.cols[i] = cols[i]; a.beta[i] = beta[i]; }
    a.inv_std = 1.0 / std::sqrt(variance);
    a.cte = -0.5 * std::log(variance) - 0.5 * LOG_2PI;
    a.logl = nullptr; a.block_sums = bs; a.want_cdf = 0;
    launch_lg_logl(a, t->dtype, ctx->stream);
    std::vector<double> hb((size_t)nblocks);
    HIP_CHECK(hipMemcpyAsync(hb.data(), bs, (size_t)nblocks * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    double s = 0.0;
    for (double v : hb) s += v;  // fixed order
    return s;
}

// BGe (bge.hpp:154-234).  params: iss_mu, iss_w, total_nodes, then optionally nu[n] (per table column).
double bge_score(const pbn_scoredata* sd, const Stats& st, const int* cols, int p, double iss_mu, double iss_w,
                 int total_nodes, const double* nu_all) {
    const int d = p + 1;
    std::vector<double> mu(d), sse((size_t)d * d);
    subset_moments(sd, st, cols, d, mu.data(), sse.data());
    const double N = (double)st.N;
    const double t = iss_mu * (iss_w - total_nodes - 1) / (iss_mu + 1);
    double logprob = 0.5 * (std::log(iss_mu) - std::log(N + iss_mu));
    logprob += std::lgamma(0.5 * (N + iss_w - total_nodes + p + 1)) - std::lgamma(0.5 * (iss_w - total_nodes + p + 1));
    logprob -= 0.5 * N * LOG_PI;
    std::vector<double> diff(d);
    for (int i = 0; i < d; ++i) diff[i] = nu_all ? mu[i] - nu_all[cols[i]] : 0.0;
    const double cte_r = (N * iss_mu) / (N + iss_mu);
    if (p == 0) {
        logprob += 0.5 * (iss_w - total_nodes + 1) * std::log(t);
        const double r = t + sse[0] + cte_r * diff[0] * diff[0];
        logprob -= 0.5 * (N + iss_w - total_nodes + 1) * std::log(r);
        return logprob;
    }
    logprob += 0.5 * (iss_w - total_nodes + 2 * p + 1) * std::log(t);
    std::vector<double> R((size_t)d * d), Rp((size_t)p * p);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) R[i + (size_t)j * d] = sse[i + (size_t)j * d] + (i == j ? t : 0.0) + cte_r * diff[i] * diff[j];
    for (int j = 0; j < p; ++j)
        for (int i = 0; i < p; ++i) Rp[i + (size_t)j * p] = R[(i + 1) + (size_t)(j + 1) * d];
    logprob -= 0.5 * (N + iss_w - total_nodes + p + 1) * std::log(hm::determinant(R.data(), d));
    logprob += 0.5 * (N + iss_w - total_nodes + p) * std::log(hm::determinant(Rp.data(), p));
    return logprob;
}

}  // namespace score
}  // namespace pbn

namespace pbn { namespace score {
bool lg_guard_on() {
    return knob_int("PBN_LG_GUARD", 1) != 0;   // read per call: the tests switch it
}
} }

static bool score_memo_on() {
    static const bool v = PBN_TUNE(SCORE_MEMO, 1) != 0;
    return v;
}

extern "C" {

// region moments = their segments added in segment order (see scoredata_create_impl)
static void regions_from_segments(pbn_scoredata* sd) {
    const int n = sd->n;
    if (sd->k > 0) { sd->fold.resize(sd->k); for (auto& f : sd->fold) f.zero(n); } else sd->all.zero(n);
    if (sd->n_hold > 0) sd->hold.zero(n);
    const int hold_region = sd->k > 0 ? sd->k : 1;
    for (size_t i = 0; i < sd->seg.size(); ++i) {
        const int r = sd->seg_region[i];
        Stats& dst = (sd->n_hold > 0 && r == hold_region) ? sd->hold : (sd->k > 0 ? sd->fold[r] : sd->all);
        dst.add(sd->seg[i]);
    }
    if (sd->k > 0) {
        sd->all.zero(n);
        for (int f = 0; f < sd->k; ++f) {
            sd->fold[f].N = sd->limits[f + 1] - sd->limits[f];
            sd->all.add(sd->fold[f]);
        }
    } else {
        sd->all.N = sd->n_cv;
    }
    if (sd->n_hold > 0) sd->hold.N = sd->n_hold;
}

// Row layout of the splits: HoldOut (dataset/holdout_adaptator.hpp:24-61), CrossValidation
// (dataset/crossvalidation_adaptator.hpp:17-57) and, for PBN_SPLIT_VALIDATED, the CV of the hold-out training part
// with the same seed (validated_likelihood.hpp:19-20).  Host only.
struct SplitLayout {
    std::vector<int32_t> idx, limits;
    int64_t n_cv = 0, n_hold = 0;
    int k = 0;
};
static SplitLayout split_layout(int64_t rows, int split, int k, uint32_t seed, double test_ratio) {
    SplitLayout L;
    SplitLayout* sd = &L;
    std::vector<int32_t> idx((size_t)rows);
    std::iota(idx.begin(), idx.end(), 0);
    sd->n_cv = rows;
    if (split == PBN_SPLIT_HOLDOUT || split == PBN_SPLIT_VALIDATED) {
        // holdout_adaptator.hpp:24-61
        if (test_ratio <= 0 || test_ratio >= 1.0) throw invalid_error("test_ratio must be a number between 0 and 1.");
        std::mt19937 rng{seed};
        std::shuffle(idx.begin(), idx.end(), rng);
        const int64_t test_rows = (int64_t)std::round((double)rows * test_ratio);
        const int64_t train_rows = rows - test_rows;
        if (test_rows == 0 || train_rows == 0)
            throw invalid_error("Wrong test_ratio (" + std::to_string(test_ratio) + "selected for HoldOut.\nGenerated train instances: " +
                                std::to_string(train_rows) + "\nGenerated test instances: " + std::to_string(test_rows));
        sd->n_cv = train_rows;
        sd->n_hold = test_rows;
    }
    if (split == PBN_SPLIT_CV || split == PBN_SPLIT_VALIDATED) {
        // crossvalidation_adaptator.hpp:17-57 on the (hold-out) training part; for VALIDATED the CV object is
        // built on training_data() with the same seed (validated_likelihood.hpp:19-20)
        const int64_t n = sd->n_cv;
        if (k <= 1 || k > n)
            throw invalid_error("Cannot split " + std::to_string(n) + " instances into " + std::to_string(k) + " folds.");
        std::vector<int32_t> local((size_t)n);
        std::iota(local.begin(), local.end(), 0);
        std::mt19937 rng{seed};
        std::shuffle(local.begin(), local.end(), rng);
        std::vector<int32_t> tmp(idx.begin(), idx.begin() + n);
        for (int64_t i = 0; i < n; ++i) idx[i] = tmp[local[i]];
        const int fold_size = (int)(n / k), extra = (int)(n % k);
        sd->k = k;
        sd->limits.assign(1, 0);
        int cur = 0;
        for (int i = 0; i < extra; ++i) { cur += fold_size + 1; sd->limits.push_back(cur); }
        for (int i = extra; i < k; ++i) { cur += fold_size; sd->limits.push_back(cur); }
    }
    L.idx = std::move(idx);
    return L;
}

static int scoredata_create_impl(pbn_ctx* ctx, const pbn_table* table, int split, int k, uint32_t seed, double test_ratio,
                                 int rank, int world, pbn_scoredata** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !table || !out) throw invalid_error("pbn_scoredata_create: null argument");
        if (world < 1 || rank < 0 || rank >= world) throw invalid_error("pbn_scoredata_create_sharded: rank / world out of range");
        if (table->n_cols <= 0) throw invalid_error("pbn_scoredata_create: table has no columns");
        HIP_CHECK(hipSetDevice(ctx->device));
        auto sd = std::make_unique<pbn_scoredata>();
        sd->ctx = ctx; sd->dtype = table->dtype; sd->n = table->n_cols; sd->split = split; sd->src = table;
        const int64_t rows = table->n_rows;
        SplitLayout lay = split_layout(rows, split, k, seed, test_ratio);
        sd->n_cv = lay.n_cv; sd->n_hold = lay.n_hold; sd->k = lay.k; sd->limits = lay.limits;
        sd->perm = std::move(lay.idx);   // (2M rows: 8 MB - moved, not copied twice)
        const std::vector<int32_t>& idx = sd->perm;
        if (split != PBN_SPLIT_NONE) {
            pbn_table* pt = nullptr;
            int rc = pbn_table_take(table, idx.data(), rows, &pt);
            if (rc != PBN_OK) throw device_error(pbn_last_error());
            sd->perm_table = pt;
        }
        // pilot shifts over the CV region of the (permuted) table
        const pbn_table* t = sd->table();
        sd->shift_dev.alloc((size_t)sd->n);
        for (int c0 = 0; c0 < sd->n; c0 += 64) {
            GramCols gc{};
            const int d = std::min(64, sd->n - c0);
            for (int i = 0; i < d; ++i) gc.cols[i] = c0 + i;
            launch_pilot(t->data, t->ld, gc, d, 0, nullptr, sd->n_cv, t->dtype, sd->shift_dev.p, ctx->stream);
        }
        sd->shift.resize(sd->n);
        HIP_CHECK(hipMemcpyAsync(sd->shift.data(), sd->shift_dev.p, sd->n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        // moments: every region in PBN_MOMENT_SUPERBLOCKS super-blocks (boundaries: multiples of 64 rows, a function of the
        // region's length only); rank r of `world` computes segments [S r / world, S (r + 1) / world) and leaves the others zero;
        // the caller adds the ranks' buffers (exact: every segment is non-zero on one rank only) and installs them
        // (pbn_scoredata_moments), and regions_from_segments adds a region's segments in segment order: the totals are the same
        // bit for bit for every world size.
        // (16 super-blocks up to 128 columns; wider tables fewer - a segment is n + n^2 doubles on every rank, 176 of them at 10 folds +
        //  hold-out: 350 MB per rank at n = 500 - down to 2 from 512 columns: the count is part of the summation order, so it is a
        //  function of n alone)
        static const int SB_env = std::min(1024, std::max(0, PBN_TUNE(MOMENT_SUPERBLOCKS, 0)));
        const int SB = SB_env > 0 ? SB_env : (sd->n <= 128 ? 16 : (sd->n <= 256 ? 8 : (sd->n <= 512 ? 4 : 2)));
        auto add_region = [&](int region, int64_t r0, int64_t len) {
            int64_t prev = 0;
            for (int i = 1; i <= SB; ++i) {
                int64_t b = i == SB ? len : (len * i / SB + 63) / 64 * 64;
                b = std::min(b, len);
                sd->seg_region.push_back(region);
                sd->seg_r0.push_back(r0 + prev);
                sd->seg_r1.push_back(r0 + std::max(prev, b));
                prev = std::max(prev, b);
            }
        };
        int region = 0;
        if (sd->k > 0) for (int f = 0; f < sd->k; ++f) add_region(region++, sd->limits[f], sd->limits[f + 1] - sd->limits[f]);
        else add_region(region++, 0, sd->n_cv);
        if (sd->n_hold > 0) add_region(region++, sd->n_cv, sd->n_hold);
        const size_t S = sd->seg_region.size();
        sd->seg.resize(S);
        for (auto& st : sd->seg) st.zero(sd->n);
        compute_stats_segments(sd.get(), sd->seg_r0, sd->seg_r1, S * (size_t)rank / (size_t)world, S * (size_t)(rank + 1) / (size_t)world, sd->seg);
        regions_from_segments(sd.get());
        sd->partial = world > 1;
        *out = sd.release();
    });
}

int pbn_scoredata_create(pbn_ctx* ctx, const pbn_table* table, int split, int k, uint32_t seed, double test_ratio,
                         pbn_scoredata** out) {
    return scoredata_create_impl(ctx, table, split, k, seed, test_ratio, 0, 1, out);
}

int pbn_scoredata_create_sharded(pbn_ctx* ctx, const pbn_table* table, int split, int k, uint32_t seed, double test_ratio,
                                 int rank, int world, pbn_scoredata** out) {
    return scoredata_create_impl(ctx, table, split, k, seed, test_ratio, rank, world, out);
}

// Score data without a table (learning/scores/bic.cpp:66-96, cv_likelihood.cpp:5-25, bde.cpp:5-47 on an all-discrete DataFrame): the split
// layout of scoredata_create_impl for the same rows, split, k, seed and ratio; n = 0, no pilot shifts, no moments.  The codes follow
// through pbn_scoredata_set_discrete as ids 0 .. n_disc - 1.
int pbn_scoredata_create_discrete(pbn_ctx* ctx, int64_t n_rows, int split, int k, uint32_t seed, double test_ratio, pbn_scoredata** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !out) throw invalid_error("pbn_scoredata_create_discrete: null argument");
        if (n_rows <= 0 || n_rows > INT32_MAX) throw invalid_error("pbn_scoredata_create_discrete: row count out of range");
        if (split < PBN_SPLIT_NONE || split > PBN_SPLIT_VALIDATED) throw invalid_error("pbn_scoredata_create_discrete: unknown split");
        HIP_CHECK(hipSetDevice(ctx->device));
        auto sd = std::make_unique<pbn_scoredata>();
        sd->ctx = ctx; sd->n = 0; sd->split = split; sd->discrete_only = true;
        SplitLayout lay = split_layout(n_rows, split, k, seed, test_ratio);
        sd->n_cv = lay.n_cv; sd->n_hold = lay.n_hold; sd->k = lay.k; sd->limits = lay.limits;
        sd->perm = std::move(lay.idx);
        *out = sd.release();
    });
}

// Serialised moments: for each SEGMENT (scoredata_create_impl: the regions' super-blocks, in order) S[n] then G[n*n].
// set == 0 copies them out (segments this rank did not compute are zero), set != 0 installs all of them, rebuilds the
// regions' totals in segment order and clears the partial flag.
int pbn_scoredata_moments(pbn_scoredata* sd, double* buf, int64_t* len, int set) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_moments: null argument");
        if (sd->discrete_only) throw invalid_error("pbn_scoredata_moments: discrete-only score data has no table and no moments");
        const size_t per = (size_t)sd->n + (size_t)sd->n * sd->n;
        if (len) *len = (int64_t)(per * sd->seg.size());
        if (!buf) return;
        double* p = buf;
        for (Stats& st : sd->seg) {
            if (set) {
                std::memcpy(st.S.data(), p, sd->n * sizeof(double));
                std::memcpy(st.G.data(), p + sd->n, (size_t)sd->n * sd->n * sizeof(double));
            } else {
                std::memcpy(p, st.S.data(), sd->n * sizeof(double));
                std::memcpy(p + sd->n, st.G.data(), (size_t)sd->n * sd->n * sizeof(double));
            }
            p += per;
        }
        if (!set) return;
        regions_from_segments(sd);
        sd->partial = false;
        sd->kde_cache.clear();
        sd->term_total.clear();
        sd->score_memo.clear();
    });
}

void pbn_scoredata_destroy(pbn_scoredata* sd) {
    if (!sd) return;
    pbn::ctx_pin pin_(sd->ctx);
    std::lock_guard<std::recursive_mutex> lock_(mu_of(sd));
    if (sd->perm_table) pbn_table_destroy(sd->perm_table);
    delete sd;
}

// Attach the dictionary-encoded (discrete) columns: codes[j][r] = dictionary index of SOURCE row r.
int pbn_scoredata_set_discrete(pbn_scoredata* sd, int n_disc, const int32_t* const* codes, const int* cardinality) {
    return guarded(mu_of(sd), [&] {
        if (!sd || (n_disc > 0 && (!codes || !cardinality))) throw invalid_error("pbn_scoredata_set_discrete: null argument");
        const int64_t rows = (int64_t)sd->perm.size();
        // everything derived from the previous codes (device row lists of the groupings, per-configuration KDE sums, memoised
        // local scores) is stale: let the work in flight finish, then drop it
        HIP_CHECK(hipStreamSynchronize(sd->ctx->stream));
        sd->ctx->sync_lanes(pbn_ctx::MAX_PARKED);
        sd->groupings.clear();
        sd->kde_cache.clear();
        sd->term_total.clear();
        sd->score_memo.clear();
        sd->n_disc = n_disc;
        sd->codes.assign(n_disc, std::vector<int32_t>((size_t)rows));
        sd->card.assign(cardinality, cardinality + n_disc);
        sd->disc_null.assign(n_disc, 0);
        sd->has_disc_nulls = false;
        // -1 = null, for BIC / BDe score data only (bic.cpp:66-96 and bde.cpp count over the rows valid in the family's columns,
        // discrete_indices.cpp:134-150); the likelihood scores' tables were filtered before they were split and hold none
        const bool nulls_ok = sd->split == PBN_SPLIT_NONE;
        for (int j = 0; j < n_disc; ++j)
            for (int64_t r = 0; r < rows; ++r) {
                const int32_t v = codes[j][sd->perm[r]];
                if (v == -1 && nulls_ok) { sd->disc_null[j] = 1; sd->has_disc_nulls = true; }
                else if (v < 0 || v >= cardinality[j]) throw invalid_error("pbn_scoredata_set_discrete: code out of range");
                sd->codes[j][r] = v;
            }
        family_codes_upload(sd);
    });
}

// Validity of the continuous columns for BIC / BGe on tables with nulls (bic.cpp:12-27 uses
// valid_rows(variable, parents); bge.hpp:52-72 drops its cache when any column has nulls): masks[c] is a byte
// array (1 = valid) in source row order, or NULL when column c has no nulls.  Likelihood scores never see nulls:
// CrossValidation / HoldOut keep only rows valid in every column (crossvalidation_adaptator.hpp:24-37).
int pbn_scoredata_set_validity(pbn_scoredata* sd, const uint8_t* const* masks) {
    return guarded(mu_of(sd), [&] {
        if (!sd || !masks) throw invalid_error("pbn_scoredata_set_validity: null argument");
        if (sd->discrete_only) throw invalid_error("pbn_scoredata_set_validity: discrete-only score data has no continuous columns");
        if (sd->split != PBN_SPLIT_NONE) throw invalid_error("pbn_scoredata_set_validity: only for BIC / BGe score data");
        const int64_t rows = (int64_t)sd->perm.size();
        // what was derived under the previous masks (cell moments of the groupings) is stale: let the work in flight finish, then drop it
        HIP_CHECK(hipStreamSynchronize(sd->ctx->stream));
        sd->ctx->sync_lanes(pbn_ctx::MAX_PARKED);
        sd->groupings.clear();
        sd->valid.assign(sd->n, {});
        sd->has_nulls = false;
        for (int c = 0; c < sd->n; ++c)
            if (masks[c]) {
                sd->valid[c].assign(masks[c], masks[c] + rows);
                sd->has_nulls = true;
            }
        masked_validity_upload(sd);   // the same bits as words on the device, for the masked pass (masked_moments.hip)
    });
}

// Bandwidth selector used for every CKDE the engine fits while scoring (CKDEType::new_factor with construction
// arguments, cv_likelihood.hpp:19-27; selectors kde/NormalReferenceRule.hpp, kde/ScottsBandwidth.hpp).
int pbn_scoredata_set_selector(pbn_scoredata* sd, int selector) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_set_selector: null argument");
        if (selector != PBN_SEL_NORMAL_REFERENCE && selector != PBN_SEL_SCOTT) throw invalid_error("pbn_scoredata_set_selector: unknown selector");
        sd->selector = selector;
        sd->kde_cache.clear();
        sd->term_total.clear();
        sd->score_memo.clear();
    });
}

// Set-function cache of the CKDE likelihood scores: entries held, sweeps launched so far.
int pbn_scoredata_cache_stats(const pbn_scoredata* sd, int64_t* entries, int64_t* sweeps) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_cache_stats: null argument");
        if (entries) *entries = (int64_t)sd->kde_cache.size();
        if (sweeps) *sweeps = sd->kde_sweeps;
    });
}

// The same layout without a table or a device (CrossValidation / HoldOut as stand-alone objects): perm has n_rows
// entries, limits k + 1 (nullable when k <= 1).
int pbn_split_layout(int64_t n_rows, int split, int k, uint32_t seed, double test_ratio, int32_t* perm, int32_t* limits,
                     int64_t* n_cv, int64_t* n_hold) {
    return guarded([&] {
        if (n_rows < 0 || !perm) throw invalid_error("pbn_split_layout: bad argument");
        SplitLayout lay = split_layout(n_rows, split, k, seed, test_ratio);
        std::memcpy(perm, lay.idx.data(), lay.idx.size() * sizeof(int32_t));
        if (limits && !lay.limits.empty()) std::memcpy(limits, lay.limits.data(), lay.limits.size() * sizeof(int32_t));
        if (n_cv) *n_cv = lay.n_cv;
        if (n_hold) *n_hold = lay.n_hold;
    });
}

int pbn_scoredata_layout(const pbn_scoredata* sd, int32_t* perm, int32_t* limits, int64_t* n_cv, int64_t* n_hold) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_layout: null argument");
        if (perm) std::memcpy(perm, sd->perm.data(), sd->perm.size() * sizeof(int32_t));
        if (limits && sd->k > 0) std::memcpy(limits, sd->limits.data(), sd->limits.size() * sizeof(int32_t));
        if (n_cv) *n_cv = sd->n_cv;
        if (n_hold) *n_hold = sd->n_hold;
    });
}

// MLE<LinearGaussianCPD>::estimate over the CV/training region (all rows for PBN_SPLIT_NONE).
int pbn_lg_fit(const pbn_scoredata* sd, int var, const int* parents, int p, double* beta, double* variance) {
    return guarded(mu_of(sd), [&] {
        if (!sd || !beta || !variance) throw invalid_error("pbn_lg_fit: null argument");
        if (sd->discrete_only) throw invalid_error("pbn_lg_fit: discrete-only score data has no continuous columns");
        if (sd->partial) throw invalid_error("pbn_lg_fit: row-sharded score data needs pbn_scoredata_moments(set) first");
        std::vector<int> cols(p + 1);
        cols[0] = var;
        for (int i = 0; i < p; ++i) cols[i + 1] = parents[i];
        for (int c : cols)
            if (c < 0 || c >= sd->n) throw invalid_error("pbn_lg_fit: column out of range");
        std::vector<double> mu(p + 1), sse((size_t)(p + 1) * (p + 1));
        subset_moments(sd, sd->all, cols.data(), p + 1, mu.data(), sse.data());
        bool suspect = false;
        *variance = lg_fit(sd->all.N, p, mu.data(), sse.data(), beta, &suspect);
        if (suspect && lg_guard_on() && p + 1 <= 16 && !sd->has_nulls)
            *variance = lg_fit_accurate(sd->table(), cols.data(), p + 1, 0, sd->n_cv, 0, sd->n_cv, nullptr, beta);
    });
}

// MLE<LinearGaussianCPD>::estimate on a table row range (one Gram pass + host solve).
int pbn_lg_fit_table(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, double* beta, double* variance) {
    return guarded(mu_of(t), [&] {
        if (!beta || !variance) throw invalid_error("pbn_lg_fit_table: null output");
        check_cols(t, cols, d, "pbn_lg_fit_table");
        check_range(t, row0, n, "pbn_lg_fit_table");
        if (d < 1 || d > 64) throw invalid_error("pbn_lg_fit_table: between 1 and 64 columns (variable + evidence) are supported");
        HIP_CHECK(hipSetDevice(t->ctx->device));
        std::vector<double> mu(d), sse((size_t)d * d);
        int rc = pbn_table_sse(t, cols, d, row0, n, mu.data(), sse.data());
        if (rc != PBN_OK) throw device_error(pbn_last_error());
        bool suspect = false;
        *variance = lg_fit(n, d - 1, mu.data(), sse.data(), beta, &suspect);
        if (suspect && lg_guard_on() && d <= 16) *variance = lg_fit_accurate(t, cols, d, row0, n, 0, n, nullptr, beta);
    });
}

// LinearGaussianCPD::logl / slogl (factors/continuous/LinearGaussianCPD.cpp:92-149,251-292).
static int lg_eval(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const double* beta, double variance,
                   double* out_logl, double* out_slogl, int want_cdf) {
    return guarded(mu_of(t), [&] {
        check_cols(t, cols, d, "pbn_lg_logl");
        check_range(t, row0, n, "pbn_lg_logl");
        if (!beta) throw invalid_error("pbn_lg_logl: null beta");
        if (d < 1 || d > 64) throw invalid_error("pbn_lg_logl: between 1 and 64 columns are supported");
        pbn_ctx* ctx = t->ctx;
        HIP_CHECK(hipSetDevice(ctx->device));
        if (n == 0) { if (out_slogl) *out_slogl = 0.0; return; }
        const int64_t nblocks = ceil_div(n, 256);
        dev_buf<double> dlogl;
        if (out_logl) dlogl.alloc((size_t)n);
        ctx->scratch_misc.reserve((size_t)(nblocks + 1) * sizeof(double));
        double* bs = (double*)ctx->scratch_misc.p;
        LgArgs a{};
        a.base = t->data; a.ld = t->ld; a.p = d - 1; a.row0 = row0; a.n = n;
        for (int i = 0; i < d; ++i) { a.gc.cols[i] = cols[i]; a.beta[i] = beta[i]; }
        lg_constants(variance, &a.inv_std, &a.cte);
        a.logl = dlogl.p; a.block_sums = bs; a.want_cdf = want_cdf;
        launch_lg_logl(a, t->dtype, ctx->stream);
        if (out_logl) HIP_CHECK(hipMemcpyAsync(out_logl, dlogl.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        std::vector<double> hb((size_t)nblocks);
        HIP_CHECK(hipMemcpyAsync(hb.data(), bs, (size_t)nblocks * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        if (out_slogl) {
            double s = 0.0;
            for (double v : hb) s += v;  // fixed order
            *out_slogl = s;
        }
    });
}

int pbn_lg_logl(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const double* beta, double variance,
                double* out_logl, double* out_slogl) {
    return lg_eval(t, cols, d, row0, n, beta, variance, out_logl, out_slogl, 0);
}

// LinearGaussianCPD::cdf (factors/continuous/LinearGaussianCPD.cpp:171-249): Phi((y - beta.x) / sigma) per row.
int pbn_lg_cdf(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n, const double* beta, double variance,
               double* out) {
    if (!out && n > 0) { set_last_error("pbn_lg_cdf: null output"); return PBN_ERR_INVALID; }
    return lg_eval(t, cols, d, row0, n, beta, variance, out, nullptr, 1);
}

// ---- test aids (not part of the C ABI header) -----------------------------------------------------------------------
// pbn_debug_scoredata_shifts: the handle's pilot shifts, one double per continuous column.
int pbn_debug_scoredata_shifts(const pbn_scoredata* sd, double* out) {
    return guarded(mu_of(sd), [&] {
        if (!sd || !out) throw invalid_error("pbn_debug_scoredata_shifts: null argument");
        std::copy(sd->shift.begin(), sd->shift.end(), out);
    });
}

// pbn_debug_gram_rows: gram_raw through a device row list, as the candidates of a table with nulls reach it (valid_row_moments above,
// score_hybrid's filtered lists).  rows: n_rows >= 1 table row ids on the host (any order, repeats allowed), shift: one double per TABLE
// column, on the host; both are uploaded here.  cols: d table columns (1 .. 64).  S: d sums, G: d * d products, column-major, of the
// shifted columns over the list - raw, as gram_raw returns them.
int pbn_debug_gram_rows(const pbn_table* t, int d, const int* cols, const int32_t* rows, int64_t n_rows, const double* shift, double* S, double* G) {
    return guarded(mu_of(t), [&] {
        if (!t || !cols || !rows || !shift || !S || !G) throw invalid_error("pbn_debug_gram_rows: null argument");
        if (d < 1 || d > 64) throw invalid_error("pbn_debug_gram_rows: between 1 and 64 columns");
        check_cols(t, cols, d, "pbn_debug_gram_rows");
        if (n_rows < 1 || n_rows > 0x7fffffffll) throw invalid_error("pbn_debug_gram_rows: a row list of 1 .. 2^31 - 1 entries");
        for (int64_t r = 0; r < n_rows; ++r)
            if (rows[r] < 0 || rows[r] >= t->n_rows) throw invalid_error("pbn_debug_gram_rows: row list entry out of range");
        HIP_CHECK(hipSetDevice(t->ctx->device));
        dev_buf<int32_t> drows((size_t)n_rows + 16);   // (the lists of the engine carry the same slack)
        dev_buf<double> dshift((size_t)t->n_cols);
        HIP_CHECK(hipMemcpy(drows.p, rows, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(dshift.p, shift, (size_t)t->n_cols * sizeof(double), hipMemcpyHostToDevice));
        gram_raw(t, cols, d, 0, n_rows, drows.p, dshift.p, S, G);   // synchronises
    });
}

// pbn_debug_scoredata_segments: compute_stats_segments, the segmented form of the contiguous Gram kernels, on row ranges given by the caller.
// n_seg > 0: segment i is rows [r0[i], r1[i]) of the handle's (permuted) table, 0 <= r0[i] <= r1[i] <= rows; ranges may be empty and may
// overlap.  S: n_seg * n shifted column sums, G: n_seg * n * n shifted products (column-major, symmetric) over ALL n continuous columns,
// centred on the handle's pilot shifts (pbn_debug_scoredata_shifts).  rec: 4 + n_seg int64 - the pieces launched (4 096 rows each,
// PBN_MOMENT_SEG_ROWS), the launches (1 up to 64 columns, one per pair of 32-column blocks above), the table's element size in bytes, NCT
// of the last launch, then the row count N the engine recorded per segment.
// n_seg == 0: reports the handle's own segments instead - rec[0] = their number M, then per segment (region, r0, r1) in rec[1 + 3 i ..],
// and, where S and G are non-null, the installed moments seg[i].S (M * n) and seg[i].G (M * n * n).  rec must hold 1 + 3 M entries; with
// S == G == null only rec[0] is written, so that the caller can size the second call.
int pbn_debug_scoredata_segments(pbn_scoredata* sd, int n_seg, const int64_t* r0, const int64_t* r1, double* S, double* G, int64_t* rec) {
    return guarded(mu_of(sd), [&] {
        if (!sd || !rec || n_seg < 0) throw invalid_error("pbn_debug_scoredata_segments: bad argument");
        if (sd->discrete_only) throw invalid_error("pbn_debug_scoredata_segments: discrete-only score data has no continuous columns");
        const size_t n = (size_t)sd->n;
        if (n_seg == 0) {
            const size_t M = sd->seg.size();
            rec[0] = (int64_t)M;
            if (!S && !G) return;
            if (!S || !G) throw invalid_error("pbn_debug_scoredata_segments: S and G together");
            for (size_t i = 0; i < M; ++i) {
                rec[1 + 3 * i] = sd->seg_region[i]; rec[2 + 3 * i] = sd->seg_r0[i]; rec[3 + 3 * i] = sd->seg_r1[i];
                std::copy(sd->seg[i].S.begin(), sd->seg[i].S.end(), S + i * n);
                std::copy(sd->seg[i].G.begin(), sd->seg[i].G.end(), G + i * n * n);
            }
            return;
        }
        if (!r0 || !r1 || !S || !G) throw invalid_error("pbn_debug_scoredata_segments: null argument");
        const int64_t rows = sd->table()->n_rows;
        for (int i = 0; i < n_seg; ++i)
            if (r0[i] < 0 || r1[i] < r0[i] || r1[i] > rows) throw invalid_error("pbn_debug_scoredata_segments: row range out of bounds");
        HIP_CHECK(hipSetDevice(sd->ctx->device));
        std::vector<int64_t> a(r0, r0 + n_seg), b(r1, r1 + n_seg);
        std::vector<Stats> out((size_t)n_seg);
        compute_stats_segments(sd, a, b, 0, (size_t)n_seg, out, rec);
        for (int i = 0; i < n_seg; ++i) {
            rec[4 + i] = out[i].N;
            std::copy(out[i].S.begin(), out[i].S.end(), S + (size_t)i * n);
            std::copy(out[i].G.begin(), out[i].G.end(), G + (size_t)i * n * n);
        }
    });
}

}  // extern "C"

// ---- the batch engine: score_batch_body checks the call and sends every candidate to one of score_hybrid_candidate (a discrete column
// involved), score_gaussian_candidate (BIC, BGe, LinearGaussian likelihood) or the list of plain CKDE candidates that score_ckde_terms
// (score_terms.hip) evaluates together after the loop.  DESIGN.md 3.5 has the map. ----
namespace pbn {
namespace score {

size_t score_cache_budget() {
    static const size_t v = (size_t)std::max(1ll, knob_ll("PBN_SCORE_CACHE_ENTRIES", 1ll << 21));
    return v;
}

void candidate_cols(const BatchArgs& a, int c, std::vector<int>& cols) {
    const int p = a.n_parents(c);
    cols.resize(p + 1);
    cols[0] = a.var[c];
    for (int i = 0; i < p; ++i) cols[i + 1] = a.parents[a.par_off[c] + i];
}

namespace {

// the gather list of a candidate's valid rows (DataFrame::combined_bitmap, dataset.cpp:208-235) -> sd->rows_dev
int64_t gather_rows(pbn_scoredata* sd, const std::vector<int>& cs) {
    const int64_t rows = (int64_t)sd->perm.size();
    std::vector<int32_t> keep;
    keep.reserve(rows);
    for (int64_t r = 0; r < rows; ++r) {
        bool ok = true;
        for (int cc : cs) ok = ok && (sd->valid[cc].empty() || sd->valid[cc][r]);
        if (ok) keep.push_back((int32_t)r);
    }
    sd->rows_dev.reserve(keep.size() + 16);
    if (!keep.empty()) {
        HIP_CHECK(hipMemcpyAsync(sd->rows_dev.p, keep.data(), keep.size() * sizeof(int32_t), hipMemcpyHostToDevice, sd->ctx->stream));
        HIP_CHECK(hipStreamSynchronize(sd->ctx->stream));   // keep goes out of scope
    }
    return (int64_t)keep.size();
}

// Tables with nulls: the plain BIC / BGe candidates that involve a column with nulls, deduplicated by ordered column list, take their
// moments over the rows valid in all of their columns from ONE masked pass over the batch (masked_moments.hip) instead of a host
// loop over the rows, an upload and a gathered Gram each.  (More than 8 columns, or PBN_NULL_MOMENTS=0: the per-candidate path.)
struct MaskedPlan {
    std::map<std::vector<int>, size_t> unit_of;   // ordered column list -> unit of the pass
    std::vector<std::vector<MaskedMoments>> moments;
};
MaskedPlan masked_prepass(pbn_scoredata* sd, const BatchArgs& a, std::vector<int>& cols) {
    MaskedPlan plan;
    if (!sd->has_nulls || (a.kind != PBN_SCORE_BIC && a.kind != PBN_SCORE_BGE) || !masked_moments_on()) return plan;
    std::vector<MaskedUnit> units;
    for (int c = 0; c < a.n_cand; ++c) {
        if (a.n_parents(c) + 1 > MASKED_MAX_COLS) continue;
        candidate_cols(a, c, cols);
        bool plain = true, involved = false;
        for (int cc : cols) {
            plain = plain && cc >= 0 && cc < sd->n;   // (out of range: the candidate loop throws; discrete: hybrid.hip)
            involved = involved || (plain && !sd->valid[cc].empty());
        }
        if (!plain || !involved || plan.unit_of.count(cols)) continue;
        plan.unit_of.emplace(cols, units.size());
        units.push_back(MaskedUnit{cols, nullptr, 0, {}});
    }
    masked_moments(sd, units, plan.moments);
    return plan;
}

// Moments of a BIC / BGe candidate over the rows valid in all of its columns -> `gathered` (true), or false when none of its columns has
// nulls and sd->all serves.  From the masked plan where it holds the candidate (*from_masked: no gather list on the device yet), else
// from a gather list of the valid rows (left in sd->rows_dev) and a gathered Gram.
bool valid_row_moments(pbn_scoredata* sd, const std::vector<int>& cols, const MaskedPlan& plan, Stats& gathered, bool* from_masked) {
    const int d = (int)cols.size();
    bool involved = false;
    for (int cc : cols) involved = involved || !sd->valid[cc].empty();
    if (!involved) return false;
    const auto mit = plan.unit_of.find(cols);
    if (mit != plan.unit_of.end()) {
        masked_to_stats(sd, cols.data(), d, plan.moments[mit->second][0], gathered);
        *from_masked = true;
        return true;
    }
    if (d > 64) throw invalid_error("pbn_score_batch: more than 64 columns in one candidate");
    const int64_t kept = gather_rows(sd, cols);
    std::vector<double> S(d), G((size_t)d * d);
    if (kept > 0) gram_raw(sd->table(), cols.data(), d, 0, kept, sd->rows_dev.p, sd->shift_dev.p, S.data(), G.data());
    gathered.zero(sd->n);
    gathered.N = kept;
    for (int i = 0; i < d; ++i) {
        gathered.S[cols[i]] = S[i];
        for (int j = 0; j < d; ++j) gathered.G[cols[i] + (size_t)cols[j] * sd->n] = G[i + (size_t)j * d];
    }
    return true;
}

struct BgeParams {   // iss_mu, iss_w, total_nodes, then optionally nu[n] (per table column)
    double iss_mu, iss_w;
    int total_nodes;
    const double* nu;
};

// BIC, BGe and the CV / hold-out likelihood of a LinearGaussianCPD over continuous columns (s.cols): host arithmetic on the regions' moments
double score_gaussian_candidate(pbn_scoredata* sd, int kind, int nt, const BgeParams& bge, const MaskedPlan& plan, ScoreScratch& s) {
    const pbn_table* t = sd->table();
    const std::vector<int>& cols = s.cols;
    const int d = (int)cols.size(), p = d - 1;
    s.mu.resize(d); s.sse.resize((size_t)d * d); s.beta.resize(d);
    if (kind == PBN_SCORE_BIC || kind == PBN_SCORE_BGE) {
        const Stats* full = &sd->all;
        Stats gathered;
        bool from_masked = false;
        if (sd->has_nulls && valid_row_moments(sd, cols, plan, gathered, &from_masked)) full = &gathered;
        if (kind == PBN_SCORE_BGE) return bge_score(sd, *full, cols.data(), p, bge.iss_mu, bge.iss_w, bge.total_nodes, bge.nu);
        if (nt != PBN_NODE_LG) throw invalid_error("BIC: only LinearGaussianCPD node types are implemented on device");
        subset_moments(sd, *full, cols.data(), d, s.mu.data(), s.sse.data());
        bool suspect = false;
        double v = lg_fit(full->N, p, s.mu.data(), s.sse.data(), s.beta.data(), &suspect);
        if (suspect && lg_guard_on() && d <= 16) {   // nearly collinear parents / nearly exact fit: double-double refit
            if (from_masked && gather_rows(sd, cols) != full->N) throw device_error("masked moments: the pass and the validity masks disagree on the valid rows");
            if (full == &gathered) v = lg_fit_accurate(t, cols.data(), d, 0, full->N, 0, full->N, sd->rows_dev.p, s.beta.data());
            else v = lg_fit_accurate(t, cols.data(), d, 0, sd->n_cv, 0, sd->n_cv, nullptr, s.beta.data());
        }
        return bic_lg(full->N, p, v);
    }
    const bool cv = kind == PBN_SCORE_CVLIK;
    double acc = 0.0;
    for (int f = 0; f < (cv ? sd->k : 1); ++f) {
        const Stats* tr = &sd->all;
        const Stats* te = &sd->hold;
        if (cv) { stats_minus(sd->all, sd->fold[f], s.train); tr = &s.train; te = &sd->fold[f]; }
        subset_moments(sd, *tr, cols.data(), d, s.mu.data(), s.sse.data());
        bool suspect = false;
        double v = lg_fit(tr->N, p, s.mu.data(), s.sse.data(), s.beta.data(), &suspect);
        if (suspect && lg_guard_on() && d <= 16) {
            if (cv) v = lg_fit_accurate(t, cols.data(), d, 0, sd->limits[f], sd->limits[f + 1], tr->N, nullptr, s.beta.data());
            else v = lg_fit_accurate(t, cols.data(), d, 0, sd->n_cv, 0, sd->n_cv, nullptr, s.beta.data());
            // and the test fold's log-likelihood from its rows, as the reference evaluates it
            const int64_t te0 = cv ? sd->limits[f] : sd->n_cv;
            acc += lg_slogl_from_rows(t, cols.data(), d, te0, te->N, nullptr, s.beta.data(), v);
            continue;
        }
        acc += lg_slogl_from_moments(sd, *te, cols.data(), p, s.beta.data(), v);
    }
    return acc;
}

// hybrid CKDE candidates of a call go into one HybridBatch (hybrid.hip): begun with the first of them, enqueued as they come, finished
// together after the candidate loop
struct LazyHybridBatch {
    pbn_scoredata* sd;
    const bool on = knob_int("PBN_HYBRID_BATCH", 1) != 0;   // (per call: the tests switch it)
    std::unique_ptr<HybridBatch, void (*)(HybridBatch*) noexcept> hb{nullptr, hybrid_batch_end};
    HybridBatch* get() {
        if (!on) return nullptr;
        if (!hb) hb.reset(hybrid_batch_begin(sd));
        return hb.get();
    }
};

// A candidate with a discrete column (cols = [variable, parents]): the memo, the hand-off of an all-discrete family to the call's
// discrete batch, or score_hybrid - whose score may arrive only when the hybrid batch is flushed.
// Likelihood scores of DiscreteAdaptator factors cost k x configurations sweeps / Gram passes each, and a hill-climb asks for the same
// (variable, type, parent SET) again and again: every RemoveArc cell is the local score the node had before that arc was added, every
// FlipArc cell's source side likewise.  They are remembered by parent set (score_hybrid evaluates the continuous parents in ascending
// order and the discrete ones in canonical order: the value does not depend on the order they were given in).  BIC stays out: bic_clg ties.
void score_hybrid_candidate(pbn_scoredata* sd, const BatchArgs& a, int c, int nt, const std::vector<int>& cols, LazyHybridBatch& batch,
                            std::vector<DiscreteCand>& discrete) {
    const int kind = a.kind, p = (int)cols.size() - 1;
    double* out = a.out + c;
    if (a.parts_out) {   // a share of the candidate: never memoised
        HybridParts hp{a.parts_rank, a.parts_world, a.parts_out + (size_t)c * PBN_HYBRID_PARTS};
        HybridSink sink{out, {}};
        *out = score_hybrid(sd, kind, cols[0], nt, cols.data() + 1, p, &hp, batch.get(), &sink);
        return;
    }
    const bool memo = score_memo_on() && !sd->force_precise && (kind == PBN_SCORE_CVLIK || kind == PBN_SCORE_HOLDOUT);   // (discrete factors too)
    std::vector<int> key;
    if (memo) {
        key.assign(cols.begin() + 1, cols.end());
        std::sort(key.begin(), key.end());
        key.insert(key.begin(), {kind, nt, cols[0]});
        auto it = sd->score_memo.find(key);
        if (it != sd->score_memo.end()) { *out = it->second; ++sd->memo_hits; return; }
    }
    if (cols[0] >= sd->n) {
        check_discrete_candidate(sd, kind, nt, cols.data() + 1, p);
        discrete.push_back(DiscreteCand{cols[0], std::vector<int>(cols.begin() + 1, cols.end()), out, key});
        return;
    }
    HybridSink sink{out, key};   // (key empty without the memo)
    bool deferred = false;
    *out = score_hybrid(sd, kind, cols[0], nt, cols.data() + 1, p, nullptr, batch.get(), &sink, &deferred);
    if (memo && !deferred) sd->score_memo[key] = *out;
}

}  // namespace

void score_batch_body(pbn_scoredata* sd, const BatchArgs& a) {
    if (!sd || !a.var || !a.par_off || !a.out) throw invalid_error("pbn_score_batch: null argument");
    pbn_ctx* ctx = sd->ctx;
    const int kind = a.kind;
    if (sd->partial) throw invalid_error("pbn_score_batch: row-sharded score data needs pbn_scoredata_moments(set) first");
    HIP_CHECK(hipSetDevice(ctx->device));
    if ((kind == PBN_SCORE_CVLIK) && sd->k <= 0) throw invalid_error("pbn_score_batch: score data has no CV folds");
    if ((kind == PBN_SCORE_HOLDOUT) && sd->n_hold <= 0) throw invalid_error("pbn_score_batch: score data has no hold-out split");
    // The set-function cache and the local-score memo grow by one entry per (region, configuration, term) and per hybrid
    // candidate (~150 B a node): a long search over hybrid candidates would take gigabytes.  Both are pure accelerators -
    // beyond PBN_SCORE_CACHE_ENTRIES entries (default 2^21, ~300 MB) they start over, at a batch boundary (no entry of
    // the batch being assembled is lost).
    if (sd->kde_cache.size() > score_cache_budget()) { sd->kde_cache.clear(); ++sd->cache_resets; }
    // (term_total is trimmed in pbn_score_terms_put only: every rank of a job reaches that call with the same state, whereas a rank
    //  whose dealt list is empty skips the evaluation call - trimming here would let the ranks' "missing" lists drift apart)
    if (sd->score_memo.size() > score_cache_budget()) { sd->score_memo.clear(); ++sd->cache_resets; }
    if (kind < PBN_SCORE_BIC || kind > PBN_SCORE_BDE) throw invalid_error("pbn_score_batch: unknown score kind");
    if (kind == PBN_SCORE_BGE && sd->discrete_only) throw invalid_error("BGe is not defined for networks with discrete variables.");
    // BDe: the imaginary sample size; the discrete candidates of the call (variable a dictionary column) are collected here, counted
    // together - all their families in one device pass - and finished after the loop (hybrid.hip, family_counts.hip)
    const double bde_iss = (kind == PBN_SCORE_BDE && a.n_params >= 1 && a.params) ? a.params[0] : 1.0;
    if (kind == PBN_SCORE_BDE && !(bde_iss > 0)) throw invalid_error("BDe: the imaginary sample size must be positive");
    BgeParams bge{1, (double)(sd->n + 2), sd->n, nullptr};
    if (kind == PBN_SCORE_BGE) {
        if (a.n_params >= 1) bge.iss_mu = a.params[0];
        if (a.n_params >= 2) bge.iss_w = a.params[1];
        if (a.n_params >= 3) bge.total_nodes = (int)a.params[2];
        if (a.n_params >= 3 + sd->n) bge.nu = a.params + 3;
    }
    ScoreScratch s;
    std::vector<DiscreteCand> discrete;
    std::vector<int> pending;   // plain CKDE candidates
    LazyHybridBatch hbatch{sd};
    const MaskedPlan plan = masked_prepass(sd, a, s.cols);
    const bool likelihood = kind == PBN_SCORE_CVLIK || kind == PBN_SCORE_HOLDOUT;
    for (int c = 0; c < a.n_cand; ++c) {
        candidate_cols(a, c, s.cols);
        bool hybrid = false;
        for (int cc : s.cols) {
            if (cc < 0 || cc >= sd->n + sd->n_disc) throw invalid_error("pbn_score_batch: column out of range");
            if (cc >= sd->n) hybrid = true;
        }
        const int nt = a.node_type ? a.node_type[c] : PBN_NODE_LG;
        if (hybrid) { score_hybrid_candidate(sd, a, c, nt, s.cols, hbatch, discrete); continue; }
        if (kind == PBN_SCORE_BDE) throw invalid_error("BDe is defined for discrete variables with discrete parents only.");
        if (!likelihood || nt == PBN_NODE_LG) { a.out[c] = score_gaussian_candidate(sd, kind, nt, bge, plan, s); continue; }
        if (nt != PBN_NODE_CKDE) throw invalid_error("pbn_score_batch: unknown node type");
        ctx->scratch_misc.reserve(1);  // touched by kde_eval_enqueue
        pending.push_back(c);
    }
    hybrid_batch_flush(hbatch.hb.get());   // (before the plain CKDE units take the context's result slots)
    hbatch.hb.reset();
    score_discrete_batch(sd, kind, bde_iss, discrete);
    if (!pending.empty()) score_ckde_terms(sd, a, pending, s);
}

int score_batch_local(pbn_scoredata* sd, int kind, int n_cand, const int* var, const int* node_type, const int* par_off, const int* parents,
                      const double* params, int n_params, double* out) {
    BatchArgs a;
    a.kind = kind; a.n_cand = n_cand; a.var = var; a.node_type = node_type; a.par_off = par_off; a.parents = parents;
    a.params = params; a.n_params = n_params; a.out = out;
    return guarded(mu_of(sd), [&] { score_batch_body(sd, a); });
}

}  // namespace score
}  // namespace pbn

extern "C" {

int pbn_scoredata_set_precise(pbn_scoredata* sd, int on) {
    return guarded(mu_of(sd), [&] {
        if (!sd) throw invalid_error("pbn_scoredata_set_precise: null handle");
        sd->force_precise = on != 0;
    });
}

int pbn_score_batch(pbn_scoredata* sd, int kind, int n_cand, const int* var, const int* node_type, const int* par_off,
                    const int* parents, const double* params, int n_params, double* out) {
    if (sd && sd->has_comm) {   // one process per GPU (pbn_scoredata_set_comm): this rank's share + one all-gather (shard.hip)
        // (no lock held across the host's collective: the evaluations inside take the handle's lock themselves)
        try {
            pbn::score::score_batch_sharded(sd, kind, n_cand, var, node_type, par_off, parents, params, n_params, out);
            return PBN_OK;
        } catch (const invalid_error& e) { set_last_error(e.what()); return PBN_ERR_INVALID;
        } catch (const singular_error& e) { set_last_error(e.what()); return PBN_ERR_SINGULAR;
        } catch (const std::exception& e) { set_last_error(e.what()); return PBN_ERR_DEVICE; }
    }
    return pbn::score::score_batch_local(sd, kind, n_cand, var, node_type, par_off, parents, params, n_params, out);
}

}  // extern "C"

