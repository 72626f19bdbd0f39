// RCoT: the randomized conditional correlation test (learning/independences/continuous/RCoT.{hpp,cpp}; the weighted chi-square
// sums of util/chisquaresum.hpp).  SURVEY.md §2 row 13.
//
// A test x _||_ y | Z maps every row to random Fourier features f = sqrt(2) cos(v W + b) of x (nxy of them), y (nxy) and Z (nz),
// standardises them, and compares the residual cross-covariance of the x and y features (after the linear projection on the Z
// features) with its null law, a weighted sum of chi-squares whose weights are the eigenvalues of the uncentred covariance of
// the nxy^2 residual products rx_i ry_j.  The reference materialises the N x (2 nxy + nz) feature matrix and does the covariance
// and projection work as dense products on one CPU thread.  Here a test is two device passes over its rows, and the features are
// generated in LDS and never written to memory:
//   K1 (rcot_gram_kernel)  features of a 16-row chunk -> LDS; the Gram of [f, 1] (sums, cross products, the valid-row count in
//                          its last column) on v_mfma_f64_16x16x4_f64, the tile pairs spread over the block's four waves;
//   host                   means, sds, the normalised covariance blocks, (Czz + 1e-10 I)^-1, Cxy_z, sta, and ONE coefficient
//                          matrix P ((F + 1) x 2 nxy) with [rx | ry] = [f, 1] P (normalisation and projection folded);
//   K2 (rcot_prod_kernel)  the same features again (same instructions on the same inputs: the same bits), [f, 1] P on MFMA
//                          (k-steps split over the waves), the nxy^2 products, and their uncentred Gram on MFMA.
// Per-block partials are summed in block order by rcot_reduce_kernel.  A batch of tests shares one K1 and one K2 launch (per
// memory chunk); the row partition of a test depends only on the table's row count, so its result does not depend on the batch.
//
// Deliberate differences from the reference (DESIGN.md "RCoT"):
//  * Seeding: every test draws W and b from std::mt19937 seeded by a std::seed_seq of (handle seed, min(x, y), max(x, y), the
//    sorted Z set actually used, the role) - the role being the smaller variable, the larger one, or Z - in the reference's draw
//    order inside a role (W column by column from std::normal_distribution<double>, then b from std::uniform_real_distribution
//    <double>).  The reference seeds from std::random_device in every call; here a p-value is a pure function of (seed, test),
//    symmetric in x and y and in the order of Z.
//  * fp32 tables are promoted to fp64 and every feature / Gram is fp64 (the reference computes in float): more accurate, not
//    bit-compatible.
//  * Nulls with several Z columns: the reference's contains_null branch of pvalue(x, y, vector) loops on `z_sse.rows()` as its
//    condition (never false); here it does what its null-free branch does, on the rows valid in all of the test's variables.
//  * HBE at a statistic below the support of its gamma law answers 1 (boost raises a domain error there); no positive weight
//    at all answers 1.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <complex>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <random>
#include <vector>

#include "common.hpp"
#include "hostmath.hpp"
#include "specfun.hpp"

using namespace pbn;

#define RCOT_MAX_FP 256      // 2 nxy + nz + 1 (the ones column) <= 256: at most 16 column tiles in K1
#define RCOT_MAX_NXY 8       // nxy^2 <= 64 products: at most 4 column tiles in K2
#define RCOT_MAX_IN 64       // x, y and at most 62 conditioning columns
#define RCOT_CHUNK 16        // rows per LDS chunk (four k-steps of 16x16x4)
#define RCOT_SIGMA_ROWS 500  // rf_sigma_impl's window
#define RCOT_PILOT_ROWS 64   // rows of the window whose feature means are the pilot shifts

namespace {

typedef double d4 __attribute__((ext_vector_type(4)));

struct RcotTest {
    int32_t col[RCOT_MAX_IN];   // input columns: x (the smaller index), y, the k Z columns used (sorted), then validity-only ones
    int32_t nin;                // 2 + k + the validity-only columns
    int32_t k;                  // Z columns made into features
    int32_t F;                  // features: 2 nxy + (k ? nz : 0); column F of [f, 1] is the ones column
    int32_t nxy;
    int32_t nt;                 // K1 column tiles: ceil((F + 1) / 16)
    int32_t kw;                 // W row length: max(1, k)
    int32_t ntq;                // K2 product tiles: ceil(nxy^2 / 16)
    int64_t par;                // offset in the parameter buffer: W [16 nt][kw], then b [16 nt], then the pilot shift [16 nt]
    int64_t proj;               // offset in the parameter buffer: P [16 nt][16] (row = feature, column = residual; rx 0 .. nxy-1, ry nxy .. 2 nxy-1)
};

// feature c of a row (values v[0 .. nin-1] in LDS) minus its pilot shift (the feature's mean over the first rows of the test, taken
// on the host: the Gram of the shifted features has no cancellation against n m m^T, and neither has the folded projection P); the
// same function, with rounding fixed by explicit intrinsics, in K1 and K2
__device__ __forceinline__ double rcot_feature(const double* v, int c, int F, int nxy, int k, int kw, const double* W, const double* b,
                                               const double* shift) {
    if (c >= F) return c == F ? 1.0 : 0.0;
    const double* w = W + (size_t)c * kw;
    double acc;
    if (c < nxy) acc = __dmul_rn(v[0], w[0]);
    else if (c < 2 * nxy) acc = __dmul_rn(v[1], w[0]);
    else {
        acc = __dmul_rn(v[2], w[0]);
        for (int d = 1; d < k; ++d) acc = __fma_rn(v[2 + d], w[d], acc);
    }
    return __dsub_rn(__dmul_rn(1.4142135623730950488, cos(__dadd_rn(acc, b[c]))), shift[c]);
}

// LDS row stride of the feature chunk: 16 mod 32 doubles, so that the four rows of a k-step fall on distinct banks
__host__ __device__ __forceinline__ int rcot_stride(int fp) { return (fp % 32 == 16) ? fp : fp + 16; }
inline int lds_stride(int fp) { return rcot_stride(fp); }

// one 16-row chunk: stage the inputs, mark the valid rows, evaluate the features of [f, 1] (zero on rows that are not valid)
__device__ __forceinline__ void rcot_fill(const double* __restrict__ cols, int64_t N, const RcotTest& t, const double* W, const double* b,
                                          const double* shift, int64_t r0, int64_t r1, double* vals, int vs, int* valid, double* feat, int S) {
    const int tid = threadIdx.x;
    for (int e = tid; e < RCOT_CHUNK * t.nin; e += 256) {
        const int r = e % RCOT_CHUNK, d = e / RCOT_CHUNK;
        const int64_t row = r0 + r;
        vals[r * vs + d] = row < r1 ? cols[(int64_t)t.col[d] * N + row] : NAN;
    }
    __syncthreads();
    if (tid < RCOT_CHUNK) {
        int ok = 1;
        for (int d = 0; d < t.nin; ++d) ok &= !isnan(vals[tid * vs + d]);
        valid[tid] = ok;
    }
    __syncthreads();
    const int fp = 16 * t.nt;
    const int k = t.k;
    for (int e = tid; e < RCOT_CHUNK * fp; e += 256) {
        const int r = e / fp, c = e % fp;
        feat[r * S + c] = valid[r] ? rcot_feature(vals + r * vs, c, t.F, t.nxy, k, t.kw, W, b, shift) : 0.0;
    }
    __syncthreads();
}

// block table: [4 b] test, [4 b + 1] first row, [4 b + 2] end row, [4 b + 3] offset of the block's partial.
// Dynamic LDS, sized by the launch's largest test: feat [16][S] (S = the largest rcot_stride), vals [16][vs] (vs = the largest 2 + k),
// and in K2 also P [16 nt][16] - a launch of no-Z tests (F = 10: one tile) takes a few KB and runs several blocks per CU.
template <int PPW>
__global__ __launch_bounds__(256) void rcot_gram_kernel(const double* __restrict__ cols, int64_t N, const RcotTest* __restrict__ tests,
                                                        const double* __restrict__ par, const int64_t* __restrict__ blk, double* __restrict__ part,
                                                        int s_max, int vs) {
    extern __shared__ double smem[];
    double* feat = smem;
    double* vals = smem + RCOT_CHUNK * s_max;
    __shared__ int valid[RCOT_CHUNK];
    const RcotTest& t = tests[blk[4 * blockIdx.x]];
    const int64_t row0 = blk[4 * blockIdx.x + 1], row1 = blk[4 * blockIdx.x + 2];
    double* out = part + blk[4 * blockIdx.x + 3];
    const double* W = par + t.par;
    const double* b = W + (size_t)16 * t.nt * t.kw;
    const double* shift = b + 16 * t.nt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = rcot_stride(16 * t.nt);
    const int np = t.nt * (t.nt + 1) / 2;
    int pi[PPW], pj[PPW];
#pragma unroll
    for (int q = 0; q < PPW; ++q) {   // pair p = wave + 4 q -> tiles (I, J), I <= J, row-major over the upper triangle
        int p = wave + 4 * q, I = 0;
        if (p >= np) p = 0;
        while (p >= t.nt - I) { p -= t.nt - I; ++I; }
        pi[q] = I; pj[q] = I + p;
    }
    d4 acc[PPW];
#pragma unroll
    for (int q = 0; q < PPW; ++q) acc[q] = d4{0, 0, 0, 0};
    for (int64_t r0 = row0; r0 < row1; r0 += RCOT_CHUNK) {
        rcot_fill(cols, N, t, W, b, shift, r0, row1, vals, vs, valid, feat, S);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double* fr = feat + (4 * s + (lane >> 4)) * S + (lane & 15);
#pragma unroll
            for (int q = 0; q < PPW; ++q)
                if (wave + 4 * q < np) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[16 * pi[q]], fr[16 * pj[q]], acc[q], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PPW; ++q)
        if (wave + 4 * q < np)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(wave + 4 * q) * 256 + lane * 4 + r] = acc[q][r];
}

// K2: residuals [rx | ry] = [f, 1] P, the nxy^2 products rx_i ry_j, their uncentred Gram (at most 4 tiles: 10 pairs, 3 per wave)
__global__ __launch_bounds__(256) void rcot_prod_kernel(const double* __restrict__ cols, int64_t N, const RcotTest* __restrict__ tests,
                                                        const double* __restrict__ par, const int64_t* __restrict__ blk, double* __restrict__ part,
                                                        int s_max, int vs) {
    extern __shared__ double smem[];
    double* feat = smem;
    double* vals = smem + RCOT_CHUNK * s_max;
    double* Pl = vals + RCOT_CHUNK * vs;
    __shared__ int valid[RCOT_CHUNK];
    __shared__ double red[4][RCOT_CHUNK][17];
    __shared__ double res[RCOT_CHUNK][17];
    __shared__ double prod[RCOT_CHUNK][65];
    const RcotTest& t = tests[blk[4 * blockIdx.x]];
    const int64_t row0 = blk[4 * blockIdx.x + 1], row1 = blk[4 * blockIdx.x + 2];
    double* out = part + blk[4 * blockIdx.x + 3];
    const double* W = par + t.par;
    const double* b = W + (size_t)16 * t.nt * t.kw;
    const double* shift = b + 16 * t.nt;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fp = 16 * t.nt, S = rcot_stride(fp);
    for (int e = tid; e < fp * 16; e += 256) Pl[e] = par[t.proj + e];
    const int nq = t.nxy * t.nxy, qp = 16 * t.ntq;
    const int np = t.ntq * (t.ntq + 1) / 2;
    int pi[3], pj[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        int p = wave + 4 * q, I = 0;
        if (p >= np) p = 0;
        while (p >= t.ntq - I) { p -= t.ntq - I; ++I; }
        pi[q] = I; pj[q] = I + p;
    }
    d4 acc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) acc[q] = d4{0, 0, 0, 0};
    for (int64_t r0 = row0; r0 < row1; r0 += RCOT_CHUNK) {
        rcot_fill(cols, N, t, W, b, shift, r0, row1, vals, vs, valid, feat, S);   // (its first barrier also covers the Pl fill)
        // projection: wave w takes k-steps w, w + 4, ...; A[i][k] = feature k of row i, B[k][j] = P[k][j]
        d4 pr = d4{0, 0, 0, 0};
        for (int s = wave; s < fp / 4; s += 4) {
            const int kk = 4 * s + (lane >> 4);
            pr = __builtin_amdgcn_mfma_f64_16x16x4f64(feat[(lane & 15) * S + kk], Pl[kk * 16 + (lane & 15)], pr, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave][(lane >> 4) + 4 * r][lane & 15] = pr[r];
        __syncthreads();
        {
            const int row = tid >> 4, c = tid & 15;
            res[row][c] = ((red[0][row][c] + red[1][row][c]) + red[2][row][c]) + red[3][row][c];
        }
        __syncthreads();
        for (int e = tid; e < RCOT_CHUNK * qp; e += 256) {
            const int row = e / qp, c = e % qp;
            prod[row][c] = c < nq ? res[row][c / t.nxy] * res[row][t.nxy + c % t.nxy] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const double* fr = &prod[4 * s + (lane >> 4)][lane & 15];
#pragma unroll
            for (int q = 0; q < 3; ++q)
                if (wave + 4 * q < np) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(fr[16 * pi[q]], fr[16 * pj[q]], acc[q], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
        if (wave + 4 * q < np)
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(size_t)(wave + 4 * q) * 256 + lane * 4 + r] = acc[q][r];
}

// sum of a test's block partials in block order: grid (elements / 256, tests); seg[4 t] first partial offset, [4 t + 1] number of
// blocks, [4 t + 2] elements (the test's pairs x 256), [4 t + 3] offset of its output
__global__ __launch_bounds__(256) void rcot_reduce_kernel(const double* __restrict__ part, const int64_t* __restrict__ seg, double* __restrict__ out) {
    const int64_t off = seg[4 * blockIdx.y], nb = seg[4 * blockIdx.y + 1], ws = seg[4 * blockIdx.y + 2], oo = seg[4 * blockIdx.y + 3];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= ws) return;
    double v = 0.0;
    for (int64_t i = 0; i < nb; ++i) v += part[off + i * ws + e];
    out[oo + e] = v;
}

// ---- host maths ------------------------------------------------------------------------------------------------------------------

// Brent's root finder on [ax, bx] (Forsythe, Malcolm & Moler's zeroin, as util/uniroot.hpp uses it): bisection safeguarding
// inverse quadratic / secant steps; throws when maxit iterations do not reach the tolerance 4 eps |b| + tol.
template <typename F>
double brent_root(F f, double ax, double bx, double tol, int maxit) {
    double a = ax, b = bx, c = a;
    double fa = f(a), fb = f(b), fc = fa;
    if (fa == 0.0) return a;
    if (fb == 0.0) return b;
    for (int it = 0; it <= maxit; ++it) {
        const double prev = b - a;
        if (std::fabs(fc) < std::fabs(fb)) {
            a = b; b = c; c = a;
            fa = fb; fb = fc; fc = fa;
        }
        const double tol_act = 2.0 * std::numeric_limits<double>::epsilon() * std::fabs(b) + tol / 2;
        double step = (c - b) / 2;
        if (std::fabs(step) <= tol_act || fb == 0.0) return b;
        if (std::fabs(prev) >= tol_act && std::fabs(fa) > std::fabs(fb)) {
            double p, q;
            const double cb = c - b;
            if (a == c) {
                const double t1 = fb / fa;
                p = cb * t1;
                q = 1.0 - t1;
            } else {
                const double qa = fa / fc, t1 = fb / fc, t2 = fb / fa;
                p = t2 * (cb * qa * (qa - t1) - (b - a) * (t1 - 1.0));
                q = (qa - 1.0) * (t1 - 1.0) * (t2 - 1.0);
            }
            if (p > 0) q = -q;
            else p = -p;
            if (p < 0.75 * cb * q - std::fabs(tol_act * q) / 2 && p < std::fabs(prev * q / 2)) step = p / q;
        }
        if (std::fabs(step) < tol_act) step = step > 0 ? tol_act : -tol_act;
        a = b; fa = fb;
        b += step;
        fb = f(b);
        if ((fb > 0 && fc > 0) || (fb < 0 && fc < 0)) { c = a; fc = fa; }
    }
    throw invalid_error("RCoT: root finder did not converge");
}

// Real parts of the four roots of c[0] x^4 + c[1] x^3 + ... + c[4] (Aberth-Ehrlich iteration, then Newton polishing)
void quartic_real_parts(const double* c, double* re) {
    typedef std::complex<double> cd;
    if (!(c[0] != 0.0) || !std::isfinite(c[0])) throw invalid_error("RCoT: degenerate quartic");
    double a[5];
    for (int i = 0; i < 5; ++i) {
        a[i] = c[i] / c[0];
        if (!std::isfinite(a[i])) throw invalid_error("RCoT: degenerate quartic");
    }
    auto poly = [&](cd x, cd& d) {
        cd p = a[0], dp = 0.0;
        for (int i = 1; i < 5; ++i) { dp = dp * x + p; p = p * x + a[i]; }
        d = dp;
        return p;
    };
    double bound = 0.0;
    for (int i = 1; i < 5; ++i) bound = std::max(bound, std::fabs(a[i]));
    const double radius = 1.0 + bound;
    cd z[4];
    for (int k = 0; k < 4; ++k) z[k] = std::polar(0.5 * radius, 0.4 + 2.0 * M_PI * k / 4.0);
    for (int it = 0; it < 500; ++it) {
        double moved = 0.0;
        for (int k = 0; k < 4; ++k) {
            cd d;
            const cd p = poly(z[k], d);
            if (p == 0.0) continue;
            const cd ratio = p / d;
            cd s = 0.0;
            for (int j = 0; j < 4; ++j)
                if (j != k) s += 1.0 / (z[k] - z[j]);
            const cd w = ratio / (1.0 - ratio * s);
            z[k] -= w;
            moved = std::max(moved, std::abs(w) / std::max(1.0, std::abs(z[k])));
        }
        if (moved < 1e-15) break;
    }
    for (int k = 0; k < 4; ++k) {
        for (int it = 0; it < 3; ++it) {
            cd d;
            const cd p = poly(z[k], d);
            if (d == 0.0) break;
            z[k] -= p / d;
        }
        re[k] = z[k].real();
        if (!std::isfinite(re[k])) throw invalid_error("RCoT: quartic roots not finite");
    }
}

// Solve the n x n system a x = rhs (column-major; LU with partial pivoting); throws when singular
void lu_solve(std::vector<double> a, int n, std::vector<double>& x) {
    std::vector<int> piv(n);
    if (hm::lu(a.data(), n, piv.data()) == 0) throw invalid_error("RCoT: singular system");
    for (int k = 0; k < n; ++k) std::swap(x[k], x[piv[k]]);
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < i; ++k) x[i] -= a[i + k * n] * x[k];
    for (int i = n - 1; i >= 0; --i) {
        for (int k = i + 1; k < n; ++k) x[i] -= a[i + k * n] * x[k];
        x[i] /= a[i + i * n];
    }
    for (double v : x)
        if (!std::isfinite(v)) throw invalid_error("RCoT: singular system");
}

// Hall-Buckley-Eagleson: a gamma law matching the first three cumulants
double hbe_sf(const std::vector<double>& w, double q) {
    if (w.empty()) return 1.0;
    double k1 = 0, s2 = 0, s3 = 0;
    for (double v : w) { k1 += v; s2 += v * v; s3 += v * v * v; }
    const double k2 = 2 * s2, k3 = 8 * s3;
    const double nu = 8 * (k2 * k2 * k2) / (k3 * k3);
    const double stat = std::sqrt(2 * nu / k2) * (q - k1) + nu;
    if (!std::isfinite(stat) || !std::isfinite(nu) || !(nu > 0)) throw invalid_error("RCoT: HBE approximation undefined for these weights");
    if (stat <= 0) return 1.0;   // below the support of the gamma law
    return gamma_q(nu / 2, stat / 2);
}

// Lindsay-Pilla-Basak with four support points: moments from the cumulants, the lambda-modified moment determinants, the
// quartic of the support points, the mixture weights from a Vandermonde system, a mixture of gamma tails.  Throws on any
// degenerate step (the caller falls back to HBE).
double lpb4_sf(const std::vector<double>& w, double q) {
    const int p = 4, nm = 2 * p;
    if ((int)w.size() < p) throw invalid_error("lbp4 requires at least 4 coefficients.");
    double kap[nm + 1] = {0}, mom[nm + 1] = {0};
    double fact = 1.0;   // 2^(r-1) (r-1)!
    for (int r = 1; r <= nm; ++r) {
        if (r > 1) fact *= 2.0 * (r - 1);
        double s = 0;
        for (double v : w) s += std::pow(v, r);
        kap[r] = fact * s;
    }
    mom[0] = 1.0;
    for (int n = 1; n <= nm; ++n) {   // m_n = sum_j C(n-1, j-1) kappa_j m_(n-j)
        double s = 0, binom = 1.0;
        for (int j = 1; j <= n; ++j) {
            s += binom * kap[j] * mom[n - j];
            binom = binom * (n - j) / j;
        }
        mom[n] = s;
    }
    // delta(i, j) = m_(i+j) / prod_(l=1)^(i+j-1) (1 + l lambda), size s x s
    auto delta = [&](int s, double lam) {
        std::vector<double> d((size_t)s * s);
        for (int j = 0; j < s; ++j)
            for (int i = 0; i < s; ++i) {
                double den = 1.0;
                for (int l = 1; l <= i + j - 1; ++l) den *= 1.0 + l * lam;
                d[i + (size_t)j * s] = mom[i + j] / den;
            }
        return d;
    };
    double lam = mom[2] / (mom[1] * mom[1]) - 1.0;
    for (int i = 2; i <= p; ++i) {
        auto f = [&](double x) { auto d = delta(i + 1, x); return hm::determinant(d.data(), i + 1); };
        lam = brent_root(f, 0.0, lam, 1e-9, 1000);
    }
    auto M = delta(p + 1, lam);
    double coef[p + 1];
    for (int i = 0; i <= p; ++i) {   // coefficient of x^i: the determinant with the last column e_i
        auto Mi = M;
        for (int r = 0; r <= p; ++r) Mi[r + (size_t)p * (p + 1)] = r == i ? 1.0 : 0.0;
        coef[p - i] = hm::determinant(Mi.data(), p + 1);
    }
    double mu[p];
    quartic_real_parts(coef, mu);
    std::vector<double> V((size_t)p * p), pi(p);
    for (int c = 0; c < p; ++c) {
        double pw = 1.0;
        for (int r = 0; r < p; ++r) { V[r + (size_t)c * p] = pw; pw *= mu[c]; }
    }
    for (int r = 0; r < p; ++r) {
        double den = 1.0;
        for (int l = 1; l <= r - 1; ++l) den *= 1.0 + l * lam;
        pi[r] = mom[r] / den;
    }
    lu_solve(V, p, pi);
    const double shape = 1.0 / lam;
    if (!(shape > 0) || !std::isfinite(shape)) throw invalid_error("RCoT: LPB4 shape out of range");
    double res = 0;
    for (int i = 0; i < p; ++i) {
        const double theta = mu[i] * lam;
        if (!(theta > 0) || !std::isfinite(theta)) throw invalid_error("Wrong theta parameter.");
        res += pi[i] * gamma_q(shape, q / theta);
    }
    if (!std::isfinite(res)) throw invalid_error("RCoT: LPB4 not finite");
    return res;
}

// method 0: the reference's rule (HBE below 4 positive weights, else LPB4 falling back to HBE); 1: HBE; 2: LPB4 only.  *used:
// 1 = HBE answered, 2 = LPB4 answered.  Negative results become 0.
double chisq_sum_sf(const double* weights, int n, double q, int method, int* used) {
    std::vector<double> w;
    for (int i = 0; i < n; ++i)
        if (weights[i] > 0) w.push_back(weights[i]);
    double p;
    int u = 1;
    if (method == 2) { p = lpb4_sf(w, q); u = 2; }
    else if (method == 1 || (int)w.size() < 4) p = hbe_sf(w, q);
    else {
        try { p = lpb4_sf(w, q); u = 2; }
        catch (const std::exception&) { p = hbe_sf(w, q); u = 1; }
    }
    if (used) *used = u;
    return p < 0 ? 0.0 : p;
}

// rf_sigma_impl: median Euclidean distance between the first min(500, n) rows; 0 -> 1.  rows[d][i] (i < n)
double rf_sigma(const std::vector<const double*>& cols, const std::vector<int64_t>& rows) {
    const int64_t r = std::min<int64_t>(RCOT_SIGMA_ROWS, (int64_t)rows.size());
    const size_t d = cols.size();
    std::vector<double> win((size_t)r * d);   // the window's rows, row-major
    for (int64_t i = 0; i < r; ++i)
        for (size_t c = 0; c < d; ++c) win[(size_t)i * d + c] = cols[c][rows[(size_t)i]];
    std::vector<double> dist((size_t)(r * (r - 1) / 2));
    size_t o = 0;
    for (int64_t i = 1; i < r; ++i)
        for (int64_t j = 0; j < i; ++j) {
            double s = 0;
            for (size_t c = 0; c < d; ++c) { const double t = win[(size_t)j * d + c] - win[(size_t)i * d + c]; s += t * t; }
            dist[o++] = std::sqrt(s);
        }
    if (dist.empty()) return 1.0;
    const size_t m = dist.size() / 2;
    double median;
    if (dist.size() % 2 == 1) {
        std::nth_element(dist.begin(), dist.begin() + m, dist.end());
        median = dist[m];
    } else {
        std::nth_element(dist.begin(), dist.begin() + m, dist.end());   // the lower middle value: the largest of the m below it
        median = 0.5 * (*std::max_element(dist.begin(), dist.begin() + m) + dist[m]);
    }
    return median == 0 ? 1.0 : median;
}

}  // namespace

struct pbn_rcot {
    pbn::ctx_ptr ctx;
    int64_t N = 0;
    int n_vars = 0, nxy = 5, nz = 100;
    uint32_t seed = 0;
    std::vector<std::vector<double>> cols;   // normalised host columns (NaN = null)
    std::vector<char> has_null, constant;    // constant: every valid value equal (sse 0)
    std::vector<double> sigma1;              // rf_sigma of each null-free column alone
    std::vector<int> order;                  // pbn_rcot_set_order: callback index -> column
    pbn::dev_buf<double> d_cols;             // [n_vars][N]
    pbn::dev_buf<double> d_par, d_part, d_out;
    pbn::dev_buf<int64_t> d_blk, d_seg;
    pbn::dev_buf<RcotTest> d_tests;
};

namespace {

struct Plan {
    int a = 0, b = 0;
    std::vector<int> z;          // conditioning columns used (sorted, constant ones dropped)
    std::vector<int> zv;         // every Z column dropped: those with nulls, read for validity only (the reference's rows for RIT)
    bool trivial = false;        // x or y constant: p = 1
    int F = 0, k = 0;
    double sigma[3] = {0, 0, 0};
    std::vector<double> W, bias; // W: x (nxy), y (nxy), z (k x nz, d fastest); bias: x, y, z
    std::vector<double> shift;   // pilot shift of every feature (F): its mean over the first RCOT_PILOT_ROWS rows of the window
    int64_t n_valid = 0;
    std::vector<double> P;       // [16 nt][16]
    double sta = 0;
    std::vector<double> eig;     // positive eigenvalues
    int used = 0;                // 0 trivial, 1 HBE, 2 LPB4
    double p = 1.0;
    int nt() const { return (F + 1 + 15) / 16; }
};

int64_t rows_per_block(int64_t N) { return std::max<int64_t>(1024, (ceil_div(N, 512) + 15) / 16 * 16); }

void seed_rng(std::mt19937& rng, const pbn_rcot* h, const Plan& pl, uint32_t role) {
    std::vector<uint32_t> words{h->seed, (uint32_t)pl.a, (uint32_t)pl.b, (uint32_t)pl.z.size(), role};
    for (int c : pl.z) words.push_back((uint32_t)c);
    std::seed_seq sq(words.begin(), words.end());
    rng.seed(sq);
}

// random_fourier_features' draws for one role: W (dims x nf) column by column, scaled by 1 / sigma, then b * 2 pi
void draw(const pbn_rcot* h, const Plan& pl, uint32_t role, int dims, int nf, double sigma, double* W, double* b) {
    std::mt19937 rng;
    seed_rng(rng, h, pl, role);
    std::normal_distribution<double> normal;
    for (int j = 0; j < nf; ++j)
        for (int i = 0; i < dims; ++i) W[i + (size_t)j * dims] = normal(rng) * (1 / sigma);
    std::uniform_real_distribution<double> unif;
    for (int j = 0; j < nf; ++j) b[j] = unif(rng) * (2 * M_PI);
}

Plan plan_test(pbn_rcot* h, int v1, int v2, int n_cond, const int* cond) {
    auto map = [&](int v) {
        if (!h->order.empty()) {
            if (v < 0 || v >= (int)h->order.size()) throw invalid_error("RCoT: variable index out of range");
            v = h->order[(size_t)v];
        }
        if (v < 0 || v >= h->n_vars) throw invalid_error("RCoT: variable index out of range");
        return v;
    };
    Plan pl;
    const int x = map(v1), y = map(v2);
    if (x == y) throw invalid_error("RCoT: x and y must be different variables");
    pl.a = std::min(x, y); pl.b = std::max(x, y);
    std::vector<int> z;
    for (int i = 0; i < n_cond; ++i) z.push_back(map(cond[i]));
    std::sort(z.begin(), z.end());
    z.erase(std::unique(z.begin(), z.end()), z.end());
    if ((int)z.size() > RCOT_MAX_IN - 2) throw invalid_error("RCoT: at most 62 conditioning variables");
    std::vector<int> all{pl.a, pl.b};
    all.insert(all.end(), z.begin(), z.end());
    bool nulls = false;
    for (int c : all) nulls |= h->has_null[(size_t)c] != 0;
    // rows valid in every variable of the test: needed on the host only with nulls (constancy and the sigma window)
    std::vector<int64_t> window;
    auto constant_on = [&](int c, const std::vector<int64_t>* rows) {
        if (!rows) return h->constant[(size_t)c] != 0;
        const double* v = h->cols[(size_t)c].data();
        for (int64_t r : *rows)
            if (v[r] != v[(*rows)[0]]) return false;
        return true;
    };
    std::vector<int64_t> valid_rows;
    if (nulls) {
        for (int64_t r = 0; r < h->N; ++r) {
            bool ok = true;
            for (int c : all) ok &= !std::isnan(h->cols[(size_t)c][(size_t)r]);
            if (ok) valid_rows.push_back(r);
        }
    }
    const std::vector<int64_t>* vr = nulls ? &valid_rows : nullptr;
    if (nulls && valid_rows.size() < 2) { pl.trivial = true; return pl; }
    if (constant_on(pl.a, vr) || constant_on(pl.b, vr)) { pl.trivial = true; return pl; }
    for (int c : z)
        if (!constant_on(c, vr)) pl.z.push_back(c);
    pl.k = (int)pl.z.size();
    // every Z column constant: the reference runs RIT on the rows valid in x, y and all of Z, so the device passes still skip the
    // rows where a dropped column is null (with only some of them dropped, the rows valid in x, y and the columns used: DESIGN §3.9)
    if (!pl.k && vr)
        for (int c : z)
            if (h->has_null[(size_t)c]) pl.zv.push_back(c);
    pl.F = 2 * h->nxy + (pl.k ? h->nz : 0);
    // sigma window: the first 500 rows valid in x, y and the Z columns used (the dropped ones were only constant, not null-free
    // on the same rows: with nulls the window follows the reference and takes the rows valid in all the test's variables)
    if (vr) window.assign(valid_rows.begin(), valid_rows.begin() + std::min<size_t>(valid_rows.size(), RCOT_SIGMA_ROWS));
    else for (int64_t r = 0; r < std::min<int64_t>(h->N, RCOT_SIGMA_ROWS); ++r) window.push_back(r);
    auto sigma_of = [&](const std::vector<int>& cs) {
        if (!vr && cs.size() == 1) return h->sigma1[(size_t)cs[0]];
        std::vector<const double*> p;
        for (int c : cs) p.push_back(h->cols[(size_t)c].data());
        return rf_sigma(p, window);
    };
    pl.sigma[0] = sigma_of({pl.a});
    pl.sigma[1] = sigma_of({pl.b});
    pl.sigma[2] = pl.k ? sigma_of(pl.z) : 0.0;
    const int nxy = h->nxy;
    pl.W.assign((size_t)2 * nxy + (size_t)pl.k * h->nz, 0.0);
    pl.bias.assign((size_t)2 * nxy + (pl.k ? h->nz : 0), 0.0);
    draw(h, pl, 0, 1, nxy, pl.sigma[0], pl.W.data(), pl.bias.data());
    draw(h, pl, 1, 1, nxy, pl.sigma[1], pl.W.data() + nxy, pl.bias.data() + nxy);
    if (pl.k) draw(h, pl, 2, pl.k, h->nz, pl.sigma[2], pl.W.data() + 2 * nxy, pl.bias.data() + 2 * nxy);
    // pilot shifts (host cos: any constant works, K1 and K2 subtract the same one)
    const size_t np_rows = std::min<size_t>(window.size(), RCOT_PILOT_ROWS);
    pl.shift.assign((size_t)pl.F, 0.0);
    for (int c = 0; c < pl.F; ++c) {
        double s = 0;
        for (size_t i = 0; i < np_rows; ++i) {
            const int64_t r = window[i];
            double arg;
            if (c < 2 * nxy) arg = h->cols[(size_t)(c < nxy ? pl.a : pl.b)][(size_t)r] * pl.W[(size_t)c];
            else {
                arg = 0;
                for (int d = 0; d < pl.k; ++d) arg += h->cols[(size_t)pl.z[(size_t)d]][(size_t)r] * pl.W[(size_t)2 * nxy + d + (size_t)(c - 2 * nxy) * pl.k];
            }
            s += std::sqrt(2.0) * std::cos(arg + pl.bias[(size_t)c]);
        }
        pl.shift[(size_t)c] = np_rows ? s / (double)np_rows : 0.0;
    }
    return pl;
}

// between the passes: from the Gram of [f, 1] (n x n, n = F + 1) the statistic and the coefficient matrix P
void solve_between(const pbn_rcot* h, Plan& pl, const std::vector<double>& G) {
    const int n = pl.F + 1, F = pl.F, nxy = h->nxy, nzf = pl.k ? h->nz : 0;
    const double cnt = G[(size_t)F + (size_t)F * n];
    pl.n_valid = (int64_t)std::llround(cnt);
    if (pl.n_valid < 2) throw invalid_error("RCoT: fewer than 2 valid rows");
    std::vector<double> mean(F), sd(F);
    for (int i = 0; i < F; ++i) mean[i] = G[i + (size_t)F * n] / cnt;
    auto cov = [&](int i, int j) { return (G[i + (size_t)j * n] - cnt * mean[i] * mean[j]) / (cnt - 1); };
    for (int i = 0; i < F; ++i) { const double v = cov(i, i); sd[i] = v > 0 ? std::sqrt(v) : 0.0; }
    // covariance of the normalised features (a constant feature normalises to 0)
    auto ncov = [&](int i, int j) { return (sd[i] > 0 && sd[j] > 0) ? cov(i, j) / (sd[i] * sd[j]) : 0.0; };
    const int xo = 0, yo = nxy, zo = 2 * nxy;
    std::vector<double> A((size_t)nzf * nxy, 0.0), B((size_t)nzf * nxy, 0.0);   // iCzz Czx, iCzz Czy (nz x nxy)
    std::vector<double> Cxy_z((size_t)nxy * nxy);
    for (int j = 0; j < nxy; ++j)
        for (int i = 0; i < nxy; ++i) Cxy_z[i + (size_t)j * nxy] = ncov(xo + i, yo + j);
    if (nzf) {
        std::vector<double> Czz((size_t)nzf * nzf), iCzz((size_t)nzf * nzf);
        for (int j = 0; j < nzf; ++j)
            for (int i = 0; i < nzf; ++i) Czz[i + (size_t)j * nzf] = ncov(zo + i, zo + j) + (i == j ? 1e-10 : 0.0);
        if (!hm::inverse(Czz.data(), nzf, iCzz.data())) throw singular_error("RCoT: singular covariance of the Z features");
        for (int j = 0; j < nxy; ++j)
            for (int i = 0; i < nzf; ++i) {
                double sa = 0, sb = 0;
                for (int l = 0; l < nzf; ++l) {
                    sa += iCzz[i + (size_t)l * nzf] * ncov(zo + l, xo + j);
                    sb += iCzz[i + (size_t)l * nzf] * ncov(zo + l, yo + j);
                }
                A[i + (size_t)j * nzf] = sa;
                B[i + (size_t)j * nzf] = sb;
            }
        for (int j = 0; j < nxy; ++j)
            for (int i = 0; i < nxy; ++i) {   // Cxy - Cxz iCzz Czy
                double s = 0;
                for (int l = 0; l < nzf; ++l) s += ncov(xo + i, zo + l) * B[l + (size_t)j * nzf];
                Cxy_z[i + (size_t)j * nxy] -= s;
            }
    }
    double ss = 0;
    for (double v : Cxy_z) ss += v * v;
    pl.sta = cnt * ss;
    // P: residual r_j = g_j - sum_l g_zl A_lj with g = (f - mean) / sd, as coefficients of [f, 1]
    const int fp = 16 * pl.nt();
    pl.P.assign((size_t)fp * 16, 0.0);
    auto put = [&](int o, const std::vector<double>& Mz) {
        for (int j = 0; j < nxy; ++j) {
            double* col = &pl.P[0];
            const int out = o / nxy * nxy + j;   // 0 .. nxy-1 for x, nxy .. 2 nxy-1 for y
            const int fi = o + j;
            double c1 = 0;
            if (sd[fi] > 0) { col[(size_t)fi * 16 + out] = 1 / sd[fi]; c1 -= mean[fi] / sd[fi]; }
            for (int l = 0; l < nzf; ++l) {
                const int fz = zo + l;
                if (!(sd[fz] > 0)) continue;
                const double a = Mz[l + (size_t)j * nzf];
                col[(size_t)fz * 16 + out] -= a / sd[fz];
                c1 += a * mean[fz] / sd[fz];
            }
            col[(size_t)F * 16 + out] = c1;
        }
    };
    put(xo, A);
    put(yo, B);
}

void finish_test(const pbn_rcot* h, Plan& pl, const std::vector<double>& Gq) {
    const int m = h->nxy * h->nxy;
    std::vector<double> M((size_t)m * m), ev(m);
    for (size_t i = 0; i < M.size(); ++i) M[i] = Gq[i] / (double)pl.n_valid;
    hm::sym_eigenvalues(M.data(), m, ev.data());
    pl.eig.clear();
    for (double v : ev)
        if (v > 0) pl.eig.push_back(v);
    std::sort(pl.eig.begin(), pl.eig.end());
    const int method = (pl.k && h->nz == 1) ? 1 : 0;
    pl.p = chisq_sum_sf(pl.eig.data(), (int)pl.eig.size(), pl.sta, method, &pl.used);
}

// unpack a reduced tile-pair image (pair p = upper-triangle row-major, lane-major elements) into a full symmetric n x n matrix
std::vector<double> unpack(const double* img, int nt, int n) {
    std::vector<double> G((size_t)n * n, 0.0);
    int p = 0;
    for (int I = 0; I < nt; ++I)
        for (int J = I; J < nt; ++J, ++p)
            for (int lane = 0; lane < 64; ++lane)
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * I + (lane >> 4) + 4 * r, j = 16 * J + (lane & 15);
                    if (i < n && j < n) { G[i + (size_t)j * n] = img[(size_t)p * 256 + lane * 4 + r]; G[j + (size_t)i * n] = G[i + (size_t)j * n]; }
                }
    return G;
}

// what a K1 / K2 launch took (pbn_debug_rcot's launch log): K1's rcot_gram_kernel instantiation PPW or K2's product tiles, dynamic
// LDS bytes, blocks
struct Launched {
    int variant = 0;
    size_t lds = 0;
    unsigned blocks = 0;
};

template <typename K>
Launched launch_pass(pbn_rcot* h, int pass, const std::vector<Plan*>& ps, std::vector<std::vector<double>>& results) {
    pbn_ctx* ctx = h->ctx;
    const int64_t rpb = rows_per_block(h->N), nb = ceil_div(h->N, rpb);
    std::vector<RcotTest> ts(ps.size());
    std::vector<double> par;
    std::vector<int64_t> blk, seg;
    int64_t part_elems = 0, out_elems = 0;
    int max_np = 0, max_ws = 0, s_max = 16, vs = 2, fp_max = 16;
    for (size_t t = 0; t < ps.size(); ++t) {
        const Plan& pl = *ps[t];
        RcotTest& d = ts[t];
        std::memset(&d, 0, sizeof d);
        d.col[0] = pl.a; d.col[1] = pl.b;
        for (int i = 0; i < pl.k; ++i) d.col[2 + i] = pl.z[(size_t)i];
        for (size_t i = 0; i < pl.zv.size(); ++i) d.col[2 + pl.k + i] = pl.zv[i];
        d.nin = 2 + pl.k + (int)pl.zv.size(); d.k = pl.k; d.F = pl.F; d.nxy = h->nxy; d.nt = pl.nt(); d.kw = std::max(1, pl.k);
        d.ntq = (h->nxy * h->nxy + 15) / 16;
        const int fp = 16 * d.nt;
        d.par = (int64_t)par.size();
        std::vector<double> W((size_t)fp * d.kw, 0.0), b((size_t)fp, 0.0);
        const int nxy = h->nxy;
        for (int c = 0; c < 2 * nxy; ++c) { W[(size_t)c * d.kw] = pl.W[(size_t)c]; b[(size_t)c] = pl.bias[(size_t)c]; }
        for (int j = 0; j < pl.F - 2 * nxy; ++j) {
            for (int dd = 0; dd < pl.k; ++dd) W[(size_t)(2 * nxy + j) * d.kw + dd] = pl.W[(size_t)2 * nxy + dd + (size_t)j * pl.k];
            b[(size_t)(2 * nxy + j)] = pl.bias[(size_t)(2 * nxy + j)];
        }
        par.insert(par.end(), W.begin(), W.end());
        par.insert(par.end(), b.begin(), b.end());
        std::vector<double> shift((size_t)fp, 0.0);
        std::copy(pl.shift.begin(), pl.shift.end(), shift.begin());
        par.insert(par.end(), shift.begin(), shift.end());
        s_max = std::max(s_max, lds_stride(fp));
        vs = std::max(vs, d.nin);
        fp_max = std::max(fp_max, fp);
        d.proj = (int64_t)par.size();
        if (pass == 2) par.insert(par.end(), pl.P.begin(), pl.P.end());
        const int np = pass == 1 ? d.nt * (d.nt + 1) / 2 : d.ntq * (d.ntq + 1) / 2;
        max_np = std::max(max_np, np);
        const int64_t ws = (int64_t)np * 256;
        max_ws = std::max<int>(max_ws, (int)ws);
        seg.insert(seg.end(), {part_elems, nb, ws, out_elems});
        for (int64_t i = 0; i < nb; ++i) {
            blk.insert(blk.end(), {(int64_t)t, i * rpb, std::min(h->N, (i + 1) * rpb), part_elems});
            part_elems += ws;
        }
        out_elems += ws;
    }
    h->d_tests.reserve(ts.size());
    h->d_par.reserve(par.size());
    h->d_blk.reserve(blk.size());
    h->d_seg.reserve(seg.size());
    h->d_part.reserve((size_t)part_elems);
    h->d_out.reserve((size_t)out_elems);
    HIP_CHECK(hipMemcpyAsync(h->d_tests.p, ts.data(), ts.size() * sizeof(RcotTest), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(h->d_par.p, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(h->d_blk.p, blk.data(), blk.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(h->d_seg.p, seg.data(), seg.size() * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    const unsigned nblk = (unsigned)(blk.size() / 4);
    Launched l;
    {
        KernelTimer kt(ctx, pass == 1 ? PBN_K_GRAM : PBN_K_RCOT_PROD);
        l = K{}(h, max_np, nblk, s_max, vs, fp_max);
    }
    l.blocks = nblk;
    {
        KernelTimer kt(ctx, PBN_K_FINISH);
        hipLaunchKernelGGL(rcot_reduce_kernel, dim3((unsigned)ceil_div(max_ws, 256), (unsigned)ps.size()), dim3(256), 0, ctx->stream,
                           h->d_part.p, h->d_seg.p, h->d_out.p);
    }
    HIP_CHECK(hipGetLastError());
    std::vector<double> host((size_t)out_elems);
    HIP_CHECK(hipMemcpyAsync(host.data(), h->d_out.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    results.resize(ps.size());
    for (size_t t = 0; t < ps.size(); ++t) {
        const int n = pass == 1 ? ps[t]->F + 1 : h->nxy * h->nxy;
        const int nt = pass == 1 ? ts[t].nt : ts[t].ntq;
        results[t] = unpack(host.data() + seg[4 * t + 3], nt, n);
    }
    return l;
}

// dynamic LDS of a launch (see rcot_gram_kernel); more than the default 64 KiB is asked for explicitly (gfx950 has 160 KiB per CU)
template <typename Kern>
size_t lds_bytes(Kern kern, int s_max, int vs, int p_doubles) {
    const size_t bytes = (size_t)(RCOT_CHUNK * s_max + RCOT_CHUNK * vs + p_doubles) * sizeof(double);
    HIP_CHECK(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return bytes;
}

struct LaunchGram {
    template <int P>
    static Launched go(pbn_rcot* h, unsigned nblk, int s_max, int vs) {
        Launched l;
        l.variant = P;
        l.lds = lds_bytes(rcot_gram_kernel<P>, s_max, vs, 0);
        hipLaunchKernelGGL(rcot_gram_kernel<P>, dim3(nblk), dim3(256), l.lds, h->ctx->stream, h->d_cols.p, h->N, h->d_tests.p, h->d_par.p,
                           h->d_blk.p, h->d_part.p, s_max, vs);
        return l;
    }
    Launched operator()(pbn_rcot* h, int max_np, unsigned nblk, int s_max, int vs, int) const {
        const int ppw = (max_np + 3) / 4;
        if (ppw <= 1) return go<1>(h, nblk, s_max, vs);
        if (ppw <= 2) return go<2>(h, nblk, s_max, vs);
        if (ppw <= 4) return go<4>(h, nblk, s_max, vs);
        if (ppw <= 8) return go<8>(h, nblk, s_max, vs);
        if (ppw <= 16) return go<16>(h, nblk, s_max, vs);
        return go<34>(h, nblk, s_max, vs);
    }
};
struct LaunchProd {
    Launched operator()(pbn_rcot* h, int, unsigned nblk, int s_max, int vs, int fp_max) const {
        Launched l;
        l.variant = (h->nxy * h->nxy + 15) / 16;
        l.lds = lds_bytes(rcot_prod_kernel, s_max, vs, fp_max * 16);
        hipLaunchKernelGGL(rcot_prod_kernel, dim3(nblk), dim3(256), l.lds, h->ctx->stream, h->d_cols.p, h->N, h->d_tests.p, h->d_par.p,
                           h->d_blk.p, h->d_part.p, s_max, vs);
        return l;
    }
};

// pbn_debug_rcot (test aid, not part of the C ABI header; see its definition): what run_plans records while it is armed
std::atomic<bool> g_rcot_capture{false};
std::mutex g_rcot_mu;
std::vector<double> g_rcot_rec;
std::vector<int64_t> g_rcot_log;

void debug_log_launch(int pass, const Launched& l, size_t tests) {
    std::lock_guard<std::mutex> lk(g_rcot_mu);
    g_rcot_log.insert(g_rcot_log.end(), {(int64_t)pass, (int64_t)l.variant, (int64_t)tests, (int64_t)l.lds, (int64_t)l.blocks});
}

void debug_record(const pbn_rcot* h, const Plan& pl, const std::vector<double>& G1, const std::vector<double>& G2) {
    const int n = pl.F + 1, nxy = h->nxy;
    std::vector<int> cols{pl.a, pl.b};
    cols.insert(cols.end(), pl.z.begin(), pl.z.end());
    cols.insert(cols.end(), pl.zv.begin(), pl.zv.end());
    std::vector<double> r{(double)pl.F, (double)nxy, (double)pl.k, (double)h->nz, (double)pl.n_valid, (double)cols.size()};
    r.insert(r.end(), cols.begin(), cols.end());
    r.insert(r.end(), pl.W.begin(), pl.W.end());
    r.insert(r.end(), pl.bias.begin(), pl.bias.end());
    r.insert(r.end(), pl.shift.begin(), pl.shift.end());
    r.insert(r.end(), G1.begin(), G1.end());
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 2 * nxy; ++j) r.push_back(pl.P[(size_t)i * 16 + j]);
    r.insert(r.end(), G2.begin(), G2.end());
    std::lock_guard<std::mutex> lk(g_rcot_mu);
    g_rcot_rec.insert(g_rcot_rec.end(), r.begin(), r.end());
}

// all non-trivial plans: K1 for a memory chunk of tests, the host step, K2, the p-values
void run_plans(pbn_rcot* h, std::vector<Plan>& plans) {
    HIP_CHECK(hipSetDevice(h->ctx->device));
    const int64_t nb = ceil_div(h->N, rows_per_block(h->N));
    const int64_t budget = (int64_t)48 << 20;   // partial doubles per launch (384 MiB)
    const bool dbg = g_rcot_capture.load(std::memory_order_relaxed);
    std::vector<Plan*> todo;
    for (auto& pl : plans)
        if (!pl.trivial) todo.push_back(&pl);
    size_t i = 0;
    while (i < todo.size()) {
        std::vector<Plan*> chunk;
        int64_t used = 0;
        while (i < todo.size()) {
            const int nt = todo[i]->nt();
            const int64_t need = nb * (int64_t)(nt * (nt + 1) / 2) * 256;
            if (!chunk.empty() && used + need > budget) break;
            chunk.push_back(todo[i++]);
            used += need;
        }
        std::vector<std::vector<double>> res, g1;
        const Launched l1 = launch_pass<LaunchGram>(h, 1, chunk, res);
        for (size_t t = 0; t < chunk.size(); ++t) solve_between(h, *chunk[t], res[t]);
        if (dbg) { debug_log_launch(1, l1, chunk.size()); g1 = res; }
        const Launched l2 = launch_pass<LaunchProd>(h, 2, chunk, res);
        if (dbg) {
            debug_log_launch(2, l2, chunk.size());
            for (size_t t = 0; t < chunk.size(); ++t) debug_record(h, *chunk[t], g1[t], res[t]);
        }
        for (size_t t = 0; t < chunk.size(); ++t) finish_test(h, *chunk[t], res[t]);
    }
}

}  // namespace

extern "C" {

int pbn_rcot_create(pbn_ctx* ctx, const double* const* cols, int n_vars, int64_t N, int nxy, int nz, uint32_t seed, pbn_rcot** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !cols || !out) throw invalid_error("pbn_rcot_create: null argument");
        if (n_vars < 2) throw invalid_error("DataFrame does not contain enough continuous columns.");
        if (nxy < 1 || nz < 1) throw invalid_error("RCoT: the numbers of random Fourier features must be positive");
        if (nxy > RCOT_MAX_NXY) throw invalid_error("RCoT: random_fourier_xy must be at most 8 (random_fourier_xy^2 <= 64 products)");
        if (2 * nxy + nz + 1 > RCOT_MAX_FP) throw invalid_error("RCoT: 2 * random_fourier_xy + random_fourier_z must be at most 255");
        if (N < 1) throw invalid_error("RCoT: empty table");
        HIP_CHECK(hipSetDevice(ctx->device));
        auto h = std::make_unique<pbn_rcot>();
        h->ctx = ctx; h->N = N; h->n_vars = n_vars; h->nxy = nxy; h->nz = nz; h->seed = seed;
        h->cols.resize((size_t)n_vars);
        h->has_null.assign((size_t)n_vars, 0);
        h->constant.assign((size_t)n_vars, 0);
        h->sigma1.assign((size_t)n_vars, std::nan(""));
        std::vector<int64_t> head;
        for (int64_t r = 0; r < std::min<int64_t>(N, RCOT_SIGMA_ROWS); ++r) head.push_back(r);
        for (int j = 0; j < n_vars; ++j) {
            // DataFrame::normalize: centre and scale every column over its valid values (sd over n - 1); constant -> 0
            std::vector<double>& c = h->cols[(size_t)j];
            c.assign(cols[j], cols[j] + N);
            double s = 0;
            int64_t n = 0;
            for (double v : c)
                if (!std::isnan(v)) { s += v; ++n; }
            h->has_null[(size_t)j] = n < N;
            const double mean = n ? s / n : 0.0;
            double ss = 0;
            for (double v : c)
                if (!std::isnan(v)) ss += (v - mean) * (v - mean);
            const double sd = n > 1 ? std::sqrt(ss / (n - 1)) : 0.0;
            for (double& v : c)
                if (!std::isnan(v)) v = sd != 0 ? (v - mean) * (1 / sd) : 0.0;
            bool cst = true;
            double first = std::nan("");
            for (double v : c)
                if (!std::isnan(v)) {
                    if (std::isnan(first)) first = v;
                    else if (v != first) { cst = false; break; }
                }
            h->constant[(size_t)j] = cst;
            if (!h->has_null[(size_t)j]) h->sigma1[(size_t)j] = rf_sigma({c.data()}, head);
        }
        h->d_cols.alloc((size_t)n_vars * N);
        for (int j = 0; j < n_vars; ++j)
            HIP_CHECK(hipMemcpyAsync(h->d_cols.p + (size_t)j * N, h->cols[(size_t)j].data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = h.release();
    });
}

void pbn_rcot_destroy(pbn_rcot* h) {
    if (!h) return;
    pbn::ctx_pin pin_(h->ctx);
    std::lock_guard<std::recursive_mutex> lock_(mu_of(h));
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    delete h;
}

int pbn_rcot_set_order(pbn_rcot* h, int n, const int* ids) {
    return guarded(mu_of(h), [&] {
        if (!h || (n > 0 && !ids)) throw invalid_error("pbn_rcot_set_order: null argument");
        for (int i = 0; i < n; ++i)
            if (ids[i] < 0 || ids[i] >= h->n_vars) throw invalid_error("pbn_rcot_set_order: index out of range");
        h->order.assign(ids, ids + (n > 0 ? n : 0));
    });
}

void pbn_rcot_pvalue_batch(void* user, int n_tests, const int* v1, const int* v2, const int* cond_off, const int* cond, double* out) {
    pbn_rcot* h = (pbn_rcot*)user;
    const int rc = guarded(mu_of(h), [&] {
        if (!h || n_tests < 0 || (n_tests > 0 && (!v1 || !v2 || !cond_off || !out))) throw invalid_error("pbn_rcot_pvalue_batch: null argument");
        std::vector<Plan> plans;
        plans.reserve((size_t)n_tests);
        for (int i = 0; i < n_tests; ++i) {
            const int nc = cond_off[i + 1] - cond_off[i];
            if (nc > 0 && !cond) throw invalid_error("pbn_rcot_pvalue_batch: null argument");
            plans.push_back(plan_test(h, v1[i], v2[i], nc, nc > 0 ? cond + cond_off[i] : nullptr));
        }
        run_plans(h, plans);
        for (int i = 0; i < n_tests; ++i) out[i] = plans[(size_t)i].p;
    });
    if (rc != PBN_OK && out)
        for (int i = 0; i < n_tests; ++i) out[i] = std::nan("");
}

double pbn_rcot_pvalue(void* user, int v1, int v2, int n_cond, const int* cond) {
    const int off[2] = {0, n_cond};
    double p = std::nan("");
    pbn_rcot_pvalue_batch(user, 1, &v1, &v2, off, cond, &p);
    return p;
}

int pbn_rcot_detail(pbn_rcot* h, int v1, int v2, int n_cond, const int* cond, int64_t* n_valid, double* sigma, double* W, double* b,
                    int* z_used, int* n_z_used, double* sta, double* eig, int* n_eig, int* method, double* pvalue) {
    return guarded(mu_of(h), [&] {
        if (!h || (n_cond > 0 && !cond)) throw invalid_error("pbn_rcot_detail: null argument");
        std::vector<Plan> plans{plan_test(h, v1, v2, n_cond, cond)};
        run_plans(h, plans);
        const Plan& pl = plans[0];
        if (n_valid) *n_valid = pl.n_valid;
        if (sigma) std::copy(pl.sigma, pl.sigma + 3, sigma);
        if (W) std::copy(pl.W.begin(), pl.W.end(), W);
        if (b) std::copy(pl.bias.begin(), pl.bias.end(), b);
        if (z_used) std::copy(pl.z.begin(), pl.z.end(), z_used);
        if (n_z_used) *n_z_used = pl.trivial ? -1 : pl.k;
        if (sta) *sta = pl.sta;
        if (eig) std::copy(pl.eig.begin(), pl.eig.end(), eig);
        if (n_eig) *n_eig = (int)pl.eig.size();
        if (method) *method = pl.used;
        if (pvalue) *pvalue = pl.p;
    });
}

// pbn_debug_rcot (test aid, not part of the C ABI header): op 1 arms the capture and clears it, op 0 disarms and clears.  While armed,
// run_plans appends one record per test it runs, in plan order, and one launch-log entry per K1 / K2 launch.  op 2 copies up to `cap`
// doubles of the records into out, op 3 up to `cap` int64 of the launch log; both return how many are held.
//   record: F, nxy, k, nz, n_valid, nc, the nc columns read (x, y, the Z columns used, then those read for validity only), W (2 nxy + k nz,
//           as pbn_rcot_detail), b (F), the pilot shift (F), the unpacked K1 Gram ((F + 1)^2), P (F + 1 rows of 2 nxy: row = feature of
//           [f, 1], columns rx then ry), the unpacked K2 Gram (nxy^4)
//   launch: pass (1 = K1, 2 = K2), the rcot_gram_kernel instantiation PPW (K1) or the product tiles ntq (K2), tests, dynamic LDS
//           bytes, blocks
// Unarmed, run_plans pays one flag test; no kernel and no result depends on it.
int64_t pbn_debug_rcot(int op, void* out, int64_t cap) {
    std::lock_guard<std::mutex> lk(g_rcot_mu);
    if (op == 0 || op == 1) {
        g_rcot_rec.clear();
        g_rcot_log.clear();
        g_rcot_capture.store(op == 1);
        return 0;
    }
    if (op == 2) {
        for (int64_t i = 0; out && i < (int64_t)g_rcot_rec.size() && i < cap; ++i) ((double*)out)[i] = g_rcot_rec[(size_t)i];
        return (int64_t)g_rcot_rec.size();
    }
    if (op == 3) {
        for (int64_t i = 0; out && i < (int64_t)g_rcot_log.size() && i < cap; ++i) ((int64_t*)out)[i] = g_rcot_log[(size_t)i];
        return (int64_t)g_rcot_log.size();
    }
    return -1;
}

int pbn_rcot_chisq_sum_sf(const double* weights, int n, double q, int method, double* out) {
    return guarded([&] {
        if ((n > 0 && !weights) || !out || n < 0) throw invalid_error("pbn_rcot_chisq_sum_sf: null argument");
        if (method < 0 || method > 2) throw invalid_error("pbn_rcot_chisq_sum_sf: method must be 0 (auto), 1 (HBE) or 2 (LPB4)");
        int used = 0;
        *out = chisq_sum_sf(weights, n, q, method, &used);
    });
}

}  // extern "C"
