// Ill-conditioned LinearGaussianCPD fits: moments in double-double, solved in double-double.
//
// Reference: MLE<LinearGaussianCPD> with >= 3 parents runs Eigen's ColPivHouseholderQR on the N x (p+1) design matrix
// (/root/reference/pybnesian/learning/parameters/mle_LinearGaussianCPD.hpp:152-193), error ~ kappa * eps.  The score engine
// solves the normal equations on one-pass fp64 moments instead (scoring.hip, lg_fit): kappa^2 * eps.  That is invisible on
// ordinary tables and wrong by more than the 1e-6 parity bar when parents are nearly collinear (kappa >~ 1e5) or the fit is
// nearly exact (1 - R^2 <~ 1e-8).  lg_fit flags those cases (smallest pivot ratio of its diagonally pivoted Cholesky, RSS /
// SSE_y) and the callers come here: ONE more pass over the candidate's rows accumulates the RAW moments sum x_i,
// sum x_i x_j in double-double (TwoProd by FMA: every product exact, TwoSum accumulation: ~1e-32 relative), and the
// centring, the pivoted Cholesky, the solves and the residual sum of squares (a Schur complement) run in double-double on the
// host on (p+1)^2 numbers.  The result is the least-squares solution of the DATA to full double precision - at least as
// accurate as the reference's Householder QR - at the cost of a rare extra pass; no N x (p+1) copy, no QR kernel.
// Rank decision (lg_dd_solve.hpp, which holds the host solve and states the reason): a pivot marks a dependent column
// (coefficient 0) when it is below (eps (p+1))^2 of the largest one - the square of ColPivHouseholderQR's default threshold on
// |R_kk| / |R_00|; the reference pivots the uncentred matrix with its ones column, here the centred one: the decisions can only
// differ for kappa ~ 1e15 - OR when it does not rise above the roundoff that the raw double-double moments carry into the
// centred ones, 64 * 2^-104 * max(G_ii, C_ii * max_j G_jj / C_jj): with column means tens of sigma from zero that noise is far
// above the first threshold, and an exactly dependent parent would otherwise keep a pivot of pure noise.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "common.hpp"
#include "scoring_internal.hpp"

#define PBN_DD_FN __host__ __device__ inline
#include "lg_dd_solve.hpp"

namespace pbn {
namespace score {

namespace {

constexpr int DD_MAX_D = 16;   // variable + up to 15 parents
constexpr int DD_BLOCKS = 128;

struct DdGramArgs {
    const void* base;
    int64_t ld;
    int cols[DD_MAX_D];
    int d;
    int64_t row0, n0, row1;   // logical row r -> r < n0 ? row0 + r : row1 + (r - n0), then through `rows` if given
    const int32_t* rows;
    int64_t n;
    double* partial;          // [tile][block][20][2]: 16 products + 4 sums, (hi, lo)
};

__device__ inline dd wave_sum_dd(dd v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        dd o;
        o.hi = __shfl_xor(v.hi, off);
        o.lo = __shfl_xor(v.lo, off);
        v = dd_add(v, o);
    }
    return v;
}

// grid (DD_BLOCKS, tiles): tile = (I, J), I <= J, of 4-column groups; 16 products x_{4I+i} x_{4J+j} + the sums of group J
template <typename T>
__global__ __launch_bounds__(256) void gram_dd_kernel(DdGramArgs a) {
    int I = 0, J = 0;
    {
        const int ng = (a.d + 3) / 4;
        int t = blockIdx.y;
        for (I = 0; I < ng; ++I) {
            if (t < ng - I) { J = I + t; break; }
            t -= ng - I;
        }
    }
    const T* ci[4];
    const T* cj[4];
    bool vi[4], vj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        vi[k] = 4 * I + k < a.d;
        vj[k] = 4 * J + k < a.d;
        ci[k] = (const T*)a.base + (int64_t)a.cols[vi[k] ? 4 * I + k : 0] * a.ld;
        cj[k] = (const T*)a.base + (int64_t)a.cols[vj[k] ? 4 * J + k : 0] * a.ld;
    }
    dd acc[20];
#pragma unroll
    for (int k = 0; k < 20; ++k) acc[k] = {0.0, 0.0};
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < a.n; r += (int64_t)gridDim.x * 256) {
        int64_t src = r < a.n0 ? a.row0 + r : a.row1 + (r - a.n0);
        if (a.rows) src = a.rows[src];
        double x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = vi[k] ? (double)ci[k][src] : 0.0;
            y[k] = vj[k] ? (double)cj[k][src] : 0.0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i * 4 + j] = dd_add_prod(acc[i * 4 + j], x[i], y[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[16 + j] = dd_add(acc[16 + j], {y[j], 0.0});
    }
    __shared__ double red[4][20][2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 20; ++k) {
        const dd v = wave_sum_dd(acc[k]);
        if (lane == 0) { red[wave][k][0] = v.hi; red[wave][k][1] = v.lo; }
    }
    __syncthreads();
    if (threadIdx.x < 20) {
        const int k = threadIdx.x;
        dd v = {red[0][k][0], red[0][k][1]};
        for (int w = 1; w < 4; ++w) v = dd_add(v, {red[w][k][0], red[w][k][1]});
        double* o = a.partial + (((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 20 + k) * 2;
        o[0] = v.hi;
        o[1] = v.lo;
    }
}

}  // namespace

// Raw moments of `d` columns over the described rows in double-double, then the exact least-squares fit.
double lg_fit_accurate(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n0, int64_t row1, int64_t n,
                       const int32_t* dev_rows, double* beta, int* rank) {
    if (d > DD_MAX_D) throw invalid_error("lg_fit_accurate: more than 15 parents");
    pbn_ctx* ctx = t->ctx;
    const int ng = (d + 3) / 4, tiles = ng * (ng + 1) / 2;
    const int nblocks = (int)std::max<int64_t>(1, std::min<int64_t>(DD_BLOCKS, ceil_div(n, 256)));
    const size_t count = (size_t)tiles * nblocks * 40;
    ctx->scratch_red.reserve(count);
    DdGramArgs a{};
    a.base = t->data; a.ld = t->ld; a.d = d;
    for (int i = 0; i < d; ++i) a.cols[i] = cols[i];
    a.row0 = row0; a.n0 = n0; a.row1 = row1; a.rows = dev_rows; a.n = n; a.partial = ctx->scratch_red.p;
    const dim3 grid((unsigned)nblocks, (unsigned)tiles), block(256);
    {
        KernelTimer kt(ctx, PBN_K_GRAM);
        if (t->dtype == PBN_F64) hipLaunchKernelGGL(gram_dd_kernel<double>, grid, block, 0, ctx->stream, a);
        else hipLaunchKernelGGL(gram_dd_kernel<float>, grid, block, 0, ctx->stream, a);
        HIP_CHECK(hipGetLastError());
    }
    std::vector<double> h(count);
    HIP_CHECK(hipMemcpyAsync(h.data(), ctx->scratch_red.p, count * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    // raw moments, blocks added in order
    std::vector<dd> S(d, dd{0, 0}), G((size_t)d * d, dd{0, 0});
    int tile = 0;
    for (int I = 0; I < ng; ++I)
        for (int J = I; J < ng; ++J, ++tile) {
            dd acc[20];
            for (auto& v : acc) v = {0, 0};
            for (int b = 0; b < nblocks; ++b) {
                const double* o = h.data() + ((size_t)tile * nblocks + b) * 40;
                for (int k = 0; k < 20; ++k) acc[k] = dd_add(acc[k], {o[2 * k], o[2 * k + 1]});
            }
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * I + i, c = 4 * J + j;
                    if (r < d && c < d) G[r + (size_t)c * d] = G[c + (size_t)r * d] = acc[i * 4 + j];
                }
            if (I == 0)   // the sums of group J ride with every tile (*, J); take them from (0, J)
                for (int j = 0; j < 4; ++j)
                    if (4 * J + j < d) S[4 * J + j] = acc[16 + j];
        }
    return lg_dd_solve(n, d, S.data(), G.data(), beta, rank);
}

}  // namespace score
}  // namespace pbn

using namespace pbn;
using namespace pbn::score;

extern "C" {

// pbn_debug_lg_fit_accurate (test aid, not part of the C ABI header): lg_fit_accurate as its callers reach it, on any of its addressing
// forms.  Logical row r < n is r < n0 ? row0 + r : row1 + (r - n0), an index into host_rows (n_rows entries, uploaded here) when that
// is given and a table row otherwise; beta: d values, *rank: the number of parents the rank decision kept.  Every addressed row is
// checked against the table before the launch.
int pbn_debug_lg_fit_accurate(const pbn_table* t, const int* cols, int d, int64_t row0, int64_t n0, int64_t row1, int64_t n,
                              const int32_t* host_rows, int64_t n_rows, double* beta, double* variance, int* rank) {
    return guarded(mu_of(t), [&] {
        if (!t || !cols || !beta || !variance || !rank) throw invalid_error("pbn_debug_lg_fit_accurate: null argument");
        if (d < 1 || d > DD_MAX_D) throw invalid_error("pbn_debug_lg_fit_accurate: between 1 and 16 columns");
        for (int i = 0; i < d; ++i)
            if (cols[i] < 0 || cols[i] >= t->n_cols) throw invalid_error("pbn_debug_lg_fit_accurate: column index out of range");
        const int64_t limit = host_rows ? n_rows : t->n_rows;
        if (n < 0 || n0 < 0 || n0 > n || row0 < 0 || row1 < 0 || limit < 0 || row0 + n0 > limit || row1 + (n - n0) > limit)
            throw invalid_error("pbn_debug_lg_fit_accurate: row ranges out of bounds");
        HIP_CHECK(hipSetDevice(t->ctx->device));
        dev_buf<int32_t> rows;
        if (host_rows) {
            for (int64_t r = 0; r < n_rows; ++r)
                if (host_rows[r] < 0 || host_rows[r] >= t->n_rows) throw invalid_error("pbn_debug_lg_fit_accurate: row list entry out of range");
            rows.alloc((size_t)n_rows + 1);
            if (n_rows > 0) HIP_CHECK(hipMemcpy(rows.p, host_rows, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        *variance = lg_fit_accurate(t, cols, d, row0, n0, row1, n, rows.p, beta, rank);
    });
}

}  // extern "C"
