// Fitting the conditional linear Gaussian nodes of a network in one device pass (DiscreteAdaptator<LinearGaussianCPD>::fit,
// factors/discrete/DiscreteAdaptator.hpp:201-276, over learning/parameters/mle_LinearGaussianCPD.hpp) - instead of, per node and
// configuration of its discrete parents, a row selection on the host, a take, an upload of the slice, one Gram launch and a wait.
//
// A CELL is a (node, configuration) pair.  Its record on the device is S1 = 1 + D + D (D + 1) / 2 doubles - the number of its rows, the
// D sums and the upper triangle of the D x D products (row-major: (0,0) (0,1) .. (0,D-1) (1,1) ..) of the node's D = p + 1 continuous
// columns, the variable first - every value taken about the column's PILOT SHIFT, which is the column's value in the table's first
// row: a value of the data, the same for every cell and every node that reads the column.  A float column is widened before the
// shift is taken off, as in seg_moments_kernel (hybrid.hip).
//
// clg_fit_moments_kernel: grid = (row chunk, node of D columns), 256 threads.  A chunk is `tiles_per_chunk` consecutive tiles of
// FIT_TILE = 1 024 rows - at most FIT_MAX_CHUNKS chunks, whatever the device.  Per tile a lane holds 4 rows (256 apart): their key
// - sum code_j * stride_j, the first parent fastest; no key when a code is -1 - and their D shifted values, in registers.  The
// block marks the tile's configurations in an LDS bit set (integer atomics: the set is the same in any order) and loops over the marked ones:
// every lane adds `key == c ? x : 0` into S1 accumulators, the wave folds them with a fixed reduce-scatter butterfly (step h: a
// lane keeps the half of its values its bit h selects and adds the partner's: S1 exchanges in all where a plain butterfly takes
// 6 S1; lane l ends with value l), the four waves' values are added in wave order and the result is added to the chunk's record of
// the cell - which this block alone writes, tile after tile.  clg_fit_reduce_kernel adds a cell's chunk records in chunk order.
// No floating-point atomics, one order of additions: two calls on the same inputs give the same bits.
//
// The host finishes a cell as every other moment path does: mean = shift + S / N, centred SSE = G - S S' / N, then lg_fit
// (scoring.hip) - the one solver.  A fit lg_fit marks suspect is NOT refitted here: the cell is reported (status 2) and its caller
// refits it from the rows, as pbn_lg_fit_table would have.
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "common.hpp"
#include "discrete_model.hpp"
#include "net_eval.hpp"
#include "scoring_internal.hpp"

using namespace pbn;
using namespace pbn::score;

namespace {

constexpr int BLOCK = 256;
constexpr int V = 4;                                    // rows of a lane, BLOCK apart
constexpr int FIT_TILE = PBN_CLG_FIT_TILE_ROWS;         // rows of a tile
constexpr int FIT_MAX_CHUNKS = 512;                     // chunk records of a cell: a fixed number, so the order of the additions is the device's on any device
constexpr int FIT_MAX_D = 8;                            // the variable and 7 continuous parents
constexpr int FIT_MAX_DISCRETE_PARENTS = 7;
constexpr int FIT_MAX_CONFIGS = PBN_CLG_FIT_MAX_CONFIGS;

static_assert(FIT_TILE == BLOCK * V, "a tile is four rows a lane");
static_assert(FIT_MAX_CONFIGS % 32 == 0, "the configurations' bit set is whole words");

constexpr int stats_of(int D) { return 1 + D + D * (D + 1) / 2; }
constexpr int pow2_ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

struct FitNode {
    int D, m;                        // continuous columns (the variable first), discrete parents
    int ccol[FIT_MAX_D];             // columns of the continuous table
    int dcol[FIT_MAX_DISCRETE_PARENTS];
    uint32_t stride[FIT_MAX_DISCRETE_PARENTS];
    uint32_t G;                      // configurations
    int64_t slot_off;                // first double of the node's cells in a chunk's record
};

// The wave's sums of a[0 .. S1): lane l returns the sum of a[l & (P - 1)] (P = S1 rounded up to a power of two; the values past S1 are
// zeros the compiler drops).  A fixed tree: the result is a function of the 64 lanes' values alone.
// (the steps are templates, not loops over h: every index into `a` is then a constant and the array stays in registers)
template <int S1, int OFF, int P>
__device__ __forceinline__ void wave_fold_whole(double (&a)[P]) {   // plain butterfly steps while a lane pair shares every value
    if constexpr (OFF >= P) {
#pragma unroll
        for (int i = 0; i < S1; ++i) a[i] += __shfl_xor(a[i], OFF);
        wave_fold_whole<S1, OFF / 2, P>(a);
    }
}
template <int H, int P>
__device__ __forceinline__ void wave_fold_halves(double (&a)[P], int lane) {
    if constexpr (H >= 1) {
        const bool up = (lane & H) != 0;
#pragma unroll
        for (int i = 0; i < H; ++i) {
            const double keep = up ? a[i + H] : a[i], send = up ? a[i] : a[i + H];
            a[i] = keep + __shfl_xor(send, H);
        }
        wave_fold_halves<H / 2, P>(a, lane);
    }
}
template <int S1, int P>
__device__ __forceinline__ double wave_fold(double (&a)[P], int lane) {
    wave_fold_whole<S1, 32, P>(a);
    wave_fold_halves<P / 2, P>(a, lane);
    return a[0];
}

// partial: [n_chunks][slots] doubles, zeroed before the launch.  codes: [n_dcols][n_rows].  n_rows >= 1.
template <typename T, int D>
__global__ __launch_bounds__(BLOCK) void clg_fit_moments_kernel(const FitNode* __restrict__ nodes, const int* __restrict__ list,
                                                                const int32_t* __restrict__ codes, const T* __restrict__ base, int64_t ld,
                                                                int64_t n_rows, int tiles_per_chunk, int n_tiles, double* __restrict__ partial,
                                                                int64_t slots) {
    constexpr int S1 = stats_of(D), P = pow2_ceil(S1);
    __shared__ uint32_t present[FIT_MAX_CONFIGS / 32];
    __shared__ double red[2][BLOCK / 64][P];
    const FitNode& nd = nodes[list[blockIdx.y]];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t n32 = (uint32_t)n_rows, G = nd.G;   // rows in 32 bits: a pbn_dtable has at most 2^31 - 1 of them
    const int m = nd.m;
    const T* col[D];
    double shift[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
        col[j] = base + (int64_t)nd.ccol[j] * ld;
        shift[j] = (double)col[j][0];
    }
    double* mine = partial + (int64_t)blockIdx.x * slots + nd.slot_off;
    const int tile0 = blockIdx.x * tiles_per_chunk, tile1 = min(tile0 + tiles_per_chunk, n_tiles);
    int par = 0;
    for (int tile = tile0; tile < tile1; ++tile) {
        uint32_t key[V];
        bool ok[V];
        double x[V][D];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const uint32_t r = (uint32_t)tile * (uint32_t)FIT_TILE + (uint32_t)(i * BLOCK + t);
            const uint32_t src = min(r, n32 - 1u);   // a row past the end reads the last row instead; it is in no cell
            uint32_t k = 0u;
            int32_t any = 0;   // the codes or-ed: negative when one of them is -1
            for (int j = 0; j < m; ++j) {
                const int32_t code = codes[(int64_t)nd.dcol[j] * n_rows + src];
                k += (uint32_t)code * nd.stride[j];
                any |= code;
            }
            key[i] = k;
            ok[i] = (r < n32) & (any >= 0) & (k < G);
#pragma unroll
            for (int j = 0; j < D; ++j) x[i][j] = (double)col[j][src] - shift[j];
        }
        __syncthreads();   // the last tile's loop over `present` is over
        for (uint32_t w = t; w < (G + 31u) / 32u; w += BLOCK) present[w] = 0u;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (ok[i]) atomicOr(&present[key[i] >> 5], 1u << (key[i] & 31u));
        __syncthreads();
        for (uint32_t c = 0; c < G; ++c) {
            if (!((present[c >> 5] >> (c & 31u)) & 1u)) continue;   // (the same for the whole block)
            double a[P];
#pragma unroll
            for (int s = 0; s < P; ++s) a[s] = 0.0;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const bool sel = ok[i] & (key[i] == c);
                double xm[D];   // both factors of a product are masked: a NaN of another cell's row must not reach this one
#pragma unroll
                for (int j = 0; j < D; ++j) xm[j] = sel ? x[i][j] : 0.0;
                a[0] += sel ? 1.0 : 0.0;
                int pos = 1 + D;
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    a[1 + j] += xm[j];
#pragma unroll
                    for (int k2 = j; k2 < D; ++k2) { a[pos] = __builtin_fma(xm[j], xm[k2], a[pos]); ++pos; }
                }
            }
            const double v = wave_fold<S1, P>(a, lane);
            if (lane < P) red[par][wave][lane] = v;
            // one barrier a configuration: the buffer written next is the other one, and whoever writes this one again has passed the
            // next configuration's barrier, which every reader of this one reaches only after its read
            __syncthreads();
            if (t < S1) mine[(int64_t)c * S1 + t] += ((red[par][0][t] + red[par][1][t]) + red[par][2][t]) + red[par][3][t];
            par ^= 1;
        }
    }
}

// out[s] = the chunk records' s-th doubles added in chunk order from 0.0
__global__ __launch_bounds__(BLOCK) void clg_fit_reduce_kernel(const double* __restrict__ partial, int64_t slots, int n_chunks, double* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (s >= slots) return;
    double v = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) v += partial[(int64_t)ch * slots + s];
    out[s] = v;
}

// out[c] = column c's first row, widened: the pilot shifts
template <typename T>
__global__ __launch_bounds__(BLOCK) void clg_fit_shift_kernel(const T* __restrict__ base, int64_t ld, int n_cols, double* __restrict__ out) {
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < n_cols) out[c] = (double)base[(int64_t)c * ld];
}

template <typename T, int D>
void launch_moments_d(const dim3& grid, hipStream_t st, const FitNode* nodes, const int* list, const pbn_dtable* dt, const pbn_table* t, int tiles_per_chunk,
                      int n_tiles, double* partial, int64_t slots) {
    hipLaunchKernelGGL((clg_fit_moments_kernel<T, D>), grid, dim3(BLOCK), 0, st, nodes, list, dt->codes_dev.p, (const T*)t->data, t->ld, t->n_rows,
                       tiles_per_chunk, n_tiles, partial, slots);
}

template <typename T>
void launch_moments(int D, const dim3& grid, hipStream_t st, const FitNode* nodes, const int* list, const pbn_dtable* dt, const pbn_table* t,
                    int tiles_per_chunk, int n_tiles, double* partial, int64_t slots) {
    switch (D) {
        case 1: launch_moments_d<T, 1>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 2: launch_moments_d<T, 2>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 3: launch_moments_d<T, 3>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 4: launch_moments_d<T, 4>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 5: launch_moments_d<T, 5>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 6: launch_moments_d<T, 6>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        case 7: launch_moments_d<T, 7>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
        default: launch_moments_d<T, 8>(grid, st, nodes, list, dt, t, tiles_per_chunk, n_tiles, partial, slots); break;
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace

extern "C" {

int pbn_clg_fit(pbn_ctx* ctx, const pbn_dtable* dt, const pbn_table* t, int n_nodes, const int* var, const int* dpar_off, const int* dparents,
                const int* cpar_off, const int* cparents, const int64_t* cell_off, const int64_t* param_off, int64_t* rows, double* params,
                unsigned char* status, double* shift, double* moments, int64_t* launches) {
    return guarded(mu_of(ctx), [&] {
        const char* who = "pbn_clg_fit";
        auto bad = [&](const char* what) { return invalid_error(std::string(who) + ": " + what); };
        if (!ctx || !dt || !t || !var || !dpar_off || !dparents || !cpar_off || !cparents || !cell_off || !param_off || !rows || !params || !status)
            throw bad("null argument");
        if (ctx != dt->ctx.p || ctx != t->ctx.p) throw bad("the tables belong to different contexts");
        if (dt->n_rows != t->n_rows) throw bad("the two tables differ in their number of rows");
        if (n_nodes < 1) throw bad("at least one node");
        if (dpar_off[0] != 0 || cpar_off[0] != 0 || cell_off[0] != 0 || param_off[0] != 0) throw bad("the offsets do not start at 0");
        std::vector<FitNode> nodes((size_t)n_nodes);
        std::vector<int> keys;
        for (int n = 0; n < n_nodes; ++n) {
            const int dp = dpar_off[n + 1] - dpar_off[n], p = cpar_off[n + 1] - cpar_off[n];
            if (dp < 0 || p < 0) throw bad("bad offsets");
            if (dp < 1) throw bad("a node without discrete parents");
            if (dp > FIT_MAX_DISCRETE_PARENTS) throw bad("a node with more than 7 discrete parents");
            if (1 + p > FIT_MAX_D) throw bad("a node with more than 8 continuous family columns");
            FitNode& d = nodes[(size_t)n];
            d = FitNode{};
            d.D = p + 1;
            d.m = dp;
            d.ccol[0] = var[n];
            for (int j = 0; j < p; ++j) d.ccol[1 + j] = cparents[cpar_off[n] + j];
            for (int j = 0; j < d.D; ++j)
                if (d.ccol[j] < 0 || d.ccol[j] >= t->n_cols) throw bad("column out of range");
            keys.assign(dparents + dpar_off[n], dparents + dpar_off[n] + dp);
            check_family_cols(dt->n_cols, keys, who);
            std::copy(keys.begin(), keys.end(), d.dcol);
            const int64_t G = family_strides(dt->card, keys, d.stride, FIT_MAX_CONFIGS);
            if (G > FIT_MAX_CONFIGS) throw bad("a node with more configurations than PBN_CLG_FIT_MAX_CONFIGS");
            d.G = (uint32_t)G;
            if (cell_off[n + 1] - cell_off[n] != G) throw bad("the cell offsets do not match the cardinalities");
            if (param_off[n + 1] - param_off[n] != G * (p + 2)) throw bad("the parameter offsets do not match the cardinalities");
        }
        // every family is within the caps: only now are the outputs written
        const int64_t n_cells = cell_off[n_nodes], n_rows = t->n_rows;
        std::fill(rows, rows + n_cells, (int64_t)0);
        std::fill(status, status + n_cells, (unsigned char)0);
        std::fill(params, params + param_off[n_nodes], 0.0);
        std::vector<int64_t> mom_off((size_t)n_nodes + 1, 0), shift_off((size_t)n_nodes + 1, 0);   // of the two optional outputs
        for (int n = 0; n < n_nodes; ++n) {
            const int D = nodes[(size_t)n].D;
            mom_off[(size_t)n + 1] = mom_off[(size_t)n] + (int64_t)nodes[(size_t)n].G * (stats_of(D) - 1);
            shift_off[(size_t)n + 1] = shift_off[(size_t)n] + (int64_t)nodes[(size_t)n].G * D;
        }
        if (moments) std::fill(moments, moments + mom_off[(size_t)n_nodes], 0.0);
        if (shift) std::fill(shift, shift + shift_off[(size_t)n_nodes], 0.0);
        if (launches) *launches = 0;
        if (n_rows == 0) return;

        HIP_CHECK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const int n_tiles = (int)ceil_div(n_rows, FIT_TILE);
        const int tiles_per_chunk = (int)ceil_div(n_tiles, FIT_MAX_CHUNKS);
        const int n_chunks = (int)ceil_div(n_tiles, tiles_per_chunk);
        int64_t n_launches = 0;

        dev_buf<double> shift_dev((size_t)t->n_cols);
        if (t->dtype == PBN_F64)
            hipLaunchKernelGGL((clg_fit_shift_kernel<double>), dim3((unsigned)ceil_div(t->n_cols, BLOCK)), dim3(BLOCK), 0, st, (const double*)t->data, t->ld,
                               t->n_cols, shift_dev.p);
        else
            hipLaunchKernelGGL((clg_fit_shift_kernel<float>), dim3((unsigned)ceil_div(t->n_cols, BLOCK)), dim3(BLOCK), 0, st, (const float*)t->data, t->ld,
                               t->n_cols, shift_dev.p);
        HIP_CHECK(hipGetLastError());
        ++n_launches;
        std::vector<double> col_shift((size_t)t->n_cols);
        HIP_CHECK(hipMemcpyAsync(col_shift.data(), shift_dev.p, col_shift.size() * sizeof(double), hipMemcpyDeviceToHost, st));

        // a chunk's record: every node's cells one after the other
        int64_t slots = 0;
        for (FitNode& d : nodes) {
            d.slot_off = slots;
            slots += (int64_t)d.G * stats_of(d.D);
        }
        // the nodes by their number of columns: one launch per D that occurs
        std::vector<int> list;
        int first_of[FIT_MAX_D + 2];
        for (int D = 1; D <= FIT_MAX_D; ++D) {
            first_of[D] = (int)list.size();
            for (int n = 0; n < n_nodes; ++n)
                if (nodes[(size_t)n].D == D) list.push_back(n);
        }
        first_of[FIT_MAX_D + 1] = (int)list.size();
        dev_buf<FitNode> nodes_dev((size_t)n_nodes);
        dev_buf<int> list_dev((size_t)n_nodes);
        dev_buf<double> partial_dev((size_t)slots * n_chunks), out_dev((size_t)slots);
        HIP_CHECK(hipMemcpyAsync(nodes_dev.p, nodes.data(), (size_t)n_nodes * sizeof(FitNode), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(list_dev.p, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(partial_dev.p, 0, (size_t)slots * n_chunks * sizeof(double), st));
        for (int D = 1; D <= FIT_MAX_D; ++D) {
            const int count = first_of[D + 1] - first_of[D];
            if (!count) continue;
            const dim3 grid((unsigned)n_chunks, (unsigned)count);
            if (t->dtype == PBN_F64)
                launch_moments<double>(D, grid, st, nodes_dev.p, list_dev.p + first_of[D], dt, t, tiles_per_chunk, n_tiles, partial_dev.p, slots);
            else
                launch_moments<float>(D, grid, st, nodes_dev.p, list_dev.p + first_of[D], dt, t, tiles_per_chunk, n_tiles, partial_dev.p, slots);
            ++n_launches;
        }
        hipLaunchKernelGGL(clg_fit_reduce_kernel, dim3((unsigned)ceil_div(slots, BLOCK)), dim3(BLOCK), 0, st, partial_dev.p, slots, n_chunks, out_dev.p);
        HIP_CHECK(hipGetLastError());
        ++n_launches;
        std::vector<double> out((size_t)slots);
        HIP_CHECK(hipMemcpyAsync(out.data(), out_dev.p, (size_t)slots * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));

        std::vector<double> mu(FIT_MAX_D), sse((size_t)FIT_MAX_D * FIT_MAX_D), G2((size_t)FIT_MAX_D * FIT_MAX_D), beta(FIT_MAX_D);
        const bool guard = lg_guard_on();
        for (int n = 0; n < n_nodes; ++n) {
            const FitNode& d = nodes[(size_t)n];
            const int D = d.D, p = D - 1, S1 = stats_of(D);
            for (int64_t c = 0; c < (int64_t)d.G; ++c) {
                const double* rec = out.data() + d.slot_off + c * S1;
                const int64_t cell = cell_off[n] + c, N = (int64_t)rec[0];
                rows[cell] = N;
                if (moments) std::copy(rec + 1, rec + S1, moments + mom_off[(size_t)n] + c * (S1 - 1));
                if (shift)
                    for (int j = 0; j < D; ++j) shift[shift_off[(size_t)n] + c * D + j] = col_shift[(size_t)d.ccol[j]];
                if (N == 0) continue;
                const double* S = rec + 1;
                const double* U = rec + 1 + D;
                int pos = 0;
                for (int i = 0; i < D; ++i)
                    for (int j = i; j < D; ++j, ++pos) G2[i + (size_t)j * D] = G2[j + (size_t)i * D] = U[pos];
                const double Nd = (double)N;
                for (int i = 0; i < D; ++i) mu[i] = col_shift[(size_t)d.ccol[i]] + S[i] / Nd;
                for (int j = 0; j < D; ++j)
                    for (int i = 0; i < D; ++i) sse[i + (size_t)j * D] = G2[i + (size_t)j * D] - S[i] * S[j] / Nd;
                bool suspect = false;
                const double variance = lg_fit(N, p, mu.data(), sse.data(), beta.data(), &suspect);
                if (suspect && guard && D <= 16) {   // pbn_lg_fit_table's condition: the caller refits this cell from its rows
                    status[cell] = 2;
                    continue;
                }
                double* dst = params + param_off[n] + c * (p + 2);
                std::copy(beta.begin(), beta.begin() + D, dst);
                dst[D] = variance;
                status[cell] = 1;
            }
        }
        if (launches) *launches = n_launches;
    });
}

}  // extern "C"
