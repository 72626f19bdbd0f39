// Evaluating a network of LinearGaussianCPDs in one device pass (models/BayesianNetwork.hpp:997-1022 BNGeneric::logl / slogl over
// factors/continuous/LinearGaussianCPD.cpp:92-149) - instead of one pbn_lg_logl launch, one buffer of `rows` doubles and one copy of
// it to the host per node.
//
// pbn_gnet: the nodes' descriptors (variable column, parent range, coefficient offset, inv_std, cte) and the concatenated parents and
// coefficients, on the device.  gnet_logl_kernel covers the whole table and every node in one launch: 256 threads, a tile of 1 024 rows,
// a lane owns rows r, r + 256, r + 512, r + 768 - four coalesced loads per column and four independent chains - and walks the nodes in
// node order; the descriptors are read with wave-uniform indices (scalar loads).  A node's value of a row is lg_rows_z / lg_value
// (stats_kernels.hpp), the text lg_logl_kernel is made of: the per-factor bits.
//   SUMS = false  the row's result starts from the first node's value and adds the others in node order - fp64 adds only, what
//                 `out = ll_0; out = out + ll_1; ...` computes on the host.
//   SUMS = true   per node and group of 256 consecutive rows one partial: lg_logl_kernel's block tree over the group's values in row
//                 order, rows past the end contributing +0.0; the four groups of a tile go through one red[4][256] buffer.  The host adds
//                 a node's partials in block order from 0.0, as lg_eval does.  No per-row vector exists in this mode.
// Columns are NOT staged in LDS: a network has any number of columns, a column is read once per family it belongs to, and a
// workgroup's 8 KiB of it stay in the L1 / L2 between those reads.  Loads are one element wide, so any leading dimension is served
// (pbn_table_from_device borrows any).
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "net_eval.hpp"
#include "stats_kernels.hpp"

using namespace pbn;

namespace {

constexpr int BLOCK = 256;
constexpr int V = 4;                 // rows of a lane, BLOCK apart: the row tile of a workgroup is 1 024
constexpr int GNET_MAX_FAMILY = 64;  // the variable and 63 parents: the cap of pbn_lg_logl / LgArgs

static_assert(BLOCK == NET_GROUP_ROWS, "a partial is one workgroup of rows");

struct GNode {
    int var;        // the variable's column
    int p;          // parents
    int par_off;    // first parent in the concatenated parents
    int beta_off;   // first coefficient (the intercept) in the concatenated coefficients: par_off + node index
    double inv_std;
    double cte;
};

}  // namespace

struct pbn_gnet {
    pbn::ctx_ptr ctx;
    int n_cols = 0;
    std::vector<GNode> nodes;
    pbn::dev_buf<GNode> nodes_dev;
    pbn::dev_buf<int> parents_dev;
    pbn::dev_buf<double> beta_dev;
    mutable int64_t launches = 0, rows = 0;
};

namespace {

// grid = row tiles.  `out`: SUMS ? [n_nodes][ceil(n_rows / 256)] partials : [n_rows] sums over the nodes.
template <typename T, bool SUMS>
__global__ __launch_bounds__(BLOCK) void gnet_logl_kernel(const GNode* __restrict__ nodes, int n_nodes, const int* __restrict__ parents,
                                                           const double* __restrict__ beta, const T* __restrict__ base, int64_t ld, int64_t n_rows,
                                                           double* __restrict__ out) {
    __shared__ double red[SUMS ? V : 1][BLOCK];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * (BLOCK * V) + t;
    int64_t src[V];   // a row past the end reads the last row instead; its value is dropped below
    bool live[V];
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const int64_t row = r + (int64_t)i * BLOCK;
        live[i] = row < n_rows;
        src[i] = live[i] ? row : n_rows - 1;
    }
    const int64_t n_groups = (n_rows + BLOCK - 1) / BLOCK;
    double acc[V];
    for (int n = 0; n < n_nodes; ++n) {
        const GNode d = nodes[n];
        double z[V];
        lg_rows_z<T, V>(base, ld, d.var, parents + d.par_off, d.p, beta + d.beta_off, src, d.inv_std, z);
        if constexpr (SUMS) {
#pragma unroll
            for (int i = 0; i < V; ++i) red[i][t] = live[i] ? lg_value(z[i], d.cte) : 0.0;
            __syncthreads();
#pragma unroll
            for (int s = BLOCK / 2; s > 0; s >>= 1) {
                if (t < s) {
#pragma unroll
                    for (int i = 0; i < V; ++i) red[i][t] += red[i][t + s];
                }
                __syncthreads();
            }
            // (lane 0 alone reads red[i][0] from here on and alone writes it for the next node: no barrier in between)
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const int64_t g = (int64_t)blockIdx.x * V + i;
                    if (g < n_groups) out[(int64_t)n * n_groups + g] = red[i][0];
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const double v = lg_value(z[i], d.cte);
                acc[i] = n == 0 ? v : acc[i] + v;
            }
        }
    }
    if constexpr (!SUMS) {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (live[i]) out[r + (int64_t)i * BLOCK] = acc[i];
    }
}

template <bool SUMS>
void launch_gnet(const pbn_gnet* g, const pbn_table* t, double* out) {
    const int64_t n = t->n_rows;
    const dim3 grid((unsigned)ceil_div(n, (int64_t)BLOCK * V)), block(BLOCK);
    hipStream_t st = g->ctx->stream;
    if (t->dtype == PBN_F64)
        hipLaunchKernelGGL((gnet_logl_kernel<double, SUMS>), grid, block, 0, st, g->nodes_dev.p, (int)g->nodes.size(), g->parents_dev.p, g->beta_dev.p,
                           (const double*)t->data, t->ld, n, out);
    else
        hipLaunchKernelGGL((gnet_logl_kernel<float, SUMS>), grid, block, 0, st, g->nodes_dev.p, (int)g->nodes.size(), g->parents_dev.p, g->beta_dev.p,
                           (const float*)t->data, t->ld, n, out);
    HIP_CHECK(hipGetLastError());
    g->launches += 1;
    g->rows += n;
}

void check_table(const pbn_gnet* g, const pbn_table* t, const char* who) {
    if (!g || !t) throw invalid_error(std::string(who) + ": null argument");
    if (g->ctx.p != t->ctx.p) throw invalid_error(std::string(who) + ": the network and the table belong to different contexts");
    if (t->n_cols < g->n_cols) throw invalid_error(std::string(who) + ": the table has fewer columns than the network");
}

}  // namespace

extern "C" {

int pbn_gnet_create(pbn_ctx* ctx, int n_cols, int n_nodes, const int* var, const int* par_off, const int* parents, const double* beta,
                    const double* variance, pbn_gnet** out) {
    return guarded(mu_of(ctx), [&] {
        if (!ctx || !out || !var || !par_off || !parents || !beta || !variance) throw invalid_error("pbn_gnet_create: null argument");
        if (n_nodes < 1 || n_cols < 1) throw invalid_error("pbn_gnet_create: a network has at least one node and one column");
        if (par_off[0] != 0) throw invalid_error("pbn_gnet_create: the parent offsets do not start at 0");
        std::unique_ptr<pbn_gnet> g(new pbn_gnet);
        g->ctx = ctx;
        g->n_cols = n_cols;
        g->nodes.resize((size_t)n_nodes);
        for (int n = 0; n < n_nodes; ++n) {
            const int p = par_off[n + 1] - par_off[n];
            if (p < 0) throw invalid_error("pbn_gnet_create: bad parent offsets");
            if (1 + p > GNET_MAX_FAMILY) throw invalid_error("pbn_gnet_create: a node with more than 64 family columns");
            if (var[n] < 0 || var[n] >= n_cols) throw invalid_error("pbn_gnet_create: column out of range");
            for (int j = 0; j < p; ++j)
                if (parents[par_off[n] + j] < 0 || parents[par_off[n] + j] >= n_cols) throw invalid_error("pbn_gnet_create: column out of range");
            GNode& d = g->nodes[(size_t)n];
            d = GNode{};
            d.var = var[n];
            d.p = p;
            d.par_off = par_off[n];
            d.beta_off = par_off[n] + n;
            lg_constants(variance[n], &d.inv_std, &d.cte);
        }
        const size_t n_par = (size_t)par_off[n_nodes], n_beta = n_par + (size_t)n_nodes;
        HIP_CHECK(hipSetDevice(ctx->device));
        g->nodes_dev.alloc((size_t)n_nodes);
        g->parents_dev.alloc(n_par + 1);   // (never empty: a network without arcs still hands the kernel a pointer)
        g->beta_dev.alloc(n_beta);
        HIP_CHECK(hipMemcpyAsync(g->nodes_dev.p, g->nodes.data(), (size_t)n_nodes * sizeof(GNode), hipMemcpyHostToDevice, ctx->stream));
        if (n_par) HIP_CHECK(hipMemcpyAsync(g->parents_dev.p, parents, n_par * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(g->beta_dev.p, beta, n_beta * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = g.release();
    });
}

void pbn_gnet_destroy(pbn_gnet* g) { destroy_handle(g); }

int pbn_gnet_logl(const pbn_gnet* g, const pbn_table* t, double* out) {
    return guarded(mu_of(t), [&] {
        check_table(g, t, "pbn_gnet_logl");
        const int64_t n = t->n_rows;
        if (n == 0) return;
        if (!out) throw invalid_error("pbn_gnet_logl: null output");
        rows_to_host(t->ctx, n, out, [&](double* dev) { launch_gnet<false>(g, t, dev); });
    });
}

int pbn_gnet_slogl(const pbn_gnet* g, const pbn_table* t, double* node_slogl) {
    return guarded(mu_of(t), [&] {
        check_table(g, t, "pbn_gnet_slogl");
        if (!node_slogl) throw invalid_error("pbn_gnet_slogl: null output");
        node_sums_to_host(t->ctx, g->nodes.size(), t->n_rows, node_slogl, [&](double* dev) { launch_gnet<true>(g, t, dev); });
    });
}

int pbn_gnet_stats(const pbn_gnet* g, int64_t* launches, int64_t* rows) {
    return handle_stats(g, "pbn_gnet_stats", &pbn_gnet::launches, &pbn_gnet::rows, launches, rows);
}

}  // extern "C"
