// Evaluating a conditional linear Gaussian network - DiscreteFactors and (C)LinearGaussianCPDs - in one device pass
// (models/BayesianNetwork.hpp:997-1022 BNGeneric::logl / slogl over factors/discrete/DiscreteAdaptator.hpp:327-348,
// factors/discrete/DiscreteFactor.cpp:91-171 and factors/continuous/LinearGaussianCPD.cpp:92-149) - instead of, per continuous node and
// configuration of its discrete parents, a row selection, a take, an upload of the slice, one pbn_lg_logl launch, a copy and a scatter.
//
// pbn_clgnet: one descriptor per node and the concatenated parameters, on the device.  A discrete node's parameters are its CPT (the
// variable fastest, the parents in the given order: pbn_dnet's layout).  A CLG node's are one record per configuration of its discrete
// parents (the first parent fastest): inv_std, cte, then the p + 1 coefficients, intercept first - p + 3 doubles, the constants from
// lg_constants on the host.  A configuration without a factor keeps its record - zeros under a NaN cte - so a row's key is an address
// whenever it is a configuration at all, and lg_value gives such a row NaN with no second look-up.
//
// clgnet_logl_kernel is gnet_logl_kernel (gaussian_model.hip) with a key in front of each node: 256 threads, a tile of 1 024 rows, a lane
// owns rows r, r + 256, r + 512, r + 768 of BOTH tables (row r of the codes is row r of the continuous table) and walks the nodes in node
// order.  The descriptors, the parent lists and the column bases are read with wave-uniform indices (scalar loads); the key is formed
// from the int32 codes as dnet_logl_kernel's int32 branch forms it; a CPT cell or a record is gathered with a per-lane index, clamped to
// 0 when the key is no address (a -1 code), and the value is masked to NaN then.  A node's records are few and every row reuses them:
// they are served from the L1 / L2, nothing is staged in LDS.  The Gaussian value is lg_rows_z_lanes / lg_value (stats_kernels.hpp):
// lg_rows_z's statements with the coefficients read per lane - the per-factor bits.
//   SUMS = false  the row's result starts from the first node's value and adds the others in node order, fp64 adds only.
//   SUMS = true   per node and group of 256 consecutive rows one partial: gnet_logl_kernel's block tree over the group's values in row
//                 order, a NaN value and a row past the end contributing +0.0.  The host adds a node's partials in block order from 0.0.
// The byte mirror of a pbn_dtable is not read: 3 bytes a row and column saved beside 8-byte doubles, for twice the instantiations.
#include <algorithm>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "common.hpp"
#include "discrete_model.hpp"
#include "net_eval.hpp"
#include "stats_kernels.hpp"

using namespace pbn;

namespace {

constexpr int BLOCK = 256;
constexpr int V = 4;                          // rows of a lane, BLOCK apart: the row tile of a workgroup is 1 024
constexpr int CLG_MAX_KEY_COLS = 8;           // a discrete family: the variable and 7 parents (pbn_dnet's cap); a CLG node: 7 parents
constexpr int CLG_MAX_DISCRETE_PARENTS = 7;
constexpr int CLG_MAX_FAMILY = 64;            // a CLG node's continuous columns, the variable and 63 parents: the cap of pbn_lg_logl
constexpr int64_t CLG_MAX_CONFIGS = PBN_CLGNET_MAX_CONFIGS;
constexpr int64_t CLG_MAX_PARAMS = PBN_CLGNET_MAX_PARAMS;

static_assert(BLOCK == NET_GROUP_ROWS, "a partial is one workgroup of rows");

struct CNode {
    int kind;        // 0 discrete, 1 CLG
    int var;         // the variable's column: of the codes (discrete) or of the continuous table (CLG)
    int m;           // key columns: the discrete family (the variable first), or a CLG node's discrete parents
    int p;           // continuous parents (CLG)
    uint32_t G;      // cells of the CPT, or configurations
    uint32_t rec;    // doubles of a record: p + 3 (CLG)
    uint32_t off;    // first parameter of the node in the concatenated parameters
    int cpar_off;    // first continuous parent in the concatenated continuous parents
    int col[CLG_MAX_KEY_COLS];
    uint32_t stride[CLG_MAX_KEY_COLS];
};

}  // namespace

struct pbn_clgnet {
    pbn::ctx_ptr ctx;
    int n_dcols = 0, n_ccols = 0;
    std::vector<int> card;
    std::vector<CNode> nodes;
    pbn::dev_buf<CNode> nodes_dev;
    pbn::dev_buf<int> cparents_dev;
    pbn::dev_buf<double> params_dev;
    mutable int64_t launches = 0, rows = 0;
};

namespace {

// grid = row tiles.  `out`: SUMS ? [n_nodes][ceil(n_rows / 256)] partials : [n_rows] sums over the nodes.  codes: [n_dcols][n_rows].
// Waves per SIMD: 7 asked for.  The per-row instantiations hold four running sums beside what the sums' hold, and per-lane records cost
// an address pair per load where gnet_logl_kernel reads a scalar: 72 VGPRs under this bound, 80 (double) / 74 (float) without it, and 12
// bytes of scratch under a bound of 8.  The SUMS instantiations take 58 and run eight.
template <typename T, bool SUMS>
__global__ __launch_bounds__(BLOCK, 7) void clgnet_logl_kernel(const CNode* __restrict__ nodes, int n_nodes, const int* __restrict__ cparents,
                                                             const double* __restrict__ params, const int32_t* __restrict__ codes,
                                                             const T* __restrict__ base, int64_t ld, int64_t n_rows, double* __restrict__ out) {
    __shared__ double red[SUMS ? V : 1][BLOCK];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int t = threadIdx.x;
    // rows in 32 bits: a pbn_dtable has at most 2^31 - 1 of them
    const uint32_t n32 = (uint32_t)n_rows, r = blockIdx.x * (uint32_t)(BLOCK * V) + t;
    uint32_t src[V];   // a row past the end reads the last row instead; its value is dropped below
#pragma unroll
    for (int i = 0; i < V; ++i) src[i] = min(r + (uint32_t)(i * BLOCK), n32 - 1u);
    const int64_t n_groups = (n_rows + BLOCK - 1) / BLOCK;
    double acc[V];
    for (int n = 0; n < n_nodes; ++n) {
        const CNode& d = nodes[n];
        uint32_t key[V];
        int32_t any[V];   // the codes or-ed: negative when one of them is -1
#pragma unroll
        for (int i = 0; i < V; ++i) { key[i] = 0u; any[i] = 0; }
        const int m = d.m;
        for (int j = 0; j < m; ++j) {
            const int32_t* col = codes + (int64_t)d.col[j] * n_rows;
            const uint32_t stride = d.stride[j];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const int32_t code = col[src[i]];
                key[i] += (uint32_t)code * stride;
                any[i] |= code;
            }
        }
        const uint32_t G = d.G;
        const double* par = params + d.off;
        double v[V];
        // the key is an address only when it is inside the CPT / the records (G >= 1: cell 0, record 0 exist)
        bool ok[V];
#pragma unroll
        for (int i = 0; i < V; ++i) {
            ok[i] = (any[i] >= 0) & (key[i] < G);
            key[i] = ok[i] ? key[i] : 0u;
        }
        if (d.kind == 0) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const double lp = par[key[i]];
                v[i] = ok[i] ? lp : nan;
            }
        } else {
            uint32_t rec[V];
            double z[V];
#pragma unroll
            for (int i = 0; i < V; ++i) rec[i] = key[i] * d.rec;
            lg_rows_z_lanes<T, V>(base, ld, d.var, cparents + d.cpar_off, d.p, par, rec, src, z);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const double val = lg_value(z[i], par[rec[i] + 1u]);   // (a configuration without a factor: cte = NaN)
                v[i] = ok[i] ? val : nan;
            }
        }
        if constexpr (SUMS) {
#pragma unroll
            for (int i = 0; i < V; ++i) red[i][t] = (r + (uint32_t)(i * BLOCK) < n32 && v[i] == v[i]) ? v[i] : 0.0;
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
            for (int i = 0; i < V; ++i) acc[i] = n == 0 ? v[i] : acc[i] + v[i];
        }
    }
    if constexpr (!SUMS) {
#pragma unroll
        for (int i = 0; i < V; ++i)
            if (r + (uint32_t)(i * BLOCK) < n32) out[r + (uint32_t)(i * BLOCK)] = acc[i];
    }
}

template <bool SUMS>
void launch_clgnet(const pbn_clgnet* g, const pbn_dtable* dt, const pbn_table* t, double* out) {
    const int64_t n = t->n_rows;
    const dim3 grid((unsigned)ceil_div(n, (int64_t)BLOCK * V)), block(BLOCK);
    hipStream_t st = g->ctx->stream;
    if (t->dtype == PBN_F64)
        hipLaunchKernelGGL((clgnet_logl_kernel<double, SUMS>), grid, block, 0, st, g->nodes_dev.p, (int)g->nodes.size(), g->cparents_dev.p,
                           g->params_dev.p, dt->codes_dev.p, (const double*)t->data, t->ld, n, out);
    else
        hipLaunchKernelGGL((clgnet_logl_kernel<float, SUMS>), grid, block, 0, st, g->nodes_dev.p, (int)g->nodes.size(), g->cparents_dev.p,
                           g->params_dev.p, dt->codes_dev.p, (const float*)t->data, t->ld, n, out);
    HIP_CHECK(hipGetLastError());
    g->launches += 1;
    g->rows += n;
}

void check_tables(const pbn_clgnet* g, const pbn_dtable* dt, const pbn_table* t, const char* who) {
    const std::string w(who);
    if (!g || !dt || !t) throw invalid_error(w + ": null argument");
    if (g->ctx.p != dt->ctx.p || g->ctx.p != t->ctx.p) throw invalid_error(w + ": the network and the tables belong to different contexts");
    if (dt->n_rows != t->n_rows) throw invalid_error(w + ": the two tables differ in their number of rows");
    if (dt->n_cols != g->n_dcols || dt->card != g->card) throw invalid_error(w + ": the code table's cardinalities are not the network's");
    if (t->n_cols < g->n_ccols) throw invalid_error(w + ": the continuous table has fewer columns than the network");
}

}  // namespace

extern "C" {

int pbn_clgnet_create(pbn_ctx* ctx, int n_dcols, const int* cardinality, int n_ccols, int n_nodes, const int* kind, const int* var,
                      const int* dpar_off, const int* dparents, const int* cpar_off, const int* cparents, const int* cfg_off,
                      const unsigned char* present, const int64_t* param_off, const double* params, pbn_clgnet** out) {
    return guarded(mu_of(ctx), [&] {
        const char* who = "pbn_clgnet_create";
        auto bad = [&](const char* what) { return invalid_error(std::string(who) + ": " + what); };
        if (!ctx || !out || !cardinality || !kind || !var || !dpar_off || !dparents || !cpar_off || !cparents || !cfg_off || !present || !param_off ||
            !params)
            throw bad("null argument");
        if (n_nodes < 1 || n_dcols < 1 || n_ccols < 1) throw bad("a network has at least one node and one column of each kind");
        if (dpar_off[0] != 0 || cpar_off[0] != 0 || cfg_off[0] != 0 || param_off[0] != 0) throw bad("the offsets do not start at 0");
        std::unique_ptr<pbn_clgnet> g(new pbn_clgnet);
        g->ctx = ctx;
        g->n_dcols = n_dcols;
        g->n_ccols = n_ccols;
        g->card.assign(cardinality, cardinality + n_dcols);
        for (int c : g->card)
            if (c < 1) throw bad("a cardinality below 1");
        g->nodes.resize((size_t)n_nodes);
        int64_t total = 0;   // doubles of parameters on the device
        std::vector<int> keys;
        for (int n = 0; n < n_nodes; ++n) {
            const int dp = dpar_off[n + 1] - dpar_off[n], p = cpar_off[n + 1] - cpar_off[n], n_cfg = cfg_off[n + 1] - cfg_off[n];
            if (dp < 0 || p < 0 || n_cfg < 0) throw bad("bad offsets");
            if (kind[n] != 0 && kind[n] != 1) throw bad("a node kind that is neither 0 (discrete) nor 1 (CLG)");
            const bool clg = kind[n] == 1;
            CNode& d = g->nodes[(size_t)n];
            d = CNode{};
            d.kind = kind[n];
            d.var = var[n];
            keys.clear();
            if (clg) {
                if (dp > CLG_MAX_DISCRETE_PARENTS) throw bad("a CLG node with more than 7 discrete parents");
                if (1 + p > CLG_MAX_FAMILY) throw bad("a CLG node with more than 64 continuous family columns");
                if (var[n] < 0 || var[n] >= n_ccols) throw bad("column out of range");
                for (int j = 0; j < p; ++j)
                    if (cparents[cpar_off[n] + j] < 0 || cparents[cpar_off[n] + j] >= n_ccols) throw bad("column out of range");
            } else {
                if (1 + dp > CLG_MAX_KEY_COLS) throw bad("a discrete node with more than 8 family variables");
                if (p != 0 || n_cfg != 0) throw bad("a discrete node with continuous parents or configuration marks");
                keys.push_back(var[n]);
            }
            keys.insert(keys.end(), dparents + dpar_off[n], dparents + dpar_off[n] + dp);
            check_family_cols(n_dcols, keys, who);
            d.m = (int)keys.size();
            std::copy(keys.begin(), keys.end(), d.col);
            const int64_t cap = clg ? CLG_MAX_CONFIGS : CLG_MAX_PARAMS;
            const int64_t G = family_strides(g->card, keys, d.stride, cap);
            if (G > cap) throw bad(clg ? "a CLG node with more than 2^20 configurations" : "the parameters exceed 2^28 doubles");
            d.G = (uint32_t)G;
            d.p = p;
            d.rec = (uint32_t)(p + 3);
            d.cpar_off = cpar_off[n];
            if (clg && n_cfg != G) throw bad("the configuration offsets do not match the cardinalities");
            if (param_off[n + 1] - param_off[n] != (clg ? G * (p + 2) : G)) throw bad("the parameter offsets do not match the cardinalities");
            d.off = (uint32_t)total;
            total += clg ? G * (p + 3) : G;
            if (total > CLG_MAX_PARAMS) throw bad("the parameters exceed 2^28 doubles");
        }
        // every family is within the caps: only now are the parameters read
        std::vector<double> dev_params((size_t)total, 0.0);
        for (int n = 0; n < n_nodes; ++n) {
            const CNode& d = g->nodes[(size_t)n];
            const double* src = params + param_off[n];
            double* dst = dev_params.data() + d.off;
            if (d.kind == 0) {
                std::copy(src, src + d.G, dst);
                continue;
            }
            const int p = d.p;
            for (int64_t c = 0; c < (int64_t)d.G; ++c) {
                double* rec = dst + (size_t)c * (size_t)(p + 3);
                if (!present[cfg_off[n] + c]) {   // zeros under a NaN cte: lg_value gives NaN
                    rec[1] = std::numeric_limits<double>::quiet_NaN();
                    continue;
                }
                const double* in = src + c * (p + 2);
                lg_constants(in[p + 1], &rec[0], &rec[1]);
                for (int j = 0; j <= p; ++j) rec[2 + j] = in[j];
            }
        }
        const size_t n_cpar = (size_t)cpar_off[n_nodes];
        HIP_CHECK(hipSetDevice(ctx->device));
        g->nodes_dev.alloc((size_t)n_nodes);
        g->cparents_dev.alloc(n_cpar + 1);   // (never empty: a network without continuous arcs still hands the kernel a pointer)
        g->params_dev.alloc(dev_params.size());
        HIP_CHECK(hipMemcpyAsync(g->nodes_dev.p, g->nodes.data(), (size_t)n_nodes * sizeof(CNode), hipMemcpyHostToDevice, ctx->stream));
        if (n_cpar) HIP_CHECK(hipMemcpyAsync(g->cparents_dev.p, cparents, n_cpar * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(g->params_dev.p, dev_params.data(), dev_params.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *out = g.release();
    });
}

void pbn_clgnet_destroy(pbn_clgnet* g) { destroy_handle(g); }

int pbn_clgnet_logl(const pbn_clgnet* g, const pbn_dtable* dt, const pbn_table* t, double* out) {
    return guarded(mu_of(t), [&] {
        check_tables(g, dt, t, "pbn_clgnet_logl");
        const int64_t n = t->n_rows;
        if (n == 0) return;
        if (!out) throw invalid_error("pbn_clgnet_logl: null output");
        rows_to_host(t->ctx, n, out, [&](double* dev) { launch_clgnet<false>(g, dt, t, dev); });
    });
}

int pbn_clgnet_slogl(const pbn_clgnet* g, const pbn_dtable* dt, const pbn_table* t, double* node_slogl) {
    return guarded(mu_of(t), [&] {
        check_tables(g, dt, t, "pbn_clgnet_slogl");
        if (!node_slogl) throw invalid_error("pbn_clgnet_slogl: null output");
        node_sums_to_host(t->ctx, g->nodes.size(), t->n_rows, node_slogl, [&](double* dev) { launch_clgnet<true>(g, dt, t, dev); });
    });
}

int pbn_clgnet_stats(const pbn_clgnet* g, int64_t* launches, int64_t* rows) {
    return handle_stats(g, "pbn_clgnet_stats", &pbn_clgnet::launches, &pbn_clgnet::rows, launches, rows);
}

}  // extern "C"
