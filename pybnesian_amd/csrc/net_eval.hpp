// What the one-pass network evaluators - discrete_model.hip (pbn_dnet), gaussian_model.hip (pbn_gnet), clg_model.hip (pbn_clgnet) - share
// on the host: the checks and strides of a family of code columns, the bodies of the *_stats and *_destroy entry points, and the two
// ways a launch's result reaches the host (the rows' values; per node the sum of its groups' partials).  Host code only: the block
// tree behind those partials stays written out in gnet_logl_kernel and clgnet_logl_kernel - as a shared __device__ function it compiled
// to other instructions (the tree's last step lost its 16-byte LDS reads).
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"

namespace pbn {

constexpr int NET_GROUP_ROWS = 256;   // consecutive rows behind one partial of a node's sum: the workgroup of the two kernels

// ---- families of code columns ----------------------------------------------------------------------------------------------------------

inline void check_family_cols(int n_cols, const std::vector<int>& cols, const char* who) {
    for (size_t a = 0; a < cols.size(); ++a) {
        if (cols[a] < 0 || cols[a] >= n_cols) throw invalid_error(std::string(who) + ": column out of range");
        for (size_t b = 0; b < a; ++b)
            if (cols[a] == cols[b]) throw invalid_error(std::string(who) + ": a column appears twice in a family");
    }
}

inline int64_t cells_of(const std::vector<int>& card, const std::vector<int>& cols, const char* who) {
    int64_t G = 1;
    for (int c : cols) {
        if (G > (std::numeric_limits<int64_t>::max() >> 1) / std::max(card[c], 1)) throw invalid_error(std::string(who) + ": a family's table has too many cells");
        G *= card[c];
    }
    return G;
}

// stride[j] of cols[j] in the family's key (the first column fastest) and the cells of the key.  Stops at the first product above
// `cap` and returns it: the caller names what was exceeded.
inline int64_t family_strides(const std::vector<int>& card, const std::vector<int>& cols, uint32_t* stride, int64_t cap) {
    int64_t G = 1;
    for (size_t j = 0; j < cols.size(); ++j) {
        stride[j] = (uint32_t)G;
        G *= card[(size_t)cols[j]];
        if (G > cap) break;
    }
    return G;
}

// ---- handles ---------------------------------------------------------------------------------------------------------------------------

template <typename H>
void destroy_handle(H* h) {
    if (!h) return;
    ctx_pin pin(h->ctx);
    std::lock_guard<std::recursive_mutex> lock(mu_of(h));
    delete h;
}

template <typename H>
int handle_stats(const H* h, const char* who, int64_t H::*launches, int64_t H::*rows, int64_t* out_launches, int64_t* out_rows) {
    return guarded(mu_of(h), [&] {
        if (!h) throw invalid_error(std::string(who) + ": null argument");
        if (out_launches) *out_launches = h->*launches;
        if (out_rows) *out_rows = h->*rows;
    });
}

// ---- a launch's result on the host -------------------------------------------------------------------------------------------------------

// launch(double* dev) fills n doubles, one per row (n >= 1); they are copied to `out`.
template <typename Launch>
void rows_to_host(pbn_ctx* ctx, int64_t n, double* out, const Launch& launch) {
    HIP_CHECK(hipSetDevice(ctx->device));
    dev_buf<double> dout((size_t)n);
    launch(dout.p);
    HIP_CHECK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// launch(double* dev) fills [N][ceil(n / 256)] partials; node i's are added in block order from 0.0 - lg_eval's
// order - into node_slogl[i].  A table without rows launches nothing and gives zeros.
template <typename Launch>
void node_sums_to_host(pbn_ctx* ctx, size_t N, int64_t n, double* node_slogl, const Launch& launch) {
    for (size_t i = 0; i < N; ++i) node_slogl[i] = 0.0;
    if (n == 0) return;
    HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n_groups = (size_t)ceil_div(n, NET_GROUP_ROWS);
    dev_buf<double> dpart(N * n_groups);
    launch(dpart.p);
    std::vector<double> part(N * n_groups);
    HIP_CHECK(hipMemcpyAsync(part.data(), dpart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < N; ++i) {
        double s = 0.0;
        for (size_t b = 0; b < n_groups; ++b) s += part[i * n_groups + b];   // fixed order: lg_eval's
        node_slogl[i] = s;
    }
}

}  // namespace pbn
