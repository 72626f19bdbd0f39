// Host side of KDE / ProductKDE / CKDE fitting and evaluation, shared by the public handles and the score
// engine.  See kde_kernels.hip (and the units its header lists) for the device side.
#include <cstdio>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <numeric>
#include <vector>

#include "hostmath.hpp"
#include "kde_kernels.hpp"
#include "kde_model.hpp"
#include "stats_kernels.hpp"

namespace pbn {

static const double LOG2E = 1.4426950408889634073599246810019;
static const double LOG_2PI = 1.8378770664093454835606594728112;

void check_cols(const pbn_table* t, const int* cols, int d, const char* who) {
    if (!t || !cols) throw invalid_error(std::string(who) + ": null argument");
    for (int i = 0; i < d; ++i)
        if (cols[i] < 0 || cols[i] >= t->n_cols) throw invalid_error(std::string(who) + ": column index out of range");
}
void check_range(const pbn_table* t, int64_t row0, int64_t n, const char* who) {
    if (row0 < 0 || n < 0 || row0 + n > t->n_rows) throw invalid_error(std::string(who) + ": row range out of bounds");
}

void bandwidth_from_cov(int selector, int kind, const double* cov, int d, int64_t n, int dtype, double* out) {
    if (!cov || !out || d <= 0) throw invalid_error("pbn_bandwidth: bad argument");
    const bool f32 = dtype == PBN_F32;
    const double N = (double)n, D = (double)d;
    auto not_enough = [&](const char* what) {
        throw singular_error(std::string(what) + " of " + std::to_string(d) + " variables cannot be estimated with " +
                             std::to_string(n) + " instances");
    };
    if (selector == PBN_SEL_SCOTT) {
        // kde/ScottsBandwidth.hpp:66-117
        if (kind == PBN_BW_DIAG) {
            if (n <= 1) not_enough("Diagonal bandwidth matrix");
            const double k = std::pow(N, -2.0 / (D + 4.0));
            for (int i = 0; i < d; ++i) out[i] = k * cov[i + (size_t)i * d];
        } else {
            if (n <= d) not_enough("Bandwidth matrix");
            if (!hm::is_psd(cov, d, f32)) throw singular_error("Covariance matrix is not positive-definite.");
            const double k = std::pow(N, -2.0 / (D + 4.0));
            for (int i = 0; i < d * d; ++i) out[i] = k * cov[i];
        }
        return;
    }
    if (selector != PBN_SEL_NORMAL_REFERENCE) throw invalid_error("pbn_bandwidth: unknown selector");
    // kde/NormalReferenceRule.hpp:12-59 (pre-checks), :72-106 (diag), :109-134 (full)
    if (n <= d) not_enough(kind == PBN_BW_DIAG ? "Diagonal bandwidth matrix" : "Bandwidth matrix");
    if (!hm::is_psd(cov, d, f32)) throw singular_error("Covariance matrix is not positive-definite.");
    if (kind == PBN_BW_FULL) {
        const double k = std::pow(4.0 / (N * (D + 2.0)), 2.0 / (D + 4.0));
        for (int i = 0; i < d * d; ++i) out[i] = k * cov[i];
        return;
    }
    // Chacon & Duong (2018) eq. 3.4: delta = diag(cov)^-1 cov
    std::vector<double> delta((size_t)d * d), dinv((size_t)d * d);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) delta[i + (size_t)j * d] = cov[i + (size_t)j * d] / cov[i + (size_t)i * d];
    if (!hm::inverse(delta.data(), d, dinv.data())) throw singular_error("Covariance matrix is not positive-definite.");
    double tr = 0.0, tr2 = 0.0;
    for (int i = 0; i < d; ++i) tr += dinv[i + (size_t)i * d];
    for (int i = 0; i < d; ++i)
        for (int k2 = 0; k2 < d; ++k2) tr2 += dinv[i + (size_t)k2 * d] * dinv[k2 + (size_t)i * d];
    const double k = 4.0 * D * std::sqrt(hm::determinant(delta.data(), d)) / (2.0 * tr2 + tr * tr);
    const double f = std::pow(k / N, 2.0 / (D + 4.0));
    for (int i = 0; i < d; ++i) out[i] = f * cov[i + (size_t)i * d];
}

// The d x d block a FULL bandwidth matrix of `rule_d` >= d variables has over d of them, from THEIR covariance alone: both library
// selectors are H = k(N, rule_d) cov (kde/ScottsBandwidth.hpp:100-117, kde/NormalReferenceRule.hpp:109-134), so the block is
// k(N, rule_d) cov_sub - the very doubles of the sub-block of bandwidth_from_cov on the whole set.  Pre-checks on the block's own columns.
void bandwidth_full_block(int selector, const double* cov, int d, int rule_d, int64_t n, int dtype, double* out) {
    if (!cov || !out || d <= 0 || rule_d < d) throw invalid_error("pbn_bandwidth: bad argument");
    if (selector != PBN_SEL_SCOTT && selector != PBN_SEL_NORMAL_REFERENCE) throw invalid_error("pbn_bandwidth: unknown selector");
    if (n <= d)
        throw singular_error("Bandwidth matrix of " + std::to_string(d) + " variables cannot be estimated with " + std::to_string(n) + " instances");
    if (!hm::is_psd(cov, d, dtype == PBN_F32)) throw singular_error("Covariance matrix is not positive-definite.");
    const double N = (double)n, D = (double)rule_d;
    const double k = selector == PBN_SEL_SCOTT ? std::pow(N, -2.0 / (D + 4.0)) : std::pow(4.0 / (N * (D + 2.0)), 2.0 / (D + 4.0));
    for (int i = 0; i < d * d; ++i) out[i] = k * cov[i];
}

KdePackBytes kde_pack_bytes(int dtype, int dm, bool cond, int64_t n) {
    const size_t es = dtype_size(dtype);
    const int64_t ntiles = ceil_div(n, 16);
    if (use_f16x2(dtype))  // [ntiles][NB][64][8 f16]; the training norm lives inside the fragments
        return {(size_t)ntiles * f16x2_mfmas(dm) * 64 * 16, 64, cond ? (size_t)ntiles * 64 * 16 : 0};
    const int KS = (dm + 3) / 4;
    // norms [ntiles][16], then the weights 2^norm [ntiles][16] of the WMUL sweep
    // ... then one double per tile: sqrt(max -norm) of its rows (PackArgs::write_r)
    return {(size_t)ntiles * KS * 64 * es, (size_t)ntiles * 16 * es * 2 + (size_t)ntiles * 8, cond ? (size_t)ntiles * 64 * es : 0};
}

void kde_prepare(KdeModel& m, int dtype, int d, int64_t n, const double* bw, int kind, bool cond, const double* center) {
    if (!bw) throw invalid_error("pbn_kde_fit: null bandwidth");
    if (d <= 0) throw invalid_error("pbn_kde_fit: no variables");
    if (n <= 0) throw invalid_error("pbn_kde_fit: no training instances");
    if (cond && d < 2) cond = false;  // CKDE without evidence is a plain KDE (CKDE.hpp:232-241)
    const int dm = cond ? d - 1 : d;
    // up to 32 main dimensions: fp64 KS <= 8 MFMAs per tile pair, fp32 (f16x2 fragments, 6 slots per dimension + 3) <= 7; the
    // classic fp32 fragments (PBN_F32_F16X2=0, a measurement switch) stay at 16
    const int max_dm = (dtype == PBN_F64 || use_f16x2(dtype)) ? 32 : 16;
    m.dtype = dtype; m.widen = false; m.d = d; m.dm = dm; m.KS = use_f16x2(dtype) ? f16x2_mfmas(dm) : (dm + 3) / 4; m.cond = cond;
    // beyond the templated shapes: the generic runtime-sized pack / sweep in fp64 fragments (kde_kernels.hpp "wide"); a conditional
    // model of that size has no fused sweep - its owner evaluates joint - marginal (capi.hip: split handles; the score engine's terms
    // are plain anyway) and kde_pack_train refuses it
    m.wide = dm > max_dm;
    if (m.wide) { m.widen = dtype == PBN_F32; m.KS = (dm + 3) / 4; }
    m.perm.assign((size_t)d, 0);
    m.N = n; m.ntiles = ceil_div(n, 16);
    if (cond) {  // evidence first, variable last
        for (int i = 0; i < d - 1; ++i) m.perm[i] = i + 1;
        m.perm[d - 1] = 0;
    } else {
        for (int i = 0; i < d; ++i) m.perm[i] = i;
    }
    // whitening matrix W (row-major lower) = sqrt(log2 e) * L^-1, with L = chol(P H P^T)
    m.W.assign((size_t)d * d, 0.0);
    const double sc = std::sqrt(LOG2E);
    double logdet_half = 0.0, logdet_half_marg = 0.0;  // sum log L_ii
    if (kind == PBN_BW_DIAG) {
        for (int i = 0; i < d; ++i) {
            const double h = bw[m.perm[i]];
            if (!(h > 0.0) || !std::isfinite(h)) throw singular_error("ProductKDE: bandwidth must be positive");
            m.W[(size_t)i * d + i] = sc / std::sqrt(h);
            logdet_half += 0.5 * std::log(h);
            if (i < dm) logdet_half_marg += 0.5 * std::log(h);
        }
    } else {
        std::vector<double> H((size_t)d * d), L((size_t)d * d), Li((size_t)d * d);
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) H[i + (size_t)j * d] = bw[m.perm[i] + (size_t)m.perm[j] * d];
        if (!hm::cholesky(H.data(), d, L.data())) throw singular_error("KDE: bandwidth matrix is not positive-definite");
        hm::lower_inverse(L.data(), d, Li.data());
        for (int i = 0; i < d; ++i) {
            for (int j = 0; j <= i; ++j) m.W[(size_t)i * d + j] = sc * Li[i + (size_t)j * d];
            logdet_half += std::log(L[i + (size_t)i * d]);
            if (i < dm) logdet_half_marg += std::log(L[i + (size_t)i * d]);
        }
    }
    // KDE.hpp:476-477 / ProductKDE.hpp:188-189
    m.lognorm = -logdet_half - 0.5 * d * LOG_2PI - std::log((double)n);
    m.lognorm_marg = -logdet_half_marg - 0.5 * dm * LOG_2PI - std::log((double)n);
    m.mu.assign(d, 0.0);
    if (center)
        for (int i = 0; i < d; ++i) m.mu[i] = center[m.perm[i]];
}

static void fill_pack_common(pbn_ctx* ctx, PackArgs& pa, const pbn_table* t, const int* cols, const KdeModel& m) {
    if (m.d > PBN_MAX_D) throw invalid_error("internal: a wide model reached the fixed-size pack arguments");
    pa.base = t->data; pa.ld = t->ld; pa.d = m.d; pa.dm = m.dm; pa.KS = m.KS;
    pa.src_f32 = (m.widen && m.dtype == PBN_F32) ? 1 : 0;
    for (int i = 0; i < m.d; ++i) pa.cols[i] = cols[m.perm[i]];
    pa.rows = nullptr;
    pa.Wdev = nullptr;
    const std::vector<double>& W = m.wfull ? m.Wrot : m.W;
    pa.wfull = m.wfull ? 1 : 0;
    if (m.d <= PBN_W_INLINE_D) {
        for (int i = 0; i < m.d * m.d; ++i) pa.W[i] = W[i];
    } else {   // too large for the kernel arguments: through the context's (lane's) scratch, in stream order behind its last reader
        ctx->scratch_w.reserve((size_t)PBN_MAX_D * PBN_MAX_D);
        HIP_CHECK(hipMemcpyAsync(ctx->scratch_w.p, W.data(), (size_t)m.d * m.d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        pa.Wdev = ctx->scratch_w.p;
    }
    for (int i = 0; i < m.d; ++i) pa.mu[i] = m.mu[i];
}


double kde_max_norm2(pbn_ctx* ctx, const KdeModel& m, const pbn_table* t, const int* cols, int64_t row0, int64_t n0, int64_t row1,
                     const int32_t* dev_rows) {
    PackArgs pa{};
    fill_pack_common(ctx, pa, t, cols, m);
    pa.rows = dev_rows;
    pa.row0 = row0; pa.n0 = n0; pa.row1 = row1; pa.n = m.N; pa.ntiles = m.ntiles;
    ctx->scratch_misc.reserve(sizeof(double));
    double* slot = (double*)ctx->scratch_misc.p;
    HIP_CHECK(hipMemsetAsync(slot, 0, sizeof(double), ctx->stream));
    launch_max_norm2(pa, t->dtype, slot, ctx->stream);
    double v = 0.0;
    HIP_CHECK(hipMemcpyAsync(&v, slot, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return v;
}

bool kde_wants_widening(double max_norm2, int dm) {
    // (read per call: tests move it inside one process; inf switches the widening off)
    // four-product fragments: the f32 accumulation of the Gram form, 2^-24 |z|^2 on an exponent, against 5e-4 (the reference tests' fp32 tolerance per
    // logl); three-product fragments (8, 9, 16...20, ... dimensions): the dropped products a2 b2, <= 2^-22 |z|^2 in the worst alignment of the
    // rounding residuals and a tenth of that typically, against twice that - both limits scale with PBN_F32_WIDEN_AT
    const double at = knob_double("PBN_F32_WIDEN_AT", 5e-4);
    if (f16x2_spd(dm) == 4) return !(max_norm2 * 5.9604644775390625e-08 <= at);
    return !(max_norm2 * 2.384185791015625e-07 <= 2.0 * at);
}

void kde_widen(KdeModel& m) {
    if (m.dtype != PBN_F32 || m.widen) return;
    m.widen = true;
    m.KS = (m.dm + 3) / 4;   // classic fp64 fragments: 4 coordinates per MFMA
}

// Morton order of the logical rows described by `pa` (already filled): whitened rows -> keys -> stable sort.  Returns the
// carved buffers inside `arena`.
struct PruneSide {
    double* zrow;        // [n][zd] in logical order
    uint32_t* keys;      // [n] sorted
    int32_t* perm;       // [n] sorted position -> logical row
    char* rest;          // first free byte behind them (256-aligned)
    uint32_t* keys_unsorted;   // [n] in logical order (what sort_keys read: pbn_debug_prune_stages)
};
static PruneSide prune_sort_side(pbn_ctx* ctx, dev_buf<char>& arena, const PackArgs& pa, int dtype, int zd, int kd, size_t extra_bytes) {
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t n = (size_t)pa.n;
    const size_t zb = al(n * zd * sizeof(double)), kb = al(n * sizeof(uint32_t)), ib = al(n * sizeof(int32_t));
    arena.reserve(zb + 2 * kb + 2 * ib + extra_bytes + 256);
    char* p = arena.p;
    PruneSide s{};
    s.zrow = (double*)p; p += zb;
    uint32_t* keys_unsorted = (uint32_t*)p; p += kb;
    s.keys = (uint32_t*)p; p += kb;
    int32_t* iota = (int32_t*)p; p += ib;
    s.perm = (int32_t*)p; p += ib;
    s.rest = p;
    s.keys_unsorted = keys_unsorted;
    launch_prune_keys(pa, dtype, zd, kd, s.zrow, keys_unsorted, iota, ctx->stream);
    sort_keys(ctx->scratch_sort, keys_unsorted, s.keys, iota, s.perm, pa.n, prune_key_bits(kd) * kd, ctx->stream);
    return s;
}

// pbn_debug_prune_stages (test aid, not part of the C ABI header; the codes are at its definition below): armed, every pruned fit
// (kde_pack_train) and every pruned evaluation (kde_eval_enqueue) copies what its prepass kernels left to the host behind a stream
// synchronisation; the last PBN_STAGES_KEEP of either kind are kept.  Unarmed it costs one atomic load per fit or evaluation.
#define PBN_STAGES_KEEP 4
static std::atomic<bool> g_stages_capture{false};
static std::mutex g_stages_mu;
struct StageFit {
    long long head[14] = {};           // N, d, dm, zdims, pdims, kdims, nsub, ntiles, wfull, cond, fdtype, src_f32, key bits, Hilbert order at 3 / 4 key dimensions
    double cell = 0.0;                 // prune_key_cell(kdims)
    std::vector<double> W, mu;         // what the kernels were handed: [d][d] row-major (Wrot where rotated), [d]
    std::vector<double> zrow, zsorted, box;
    std::vector<uint32_t> keys_unsorted, keys;
    std::vector<int32_t> perm;
};
struct StageEval {
    long long head[21] = {};           // n, nqtiles, nsplit, tps, batches_per_split, sum_only, bboxes, qlb, window, subsample, P, which, N, d, cond, fdtype, partial rows, qg, num_cus, tile bytes, KS
    double num[2] = {0.0, 0.0};        // prune_margin, log2(nsub)
    std::vector<double> zrow, subpart, qbox, qthr, qlb, bbox, part;
    std::vector<uint32_t> keys_unsorted, keys;
    std::vector<int32_t> qperm;
    std::vector<int64_t> qtpos;
};
static std::vector<StageFit> g_stage_fits;
static std::vector<StageEval> g_stage_evals;
template <typename T>
static void stage_fetch(std::vector<T>& dst, const void* src, size_t count, hipStream_t st) {
    dst.assign(count, T());
    if (count && src) HIP_CHECK(hipMemcpyAsync(dst.data(), src, count * sizeof(T), hipMemcpyDeviceToHost, st));
}
template <typename R>
static void stage_keep(std::vector<R>& all, R&& r) {
    std::lock_guard<std::mutex> lk(g_stages_mu);
    if (all.size() >= PBN_STAGES_KEEP) all.erase(all.begin());
    all.push_back(std::move(r));
}

// pbn_debug_f16_stages (test aid, not part of the C ABI header; the codes are at its definition below): armed, every evaluation of
// kde_eval_enqueue whose fragments are f16x2 (use_f16x2(fdt)), pruned or not, copies its fragments and its partial sums - before and after
// kde_far_fix_kernel - to the host behind a stream synchronisation; the last PBN_F16_STAGES_KEEP are kept.  Unarmed it costs one atomic load
// per evaluation; no kernel and no launch argument depends on it.
#define PBN_F16_STAGES_KEEP 4
static std::atomic<bool> g_f16_capture{false};
static std::mutex g_f16_mu;
struct F16Stage {
    long long head[19] = {};           // see pbn_debug_f16_stages
    double num[3] = {0.0, 0.0, 0.0};   // SweepArgs::prune_margin, the model's lognorm and lognorm_marg (FinishArgs)
    std::vector<double> W, mu;         // what the pack kernels were handed: [d][d] row-major, [d]
    std::vector<int32_t> cols, qperm;  // the table's columns in the order of W's; sorted position -> query row (pruned evaluations)
    std::vector<uint16_t> apack, axpack, bpack, bxpack;   // f16 bit patterns
    std::vector<float> npack, xnorm;
    std::vector<unsigned char> far;
    std::vector<double> part_sweep, part_fixed;
};
static std::vector<F16Stage> g_f16_stages;

// Up to 6 marginal dimensions (PBN_PRUNE_MAX_DIMS overrides): at 1e6 x 1e5 rows (tools/prune_dims67.py, boxes over 4 dimensions)
// d = 6 gains 10 % in fp64 and 9-13 % in fp32 on correlated and on independent normal data and is even on heavy-tailed data;
// d = 7 is even at best (heavy-tailed: +3...5 %), d = 8 loses 10 %.
bool kde_prune_applies(int dtype, int dm, int64_t n) {
    const int max_dims = PBN_TUNE(PRUNE_MAX_DIMS, 6);
    return knob_int("PBN_SWEEP_PRUNE", 1) && (dtype == PBN_F64 || use_f16x2(dtype)) && dm <= max_dims && n >= knob_int("PBN_PRUNE_MIN_ROWS", 32768);
}

// d = 7 and 8 (fp64 tables, plain models): the boxes cover ALL whitened dimensions, rotated to the principal axes of the training rows first,
// and the rows are sorted on the widest four of them (principal_rotation).  Boxes over 4 raw axes lost 10 % at d = 8 (tools/prune_dims67.py);
// with the rotation C2's sum-only sweep visits 0.525 of its (tile, group) blocks, 40.7 -> 27.2 ms (tools/prune_d8_estimate.py, profiles/r7/).  Per-row logl
// sweeps of these models stay unpruned (kde_eval_enqueue).  PBN_SWEEP_PRUNE=0 turns it off with the rest.
bool kde_prune_rotates(const KdeModel& m) {
    return PBN_TUNE(PRUNE_ROTATE, 1) && knob_int("PBN_SWEEP_PRUNE", 1) && m.dtype == PBN_F64 && !m.widen && !m.cond && !m.wide &&
           (m.dm == 7 || m.dm == 8) && m.N >= knob_int("PBN_PRUNE_MIN_ROWS", 32768);
}

// Eigenvectors of a symmetric n x n matrix (column-major) by cyclic Jacobi rotations: a becomes diagonal, V (column-major) holds the vectors
static void sym_eigen(std::vector<double>& a, int n, std::vector<double>& V) {
    V.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) V[i + (size_t)i * n] = 1.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) (i == j ? diag : off) += a[i + (size_t)j * n] * a[i + (size_t)j * n];
        if (off <= 1e-30 * (diag > 0 ? diag : 1.0)) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = a[p + (size_t)q * n];
                if (apq == 0.0) continue;
                const double theta = (a[q + (size_t)q * n] - a[p + (size_t)p * n]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = a[k + (size_t)p * n], akq = a[k + (size_t)q * n];
                    a[k + (size_t)p * n] = c * akp - s * akq;
                    a[k + (size_t)q * n] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = a[p + (size_t)k * n], aqk = a[q + (size_t)k * n];
                    a[p + (size_t)k * n] = c * apk - s * aqk;
                    a[q + (size_t)k * n] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k + (size_t)p * n], vkq = V[k + (size_t)q * n];
                    V[k + (size_t)p * n] = c * vkp - s * vkq;
                    V[k + (size_t)q * n] = s * vkp + c * vkq;
                }
            }
    }
}

// Rotation of the whitened training rows to their principal axes, widest first: Wrot = R W with R's rows the eigenvectors of the rows'
// covariance (O(d^3) on the host, from one copy of the whitened rows).  Orthonormal: every distance, norm and term is the same in exact
// arithmetic - only the fp64 rounding of the packed coordinates moves.  Rows with a NaN or an infinity are left out of the covariance.
static void principal_rotation(pbn_ctx* ctx, KdeModel& m, const PackArgs& pa) {
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const int d = m.d;
    const size_t n = (size_t)pa.n, zb = al(n * d * sizeof(double)), kb = al(n * sizeof(uint32_t));
    ctx->scratch_prune.reserve(zb + 2 * kb);
    double* z = (double*)ctx->scratch_prune.p;
    launch_prune_keys(pa, m.fdtype(), d, 1, z, (uint32_t*)(ctx->scratch_prune.p + zb), (int32_t*)(ctx->scratch_prune.p + zb + kb), ctx->stream);
    std::vector<double> h(n * d);
    HIP_CHECK(hipMemcpyAsync(h.data(), z, n * d * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(hipStreamSynchronize(ctx->stream));
    std::vector<double> mean(d, 0.0), cov((size_t)d * d, 0.0);
    size_t cnt = 0;
    for (size_t r = 0; r < n; ++r) {
        const double* zr = h.data() + r * d;
        bool ok = true;
        for (int i = 0; i < d; ++i) ok = ok && std::isfinite(zr[i]);
        if (!ok) continue;
        ++cnt;
        for (int i = 0; i < d; ++i) mean[i] += zr[i];
    }
    m.Wrot = m.W;
    m.wfull = true;
    if (cnt < 2) return;
    for (int i = 0; i < d; ++i) mean[i] /= (double)cnt;
    for (size_t r = 0; r < n; ++r) {
        const double* zr = h.data() + r * d;
        bool ok = true;
        for (int i = 0; i < d; ++i) ok = ok && std::isfinite(zr[i]);
        if (!ok) continue;
        for (int j = 0; j < d; ++j)
            for (int i = j; i < d; ++i) cov[i + (size_t)j * d] += (zr[i] - mean[i]) * (zr[j] - mean[j]);
    }
    for (int j = 0; j < d; ++j)
        for (int i = j; i < d; ++i) cov[j + (size_t)i * d] = cov[i + (size_t)j * d];
    std::vector<double> V;
    sym_eigen(cov, d, V);
    std::vector<int> ord(d);
    for (int i = 0; i < d; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return cov[x + (size_t)x * d] > cov[y + (size_t)y * d]; });
    for (int i = 0; i < d; ++i)        // row i of R = eigenvector ord[i]
        for (int j = 0; j < d; ++j) {
            double w = 0.0;
            for (int k = 0; k < d; ++k) w += V[k + (size_t)ord[i] * d] * m.W[(size_t)k * d + j];
            m.Wrot[(size_t)i * d + j] = w;
        }
}

// bytes of the subsample packs (kde_pack_bytes of nsub rows, each part 256-aligned)
struct SubBytes { size_t a, n, x, total; };
static SubBytes sub_bytes(const KdeModel& m, int64_t nsub) {
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const KdePackBytes pb = kde_pack_bytes(m.fdtype(), m.dm, m.cond, nsub);
    SubBytes b{al(pb.apack), al(pb.nxpack), al(pb.axpack), 0};
    b.total = b.a + b.n + b.x;
    return b;
}

// wide models: columns, centring offsets and whitening matrix through the context's (lane's) scratch, in stream order
void kde_wide_pack_args(pbn_ctx* ctx, WidePackArgs& wa, const pbn_table* t, const int* cols_whitened, int d_, int dm, const double* W, int ldw,
                        const double* mu, const double* wu) {
    const size_t d = (size_t)d_, wn = (size_t)d_ * (size_t)ldw;
    ctx->scratch_w.reserve(wn + 2 * d + d / 2 + 8);   // doubles: W | mu | wu | cols (ints)
    double* Wd = ctx->scratch_w.p;
    double* mud = Wd + wn;
    double* wud = mud + d;
    int* colsd = (int*)(wud + d);
    HIP_CHECK(hipMemcpyAsync(Wd, W, wn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));   // pageable sources: staged before the call returns
    HIP_CHECK(hipMemcpyAsync(mud, mu, d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (wu) HIP_CHECK(hipMemcpyAsync(wud, wu, d * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(colsd, cols_whitened, d * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    wa.base = t->data; wa.ld = t->ld; wa.cols = colsd; wa.mu = mud; wa.W = Wd; wa.wu = wu ? wud : nullptr;
    wa.d = d_; wa.dm = dm; wa.ldw = ldw; wa.KS = (dm + 3) / 4; wa.src_f32 = t->dtype == PBN_F32 ? 1 : 0;
}

static void fill_wide_pack(pbn_ctx* ctx, WidePackArgs& wa, const pbn_table* t, const int* cols, const KdeModel& m) {
    std::vector<int> hc((size_t)m.d);
    for (int i = 0; i < m.d; ++i) hc[i] = cols[m.perm[i]];
    kde_wide_pack_args(ctx, wa, t, hc.data(), m.d, m.d, m.W.data(), m.d, m.mu.data(), nullptr);
    wa.KS = m.KS;
}

void kde_pack_train(pbn_ctx* ctx, KdeModel& m, const pbn_table* t, const int* cols, int64_t row0, int64_t n0,
                    int64_t row1, const int32_t* dev_rows, bool prune, double* dev_max_norm2) {
    if (m.wide) {
        if (m.cond) throw invalid_error("KDE: a conditional model of more than 32 evidence variables is evaluated as joint - marginal");
        WidePackArgs wa{};
        fill_wide_pack(ctx, wa, t, cols, m);
        wa.rows = dev_rows; wa.row0 = row0; wa.n0 = n0; wa.row1 = row1; wa.n = m.N; wa.ntiles = m.ntiles; wa.is_query = 0;
        wa.pack = (double*)m.Apack; wa.npack = (double*)m.nxpack;
        m.prune = false;
        KernelTimer kt(ctx, PBN_K_PACK);
        launch_pack_wide(wa, ctx->stream);
        return;
    }
    PackArgs pa{};
    m.wfull = false;   // (set again below for a rotated model: the rotation is the training rows')
    fill_pack_common(ctx, pa, t, cols, m);
    pa.rows = dev_rows;
    pa.row0 = row0; pa.n0 = n0; pa.row1 = row1; pa.n = m.N; pa.ntiles = m.ntiles;
    pa.is_query = 0;
    if (dev_max_norm2 && m.dtype == PBN_F32 && !m.widen) launch_max_norm2(pa, t->dtype, dev_max_norm2, ctx->stream);
    m.prune = false;
    m.scr = nullptr;
    m.far_plain = nullptr;
    m.far_pack = nullptr;
    const bool rot = prune && kde_prune_rotates(m);
    if (rot || (prune && kde_prune_applies(m.fdtype(), m.dm, m.N))) {
        auto al = [](size_t x) { return (x + 255) / 256 * 256; };
        m.zdims = m.d;
        m.pdims = std::min(m.dm, std::min(PBN_TUNE(PRUNE_BOX_DIMS, 4), PBN_PRUNE_PD));   // dimensions of the Morton keys and the boxes (<= PBN_PRUNE_PD)
        m.kdims = m.pdims;
        if (rot) {   // boxes over all (rotated) dimensions, keys on the widest four
            principal_rotation(ctx, m, pa);
            for (int i = 0; i < m.d * m.d; ++i) pa.W[i] = m.Wrot[i];
            pa.wfull = 1;
            m.pdims = m.dm;
            m.kdims = 4;
        }
        const size_t box_b = al((size_t)m.ntiles * 2 * m.pdims * sizeof(double)), zs_b = al((size_t)m.N * m.zdims * sizeof(double));
        // more dimensions than the keys cover: a stratified subsample (every N / nsub-th row of the sorted order, <= 4096
        // rows, <= 1/64 of the set) is packed as well; the queries are swept against it first (kde_eval_enqueue)
        m.nsub = 0;
        if (m.d > m.pdims && PBN_TUNE(PRUNE_SUBSAMPLE, 1)) m.nsub = std::min<int64_t>(4096, m.N / 64) / 16 * 16;
        const SubBytes sb = sub_bytes(m, m.nsub);
        const PruneSide s = prune_sort_side(ctx, ctx->scratch_prune, pa, m.fdtype(), m.zdims, m.kdims, box_b + zs_b + (m.nsub ? sb.total : 0));
        double* box = (double*)s.rest;
        double* zsorted = (double*)(s.rest + box_b);
        launch_tile_boxes(s.zrow, s.perm, m.N, m.zdims, m.pdims, box, zsorted, ctx->stream);
        if (g_stages_capture.load()) {   // pbn_debug_prune_stages: before scratch_prune is used again
            StageFit f;
            const long long head[14] = {(long long)m.N, m.d, m.dm, m.zdims, m.pdims, m.kdims, (long long)m.nsub, (long long)m.ntiles, m.wfull ? 1 : 0, m.cond ? 1 : 0,
                                        m.fdtype(), pa.src_f32, prune_key_bits(m.kdims), PBN_TUNE(PRUNE_HILBERT_ND, 1)};
            for (int i = 0; i < 14; ++i) f.head[i] = head[i];
            f.cell = prune_key_cell(m.kdims);
            f.W = m.wfull ? m.Wrot : m.W;
            f.mu = m.mu;
            const size_t N = (size_t)m.N;
            stage_fetch(f.zrow, s.zrow, N * m.zdims, ctx->stream);
            stage_fetch(f.keys_unsorted, s.keys_unsorted, N, ctx->stream);
            stage_fetch(f.keys, s.keys, N, ctx->stream);
            stage_fetch(f.perm, s.perm, N, ctx->stream);
            stage_fetch(f.zsorted, zsorted, N * m.zdims, ctx->stream);
            stage_fetch(f.box, box, (size_t)m.ntiles * 2 * m.pdims, ctx->stream);
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            stage_keep(g_stage_fits, std::move(f));
        }
        pa.perm = s.perm;
        m.prune = true;
        m.tile_box = box; m.zsorted = zsorted; m.keys_sorted = s.keys;
        if (m.nsub) {
            char* sp = s.rest + box_b + zs_b;
            m.ntiles_sub = m.nsub / 16;
            m.Asub = sp; m.nxsub = sp + sb.a; m.Axsub = m.cond ? sp + sb.a + sb.n : nullptr;
        }
    }
    pa.fold_norm = 1;   // harmless for consumers whose query pack leaves the slot 0
    pa.write_w = !use_f16x2(m.fdtype());
    pa.write_r = pa.write_w && m.fdtype() == PBN_F64;
    m.tile_r = pa.write_r != 0;
    pa.pack = m.Apack; pa.npack = m.nxpack; pa.xpack = m.cond ? m.Axpack : nullptr;
    KernelTimer kt(ctx, PBN_K_PACK);
    launch_pack(pa, m.fdtype(), ctx->stream);
    if (m.prune && m.nsub) {
        PackArgs ps = pa;
        ps.perm_stride = m.N / m.nsub;
        ps.n = m.nsub; ps.ntiles = m.ntiles_sub;
        ps.pack = m.Asub; ps.npack = m.nxsub; ps.xpack = m.Axsub;
        launch_pack(ps, m.fdtype(), ctx->stream);
    }
}

// A fitted handle outlives the context's arenas: move the pruning tables of a freshly packed model into `store`.
void kde_prune_persist(pbn_ctx* ctx, KdeModel& m, dev_buf<char>& store) {
    if (!m.prune) return;
    auto al = [](size_t x) { return (x + 255) / 256 * 256; };
    const size_t box_b = al((size_t)m.ntiles * 2 * m.pdims * sizeof(double)), zs_b = al((size_t)m.N * m.zdims * sizeof(double)),
                 key_b = al((size_t)m.N * sizeof(uint32_t));
    const SubBytes sb = sub_bytes(m, m.nsub);
    // the operands of the d = 8 screen (PBN_D8_SCREEN, read here and at every evaluation: 0 at either keeps today's path)
    const bool screen = m.wfull && !m.cond && m.dm == 8 && m.zdims == 8 && m.pdims == PBN_PRUNE_PD && m.fdtype() == PBN_F64 && knob_int("PBN_D8_SCREEN", 1) != 0;
    const size_t sub_b = m.nsub ? al(sb.total) : 0, scr_b = screen ? al((size_t)m.ntiles * 16 * 32) : 0;
    const size_t plain_b = screen ? al((size_t)(ceil_div(m.ntiles, 64) + 1) * sizeof(unsigned long long)) : 0;   // the far pass's plain bits
    const size_t fpack_b = screen ? al((size_t)m.ntiles * 768) : 0;   // ... and its fp32 fragments (launch_far_pack)
    store.alloc(box_b + zs_b + key_b + sub_b + scr_b + plain_b + fpack_b);
    HIP_CHECK(hipMemcpyAsync(store.p, m.tile_box, box_b, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(store.p + box_b, m.zsorted, (size_t)m.N * m.zdims * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIP_CHECK(hipMemcpyAsync(store.p + box_b + zs_b, m.keys_sorted, (size_t)m.N * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    m.tile_box = (const double*)store.p;
    m.zsorted = (const double*)(store.p + box_b);
    m.keys_sorted = (const uint32_t*)(store.p + box_b + zs_b);
    if (m.nsub) {   // the three subsample packs are contiguous in the arena (kde_pack_train)
        char* sp = store.p + box_b + zs_b + key_b;
        HIP_CHECK(hipMemcpyAsync(sp, m.Asub, sb.total, hipMemcpyDeviceToDevice, ctx->stream));
        m.Asub = sp; m.nxsub = sp + sb.a; m.Axsub = m.cond ? sp + sb.a + sb.n : nullptr;
    }
    m.scr = nullptr;
    if (screen) {
        char* sp = store.p + box_b + zs_b + key_b + sub_b;
        KernelTimer kt(ctx, PBN_K_PACK);
        launch_screen_pack(m.zsorted, nullptr, m.N, m.ntiles, false, sp, ctx->stream);
        m.scr = sp;
        launch_far_plain((const double*)m.nxpack, m.ntiles, (unsigned long long*)(sp + scr_b), ctx->stream);
        m.far_plain = (const unsigned long long*)(sp + scr_b);
        launch_far_pack(m.Apack, m.nxpack, m.ntiles, sp + scr_b + plain_b, ctx->stream);
        m.far_pack = sp + scr_b + plain_b;
    }
}

// pbn_debug_d8_masks (test aid, not part of the C ABI header): armed, the next screened d = 8 sweep also writes its box masks, and both mask
// arrays are copied to the host behind it, with the launch's shape and the tables the masks were taken from.
// Thresholds: qrow is what every column was compared against, its query's bound less the margin (the group's, sixteen times over, where the
// launch had no per-query bounds: PBN_D8_SCREEN_ROWTHR=0, no window pass).  qthr, one number per query tile, is the LARGEST of the tile's
// sixteen: a block all of whose columns lie below their own thresholds holds no pair at or above it - the only per-tile number of which
// that is true - and where the launch compared against the group's bound it is that bound, as before.
// Partial rows: what kde_finish_kernel is about to merge, copied behind both sweeps - per (row, sorted query) a pair (o, s) that stands for
// s 2^o; rows 0 .. nsplit - 1 the fp64 sweep's, rows nsplit .. 2 nsplit - 1 the far pass's (absent where the launch ran none).
static std::atomic<bool> g_masks_capture{false};
static std::mutex g_masks_mu;
struct MaskDump {
    std::vector<unsigned long long> box, live, far;   // far: empty where the launch wrote no far words
    std::vector<double> qthr, zq, zt;  // per query tile: see above; the sorted queries' / training rows' whitened rows [n][8]
    std::vector<double> qrow;          // per sorted query, padding columns included [nqtiles * 16]
    std::vector<double> part;          // the launch's partial rows [rows][nqtiles * 16][2]: the fp64 sweep's nsplit, then the far pass's nsplit where it ran
    long long dims[6] = {0, 0, 0, 0, 0, 0};   // sweep waves, splits, batches per split, tiles per split, training tiles, queries
};
static MaskDump g_masks;

// pbn_debug_sum_window (test aid, not part of the C ABI header): capture the window bounds (query_window_kernel) of the sum-only evaluations
// that follow; returns how many the last one produced and copies up to `cap` of them - log2 units, the table's row order, -inf = none
static std::atomic<bool> g_window_capture{false};
static std::mutex g_window_mu;
static std::vector<double> g_window_lb;
static std::vector<int64_t> g_window_pos;   // pbn_debug_window_pos: per query the centre of its tile's window, a position in the sorted training order

// The front stage of a pruned handle evaluation (pbn_ctx::front): while it is open, ctx->stream and the arenas of the query side are front lane
// k's, so the routines in between keep saying ctx->stream / ctx->scratch_*.
//   open     lane k waits for `released` of its last use, and for what it has to see of ctx->stream: where the evaluation follows another front-lane
//            evaluation with no entry point of the context in between (pbn_ctx::front_exit), that is the other evaluation's query side alone - it saw
//            everything enqueued before it, and nothing it reads was enqueued since -, so the lane waits for that lane's `ready` and runs beside the
//            sweep still on ctx->stream; in every other case (another entry point in between on any handle, a nested entry point, a throw) it waits
//            for everything enqueued on ctx->stream so far
//   join     `ready` on the lane, the lane's resources back, ctx->stream waits for `ready`
//   release  `released` on ctx->stream behind the rest of the evaluation; the count of entry points is noted for the next evaluation
// A throw in between leaves the join recorded (the destructor) and the next evaluation waits in full.
static std::atomic<unsigned long long> g_front_evals{0}, g_front_chained{0};   // pbn_debug_front_lanes
struct FrontStage {
    pbn_ctx* ctx; int k = -1; bool open = false;
    FrontStage(pbn_ctx* c, bool on) : ctx(c) {
        if (!on) return;
        ctx->ensure_front();
        k = ctx->front_next;
        ctx->front_next ^= 1;
        pbn_ctx::Front& f = ctx->front[k];
        if (f.was_released) HIP_CHECK(hipStreamWaitEvent(f.stream, f.released, 0));
        const entry_mutex& mu = ctx->mu;
        const bool chained = ctx->front_exit_valid && ctx->front_last >= 0 && mu.depth == 1 && (mu.entries == ctx->front_exit || mu.entries == ctx->front_exit + 1);
        ctx->front_exit_valid = false;
        if (chained) {
            if (ctx->front_last != k) HIP_CHECK(hipStreamWaitEvent(f.stream, ctx->front[ctx->front_last].ready, 0));
        } else {
            HIP_CHECK(hipEventRecord(ctx->front_fence, ctx->stream));
            HIP_CHECK(hipStreamWaitEvent(f.stream, ctx->front_fence, 0));
        }
        ctx->swap_front(k);
        open = true;
        g_front_evals.fetch_add(1);
        if (chained) g_front_chained.fetch_add(1);
    }
    void join() {
        if (!open) return;
        open = false;
        ctx->swap_front(k);
        pbn_ctx::Front& f = ctx->front[k];
        HIP_CHECK(hipEventRecord(f.ready, f.stream));
        HIP_CHECK(hipStreamWaitEvent(ctx->stream, f.ready, 0));
        ctx->front_last = k;
    }
    void release() {
        if (k < 0) return;
        pbn_ctx::Front& f = ctx->front[k];
        HIP_CHECK(hipEventRecord(f.released, ctx->stream));
        f.was_released = true;
        ctx->front_exit = ctx->mu.entries;
        ctx->front_exit_valid = ctx->mu.depth == 1;
    }
    ~FrontStage() {
        if (!open) return;
        ctx->swap_front(k);
        pbn_ctx::Front& f = ctx->front[k];
        if (hipEventRecord(f.ready, f.stream) == hipSuccess) { (void)hipStreamWaitEvent(ctx->stream, f.ready, 0); ctx->front_last = k; }
        else (void)hipStreamSynchronize(f.stream);
    }
    FrontStage(const FrontStage&) = delete;
    FrontStage& operator=(const FrontStage&) = delete;
};

void kde_eval_enqueue(pbn_ctx* ctx, const KdeModel& m, const pbn_table* test, const int* cols, int64_t row0, int64_t n,
                      double* dev_logl, double* dev_sum, const int32_t* dev_rows, double* dev_sum_marg, bool precise, bool front_lanes) {
    check_cols(test, cols, m.d, "pbn_kde_logl");
    const bool sum_only = dev_logl == nullptr && !precise;   // only sums leave this call, at the sum-only error budget
    if (!dev_rows) check_range(test, row0, n, "pbn_kde_logl");
    if (test->dtype != m.dtype) throw invalid_error("Data type of training and test datasets is different.");
    const int fdt = m.fdtype();   // type of the fragments and of the sweep (double for a widened fp32 model)
    if (m.wide) {   // more than 32 dimensions: generic pack + sweep, plain, fp64 fragments
        if (m.cond) throw invalid_error("KDE: a conditional model of more than 32 evidence variables is evaluated as joint - marginal");
        HIP_CHECK(hipSetDevice(ctx->device));
        if (n == 0) {
            if (dev_sum) HIP_CHECK(hipMemsetAsync(dev_sum, 0, sizeof(double), ctx->stream));
            return;
        }
        const int64_t nqt = ceil_div(n, 16);
        const size_t bp = (size_t)nqt * m.KS * 64 * sizeof(double), nyb = (size_t)nqt * 16 * sizeof(double);
        ctx->scratch_q.reserve(bp + nyb + 256);
        WidePackArgs wq{};
        fill_wide_pack(ctx, wq, test, cols, m);
        wq.rows = dev_rows; wq.row0 = row0; wq.n0 = n; wq.row1 = 0; wq.n = n; wq.ntiles = nqt; wq.is_query = 1;
        wq.pack = (double*)ctx->scratch_q.p; wq.npack = (double*)(ctx->scratch_q.p + bp);
        { KernelTimer kt(ctx, PBN_K_PACK); launch_pack_wide(wq, ctx->stream); }
        int64_t ns = std::max<int64_t>(1, ceil_div((int64_t)ctx->num_cus * 8, ceil_div(nqt, 4)));
        ns = std::min<int64_t>(ns, std::max<int64_t>(1, m.ntiles / 16));
        ns = std::min<int64_t>(ns, 1024);
        const int64_t tpsw = ceil_div(m.ntiles, ns);
        ns = ceil_div(m.ntiles, tpsw);
        ctx->scratch_part.reserve((size_t)ns * nqt * 16 * 2 * sizeof(double));
        SweepArgs sw{};
        sw.Apack = m.Apack; sw.nxpack = m.nxpack; sw.Bpack = wq.pack; sw.nypack = wq.npack;
        sw.ntiles = m.ntiles; sw.nqtiles = nqt; sw.tiles_per_split = tpsw; sw.part = (double*)ctx->scratch_part.p;
        { KernelTimer kt(ctx, PBN_K_SWEEP); launch_sweep_wide(sw, m.KS, (int)ns, ctx->stream); }
        const int64_t nb = ceil_div(n, 256);
        ctx->scratch_misc.reserve((size_t)nb * 2 * sizeof(double));
        FinishArgs fw{};
        fw.part = sw.part; fw.nsplit = (int)ns; fw.nqtiles = nqt; fw.nq = n;
        fw.lognorm = m.lognorm; fw.lognorm_marg = m.lognorm_marg;
        fw.logl = dev_logl; fw.scatter = nullptr; fw.block_sums = dev_sum ? (double*)ctx->scratch_misc.p : nullptr;
        { KernelTimer kt(ctx, PBN_K_FINISH); launch_finish(fw, false, dev_sum, ctx->stream, nullptr); }
        return;
    }
    if (test->ctx->device != ctx->device) throw invalid_error("pbn_kde_logl: test table lives on another device");
    HIP_CHECK(hipSetDevice(ctx->device));
    if (n == 0) {
        if (dev_sum) HIP_CHECK(hipMemsetAsync(dev_sum, 0, sizeof(double), ctx->stream));
        if (dev_sum_marg) HIP_CHECK(hipMemsetAsync(dev_sum_marg, 0, sizeof(double), ctx->stream));
        return;
    }
    const size_t es = dtype_size(fdt);
    const int64_t nqtiles = ceil_div(n, 16);
    // a rotated (d = 7, 8) model prunes its sum-only sweeps only; per-row logl outputs take the plain sweep over the same (sorted) pack
    const bool prune = m.prune && (sum_only || !m.wfull);
    // the capture aids synchronise and read scratch: read once, and no front lane while one is armed
    const bool cap_stages = g_stages_capture.load(), cap_window = g_window_capture.load(), cap_masks = g_masks_capture.load();
    const bool cap_f16 = g_f16_capture.load();
    // The query side on a front lane (FrontStage above; the handle entry points of capi.hip ask for it, the score engine has lanes of its own): pruned
    // evaluations only.  PBN_KDE_PIPELINE=0 (read per evaluation): everything on ctx->stream, as before the lanes.
    FrontStage front(ctx, front_lanes && prune && m.d <= PBN_W_INLINE_D && !cap_stages && !cap_window && !cap_masks && !cap_f16 && knob_int("PBN_KDE_PIPELINE", 1) != 0);
    // query fragments in scratch: Bpack | nypack | Bxpack
    const bool b3 = use_f16x2(fdt);
    const size_t bpack_b = b3 ? (size_t)nqtiles * m.KS * 64 * 16 : (size_t)nqtiles * m.KS * 64 * es,
                 ny_b = (size_t)nqtiles * 16 * es,
                 bx_b = m.cond ? (b3 ? (size_t)nqtiles * 64 * 16 : (size_t)nqtiles * 64 * es) : 0,
                 xn_b = (m.cond && b3) ? (size_t)nqtiles * 16 * 4 : 0,
                 ff_b = b3 ? ((size_t)nqtiles * 16 + 255) / 256 * 256 : 0;   // f16x2 fragments: one flag per query row (beyond the f16 range)
    ctx->scratch_q.reserve(bpack_b + ny_b + bx_b + xn_b + ff_b + 512);
    char* q = ctx->scratch_q.p;
    PackArgs pa{};
    fill_pack_common(ctx, pa, test, cols, m);
    pa.rows = dev_rows;
    pa.row0 = row0; pa.n0 = n; pa.row1 = 0; pa.n = n; pa.ntiles = nqtiles;
    pa.is_query = 1;
    const bool fold = sweep_folds_norm(fdt, m.cond, m.KS, m.dm);
    pa.fold_norm = fold ? 1 : 0;
    const double* qbox = nullptr;
    const double* qthr = nullptr;
    const double* qlb = nullptr;
    const int32_t* qperm = nullptr;
    PruneSide qs{};
    // pruned sum-only sweeps of a rotated model tighten the prepass bounds with the exact terms of a window of training tiles (query_window_kernel): W tiles on either
    // side, PBN_SUM_WINDOW (0 = the prepass bounds alone).  W = 256: C2 visits 0.525 -> 0.441 of its blocks, 27.3 -> 24.3 ms;
    // 64 is even within noise, 1024 costs 3.2 ms of window for 0.435 (profiles/r8/)
    const int window = (prune && m.wfull && m.KS == 2) ? std::max(0, knob_int("PBN_SUM_WINDOW", 256)) : 0;
    const bool wdbg = window > 0 && cap_window;
    const bool sdbg = prune && cap_stages;   // pbn_debug_prune_stages
    StageEval sev;
    int64_t* qtpos = nullptr;
    double* qdbg = nullptr;
    double* qrow = nullptr;   // per query: its own sum bound where above its tile's (query_window_kernel), for the d = 8 screen's columns
    double* qwpart = nullptr;   // the partial sums of the window pass's parts
    const int wparts = window ? window_parts(nqtiles, ctx->num_cus) : 0;
    if (prune) {
        auto al = [](size_t x) { return (x + 255) / 256 * 256; };
        const size_t qbox_b = al((size_t)nqtiles * 2 * m.pdims * sizeof(double)), qthr_b = al((size_t)nqtiles * sizeof(double));
        const size_t qlb_b = al((size_t)nqtiles * 16 * sizeof(double));
        const size_t qtpos_b = (window || sdbg) ? al((size_t)nqtiles * sizeof(int64_t)) : 0, qdbg_b = wdbg ? al((size_t)nqtiles * 16 * sizeof(double)) : 0;
        const size_t qrow_b = window ? qlb_b : 0, qwpart_b = window ? al(window_part_bytes(nqtiles, wparts)) : 0;
        qs = prune_sort_side(ctx, ctx->scratch_pruneq, pa, fdt, m.zdims, m.kdims, qbox_b + qthr_b + qlb_b + qtpos_b + qdbg_b + qrow_b + qwpart_b);
        pa.perm = qs.perm;
        qperm = qs.perm;
        qbox = (double*)qs.rest; qthr = (double*)(qs.rest + qbox_b);
        static const bool use_qlb = PBN_TUNE(SWEEP_QLB, 1) != 0;   // offsets of the pruned plain sweeps from the prepass bounds
        if (use_qlb) qlb = (double*)(qs.rest + qbox_b + qthr_b);
        if (window || sdbg) qtpos = (int64_t*)(qs.rest + qbox_b + qthr_b + qlb_b);   // (armed aid: the positions are written whatever the model)
        if (wdbg) qdbg = (double*)(qs.rest + qbox_b + qthr_b + qlb_b + qtpos_b);
        if (window) qrow = (double*)(qs.rest + qbox_b + qthr_b + qlb_b + qtpos_b + qdbg_b);
        if (window) qwpart = (double*)(qs.rest + qbox_b + qthr_b + qlb_b + qtpos_b + qdbg_b + qrow_b);
    }
    pa.pack = q; pa.npack = q + bpack_b; pa.xpack = m.cond ? q + bpack_b + ny_b : nullptr;
    pa.xnorm = xn_b ? q + bpack_b + ny_b + bx_b : nullptr;
    pa.far_flag = ff_b ? (unsigned char*)(q + ((bpack_b + ny_b + bx_b + xn_b + 255) / 256) * 256) : nullptr;
    { KernelTimer kt(ctx, PBN_K_PACK); launch_pack(pa, fdt, ctx->stream); }
    const int P = m.cond ? 4 : 2;
    const bool fdbg = b3 && cap_f16;   // pbn_debug_f16_stages
    F16Stage fev;
    if (fdbg) {   // the fragments as the pack kernels left them (the copies are awaited behind the sweep)
        const size_t nq16 = (size_t)nqtiles * 16;
        fev.W = m.wfull ? m.Wrot : m.W;
        fev.mu = m.mu;
        fev.cols.assign(pa.cols, pa.cols + m.d);
        stage_fetch(fev.apack, m.Apack, (size_t)m.ntiles * m.KS * 64 * 8, ctx->stream);
        stage_fetch(fev.axpack, m.Axpack, m.cond ? (size_t)m.ntiles * 64 * 8 : 0, ctx->stream);
        stage_fetch(fev.bpack, pa.pack, (size_t)nqtiles * m.KS * 64 * 8, ctx->stream);
        stage_fetch(fev.npack, pa.npack, nq16, ctx->stream);
        stage_fetch(fev.bxpack, pa.xpack, m.cond ? (size_t)nqtiles * 64 * 8 : 0, ctx->stream);
        stage_fetch(fev.xnorm, pa.xnorm, pa.xnorm ? nq16 : 0, ctx->stream);
        stage_fetch(fev.far, pa.far_flag, pa.far_flag ? nq16 : 0, ctx->stream);
        stage_fetch(fev.qperm, qperm, qperm ? (size_t)n : 0, ctx->stream);
    }
    const bool wmul = !fold && sweep_weights_norm(fdt, m.cond, m.KS, m.dm);
    if (prune) {
        // bounds of the queries' largest exponents: neighbours in Morton order, and (more dimensions than keys) one sweep over
        // the subsample of the training rows; then per query tile the smallest bound and the box
        const double* subpart = nullptr;
        if (m.nsub) {
            ctx->scratch_part.reserve((size_t)nqtiles * 16 * P * sizeof(double));
            SweepArgs ss{};
            ss.Apack = m.Asub; ss.nxpack = m.nxsub; ss.Axpack = m.Axsub;
            ss.Bpack = pa.pack; ss.nypack = pa.npack; ss.Bxpack = pa.xpack; ss.Bxnorm = pa.xnorm;
            ss.ntiles = m.ntiles_sub; ss.nqtiles = nqtiles; ss.tiles_per_split = m.ntiles_sub;
            ss.fold = fold ? 1 : 0; ss.wmul = wmul ? 1 : 0; ss.prune = 0;
            ss.part = (double*)ctx->scratch_part.p;
            { KernelTimer kt(ctx, PBN_K_PACK); launch_sweep(ss, fdt, m.KS, m.cond, 1, ctx->stream); }
            subpart = ss.part;
        }
        launch_query_prepass(qs.zrow, qs.perm, n, qs.keys, m.zsorted, m.keys_sorted, m.N, m.zdims, m.pdims, (double*)qbox, (double*)qthr, (double*)qlb,
                             ctx->stream, subpart, P, m.cond ? 2 : 0, subpart ? std::log2((double)m.nsub) : 0.0, m.cond ? nullptr : m.tile_box, qtpos, fdt);
        if (sdbg) {   // as query_prepass_kernel left them: the window pass overwrites qthr / qlb in place, the sweep reuses scratch_part
            stage_fetch(sev.zrow, qs.zrow, (size_t)n * m.zdims, ctx->stream);
            stage_fetch(sev.keys_unsorted, qs.keys_unsorted, (size_t)n, ctx->stream);
            stage_fetch(sev.keys, qs.keys, (size_t)n, ctx->stream);
            stage_fetch(sev.qperm, qs.perm, (size_t)n, ctx->stream);
            stage_fetch(sev.subpart, subpart, subpart ? (size_t)nqtiles * 16 * P : 0, ctx->stream);
            stage_fetch(sev.qbox, qbox, (size_t)nqtiles * 2 * m.pdims, ctx->stream);
            stage_fetch(sev.qthr, qthr, (size_t)nqtiles, ctx->stream);
            stage_fetch(sev.qlb, qlb, qlb ? (size_t)nqtiles * 16 : 0, ctx->stream);
            stage_fetch(sev.qtpos, qtpos, (size_t)nqtiles, ctx->stream);
            HIP_CHECK(hipStreamSynchronize(ctx->stream));
            sev.num[1] = subpart ? std::log2((double)m.nsub) : 0.0;
        }
        if (window) {
            { KernelTimer kt(ctx, PBN_K_PACK); launch_query_window((const double*)m.Apack, (const double*)m.nxpack, (const double*)pa.pack, (const double*)pa.npack,
                                                               m.ntiles, m.N, nqtiles, n, qtpos, window, fold, (double*)qthr, (double*)qlb, qrow, qdbg, wparts, qwpart, ctx->stream); }
            if (wdbg) {   // pbn_debug_sum_window: the queries' bounds, in the table's row order
                std::vector<double> lb((size_t)n);
                std::vector<int32_t> perm((size_t)n);
                std::vector<int64_t> tpos((size_t)nqtiles);
                HIP_CHECK(hipMemcpyAsync(lb.data(), qdbg, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                HIP_CHECK(hipMemcpyAsync(tpos.data(), qtpos, (size_t)nqtiles * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_CHECK(hipMemcpyAsync(perm.data(), qperm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
                HIP_CHECK(hipStreamSynchronize(ctx->stream));
                std::lock_guard<std::mutex> lk(g_window_mu);
                g_window_lb.assign((size_t)n, -INFINITY);
                for (int64_t i = 0; i < n; ++i) g_window_lb[(size_t)perm[(size_t)i]] = lb[(size_t)i];
                g_window_pos.assign((size_t)n, -1);
                for (int64_t i = 0; i < n; ++i) g_window_pos[(size_t)perm[(size_t)i]] = tpos[(size_t)(i >> 4)];
            }
        }
    }
    front.join();   // from here on ctx->stream in call order: batch boxes, screen, sweep, far pass, finish

    // split the training tiles so that the grid is a few waves deep on every CU
    const int64_t qblocks = ceil_div(nqtiles, 4 * sweep_qg(fdt, m.cond, m.KS, prune));
    const int64_t target = (int64_t)ctx->num_cus * PBN_TUNE(SWEEP_BLOCKS_PER_CU, 24);
    int64_t nsplit = std::max<int64_t>(1, ceil_div(target, qblocks));
    // with the XCD-aware block order (xcd_block) the blocks resident on one XCD share a split: keep a split's training
    // fragments within half of the 4 MB L2, and the number of splits a multiple of 8 so that the XCDs get equal shares
    const int64_t tile_bytes = b3 ? (int64_t)m.KS * 64 * 16 + (m.cond ? 64 * 16 : 0)
                                  : ((int64_t)m.KS * 64 + 16 + (m.cond ? 64 : 0)) * (int64_t)es;
    nsplit = std::max<int64_t>(nsplit, ceil_div(m.ntiles * tile_bytes, (int64_t)PBN_TUNE(SWEEP_SPLIT_KB, 2048) * 1024));
    // pruned sweeps: a workgroup of the queries' own neighbourhood visits most tiles of its split, and those long workgroups are
    // the sweep's tail - at most PBN_PRUNE_MAX_TILES tiles per split (1e6 x 1e5 handles: fp64 -5...9 %, fp32 -7 %; the score
    // engine's slices are below that anyway - splitting THEM four times finer costs C5 12 %)
    if (prune) nsplit = std::max<int64_t>(nsplit, ceil_div(m.ntiles, (int64_t)PBN_TUNE(PRUNE_MAX_TILES, 1024)));
    if (nsplit > 1) nsplit = ceil_div(nsplit, 8) * 8;
    nsplit = std::min<int64_t>(nsplit, std::max<int64_t>(1, m.ntiles / PBN_TUNE(SWEEP_MIN_TILES, 64)));
    nsplit = std::min<int64_t>(nsplit, 4096);
    const int64_t tps = ceil_div(m.ntiles, nsplit);
    nsplit = ceil_div(m.ntiles, tps);
    // pruned fp64 plain sweeps with per-group masks walk their tiles in two levels (kde_sweep_body): the boxes of the 64-tile batches of every split,
    // behind the partials (they depend on the split size, which depends on the number of queries)
    static const int gmasks = PBN_TUNE(PRUNE_GROUP_MASKS, 1);
    const bool bboxes = prune && gmasks && !m.cond && fdt == PBN_F64 && PBN_TUNE(GROUP_BATCH_BOXES, 1) != 0;
    const size_t part_b = ((size_t)nsplit * nqtiles * 16 * P * sizeof(double) + 255) / 256 * 256;
    const size_t bbox_b = bboxes ? ((size_t)nsplit * ceil_div(tps, 64) * 2 * m.pdims * sizeof(double) + 255) / 256 * 256 : 0;
    // The f16 screen of the sum-only d = 8 sweep (kde_screen_d8.inc): the queries' operands and the mask words behind the batch boxes, in the same
    // grow-only arena in stream order.  One 64-bit word per (sweep wave, batch of a split, group): 51 MB at 1e6 x 1e5 rows (as much again for the far words, below); beyond
    // PBN_D8_SCREEN_MAX_MB (default 512) the step runs unscreened.
    // (Both knobs are read through getenv at every evaluation, like PBN_SUM_WINDOW and PBN_MAGIC_GUARD beside them: two lookups per step, so that a test or a
    // deployment can turn them between two calls of one process.)
    const bool mdbg = cap_masks;
    bool screen = prune && sum_only && m.scr != nullptr && bboxes && wmul && m.KS == 2 && m.pdims == PBN_PRUNE_PD && m.zdims == 8 && knob_int("PBN_D8_SCREEN", 1) != 0;
    const size_t scrq_b = screen ? (size_t)nqtiles * 16 * 32 : 0;
    size_t mask_b = screen ? (size_t)ceil_div(nqtiles, PBN_QG_PRUNE) * nsplit * ceil_div(tps, 64) * PBN_QG_PRUNE * sizeof(unsigned long long) : 0;
    if (screen && (double)mask_b * (mdbg ? 2.0 : 1.0) > (double)knob_int("PBN_D8_SCREEN_MAX_MB", 512) * 1048576.0) screen = false;
    if (!screen) mask_b = 0;
    // The far pass (round 16, kde_far32_d8.inc): far words beside the live words and a second set of partial rows.  Not without per-query bounds
    // (PBN_D8_SCREEN_ROWTHR=0, no window pass), with PBN_D8_FAR32=0 (read per evaluation), or where the far words would take the masks over
    // PBN_D8_SCREEN_MAX_MB: the step is then the one without the pass, bit for bit.
    const bool rowthr = screen && qrow != nullptr && knob_int("PBN_D8_SCREEN_ROWTHR", 1) != 0;
    const double ftheta = far32_theta(m.N);
    const bool far = rowthr && m.far_plain != nullptr && knob_int("PBN_D8_FAR32", 1) != 0 && ftheta >= 8.0 && ftheta + 4.0 <= prune_margin(fdt, m.N, sum_only) &&
                     (double)mask_b * (mdbg ? 3.0 : 2.0) <= (double)knob_int("PBN_D8_SCREEN_MAX_MB", 512) * 1048576.0;
    const size_t part_rows_b = far ? ((size_t)2 * nsplit * nqtiles * 16 * P * sizeof(double) + 255) / 256 * 256 : part_b;
    ctx->scratch_part.reserve(part_rows_b + bbox_b + (screen ? scrq_b + mask_b * ((mdbg ? 2 : 1) + (far ? 1 : 0)) : 0));
    SweepArgs sa{};
    sa.Apack = m.Apack; sa.nxpack = m.nxpack; sa.Axpack = m.Axpack;
    sa.Bpack = pa.pack; sa.nypack = pa.npack; sa.Bxpack = pa.xpack; sa.Bxnorm = pa.xnorm;
    sa.ntiles = m.ntiles; sa.nqtiles = nqtiles; sa.tiles_per_split = tps;
    sa.fold = fold ? 1 : 0;
    sa.wmul = wmul ? 1 : 0;
    sa.w32 = (b3 && !m.cond && (prune ? f16x2_w32p(m.dm, m.KS) : f16x2_w32(m.dm, m.KS))) ? 1 : 0;
    sa.far_span = (sum_only && prune) ? (double)knob_int("PBN_FAR_SPAN", 17) : 0.0;   // sum-only pruned sweeps: fp32 tail for tiles 26+ bits below the sum bound
    const bool guard = knob_int("PBN_MAGIC_GUARD", 1) != 0;   // 0: exp2_magic keeps its clamp everywhere (the same bits, slower: tests/test_magic_exp2_gpu.py)
    sa.tile_r = (guard && m.tile_r && !prune && sum_only) ? (const double*)((const char*)m.nxpack + (size_t)m.ntiles * 16 * es * 2) : nullptr;
    sa.fast = sum_only ? 1 : 0;   // only sums leave this call: 2^f on the fp32 transcendental unit; per-row logl keeps the polynomial
    sa.count_redo = knob_int("PBN_SWEEP_COUNT_REDO", 0);
    sa.box_full = (guard && prune && m.pdims == m.dm) ? 1 : 0;
    sa.prune = prune ? 1 : 0; sa.pdims = m.pdims; sa.prune_margin = prune_margin(fdt, m.N, sum_only); sa.tile_box = m.tile_box; sa.qtile_box = qbox; sa.qtile_thr = qthr; sa.qlb = qlb;
    sa.part = (double*)ctx->scratch_part.p;
    sa.group_masks = gmasks;
    if (bboxes) {
        double* bb = (double*)((char*)ctx->scratch_part.p + part_rows_b);
        launch_batch_boxes(m.tile_box, m.pdims, m.ntiles, tps, (int)nsplit, bb, ctx->stream);
        sa.batch_box = bb; sa.batches_per_split = (int)ceil_div(tps, 64);
    }
    static const bool log_sweeps = PBN_TUNE(SWEEP_LOG, 0) != 0;   // one line per sweep on stderr (tools/c5_sweeps.py)
    if (log_sweeps) std::fprintf(stderr, "pbn-sweep N=%lld n=%lld d=%d cond=%d prune=%d nsub=%lld nsplit=%lld\n", (long long)m.N, (long long)n, m.d, (int)m.cond, (int)prune, (long long)(prune ? m.nsub : 0), (long long)nsplit);
    if (screen) {
        char* sp = (char*)ctx->scratch_part.p + part_rows_b + bbox_b;
        sa.scr_train = m.scr; sa.scr_query = sp;
        sa.live_mask = (unsigned long long*)(sp + scrq_b);
        sa.box_mask = mdbg ? (unsigned long long*)(sp + scrq_b + mask_b) : nullptr;
        // every column against its own query's bound (round 14); 0: against its group's, the masks of round 13 bit for bit (read per evaluation)
        sa.qrow_thr = rowthr ? qrow : nullptr;
        if (far) {
            sa.far_mask = (unsigned long long*)(sp + scrq_b + mask_b * (mdbg ? 2 : 1));
            sa.tile_plain = m.far_plain;
            sa.far_theta = ftheta;
            sa.far_pack = m.far_pack;
        }
        KernelTimer kt(ctx, PBN_K_PACK);
        launch_screen_pack(qs.zrow, qs.perm, n, nqtiles, true, sp, ctx->stream);
        launch_screen_d8(sa, (int)nsplit, knob_int("PBN_D8_SCREEN_STREAM", 2), ctx->stream);   // (0: the serial kernel, 1: the ring, else the dense kernel: the same masks; read per evaluation)
    }
    {
        KernelTimer kt(ctx, PBN_K_SWEEP);
        launch_sweep(sa, fdt, m.KS, m.cond, (int)nsplit, ctx->stream);
        if (sa.far_mask) launch_sweep_far32_d8(sa, (int)nsplit, ctx->stream);
    }
    if (screen && mdbg) {
        std::lock_guard<std::mutex> lk(g_masks_mu);
        const size_t words = mask_b / sizeof(unsigned long long);
        g_masks.far.assign(sa.far_mask ? words : 0, 0ull);
        if (sa.far_mask) HIP_CHECK(hipMemcpyAsync(g_masks.far.data(), sa.far_mask, mask_b, hipMemcpyDeviceToHost, ctx->stream));
        g_masks.box.resize(words); g_masks.live.resize(words); g_masks.qthr.resize((size_t)nqtiles); g_masks.zq.resize((size_t)n * 8); g_masks.zt.resize((size_t)m.N * 8);
        HIP_CHECK(hipMemcpyAsync(g_masks.zt.data(), m.zsorted, (size_t)m.N * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        g_masks.part.resize((size_t)(sa.far_mask ? 2 * nsplit : nsplit) * (size_t)nqtiles * 16 * P);   // (a screened launch is unconditional: P = 2)
        HIP_CHECK(hipMemcpyAsync(g_masks.part.data(), sa.part, g_masks.part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        std::vector<int32_t> perm((size_t)n);
        std::vector<double> zrow((size_t)n * 8);
        HIP_CHECK(hipMemcpyAsync(g_masks.box.data(), sa.box_mask, mask_b, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(g_masks.live.data(), sa.live_mask, mask_b, hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(g_masks.qthr.data(), qthr, (size_t)nqtiles * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        g_masks.qrow.resize((size_t)nqtiles * 16);
        if (sa.qrow_thr) HIP_CHECK(hipMemcpyAsync(g_masks.qrow.data(), sa.qrow_thr, (size_t)nqtiles * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(zrow.data(), qs.zrow, (size_t)n * 8 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipMemcpyAsync(perm.data(), qs.perm, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int64_t i = 0; i < n; ++i)
            for (int k = 0; k < 8; ++k) g_masks.zq[(size_t)i * 8 + k] = zrow[(size_t)perm[(size_t)i] * 8 + k];
        for (auto& v : g_masks.qthr) v -= sa.prune_margin;
        if (sa.qrow_thr) {
            for (int64_t t = 0; t < nqtiles; ++t) {
                double top = g_masks.qrow[(size_t)t * 16] - sa.prune_margin;
                for (int c = 0; c < 16; ++c) {
                    double& v = g_masks.qrow[(size_t)t * 16 + c];
                    v -= sa.prune_margin;
                    if (v > top) top = v;   // (a NaN tile is NaN in all sixteen: top stays the first)
                }
                g_masks.qthr[(size_t)t] = top;
            }
        } else {
            for (int64_t t = 0; t < nqtiles; ++t)
                for (int c = 0; c < 16; ++c) g_masks.qrow[(size_t)t * 16 + c] = g_masks.qthr[(size_t)t];
        }
        const long long dims[6] = {(long long)ceil_div(nqtiles, PBN_QG_PRUNE), (long long)nsplit, (long long)ceil_div(tps, 64), (long long)tps, (long long)m.ntiles, (long long)n};
        for (int i = 0; i < 6; ++i) g_masks.dims[i] = dims[i];
    }
    if (fdbg) {   // the partials as the sweep left them
        stage_fetch(fev.part_sweep, sa.part, (size_t)nsplit * nqtiles * 16 * P, ctx->stream);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    // f16x2 fragments: queries beyond the f16 range were clamped by the pack - their partials are recomputed in fp64 (a flag test otherwise)
    if (b3) launch_far_fix(pa, m.Apack, m.Axpack, m.KS, m.N, m.ntiles, sa.part, (int)nsplit, nqtiles, m.cond, ctx->stream);
    if (fdbg) {   // ... and as kde_finish_kernel is about to merge them
        stage_fetch(fev.part_fixed, sa.part, (size_t)nsplit * nqtiles * 16 * P, ctx->stream);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        // the kernel launch_sweep_f16 chose: 0 = 16x16, 1 = W32 (unpruned), 2 = 16x16 pruned, 3 = W32P
        const int kernel = prune ? ((!m.cond && sa.w32 && m.KS == 1) ? 3 : 2) : ((!m.cond && sa.w32 && (m.KS == 1 || m.KS == 2)) ? 1 : 0);
        const long long head[19] = {(long long)n, (long long)m.N, m.d, m.dm, m.cond ? 1 : 0, m.KS, f16x2_spd(m.dm), (long long)m.ntiles, (long long)nqtiles,
                                    (long long)nsplit, (long long)tps, P, sa.w32, prune ? 1 : 0, sum_only ? 1 : 0, sweep_qg(fdt, m.cond, m.KS, prune), kernel,
                                    ctx->num_cus, (prune && m.nsub) ? 1 : 0};
        for (int i = 0; i < 19; ++i) fev.head[i] = head[i];
        fev.num[0] = sa.prune_margin; fev.num[1] = m.lognorm; fev.num[2] = m.lognorm_marg;
        std::lock_guard<std::mutex> lk(g_f16_mu);
        if (g_f16_stages.size() >= PBN_F16_STAGES_KEEP) g_f16_stages.erase(g_f16_stages.begin());
        g_f16_stages.push_back(std::move(fev));
    }

    if (sdbg) {   // what kde_finish_kernel is about to merge, and the batch boxes of the walk
        const long long rows = sa.far_mask ? 2 * nsplit : nsplit;
        stage_fetch(sev.part, sa.part, (size_t)rows * nqtiles * 16 * P, ctx->stream);
        stage_fetch(sev.bbox, sa.batch_box, bboxes ? (size_t)nsplit * ceil_div(tps, 64) * 2 * m.pdims : 0, ctx->stream);
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const long long head[21] = {(long long)n, (long long)nqtiles, (long long)nsplit, (long long)tps, (long long)ceil_div(tps, 64), sum_only ? 1 : 0, bboxes ? 1 : 0,
                                    qlb ? 1 : 0, window, m.nsub ? 1 : 0, P, m.cond ? 2 : 0, (long long)m.N, m.d, m.cond ? 1 : 0, fdt, rows,
                                    sweep_qg(fdt, m.cond, m.KS, true), ctx->num_cus, (long long)tile_bytes, m.KS};
        for (int i = 0; i < 21; ++i) sev.head[i] = head[i];
        sev.num[0] = sa.prune_margin;
        stage_keep(g_stage_evals, std::move(sev));
    }
    const int64_t nblocks = ceil_div(n, 256);
    ctx->scratch_misc.reserve((size_t)nblocks * 2 * sizeof(double));
    FinishArgs fa{};
    fa.part = sa.part; fa.nsplit = (int)(sa.far_mask ? 2 * nsplit : nsplit); fa.nqtiles = nqtiles; fa.nq = n;   // (the far pass's partial rows behind the sweep's)
    fa.lognorm = m.lognorm; fa.lognorm_marg = m.lognorm_marg;
    fa.logl = dev_logl; fa.scatter = qperm; fa.block_sums = dev_sum ? (double*)ctx->scratch_misc.p : nullptr;
    fa.block_sums_marg = (m.cond && dev_sum && dev_sum_marg) ? (double*)ctx->scratch_misc.p + nblocks : nullptr;
    { KernelTimer kt(ctx, PBN_K_FINISH); launch_finish(fa, m.cond, dev_sum, ctx->stream, dev_sum_marg); }
    front.release();
}

}  // namespace pbn

// capture != 0 arms the aid; what = 0 the shape (six values into dims), 1 / 2 the box / live masks, 3 per query tile the largest threshold of its
// columns (the group's where the launch screened against that: MaskDump), 4 / 5 the sorted queries' / training rows' whitened rows, 6 the
// columns' thresholds [query tiles * 16], 7 the far words, 8 the partial rows as doubles [rows][query tiles * 16][2] in the sorted query order of
// what = 4 (rows: the splits of the fp64 sweep, then - where the far pass ran - as many of the far pass; a pair (o, s) is s 2^o, as
// kde_finish_kernel reads it): copies up to cap items into out and returns how many the last screened sweep left
extern "C" int64_t pbn_debug_d8_masks(int what, void* out, int64_t cap, int capture) {
    pbn::g_masks_capture.store(capture != 0);
    std::lock_guard<std::mutex> lk(pbn::g_masks_mu);
    const pbn::MaskDump& d = pbn::g_masks;
    auto copy = [&](const void* src, size_t count, size_t size) -> int64_t {
        if (out && count) std::memcpy(out, src, std::min<size_t>(count, (size_t)std::max<int64_t>(cap, 0)) * size);
        return (int64_t)count;
    };
    switch (what) {
        case 0: return copy(d.dims, 6, sizeof(long long));
        case 1: return copy(d.box.data(), d.box.size(), 8);
        case 2: return copy(d.live.data(), d.live.size(), 8);
        case 3: return copy(d.qthr.data(), d.qthr.size(), 8);
        case 4: return copy(d.zq.data(), d.zq.size(), 8);
        case 5: return copy(d.zt.data(), d.zt.size(), 8);
        case 6: return copy(d.qrow.data(), d.qrow.size(), 8);
        case 7: return copy(d.far.data(), d.far.size(), 8);   // the far words (round 16); none where the launch wrote none
        case 8: return copy(d.part.data(), d.part.size(), 8);   // the partial rows both sweeps left for kde_finish_kernel
        default: return -1;
    }
}

// pbn_debug_front_lanes (test aid, not part of the C ABI header): evaluations whose query side went to a front lane since the last reset, and
// how many of them skipped the wait for the context's stream (FrontStage)
extern "C" void pbn_debug_front_lanes(unsigned long long* evals, unsigned long long* chained, int reset) {
    if (evals) *evals = pbn::g_front_evals.load();
    if (chained) *chained = pbn::g_front_chained.load();
    if (reset) { pbn::g_front_evals.store(0); pbn::g_front_chained.store(0); }
}

extern "C" int64_t pbn_debug_sum_window(double* out, int64_t cap, int capture) {
    pbn::g_window_capture.store(capture != 0);
    std::lock_guard<std::mutex> lk(pbn::g_window_mu);
    const int64_t n = (int64_t)pbn::g_window_lb.size();
    for (int64_t i = 0; out && i < n && i < cap; ++i) out[i] = pbn::g_window_lb[(size_t)i];
    if (!capture) { pbn::g_window_lb.clear(); pbn::g_window_pos.clear(); }
    return n;
}

// pbn_debug_window_pos (test aid, not part of the C ABI header): of the evaluation that pbn_debug_sum_window last captured, per query in the
// table's row order the training position (a row of the sorted order, 0 ... N) around whose tile its query tile's window stood - the position
// of the tile's first query; copies up to cap of them and returns how many there are.  Cleared with the bounds.
extern "C" int64_t pbn_debug_window_pos(int64_t* out, int64_t cap) {
    std::lock_guard<std::mutex> lk(pbn::g_window_mu);
    const int64_t n = (int64_t)pbn::g_window_pos.size();
    for (int64_t i = 0; out && i < n && i < cap; ++i) out[i] = pbn::g_window_pos[(size_t)i];
    return n;
}

// pbn_debug_prune_stages (test aid, not part of the C ABI header).  capture > 0 arms the aid, 0 disarms it and forgets what was kept, < 0 leaves it as it
// is (a read).  side 0 = the pruned fits, 1 = the pruned evaluations; back = 0 the last one, 1 the one before ... (PBN_STAGES_KEEP are kept);
// what = -1 returns how many are kept; size = f(what) with a null buffer.
// Copies up to cap items into out (null: none) and returns how many there are, -1 for an unknown code or a record that does not exist.
// Fits (kde_pack_train):
//   0 header, 14 int64: N, d, dm, zdims, pdims, kdims, nsub, ntiles, wfull, cond, fragment dtype, src_f32, key bits per axis, Hilbert order at 3 / 4 key dimensions
//   1 key cell (1 double)   2 whitening matrix handed to the kernels [d][d] row-major (Wrot where rotated)   3 mu [d]
//   4 zrow [N][zdims], logical order   5 unsorted keys (uint32)   6 sorted keys (uint32)   7 perm (int32)   8 zsorted [N][zdims]   9 tile_box [ntiles][2 pdims]
// Evaluations (kde_eval_enqueue):
//   0 header, 21 int64: n, nqtiles, nsplit, tps, batches_per_split, sum_only, bboxes, qlb in use, window (tiles, 0 = no window pass), subsample in use, P (doubles per
//     partial), which (slot of the subsample's sum), N, d, cond, fragment dtype, partial rows (nsplit, twice that with a far pass), query groups per wave of the
//     pruned sweep (sweep_qg), the context's num_cus, bytes of a training tile's fragments and KS - what the split rule of kde_eval_enqueue starts from
//   1 prune_margin, log2(nsub) (2 doubles)
//   4 query zrow [n][zdims], logical order   5 unsorted keys   6 sorted keys   7 qperm (int32)   8 subpart [nqtiles 16][P] (empty without a subsample)
//   9 qbox [nqtiles][2 pdims]   10 qthr [nqtiles]   11 qlb [nqtiles 16] (empty where unused)   12 qtpos (int64) [nqtiles] - 9 to 12 as query_prepass_kernel
//   left them, before the window pass   13 batch boxes [nsplit batches_per_split][2 pdims] (empty without)   14 partial rows [rows][nqtiles 16][P] as
//   kde_finish_kernel reads them
extern "C" int64_t pbn_debug_prune_stages(int side, int back, int what, void* out, int64_t cap, int capture) {
    if (capture >= 0) pbn::g_stages_capture.store(capture != 0);
    std::lock_guard<std::mutex> lk(pbn::g_stages_mu);
    if (capture == 0) { pbn::g_stage_fits.clear(); pbn::g_stage_evals.clear(); }
    auto copy = [&](const void* src, size_t count, size_t size) -> int64_t {
        if (out && count) std::memcpy(out, src, std::min<size_t>(count, (size_t)std::max<int64_t>(cap, 0)) * size);
        return (int64_t)count;
    };
    if (side == 0) {
        const auto& all = pbn::g_stage_fits;
        if (what == -1) return (int64_t)all.size();
        if (back < 0 || (size_t)back >= all.size()) return -1;
        const pbn::StageFit& f = all[all.size() - 1 - (size_t)back];
        switch (what) {
            case 0: return copy(f.head, 14, 8);
            case 1: return copy(&f.cell, 1, 8);
            case 2: return copy(f.W.data(), f.W.size(), 8);
            case 3: return copy(f.mu.data(), f.mu.size(), 8);
            case 4: return copy(f.zrow.data(), f.zrow.size(), 8);
            case 5: return copy(f.keys_unsorted.data(), f.keys_unsorted.size(), 4);
            case 6: return copy(f.keys.data(), f.keys.size(), 4);
            case 7: return copy(f.perm.data(), f.perm.size(), 4);
            case 8: return copy(f.zsorted.data(), f.zsorted.size(), 8);
            case 9: return copy(f.box.data(), f.box.size(), 8);
            default: return -1;
        }
    }
    if (side == 1) {
        const auto& all = pbn::g_stage_evals;
        if (what == -1) return (int64_t)all.size();
        if (back < 0 || (size_t)back >= all.size()) return -1;
        const pbn::StageEval& e = all[all.size() - 1 - (size_t)back];
        switch (what) {
            case 0: return copy(e.head, 21, 8);
            case 1: return copy(e.num, 2, 8);
            case 4: return copy(e.zrow.data(), e.zrow.size(), 8);
            case 5: return copy(e.keys_unsorted.data(), e.keys_unsorted.size(), 4);
            case 6: return copy(e.keys.data(), e.keys.size(), 4);
            case 7: return copy(e.qperm.data(), e.qperm.size(), 4);
            case 8: return copy(e.subpart.data(), e.subpart.size(), 8);
            case 9: return copy(e.qbox.data(), e.qbox.size(), 8);
            case 10: return copy(e.qthr.data(), e.qthr.size(), 8);
            case 11: return copy(e.qlb.data(), e.qlb.size(), 8);
            case 12: return copy(e.qtpos.data(), e.qtpos.size(), 8);
            case 13: return copy(e.bbox.data(), e.bbox.size(), 8);
            case 14: return copy(e.part.data(), e.part.size(), 8);
            default: return -1;
        }
    }
    return -1;
}

// pbn_debug_f16_stages (test aid, not part of the C ABI header).  capture > 0 arms the aid, 0 disarms it and forgets what was kept, < 0 leaves it as it
// is (a read).  back = 0 the last captured evaluation, 1 the one before ... (PBN_F16_STAGES_KEEP are kept); what = -1 returns how many are kept;
// the size of an item comes back with a null buffer.  Copies up to cap items into out (null: none) and returns how many there are, -1 for an
// unknown code or a record that does not exist.
//   0 header, 19 int64: n, N, d, dm, cond, NB (KS: 32-slot blocks of the main contraction), slots per dimension (f16x2_spd), ntiles, nqtiles, nsplit, tps
//     (tiles per split), P (doubles per partial), SweepArgs::w32, prune, sum_only, sweep_qg, kernel (0 = kde_sweep_f16_kernel unpruned, 1 =
//     kde_sweep_f16_w32_kernel, 2 = kde_sweep_f16_kernel pruned, 3 = kde_sweep_f16_w32p_kernel), the context's num_cus, 1 where a subsample
//     sweep ran in front (pruned, more dimensions than boxes)
//   1 prune_margin, lognorm, lognorm_marg as kde_finish_kernel gets them (3 doubles)   2 W [d][d] row-major as the pack kernels were handed it   3 mu [d]   4 the table's columns in W's order (int32)
//   5 training fragments [ntiles][NB][64][8] (f16 as uint16)   6 the CKDE block of the training side [ntiles][64][8] (empty unless cond)
//   7 query fragments [nqtiles][NB][64][8] as pack_rows_f16_kernel left them   8 npack [nqtiles 16] (float)   9 query CKDE block [nqtiles][64][8]
//   10 xnorm [nqtiles 16] (float; empty unless cond)   11 far flags [nqtiles 16] (bytes)   12 qperm (int32; empty unless pruned)
//   13 partials [nsplit][nqtiles 16][P] behind the sweep   14 the same behind kde_far_fix_kernel, as kde_finish_kernel reads them
extern "C" int64_t pbn_debug_f16_stages(int back, int what, void* out, int64_t cap, int capture) {
    if (capture >= 0) pbn::g_f16_capture.store(capture != 0);
    std::lock_guard<std::mutex> lk(pbn::g_f16_mu);
    if (capture == 0) pbn::g_f16_stages.clear();
    auto copy = [&](const void* src, size_t count, size_t size) -> int64_t {
        if (out && count) std::memcpy(out, src, std::min<size_t>(count, (size_t)std::max<int64_t>(cap, 0)) * size);
        return (int64_t)count;
    };
    const auto& all = pbn::g_f16_stages;
    if (what == -1) return (int64_t)all.size();
    if (back < 0 || (size_t)back >= all.size()) return -1;
    const pbn::F16Stage& e = all[all.size() - 1 - (size_t)back];
    switch (what) {
        case 0: return copy(e.head, 19, 8);
        case 1: return copy(e.num, 3, 8);
        case 2: return copy(e.W.data(), e.W.size(), 8);
        case 3: return copy(e.mu.data(), e.mu.size(), 8);
        case 4: return copy(e.cols.data(), e.cols.size(), 4);
        case 5: return copy(e.apack.data(), e.apack.size(), 2);
        case 6: return copy(e.axpack.data(), e.axpack.size(), 2);
        case 7: return copy(e.bpack.data(), e.bpack.size(), 2);
        case 8: return copy(e.npack.data(), e.npack.size(), 4);
        case 9: return copy(e.bxpack.data(), e.bxpack.size(), 2);
        case 10: return copy(e.xnorm.data(), e.xnorm.size(), 4);
        case 11: return copy(e.far.data(), e.far.size(), 1);
        case 12: return copy(e.qperm.data(), e.qperm.size(), 4);
        case 13: return copy(e.part_sweep.data(), e.part_sweep.size(), 8);
        case 14: return copy(e.part_fixed.data(), e.part_fixed.size(), 8);
        default: return -1;
    }
}
