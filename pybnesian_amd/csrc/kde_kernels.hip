// KDE / ProductKDE / CKDE log-likelihood sweep for gfx950 (MI355X).
//
// Replaces the reference's tile-of-64 OpenCL pipeline
//   substract -> solve -> square -> logl_values_mat_* -> max_mat_cols -> logsumexp_coeffs ->
//   sum_mat_cols -> finish_lse_offset -> sum1d
// (the reference's pybnesian/kde/KDE.hpp:592-640, kde/opencl_kernels/KDE.cl.src:115-233,
//  opencl/opencl_config.hpp:517-536) with three kernels:
//
//   pack_rows     z = sqrt(log2 e) * L^-1 (x - mu)  (whiten + centre + scale to base-2 units), written
//                 in MFMA 16x16x4 operand-fragment order together with -1/2 |z|^2.  After this
//                 s2(t,q) = log2(e) * (-1/2 |L^-1 (x_t - y_q)|^2) = z_t . z_q - 1/2|z_t|^2 - 1/2|z_q|^2,
//                 so the per-pair triangular solve of KDE.cl.src:123-135 disappears.
//   kde_sweep     each wave owns QG groups of 16 query rows (B fragments live in registers) and
//                 streams 16-row training tiles (A fragments, coalesced 512 B loads).  The
//                 dot products run on the matrix pipe (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32)
//                 with the accumulator pre-loaded with  -1/2|z_t|^2 - 1/2|z_q|^2 - m_q ; the VALU only
//                 evaluates 2^x and the running sum.  Online logsumexp: m_q is a per-query offset
//                 that is raised (rarely, wave-uniform slow path) when a term would overflow.
//                 No N x 64 tile is ever materialised.
//                 CKDE (COND=true): evidence-first Cholesky makes the marginal's whitened coordinates a
//                 prefix of the joint's, so ONE sweep yields both logsumexps: the joint accumulator is
//                 the marginal accumulator plus one extra augmented MFMA k-step.
//   kde_finish    merge the per-split (m, sum) partials in fixed order, add the log-normalisation,
//                 write logl and/or a deterministic tree-reduced slogl.
//
// This unit holds the sweeps: kde_sweep_body and its fp64 / f32-MFMA kernels here, the fp32 sweeps on the 16-bit matrix cores in
// kde_sweep_f16.inc (included below).  The other kernels of the pipeline:
//   kde_prepass.hip    pack_rows, the wide pack / sweep, and the keys, boxes and bounds of the pruned sweeps
//   kde_moment.hip     the tile-moment pass beside the grouped sweeps
//   kde_cdf.hip        CKDE::cdf / sample and UCV
//   kde_finish.hip     kde_finish, the final reduction, and the host predicates that pick a sweep's shape
//   kde_device.hpp     the device helpers they share
#include "common.hpp"
#include <atomic>
#include "kde_kernels.hpp"
#include "kde_group.hpp"
#include "kde_device.hpp"

namespace pbn {

// measurement aid, not part of the C ABI header: (wave, split) units of the fp64 sweep that had to redo their split checked
__device__ unsigned long long g_sweep_redo = 0, g_sweep_units = 0;
__device__ unsigned long long g_sweep_visit = 0, g_sweep_tiles = 0;
// (pruned sweeps: tiles visited / tiles offered, per wave)
// waves per SIMD the pruned fp64 sweeps are compiled for: 3 (<= 168 VGPRs) - the blind-batch shapes fit anyway, the checked
// d = 4 / 5 and norm-multiplying shapes (183-207 unconstrained) gain 3-9 % on the 1e6 x 1e5 handles; 4 (128, spills) loses on C3
#ifndef PBN_F64_PRUNE_WAVES
#define PBN_F64_PRUNE_WAVES 3
#endif
#ifndef PBN_FAR_F32
#define PBN_FAR_F32 1   // pruned plain fp64 sum-only sweeps: far tiles through the fp32 unit (kde_sweep_body: FARP; SweepArgs::far_span)
#endif
#ifndef PBN_SWEEP_UNCHECKED
#define PBN_SWEEP_UNCHECKED 1   // fp64 plain unpruned sweeps: blind first pass, checked redo (kde_sweep_kernel)
#endif

// ... for ALL of a wave's groups at once (round 9, the d = 8 shape): the tile's box is loaded once and every group's distance is taken from it - one
// round trip per batch instead of one per (batch, group).  Per group the same operations in the same order as prune_group_mask: the same masks.
template <int PD, int QG, typename BP, typename QP>
__device__ __forceinline__ void prune_group_masks_joint(BP tile_box, const QP (&qbox)[QG], int pd, int64_t tb, int64_t t1, const double (&thr)[QG], int lane,
                                                        unsigned long long (&gm)[QG]) {
    const int64_t t = tb + lane;
    bool keep[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) keep[g] = false;
    if (t < t1) {
        const BP bx = tile_box + t * 2 * pd;
        double d2[QG];
#pragma unroll
        for (int g = 0; g < QG; ++g) d2[g] = 0.0;
#pragma unroll
        for (int k = 0; k < PD; ++k)
            if (k < pd) {
                const double lo = bx[k], hi = bx[pd + k];
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    const double g1 = lo - qbox[g][pd + k], g2 = qbox[g][k] - hi;
                    double gg = g1 > g2 ? g1 : g2;
                    gg = gg > 0.0 ? gg : 0.0;
                    d2[g] = __builtin_fma(gg, gg, d2[g]);
                }
            }
#pragma unroll
        for (int g = 0; g < QG; ++g) keep[g] = !(-0.5 * d2[g] < thr[g]);
    }
#pragma unroll
    for (int g = 0; g < QG; ++g) gm[g] = __ballot(keep[g]);
}

// ... with a second, nearer threshold: `near` = the tiles that hold a term above thr_near (the others of the returned mask are the
// far tiles of the fp32 tail path)
template <int PD, typename BP>
__device__ __forceinline__ unsigned long long prune_group_mask2(BP tile_box, BP qbox, int pd, int64_t tb, int64_t t1, double thr, double thr_near, int lane,
                                                                unsigned long long& near) {
    const int64_t t = tb + lane;
    bool keep = false, kn = false;
    if (t < t1) {
        const BP bx = tile_box + t * 2 * pd;
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < PD; ++k)
            if (k < pd) {
                const double g1 = bx[k] - qbox[pd + k], g2 = qbox[k] - bx[pd + k];
                double g = g1 > g2 ? g1 : g2;
                g = g > 0.0 ? g : 0.0;
                d2 = __builtin_fma(g, g, d2);
            }
        keep = !(-0.5 * d2 < thr);
        kn = !(-0.5 * d2 < thr_near);
    }
    near = __ballot(kn);
    return __ballot(keep);
}

// GUARD of the pruned sum-only fp64 sweeps (round 6): is the LARGEST squared distance between the batch's box and the group's box at most
// PBN_OPEN_FAR2?  With boxes over all whitened dimensions every exponent of the batch's rows against the group's queries then lies at most
// PBN_OPEN_FAR2 / 2 below the offset, and exp2_magic needs no clamp for the batch (false for a box with a NaN or infinite side).
#define PBN_OPEN_FAR2 2200.0
template <int PD, typename BP>
__device__ __forceinline__ bool batch_all_near(BP bb, BP qbox, int pd) {
    double f2 = 0.0;
#pragma unroll
    for (int k = 0; k < PD; ++k)
        if (k < pd) {
            const double h1 = bb[pd + k] - qbox[k], h2 = qbox[pd + k] - bb[k];
            const double h = h1 > h2 ? h1 : h2;
            f2 = __builtin_fma(h, h, f2);
        }
    return f2 <= PBN_OPEN_FAR2;
}

// GUARD of the pruned sum-only d = 8 sweep (round 9; norms as WEIGHTS, boxes over all eight rotated dimensions).  The accumulator of a (row, query)
// pair holds x = z_t.z_q - 1/2|z_q|^2 - m_q + bias = 1/2|z_t|^2 - 1/2|z_t - z_q|^2 - m_q + bias (the norm rides in the weight), so with z_t inside
// the batch's box, z_q inside the group's box and m_lo <= m_q <= m_hi over the group's 16 queries
//   x <= 1/2 max|z_t|^2 - m_lo + bias,   max|z_t|^2 <= n2 = sum_k max(lo_k^2, hi_k^2) over the batch's box (the rotation keeps norms),
//   x >= -1/2 f2 - m_hi + bias,           f2 = the LARGEST squared distance between the two boxes (batch_all_near's).
// A batch is bare for the group when 1/2 n2 <= up = 1021 - bias + m_lo and 1/2 f2 <= dn = 1021 + bias - m_hi: every exponent inside +-1021, where
// exp2_magic and its clamped form are the same function (the clamp acts beyond +-1023; one unit covers the rounding of these sums).  False for a
// batch box with a NaN side; the caller keeps the group's side of the proof (finite queries and offsets, not the padded query tile) and the batch
// with the table's padded last tile out.
template <int PD, typename BP, typename QP>
__device__ __forceinline__ bool batch_bare_wmul(BP bb, QP qbox, int pd, double up, double dn) {
    double n2 = 0.0, f2 = 0.0;
#pragma unroll
    for (int k = 0; k < PD; ++k)
        if (k < pd) {
            const double lo = bb[k], hi = bb[pd + k];
            const double l2 = lo * lo, h2 = hi * hi;
            n2 += (l2 > h2 || l2 != l2) ? l2 : h2;
            const double d1 = hi - qbox[k], d2 = qbox[pd + k] - lo;
            const double d = (d1 > d2 || d1 != d1) ? d1 : d2;
            f2 = __builtin_fma(d, d, f2);
        }
    return 0.5 * n2 <= up && 0.5 * f2 <= dn;
}

// WMUL (d mod 4 == 0, no free K slot for the norm): the training norms enter as WEIGHTS.  The accumulator starts from the
// per-query constant alone (a persistent register quad as the MFMA's C operand, as with FOLD) and holds
// x' = z_t.z_q - 1/2|z_q|^2 - m_q + bias; the term is 2^x' * w_t with w_t = 2^(-1/2|z_t|^2) precomputed by the pack kernel, and
// the multiply rides in the running sum's FMA: no add per value for the norm.  x' >= 0 for every term that matters (x' >=
// x' - 1/2|z_t|^2 >= 0), so the v_fract form still applies; x' can exceed the exponent range only when z_t.z_q is huge (a
// far-out query next to a far-out training row): 2^x' = inf (times w = 0: NaN) fails the per-tile test `ts < big`, and the
// rare path redoes the tile the classic way (norms added to the accumulator).  Rows with -1/2|z|^2 < -1000, whose weight
// would lose bits or underflow, carry w = NaN and always take that path.
// The sweep proper.  `bid` is the workgroup's index inside ITS sweep: blockIdx.x for a stand-alone launch, the offset inside
// the unit for the grouped launches (kde_sweep_group_kernel), where `a` was assembled from the unit's record.
// EF32: 2^f of the main loop on the fp32 transcendental unit (exp2_f64_fract<true>; sweeps whose result is a sum)
// MOM (round 5): the moment pass runs beside this sweep (grouped fp64 sum-only launches of one- and two-variable units) - the sweep skips the
// pairs the pass takes (prune_group_mask3).  A template parameter, not a run-time branch:
// the kernel sits at its register limit and the extra paths cost the plain sweep 25 % when compiled in.
// PDFIX (round 9): the number of box dimensions as a compile-time fact (0: SweepArgs::pdims at run time).  With a run-time `pd` every box test
// is a chain of `if (k < pd)` blocks, each with its own loads and its own wait: eight dependent round trips per mask at d = 8.  With pd = PDFIX
// the loops unroll flat - all box loads of a test are issued before the first wait.  The launch picks the form (launch_sweep_tf: kde_sweep_pruned_d8_kernel where pdims == 8).
template <typename T, int KS, bool COND, int QG, bool FOLD, bool PRUNE, bool WMUL, bool EF32 = false, bool MOM = false, int PDMAX = PBN_PRUNE_PD, int PDFIX = 0>
__device__ __forceinline__ void kde_sweep_body(const SweepArgs& a, const unsigned bid) {
    static_assert(!WMUL || (!FOLD && !COND), "WMUL: plain sweeps without a free K slot only");
    using V = typename Tr<T>::vec4;
    // MAGIC: the accumulators of this sweep carry Tr<T>::magic() and 2^x is exp2_magic - unpruned sum-only fp64 sweeps (round 6)
    constexpr bool MAGIC = PBN_EXP2_MAGIC && EF32 && PBN_EXP2_F32 && PBN_EXP2_DEGREE <= 7 && sizeof(T) == 8 && !COND && (!PRUNE || PBN_MAGIC_PRUNED);
    // the per-query constant of the accumulators: norm (+ the magic constant, rounded to ITS grid once per query: what follows - the
    // integer offset, the bias - is exact), and 2^x of an accumulator
    auto cbase = [](T nyq) -> T { return MAGIC ? (T)(nyq + Tr<T>::magic()) : nyq; };
    auto ex2a = [](T v, T top) -> T {
        if constexpr (MAGIC) { (void)top; return Tr<T>::template ex2m<PBN_MAGIC_CLAMP != 0>(v); }
        else return Tr<T>::template ex2p<EF32>(v, top);
    };
    constexpr int WPB = sweep_block_threads(PRUNE) / 64;   // waves per workgroup
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lg = lane >> 4;
    int qx, split;
    if (PRUNE) pruned_block(a, WPB * QG, bid, qx, split);
    else xcd_block(qx, split);
    const int64_t qt0 = ((int64_t)qx * WPB + wave) * QG;
    if (qt0 >= a.nqtiles) return;  // no barriers in this kernel: idle waves just leave
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;

    const PBN_GLOBAL T* __restrict__ Ap = (const PBN_GLOBAL T*)a.Apack;
    const PBN_GLOBAL T* __restrict__ Np = (const PBN_GLOBAL T*)a.nxpack;
    const PBN_GLOBAL T* __restrict__ Wp = Np + a.ntiles * 16;   // WMUL: weights 2^norm behind the norms (PackArgs::write_w)
    const PBN_GLOBAL T* __restrict__ Xp = (const PBN_GLOBAL T*)a.Axpack;
    const PBN_GLOBAL T* __restrict__ Bp = (const PBN_GLOBAL T*)a.Bpack;
    const PBN_GLOBAL T* __restrict__ NYp = (const PBN_GLOBAL T*)a.nypack;
    const PBN_GLOBAL T* __restrict__ BXp = (const PBN_GLOBAL T*)a.Bxpack;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL double* __restrict__ QLp = (const PBN_GLOBAL double*)a.qlb;

    // ---- query-side fragments and per-query state -------------------------------------------
    T b[QG][KS];
    T ny[QG], cm[QG], m[QG];
    V cmv[QG];  // FOLD: the accumulator's start value, cm in all four rows (the training norms ride in a K slot)
    double sum[QG];
    T bxb[QG], bx[QG], mj[QG];  // CKDE: extra-step B fragment (base / current), joint offset
    double sumj[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[g][ks] = Bp[(qt * KS + ks) * 64 + lane];
        ny[g] = NYp[qt * 16 + (lane & 15)];
        sum[g] = 0.0;
        if (COND) { bxb[g] = BXp[qt * 64 + lane]; sumj[g] = 0.0; }
    }

    const T ctop = Tr<T>::top();   // leading exp2 coefficient pinned in a VGPR for the whole kernel

    // ---- tile pruning: box of this wave's queries and the exponent below which a training tile cannot matter -------
    // boxes of up to 8 dimensions in the plain fp64 shapes (d = 7, 8: kde_prune_rotates), of up to 5 in the conditional and grouped ones (their spills)
    constexpr int PDW = COND ? PBN_PRUNE_PD_NARROW : PDMAX;
    static_assert(PDFIX == 0 || (PRUNE && PDFIX <= PDW), "PDFIX: a pruned shape's own number of box dimensions");
    // pruned plain fp64 sweeps: visit masks per query group (GMASK), bit `bit` of gm[g] = group g needs this tile
    constexpr bool GMASK = PRUNE && !COND && sizeof(T) == 8;
    // The GMASK shapes test every 16-query group against its OWN box (prune_group_mask*) and every 64-tile batch against the batch boxes: the
    // shipped library provides both with every launch (launch_sweep_tf and launch_sweep_grouped refuse a launch without them), so they are
    // compile-time facts here and the box of the whole WAVE - 2 x PDW + 1 doubles, 34 VGPRs at eight dimensions, alive across the whole walk
    // only to feed the fallback prune_visit_mask - is not part of these kernels.  Builds with -DPBN_EXPERIMENTS keep the run-time choice
    // (PBN_PRUNE_GROUP_MASKS / PBN_GROUP_BATCH_BOXES = 0: tools/gmask_probe.sh).
#ifdef PBN_EXPERIMENTS
    constexpr bool WBOX = PRUNE;
    const bool gmasks = GMASK && (MOM || a.group_masks), bboxes = gmasks && a.batch_box;
#else
    constexpr bool WBOX = PRUNE && !GMASK;
    constexpr bool gmasks = GMASK, bboxes = GMASK;
#endif
    double wlo[PDW] = {}, whi[PDW] = {}, wthr = 0;
    const int pd = PRUNE ? (PDFIX ? PDFIX : a.pdims) : 0;
    // QLDS (round 9, the PDFIX shape): the boxes of the wave's own groups and their drop thresholds - the same 2 x pd + 1 doubles for every test of
    // the walk, at a uniform address - are copied to LDS once (one wave per workgroup: no barrier) and read from there: the box tests' vector-memory loads are the tile
    // or batch boxes alone, and the groups' sides arrive on the LDS counter without holding 2 x pd x QG doubles in registers across a wait
    constexpr bool QLDS = GMASK && PDFIX != 0;
    __shared__ double qbs[QLDS ? QG * (2 * PDW + 1) : 1];
    if constexpr (QLDS) {
        static_assert(QG * 2 * PDW + QG <= 64, "one lane per box coordinate and threshold");
        if (lane < QG * 2 * PDFIX) {
            const int g = lane / (2 * PDFIX);
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            qbs[lane] = QBp[qt * 2 * PDFIX + (lane - g * 2 * PDFIX)];
        } else if (lane < QG * 2 * PDFIX + QG) {
            const int g = lane - QG * 2 * PDFIX;
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            qbs[lane] = QTp[qt] - a.prune_margin;
        }
    }
    auto thr_of = [&](int g, int64_t qt) -> double {   // group g's drop threshold: its sum bound less the margin
        if constexpr (QLDS) { (void)qt; return qbs[QG * 2 * PDFIX + g]; }
        else { (void)g; return QTp[qt] - a.prune_margin; }
    };
    auto qbox_of = [&](int g, int64_t qt) {   // group g's box (query tile qt)
        if constexpr (QLDS) { (void)qt; return (const double*)&qbs[g * 2 * PDFIX]; }
        else { (void)g; return QBp + qt * 2 * pd; }
    };
    if constexpr (WBOX) {
        wthr = INFINITY;
#pragma unroll
        for (int k = 0; k < PDW; ++k) { wlo[k] = INFINITY; whi[k] = -INFINITY; }
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            const double th = QTp[qt];
            wthr = th < wthr ? th : wthr;
#pragma unroll
            for (int k = 0; k < PDW; ++k)
                if (k < pd) {
                    const double l = QBp[qt * 2 * pd + k], h = QBp[qt * 2 * pd + pd + k];
                    wlo[k] = l < wlo[k] ? l : wlo[k];
                    whi[k] = h > whi[k] ? h : whi[k];
                }
        }
        wthr -= a.prune_margin;
    }
    // ---- prologue: offsets from the first tile (max of s2 over its 16 rows) ---------------------
    {
        T af[KS];
        V nx;
        T ax = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = Ap[(t0 * KS + ks) * 64 + lane];
        if (!FOLD) nx = *(const PBN_GLOBAL V*)(Np + t0 * 16 + lg * 4);
        if (COND) ax = Xp[t0 * 64 + lane];
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            V acc = FOLD ? V{ny[g], ny[g], ny[g], ny[g]} : nx + ny[g];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = Tr<T>::mfma(af[ks], b[g][ks], acc);
            // The offsets are INTEGERS (base-2 units): then fract(s2 - m + bias) = fract(s2), so the argument of the 2^f
            // polynomial - and with it its ~2e-9 approximation error - belongs to the (training row, query) pair and not to
            // the offset, i.e. not to the split, the tile order or the pruning: sums taken in a different partition agree to
            // rounding (1e-13), not to the polynomial's error bound.  Scaling by 2^integer is exact.
            T mx = __builtin_ceil(colmax<T>(max4<T>(acc)));
            m[g] = mx;
            cm[g] = cbase(ny[g]) - mx + Tr<T>::bias();   // main-loop exponents are kept biased (Tr<T>::ex2p)
            if (FOLD || WMUL) cmv[g] = V{cm[g], cm[g], cm[g], cm[g]};
            if (COND) {
                V accj = Tr<T>::mfma(ax, bxb[g], acc);
                T mxj = __builtin_ceil(colmax<T>(max4<T>(accj)));
                mj[g] = mxj;
                bx[g] = (lg == 2) ? bxb[g] + (m[g] - mj[g]) : bxb[g];
            }
        }
    }

    // Pruned plain sweeps: the prepass knows a lower bound of every query's largest exponent over ALL training rows (its
    // Morton neighbours, the subsample sweep).  Where that bound lies above the first tile's maximum it becomes the offset: the
    // first tile of a Morton-ordered split is typically thousands of exponent units away from the queries, so the first
    // VISITED tile used to overflow 2^x and take the redo path once per (group, split); with the bound as the offset no term
    // can exceed it by more than the bound's slack (log2 of the subsample size, or the distance to the best Morton
    // neighbour), and the blind passes below never trip.  Such an offset has no term of this split behind it: an empty sum
    // stays empty (the query's largest term is never pruned, so the split that holds it has a positive sum).
    // (fused CKDE sweeps: the bound is the JOINT one, which also bounds the marginal maximum from below.)
    bool lbm[QG], lbmj[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) lbm[g] = lbmj[g] = false;
    if constexpr (PRUNE) {
        if (a.qlb) {
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
                const T lb = __builtin_ceil((T)QLp[qt * 16 + (lane & 15)]);
                // (a bound too large for T to hold to a fraction of a unit is not used: see kde_sweep_f16_kernel)
                const bool fin = (lb < (T)0 ? -lb : lb) < (sizeof(T) == 8 ? (T)0x1p50 : (T)0x1p22);
                lbm[g] = fin && lb > m[g];
                if (lbm[g]) {
                    m[g] = lb;
                    cm[g] = cbase(ny[g]) - lb + Tr<T>::bias();
                }
                if (FOLD || WMUL) cmv[g] = V{cm[g], cm[g], cm[g], cm[g]};
                if (COND) {
                    lbmj[g] = fin && lb > mj[g];
                    if (lbmj[g]) mj[g] = lb;
                    bx[g] = (lg == 2) ? bxb[g] + (m[g] - mj[g]) : bxb[g];
                }
            }
        }
    }

    // ---- main loop over training tiles: two tiles per iteration with ping-pong fragment buffers (no
    // register copies); the fragments of tile t+1 / t+2 are in flight while tile t is processed -------------
    auto load_tile = [&](int64_t t, T (&f)[KS], V& n, T& x) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) f[ks] = Ap[(t * KS + ks) * 64 + lane];
        if (!FOLD) n = *(const PBN_GLOBAL V*)((WMUL ? Wp : Np) + t * 16 + lg * 4);
        if (COND) x = Xp[t * 64 + lane];
    };
    unsigned long long gm[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) gm[g] = ~0ull;
    // FARP (round 4; sum-only pruned sweeps of the FOLD shapes, per-group masks): a tile ALL of whose terms lie more than
    // prune_margin - far_span (26 at 10^6 rows) below the group's sum bound contributes less than 2^-26 of the sum per term: its 2^x go
    // through the fp32 unit directly - cvt_f32_f64, v_exp_f32, v_add_f32: 4 issue slots per value instead of 8 - and are added in fp32
    // until the end of the blind batch.  The exponents are biased by +128 and the offsets lie within 6 units of the sum bound (the
    // prepass bounds), so x' <= 108: no overflow, and 2^x' carries the same 2^bias as the fp64 sums.  Relative error of such a term
    // 2^-24 |x'| ln 2 <= 5.3e-6, of the sum <= 5.3e-6 N 2^-26 = 8e-8 (the margin follows log2(N / 10^6), so the bound does not depend
    // on N).  A batch redone by the checked loop takes every tile through the full path.
    constexpr bool FARP = GMASK && FOLD && EF32 && PBN_FAR_F32;
    static_assert(!MOM || FARP, "the moment pass stands beside the FARP shapes only");
    unsigned long long gn[FARP ? QG : 1];
    float fs[FARP ? QG : 1];
#pragma unroll
    for (int g = 0; g < (FARP ? QG : 1); ++g) { gn[g] = ~0ull; fs[g] = 0.f; }
    // GUARDP (round 6): pruned MAGIC sweeps with the norm in a K slot and boxes over all whitened dimensions (d <= 3) - a 64-tile batch whose
    // box lies within PBN_OPEN_FAR2 of the boxes of the wave's groups runs exp2_magic without its clamp (batch_all_near, one lane-parallel
    // test per super-batch beside batch_in_reach: nothing per tile); gate_of = the group's side of the proof: offsets inside [-890, 16] (an
    // exponent is at most bias - offset), no NaN query, not the query tile with the padding rows
    constexpr bool GUARDP = MAGIC && PRUNE && GMASK && FOLD && KS == 1 && PBN_MAGIC_GUARD;
    // (taken per super-batch, from the offsets as they stand: a scalar carried around the whole walk - even one computed once before it - pushed
    // the visit masks out of the SGPRs into vector registers and lane-masked branches: 25 % of the kernel's time)
    auto gate_of = [&](int g) -> bool {
        return __builtin_amdgcn_readfirstlane(__all(a.box_full && qt0 + g < a.nqtiles - 1 && ny[g] == ny[g] && m[g] >= (T)-890 && m[g] <= (T)16)) != 0;
    };
    // GUARDW (round 9): the same for the d = 8 shape with the norms as weights and pd at compile time - batch_bare_wmul has the proof.  Taken per
    // super-batch from the offsets as they stand, like GUARDP; a checked redo is the only thing that moves an offset, and it closes the rest of
    // its super-batch (do_batch returns it), so no batch runs bare on a bound taken from older offsets.
    constexpr bool GUARDW = MAGIC && GMASK && WMUL && KS == 2 && PDFIX != 0 && PBN_MAGIC_GUARD;
    auto gate_w = [&](int g) -> bool {
        const T am = m[g] < (T)0 ? -m[g] : m[g];
        return __builtin_amdgcn_readfirstlane(__all(a.box_full && qt0 + g < a.nqtiles - 1 && ny[g] == ny[g] && am < (T)0x1p50)) != 0;
    };
    auto process_tile = [&](const int64_t t, const T (&af)[KS], const V& nx, const T ax, const int bit) {
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            if (GMASK && !((gm[g] >> bit) & 1ull)) continue;
            V acc;
            if (FOLD || WMUL) acc = cmv[g]; else acc = nx + cm[g];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = Tr<T>::mfma(af[ks], b[g][ks], acc);
            V accj;
            if (COND) accj = Tr<T>::mfma(ax, bx[g], acc);

            T e0 = ex2a(acc[0], ctop), e1 = ex2a(acc[1], ctop), e2 = ex2a(acc[2], ctop), e3 = ex2a(acc[3], ctop);
            T ts;
            if (WMUL) ts = __builtin_fma(e3, nx[3], __builtin_fma(e2, nx[2], __builtin_fma(e1, nx[1], e0 * nx[0])));   // nx holds the weights
            else ts = (e0 + e1) + (e2 + e3);
            T tsj = 0;
            bool bad = !(ts < Tr<T>::big());
            if (COND) {
                T j0 = ex2a(accj[0], ctop), j1 = ex2a(accj[1], ctop), j2 = ex2a(accj[2], ctop), j3 = ex2a(accj[3], ctop);
                tsj = (j0 + j1) + (j2 + j3);
                bad = bad || !(tsj < Tr<T>::big());
            }
            if (__builtin_expect(__any(bad), 0)) {
                // Rare wave-uniform slow path: raise the offsets to the tile maximum and redo the tile.
                if (WMUL) acc += *(const PBN_GLOBAL V*)(Np + t * 16 + lg * 4);   // the classic exponents: norms added
                T mx = __builtin_ceil(colmax<T>(max4<T>(acc)) - (MAGIC ? Tr<T>::magic() : (T)0) - Tr<T>::bias());
                if (mx > (T)0) {
                    m[g] += mx;
                    cm[g] = cbase(ny[g]) - m[g] + Tr<T>::bias();
                    if (FOLD || WMUL) cmv[g] = V{cm[g], cm[g], cm[g], cm[g]};
                    sum[g] *= exp2(-(double)mx);
                    acc -= mx;
                }
                // the SAME 2^x as the main loop (the exponents are still biased, the offsets integers): a term must come out
                // identical whichever path evaluates it, or sums taken in another tile order would differ by the polynomial's
                // error (the Morton-ordered sweeps come through here often, table-ordered ones hardly ever)
                e0 = ex2a(acc[0], ctop); e1 = ex2a(acc[1], ctop); e2 = ex2a(acc[2], ctop); e3 = ex2a(acc[3], ctop);
                ts = (e0 + e1) + (e2 + e3);
                if (COND) {
                    T mxj = __builtin_ceil(colmax<T>(max4<T>(accj)) - Tr<T>::bias());
                    if (mxj > (T)0) {
                        mj[g] += mxj;
                        sumj[g] *= exp2(-(double)mxj);
                        accj -= mxj;
                    }
                    bx[g] = (lg == 2) ? bxb[g] + (m[g] - mj[g]) : bxb[g];
                    T j0 = ex2a(accj[0], ctop), j1 = ex2a(accj[1], ctop), j2 = ex2a(accj[2], ctop), j3 = ex2a(accj[3], ctop);
                    tsj = (j0 + j1) + (j2 + j3);
                }
            }
            sum[g] += (double)ts;
            if (COND) sumj[g] += (double)tsj;
        }
    };

    T afA[KS], afB[KS];
    V nxA, nxB;
    T axA = 0, axB = 0;
    // blind accumulation (see "Unchecked passes" below): no overflow test, no separate add
    auto process_fast = [&](const T (&af)[KS], const V& nx, const int bit, auto clamp) {
        constexpr int CLAMPED = decltype(clamp)::value;   // 0: exp2_magic without its clamp (the chunk's / batch's exponents are proven inside +-1022)
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            if (GMASK && !((gm[g] >> bit) & 1ull)) continue;
            V acc;
            if (FOLD || WMUL) acc = cmv[g]; else acc = nx + cm[g];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = Tr<T>::mfma(af[ks], b[g][ks], acc);
            if constexpr (FARP) {
                if (!((gn[g] >> bit) & 1ull)) {   // a far tile of this group: the fp32 tail path
                    if constexpr (MAGIC) acc -= Tr<T>::magic();   // (exact: the accumulator sits on the constant's grid)
                    const float f0 = __builtin_amdgcn_exp2f((float)acc[0]), f1 = __builtin_amdgcn_exp2f((float)acc[1]);
                    const float f2 = __builtin_amdgcn_exp2f((float)acc[2]), f3 = __builtin_amdgcn_exp2f((float)acc[3]);
                    fs[g] += (f0 + f1) + (f2 + f3);
                    continue;
                }
            }
            T e0, e1, e2, e3;
            if constexpr (MAGIC && CLAMPED == 0) {
                e0 = Tr<T>::template ex2m<false>(acc[0]); e1 = Tr<T>::template ex2m<false>(acc[1]); e2 = Tr<T>::template ex2m<false>(acc[2]); e3 = Tr<T>::template ex2m<false>(acc[3]);
            } else {
                e0 = ex2a(acc[0], ctop); e1 = ex2a(acc[1], ctop); e2 = ex2a(acc[2], ctop); e3 = ex2a(acc[3], ctop);
            }
            if (WMUL) sum[g] = __builtin_fma(e3, nx[3], __builtin_fma(e2, nx[2], __builtin_fma(e1, nx[1], __builtin_fma(e0, nx[0], sum[g]))));
            else sum[g] += (e0 + e1) + (e2 + e3);
        }
    };
    if constexpr (PRUNE) {
        // 64 tiles per visit mask; inside a batch the kept tiles are processed two at a time with ping-pong fragment buffers
        auto run_batch = [&](int64_t tb, unsigned long long mask, auto blind) {
            constexpr int BMODE = decltype(blind)::value;   // 0: checked, 1: blind, 2: blind and without the clamp of exp2_magic (GUARDP)
            constexpr bool BLIND = BMODE != 0;
            // The prefetch of the next kept tile is UNCONDITIONAL (after the last one the current tile is simply loaded again):
            // with `if (mask) load` the two paths into the next MFMA differ in their number of loads in flight, and the compiler
            // must wait for ALL of them (s_waitcnt vmcnt(0)) - i.e. for the prefetch it has just issued - before every tile.
            int b = __builtin_ctzll(mask);
            mask &= mask - 1;
            load_tile(tb + b, afA, nxA, axA);
            for (;;) {
                const bool more = mask != 0;
                const int b2 = more ? __builtin_ctzll(mask) : b;
                mask &= mask - 1;
                load_tile(tb + b2, afB, nxB, axB);
                if constexpr (BLIND) process_fast(afA, nxA, b, std::integral_constant<int, BMODE == 2 ? 0 : 1>{}); else process_tile(tb + b, afA, nxA, axA, b);
                if (!more) break;
                const bool more2 = mask != 0;
                const int b3 = more2 ? __builtin_ctzll(mask) : b2;
                mask &= mask - 1;
                load_tile(tb + b3, afA, nxA, axA);
                if constexpr (BLIND) process_fast(afB, nxB, b2, std::integral_constant<int, BMODE == 2 ? 0 : 1>{}); else process_tile(tb + b2, afB, nxB, axB, b2);
                if (!more2) break;
                b = b3;
            }
        };
        // fp64 plain sweeps take a batch blind first (the offsets start from the prepass bounds: an overflow needs a term 896
        // exponent units above its query's bound) and redo it with the checked loop from the saved sums if a sum went bad
        // (WMUL: the weights ride in the FMA chain that runs into the running sum, as in the unpruned sweep; a NaN weight - rows beyond
        // -1/2|z|^2 = -1000 - and 2^x' = inf or NaN from a huge z_t.z_q both leave the batch's sum NaN or infinite, and the redo takes the batch
        // through process_tile, whose bad tiles add the norms back and take the classic exponents)
        constexpr bool FASTP = PBN_SWEEP_UNCHECKED && !COND && sizeof(T) == 8 && (FOLD || WMUL || KS == 1);   // the shapes that stay <= 168 VGPRs
        {
            bool count_tiles = a.count_redo && lane == 0;
            if constexpr (PDFIX != 0) count_tiles = count_tiles && a.live_mask == nullptr;   // (with masks the screen counted them)
            if (count_tiles) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0) * QG);
        }
        // Two levels: a SUPER-BATCH of 64 batches (4096 tiles) is classified first, lane = batch, against the batches' own boxes (grouped
        // sweeps: GSweepUnit::batch_box) - one round trip to L2 for 64 batches instead of one per batch, which is what the walk over a
        // split's tiles costs where most batches hold nothing for the wave (the test below is latency, not arithmetic).
        constexpr bool JOINT = GMASK && !FARP && PDFIX != 0;   // prune_group_masks_joint
        // SCR (round 11, the d = 8 shape): with SweepArgs::live_mask the visit masks were prepared by kde_screen_d8_kernel - the box masks less the
        // blocks its f16 exponents prove dead.  A super-batch's masks are loaded lane = batch with one 16-byte load (lv) and a batch takes its own
        // from there with v_readlane: no box test and no memory round trip inside the walk.  Without the pointer the kernel walks as before.
        constexpr bool SCR = GMASK && WMUL && KS == 2 && PDFIX != 0 && QG == 2;
        // (every use below sits under `if constexpr (SCR)`: the other shapes of this body compile to the code they had without it)
        bool scr = false;
        unsigned long long lv[SCR ? QG : 1];
        int jl = 0;   // the lane that holds the current batch's words
        if constexpr (SCR) {
            scr = a.live_mask != nullptr;
#pragma unroll
            for (int g = 0; g < QG; ++g) lv[g] = 0;
        }
        auto do_batch = [&](const int64_t tb, const unsigned gsel, const bool bare) -> bool {   // true: the batch was redone checked
            unsigned long long mask = 0;
            // (QLDS: the boxes are read from LDS where they are used - without this compiler barrier the reads are hoisted out of the walk and the
            // boxes of both groups, 2 x pd x QG doubles, live in vector registers from the first batch to the last)
            if constexpr (QLDS) asm volatile("" ::: "memory");
            if constexpr (GMASK) {
                mask = 0;
                bool taken = false;
                if constexpr (SCR) {
                    if (scr) {
#pragma unroll
                        for (int g = 0; g < QG; ++g) {
                            const unsigned lo = __builtin_amdgcn_readlane((unsigned)lv[g], jl), hi = __builtin_amdgcn_readlane((unsigned)(lv[g] >> 32), jl);
                            gm[g] = ((unsigned long long)hi << 32) | lo;
                            mask |= gm[g];
                        }
                        taken = true;
                    }
                }
                if (taken) {
                } else if (JOINT && gmasks && gsel == (1u << QG) - 1u) {   // in reach of every group of the wave: one pass over the tile boxes
                    decltype(qbox_of(0, 0)) qb[QG];
                    double thr[QG];
#pragma unroll
                    for (int g = 0; g < QG; ++g) {
                        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
                        qb[g] = qbox_of(g, qt);
                        thr[g] = thr_of(g, qt);
                    }
                    prune_group_masks_joint<PDW, QG>(TBp, qb, pd, tb, t1, thr, lane, gm);
#pragma unroll
                    for (int g = 0; g < QG; ++g) mask |= gm[g];
                } else if (gmasks) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) {
                        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
                        if (!((gsel >> g) & 1u)) {   // the whole batch beyond this group's reach
                            gm[g] = 0;
                            if constexpr (FARP) gn[g] = ~0ull;
                            continue;
                        }
                        if constexpr (FARP) {
                            if constexpr (MOM) {   // the moment pass takes the pairs it can expand: this sweep skips them
                                unsigned long long mx;
                                gm[g] = prune_group_mask3<PDW>(TBp, QBp + qt * 2 * pd, (const PBN_GLOBAL float*)a.tile_rad2, pd, tb, t1, QTp[qt] - a.prune_margin,
                                                                  a.far_span > 0.0 ? QTp[qt] - (a.prune_margin - a.far_span) : -INFINITY,
                                                                  QTp[qt] - (a.prune_margin + PBN_MOM_EXTRA), lane, gn[g], mx);
                                gm[g] &= ~mx;
                            } else if (a.far_span > 0.0) {
                                gm[g] = prune_group_mask2<PDW>(TBp, QBp + qt * 2 * pd, pd, tb, t1, QTp[qt] - a.prune_margin, QTp[qt] - (a.prune_margin - a.far_span), lane, gn[g]);
                            } else {
                                gm[g] = prune_group_mask<PDW>(TBp, QBp + qt * 2 * pd, pd, tb, t1, QTp[qt] - a.prune_margin, lane);
                                gn[g] = ~0ull;
                            }
                        } else {
                            gm[g] = prune_group_mask<PDW>(TBp, qbox_of(g, qt), pd, tb, t1, thr_of(g, qt), lane);
                        }
                        mask |= gm[g];
                    }
                } else if constexpr (WBOX) {
                    mask = prune_visit_mask(TBp, pd, tb, t1, wlo, whi, wthr, lane);
#pragma unroll
                    for (int g = 0; g < QG; ++g) gm[g] = mask;
                    if constexpr (FARP) {
#pragma unroll
                        for (int g = 0; g < QG; ++g) gn[g] = ~0ull;
                    }
                }
            } else if constexpr (WBOX) {
                mask = prune_visit_mask(TBp, pd, tb, t1, wlo, whi, wthr, lane);
            }
            if (!mask) return false;
            bool count_visits = a.count_redo && lane == 0;
            if constexpr (SCR) count_visits = count_visits && !scr;   // (the screen counted the blocks that pass the box test)
            if (count_visits) {
                unsigned long long v = 0;
#pragma unroll
                for (int g = 0; g < QG; ++g) v += (unsigned long long)__builtin_popcountll(GMASK ? gm[g] : mask);
                atomicAdd(&g_sweep_visit, v);   // (tile, group) pairs visited, out of QG x tiles offered
            }
            if constexpr (FASTP) {
                double saved[QG];
#pragma unroll
                for (int g = 0; g < QG; ++g) saved[g] = sum[g];
                // a proven batch runs the blind loop without the clamp, any other (2-3 % on the bench tables: wide batch boxes, the last tile and
                // the last query tile of a unit, query groups whose offsets lie beyond -890) the SAME loop with it: the same instructions but one,
                // the same order of additions, the far tiles' fp32 tail in both - a batch's sum does not depend on whether it was proven
                // (PBN_MAGIC_GUARD=0 takes every batch through the second: bit-identical scores, tests/test_magic_exp2_gpu.py)
                if ((GUARDP || GUARDW) && bare) run_batch(tb, mask, std::integral_constant<int, 2>{});
                else run_batch(tb, mask, std::integral_constant<int, 1>{});
                if constexpr (FARP) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) { sum[g] += (double)fs[g]; fs[g] = 0.f; }   // (an overflowed fp32 tail arrives as inf: the batch is redone)
                }
                bool bad = false;
#pragma unroll
                for (int g = 0; g < QG; ++g) bad = bad || !(sum[g] < 0x1p1000);
                const bool redo = __any(bad);
                if (a.count_redo && lane == 0) { atomicAdd(&g_sweep_units, 1ull); if (redo) atomicAdd(&g_sweep_redo, 1ull); }
                if (redo) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) sum[g] = saved[g];
                    run_batch(tb, mask, std::integral_constant<int, 0>{});
                }
                return redo;
            } else {
                run_batch(tb, mask, std::integral_constant<int, 0>{});
                return false;
            }
        };
        for (int64_t sb = t0; sb < t1; sb += 4096) {
            const int64_t bt = sb + 64 * lane;   // my batch's first tile
            if constexpr (QLDS) asm volatile("" ::: "memory");
            unsigned long long bm = __ballot(bt < t1), bmg[QG];
            unsigned long long bopen = ((GUARDP || GUARDW) && bboxes) ? ~0ull : 0ull;
#pragma unroll
            for (int g = 0; g < QG; ++g) bmg[g] = bm;
            if constexpr (GMASK) {
                if (bboxes) {
                    const PBN_GLOBAL double* bb = (const PBN_GLOBAL double*)a.batch_box + ((int64_t)split * a.batches_per_split + ((bt - t0) >> 6)) * 2 * pd;
                    bm = 0;
                    if constexpr (SCR) {
                      if (scr) {
                        if (bt < t1) {
                            const PBN_GLOBAL unsigned long long* lp = (const PBN_GLOBAL unsigned long long*)a.live_mask +
                                                                      (((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split + ((bt - t0) >> 6)) * QG;
#pragma unroll
                            for (int g = 0; g < QG; ++g) lv[g] = lp[g];
                            if (a.far_mask) {   // round 16: the far blocks are kde_sweep_far32_d8_kernel's
                                const PBN_GLOBAL unsigned long long* fp = (const PBN_GLOBAL unsigned long long*)a.far_mask + (lp - (const PBN_GLOBAL unsigned long long*)a.live_mask);
#pragma unroll
                                for (int g = 0; g < QG; ++g) lv[g] &= ~fp[g];
                            }
                        } else {
#pragma unroll
                            for (int g = 0; g < QG; ++g) lv[g] = 0;
                        }
                      }
                    }
#pragma unroll
                    for (int g = 0; g < QG; ++g) {
                        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
                        bool reach_known = false;
                        if constexpr (SCR) {
                            if (scr) { bmg[g] = __ballot(lv[g] != 0); reach_known = true; }
                        }
                        if (!reach_known) bmg[g] = __ballot(bt < t1 && batch_in_reach<PDW>(bb, qbox_of(g, qt), pd, thr_of(g, qt)));
                        bm |= bmg[g];
                        // open for the wave = proven for every group that reaches the batch (the batch with the table's last tile - padding
                        // rows, whose norm slot is not a distance - never)
                        if constexpr (GUARDP) bopen &= ~bmg[g] | (gate_of(g) ? __ballot(bt + 64 < a.ntiles && batch_all_near<PDW>(bb, QBp + qt * 2 * pd, pd)) : 0ull);
                        if constexpr (GUARDW) {
                            unsigned long long ob = 0;
                            if (gate_w(g)) {
                                double mlo = (double)m[g], mhi = mlo;   // over the group's 16 queries (the four row-lanes of a column hold the same offset)
#pragma unroll
                                for (int o = 1; o < 16; o <<= 1) {
                                    const double l = __shfl_xor(mlo, o), h = __shfl_xor(mhi, o);
                                    mlo = l < mlo ? l : mlo;
                                    mhi = h > mhi ? h : mhi;
                                }
                                ob = __ballot(bt + 64 < a.ntiles && batch_bare_wmul<PDW>(bb, qbox_of(g, qt), pd, 1021.0 - (double)Tr<T>::bias() + mlo, 1021.0 + (double)Tr<T>::bias() - mhi));
                            }
                            bopen &= ~bmg[g] | ob;
                        }
                    }
                }
            }
            while (bm) {
                const int j = __builtin_ctzll(bm);
                bm &= bm - 1;
                unsigned gsel = 0;
#pragma unroll
                for (int g = 0; g < QG; ++g) gsel |= (unsigned)((bmg[g] >> j) & 1ull) << g;
                if constexpr (SCR) jl = j;
                const bool redone = do_batch(sb + 64 * (int64_t)j, gsel, (GUARDP || GUARDW) && ((bopen >> j) & 1ull));
                if constexpr (GUARDW) { if (redone) bopen = 0; } else (void)redone;
            }
        }
    } else {
        // Unchecked passes (fp64 plain sweeps): the per-(tile, group) overflow test and the separate add into the running sum are
        // 2 of the 42 DP instructions.  2^x overflows only when an exponent lies 896 above the offsets (a query whose neighbours
        // are ~25 bandwidths closer than the rows that set its offset) or, with the norms as weights, when z_t.z_q alone is
        // that large (a far-out row next to a far-out query; rows beyond |z|^2 = 2000 carry a NaN weight on purpose).  So the
        // sums are accumulated blind (weights riding in the FMA chain, or plain adds) and looked at once per chunk of 32 tiles:
        // a wave that finds an infinite / NaN sum restores the sums it saved in LDS at the start of the chunk and redoes the
        // chunk with the checked loop - 32 tiles, not the split: an outlier row costs its chunk, not every query block of its
        // split (measured with whole-split redo on the C2 data, whose diagonal bandwidths leave 5 rows beyond |z|^2 = 1780: 12 % of
        // the units redone, all on the XCDs that own those splits - 76 ms instead of 50).
        // (only where the second loop body leaves the kernel at 3 waves / SIMD: <= 168 VGPRs)
        constexpr bool FAST = PBN_SWEEP_UNCHECKED && !COND && sizeof(T) == 8 && (WMUL || (FOLD && KS <= 3) || (!FOLD && KS <= 2));
        auto checked_range = [&](int64_t ta, int64_t tb) {
            load_tile(ta, afA, nxA, axA);
            for (int64_t t = ta; t < tb; t += 2) {
                const bool second = t + 1 < tb;                       // wave-uniform
                load_tile(second ? t + 1 : t, afB, nxB, axB);
                process_tile(t, afA, nxA, axA, 0);
                load_tile(t + 2 < tb ? t + 2 : t, afA, nxA, axA);
                if (second) process_tile(t + 1, afB, nxB, axB, 0);
            }
        };
        if constexpr (FAST) {
            constexpr int CH = 32;
            __shared__ double sumsave[QG][256];
            // GUARD (round 6, MAGIC sweeps): exp2_magic WITHOUT its clamp - 5 instructions per value - for the chunks whose exponents are proven
            // inside +-1022 before they are computed.  With R = sqrt(max -norm) over the chunk's rows (SweepArgs::tile_r) and, per query, NQ =
            // -norm and a = the accumulator's constant (norm - offset + bias), Cauchy-Schwarz gives |z_t.z_q| <= 2 R sqrt(NQ) in exponent units:
            //   WMUL (x = z_t.z_q + a):                      |x| <= 1022  <=  R <= min(1022 - a, 1022 + a) / (2 sqrt(NQ))
            //   norms in the accumulator (x = a + NQ - d2/2): x <= a + NQ <= 1022 and x >= a + NQ - (R + sqrt(NQ))^2 >= -1022
            //                                                              <=  R <= sqrt(1022 + a + NQ) - sqrt(NQ)
            // rlim = the smallest such bound over the wave's queries (recomputed when a checked redo moves the offsets); a chunk is taken
            // unclamped when every one of its tiles has tile_r <= rlim.  Inside the bound the clamped and the unclamped form are the same
            // function: which chunks pass changes the time, not a bit of the result.
            constexpr bool GUARD = MAGIC && PBN_MAGIC_GUARD;
            const PBN_GLOBAL double* __restrict__ TRp = (const PBN_GLOBAL double*)a.tile_r;
            double rlim = -1.0;
            auto set_rlim = [&]() {
                double lim = INFINITY;
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    const double aq = (double)(cm[g] - Tr<T>::magic()), nq = -(double)ny[g];
                    const double sq = __builtin_sqrt(nq);
                    double l;
                    if (WMUL) {
                        const double h = aq < 0.0 ? 1022.0 + aq : 1022.0 - aq;
                        l = sq > 0.0 ? 0.5 * h / sq : (h >= 0.0 ? INFINITY : -1.0);
                    } else {
                        const double top = aq + nq;
                        l = top <= 1022.0 ? __builtin_sqrt(1022.0 + top) - sq : -1.0;
                    }
                    lim = l < lim ? l : lim;   // (a NaN bound - NaN queries - never lowers the limit: their sums are NaN whatever the path)
                    if (!(l == l)) lim = -1.0;
                }
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) { const double v = __shfl_xor(lim, o); lim = v < lim ? v : lim; }
                rlim = lim;
            };
            if constexpr (GUARD) { if (TRp) set_rlim(); }
            for (int64_t tc = t0; tc < t1; tc += CH) {
                const int64_t te = tc + CH < t1 ? tc + CH : t1;
#pragma unroll
                for (int g = 0; g < QG; ++g) sumsave[g][threadIdx.x] = sum[g];
                bool open = false;
                unsigned omask = 0;   // bit i: tile tc + i is proven (a chunk with an outlier row keeps its other tiles bare)
                if constexpr (GUARD) {
                    if (TRp) {
                        const int64_t tt = tc + lane < te ? tc + lane : te - 1;
                        const unsigned long long ob = __ballot(lane < CH && TRp[tt] <= rlim);
                        omask = (unsigned)ob;
                        open = omask == 0xffffffffu;
                    }
                }
                // (measurement aid: tiles taken without the clamp / tiles, through pbn_debug_sweep_visits)
                if (GUARD && a.count_redo && lane == 0) { atomicAdd(&g_sweep_tiles, (unsigned long long)(te - tc)); atomicAdd(&g_sweep_visit, (unsigned long long)__builtin_popcount(omask & (te - tc >= 32 ? ~0u : ((1u << (te - tc)) - 1u)))); }
                load_tile(tc, afA, nxA, axA);
                if (open) {
                    for (int64_t t = tc; t < te; t += 2) {
                        const bool second = t + 1 < te;                   // wave-uniform
                        load_tile(second ? t + 1 : t, afB, nxB, axB);
                        process_fast(afA, nxA, 0, std::integral_constant<int, 0>{});
                        load_tile(t + 2 < te ? t + 2 : t, afA, nxA, axA);
                        if (second) process_fast(afB, nxB, 0, std::integral_constant<int, 0>{});
                    }
                } else {
                    for (int64_t t = tc; t < te; t += 2) {
                        const bool second = t + 1 < te;                   // wave-uniform
                        const unsigned ob = omask >> (unsigned)(t - tc);
                        load_tile(second ? t + 1 : t, afB, nxB, axB);
                        if (ob & 1u) process_fast(afA, nxA, 0, std::integral_constant<int, 0>{});
                        else process_fast(afA, nxA, 0, std::integral_constant<int, 1>{});
                        load_tile(t + 2 < te ? t + 2 : t, afA, nxA, axA);
                        if (second) {
                            if (ob & 2u) process_fast(afB, nxB, 0, std::integral_constant<int, 0>{});
                            else process_fast(afB, nxB, 0, std::integral_constant<int, 1>{});
                        }
                    }
                }
                bool bad = false;
#pragma unroll
                for (int g = 0; g < QG; ++g) bad = bad || !(sum[g] < 0x1p1000);   // not merely finite: the epilogue adds 4 lanes' sums
                const bool redo = __any(bad);
                if (a.count_redo && lane == 0) { atomicAdd(&g_sweep_units, 1ull); if (redo) atomicAdd(&g_sweep_redo, 1ull); }
                if (redo) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) sum[g] = sumsave[g][threadIdx.x];
                    checked_range(tc, te);
                    if constexpr (GUARD) { if (TRp) set_rlim(); }   // the offsets may have moved
                }
            }
        } else {
            checked_range(t0, t1);
        }
    }

    // ---- epilogue: combine the 4 row-lanes of each query column, write (m, sum) partials ---------
    PBN_GLOBAL double* part = (PBN_GLOBAL double*)a.part;
    constexpr int P = COND ? 4 : 2;
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        double s = sum[g];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        double sj = 0.0;
        if (COND) {
            sj = sumj[g];
            sj += __shfl_xor(sj, 16);
            sj += __shfl_xor(sj, 32);
        }
        // an empty sum still holds the term its offset came from (see kde_sweep_f16_kernel; 2^bias is that term here)
        // (only when the offset is a real exponent: a NaN / infinite offset - NaN queries, an all-padding split - keeps its sum)
        const bool mfin = (m[g] - m[g]) == (T)0;
        // (not with a moment pass beside this sweep: the tile the offset came from may be the other pass's - an empty sum is empty)
        if (s == 0.0 && mfin && !lbm[g] && !MOM) s = __builtin_ldexp(1.0, (int)Tr<T>::bias());
        if (COND && sj == 0.0 && (mj[g] - mj[g]) == (T)0 && !lbmj[g]) sj = __builtin_ldexp(1.0, (int)Tr<T>::bias());
        if (lg == 0 && qt0 + g < a.nqtiles) {
            PBN_GLOBAL double* o = part + ((int64_t)split * a.nqtiles * 16 + (qt0 + g) * 16 + lane) * P;
            o[0] = (double)m[g] - (double)Tr<T>::bias();   // the sums carry 2^bias
            o[1] = s;
            if (COND) { o[2] = (double)mj[g] - (double)Tr<T>::bias(); o[3] = sj; }
        }
    }
}

template <typename T, int KS, bool COND, int QG, bool FOLD, bool PRUNE, bool WMUL = false, bool EF32 = false>
__global__ __launch_bounds__(sweep_block_threads(PRUNE), PRUNE ? PBN_F64_PRUNE_WAVES : 2) void kde_sweep_kernel(SweepArgs a) {
    kde_sweep_body<T, KS, COND, QG, FOLD, PRUNE, WMUL, EF32>(a, blockIdx.x);
}
// The pruned sum-only sweep of d = 8 models on boxes over all eight rotated dimensions (bench.py's headline):
// kde_sweep_kernel<double, 2, false, PBN_QG_PRUNE, false, true, true, true> with the number of box dimensions at compile time (PDFIX)
__global__ __launch_bounds__(sweep_block_threads(true), PBN_F64_PRUNE_WAVES) void kde_sweep_pruned_d8_kernel(SweepArgs a) {
    kde_sweep_body<double, 2, false, PBN_QG_PRUNE, false, true, true, true, false, PBN_PRUNE_PD, PBN_PRUNE_PD>(a, blockIdx.x);
}

// Grouped launch (kde_group.hip): the flat grid covers the sweeps of MANY units back to back, unit-major, every unit's share
// rounded up to 64 workgroups so that one table entry per 64 workgroups names the unit.  Pruned plain fp64 sweeps only.
// (four waves per SIMD here, three for the stand-alone launches: the grouped sweeps spend more of their time in the tile walk, whose latency a
//  fourth wave covers - cv64 2.25 -> 2.19 s, C3 with 24 iterations 26.66 -> 26.04 s; the stand-alone handles lose 2-5 % at four, tools/r5_probe_q.sh)
#ifndef PBN_F64_GROUP_WAVES
#define PBN_F64_GROUP_WAVES 4
#endif
template <typename T, int KS, int QG, bool FOLD, bool WMUL, bool MOM = false>
__global__ __launch_bounds__(sweep_block_threads(true), PBN_F64_GROUP_WAVES) void kde_sweep_group_kernel(GSweepArgs g) {
    const int u = g.wg_unit[blockIdx.x >> 6];
    const GSweepUnit& su = g.units[u];
    const unsigned bid = (unsigned)((int64_t)blockIdx.x - su.wg0);
    if (bid >= (unsigned)su.nwg) return;
    SweepArgs a;
    a.Apack = su.Apack; a.nxpack = su.nxpack; a.Axpack = nullptr;
    a.Bpack = su.Bpack; a.nypack = su.nypack; a.Bxpack = nullptr; a.Bxnorm = nullptr;
    a.ntiles = su.ntiles; a.nqtiles = su.nqtiles; a.tiles_per_split = su.tps;
    a.fold = g.fold; a.count_redo = g.count_redo; a.wmul = g.wmul; a.box_full = su.box_full; a.tile_r = nullptr;
    a.prune = 1; a.pdims = su.pdims; a.prune_margin = g.prune_margin > 0.0 ? g.prune_margin : (double)su.margin;
    a.tile_box = su.tile_box; a.qtile_box = su.qtile_box; a.qtile_thr = su.qtile_thr; a.qlb = su.qlb;
    a.nsplit_grid = su.nsplit; a.part = su.part; a.group_masks = g.group_masks;
    a.far_span = g.far_span;
    a.tile_rad2 = su.tile_rad2; a.tile_mom = su.tile_mom; a.batch_box = su.batch_box; a.batches_per_split = su.nbps;
    kde_sweep_body<T, KS, false, QG, FOLD, true, WMUL, /*EF32: the engine's terms are sums*/ true, MOM, PBN_PRUNE_PD_NARROW>(a, bid);
}

// one launch site of kde_sweep_kernel: the plain fp64 shapes exist twice - FAST (SweepArgs::fast: the sweep's result is a sum over the
// test rows) and exact-polynomial (per-row logl outputs); CKDE-fused and fp32 shapes only in the second form
#define PBN_LAUNCH_SWEEP(KSv, CONDv, QGv, FOLDv, PRUNEv, WMULv)                                                                            \
    do {                                                                                                                                 \
        if constexpr (sizeof(T) == 8 && !(CONDv)) {                                                                                      \
            if (a.fast) {                                                                                                                \
                hipLaunchKernelGGL((kde_sweep_kernel<T, KSv, CONDv, QGv, FOLDv, PRUNEv, WMULv, true>), grid, block, 0, st, a);             \
                break;                                                                                                                   \
            }                                                                                                                            \
        }                                                                                                                                \
        hipLaunchKernelGGL((kde_sweep_kernel<T, KSv, CONDv, QGv, FOLDv, PRUNEv, WMULv, false>), grid, block, 0, st, a);                    \
    } while (0)

template <typename T, bool COND, bool FOLD>
static void launch_sweep_tf(const SweepArgs& a, int KS, dim3 grid, hipStream_t st) {
    constexpr int QG = SweepQG<sizeof(T) == 8, COND>::value;
    dim3 block(256);
    if (a.prune) {   // fp64, at most 6 marginal dimensions (KS <= 2)
        if constexpr (sizeof(T) == 8) {
            constexpr int QGP = COND ? PBN_QG_PRUNE_COND : PBN_QG_PRUNE;   // query groups per wave of the pruned kernels
            block = dim3(sweep_block_threads(true));
            grid = dim3((unsigned)(ceil_div(a.nqtiles, QGP) * a.nsplit_grid));   // one wave per workgroup, placed by pruned_block
#ifndef PBN_EXPERIMENTS
            // the plain pruned fp64 kernels are compiled for per-group masks and batch boxes (kde_sweep_body: gmasks / bboxes)
            if (!COND && (!a.group_masks || !a.batch_box)) throw invalid_error("KDE: pruned fp64 sweeps need per-group masks and batch boxes");
#endif
            if constexpr (!COND && !FOLD) {
                if (a.wmul && KS <= 2) {   // 4 / 8 marginal dimensions: the pruned shapes without a free K slot
                    if (KS == 1) PBN_LAUNCH_SWEEP(1, false, QGP, false, true, true);
                    // the sum-only d = 8 sweep on boxes over all eight (rotated) dimensions - the headline shape: pd at compile time (PDFIX)
                    else if (a.fast && a.pdims == PBN_PRUNE_PD) hipLaunchKernelGGL(kde_sweep_pruned_d8_kernel, grid, block, 0, st, a);
                    else PBN_LAUNCH_SWEEP(2, false, QGP, false, true, true);
                    HIP_CHECK(hipGetLastError());
                    return;
                }
            }
            if (KS == 1) PBN_LAUNCH_SWEEP(1, COND, QGP, FOLD, true, false);
            else if (KS == 2) PBN_LAUNCH_SWEEP(2, COND, QGP, FOLD, true, false);
            else throw invalid_error("KDE: pruned sweeps cover at most 8 whitened dimensions");
            HIP_CHECK(hipGetLastError());
            return;
        } else {
            throw invalid_error("KDE: pruned sweeps are fp64 only");
        }
    }
    if constexpr (sizeof(T) == 8 && !COND && !FOLD) {
        if (a.wmul) {
            switch (KS) {
                case 1: PBN_LAUNCH_SWEEP(1, false, QG, false, false, true); break;
                case 2: PBN_LAUNCH_SWEEP(2, false, QG, false, false, true); break;
                default: throw invalid_error("KDE: weighted-norm sweeps cover at most 8 whitened dimensions");
            }
            HIP_CHECK(hipGetLastError());
            return;
        }
    }
    if constexpr (sizeof(T) == 8 && !FOLD) {   // 17-32 dimensions: fp64, norms added per value, two query groups per wave (sweep_qg)
        switch (KS) {
            case 5: PBN_LAUNCH_SWEEP(5, COND, 2, false, false, false); HIP_CHECK(hipGetLastError()); return;
            case 6: PBN_LAUNCH_SWEEP(6, COND, 2, false, false, false); HIP_CHECK(hipGetLastError()); return;
            case 7: PBN_LAUNCH_SWEEP(7, COND, 2, false, false, false); HIP_CHECK(hipGetLastError()); return;
            case 8: PBN_LAUNCH_SWEEP(8, COND, 2, false, false, false); HIP_CHECK(hipGetLastError()); return;
            default: break;
        }
    }
    switch (KS) {
        case 1: PBN_LAUNCH_SWEEP(1, COND, QG, FOLD, false, false); break;
        case 2: PBN_LAUNCH_SWEEP(2, COND, QG, FOLD, false, false); break;
        case 3: PBN_LAUNCH_SWEEP(3, COND, QG, FOLD, false, false); break;
        case 4: PBN_LAUNCH_SWEEP(4, COND, QG, FOLD, false, false); break;
        default: throw invalid_error("KDE: this many whitened dimensions per sweep are not supported for the table's type");
    }
    HIP_CHECK(hipGetLastError());
}
template <typename T, bool COND>
static void launch_sweep_t(const SweepArgs& a, int KS, dim3 grid, hipStream_t st) {
    if (a.fold) launch_sweep_tf<T, COND, true>(a, KS, grid, st); else launch_sweep_tf<T, COND, false>(a, KS, grid, st);
}

// The fp32 sweeps on the 16-bit matrix cores are compiled as part of this unit.  Built apart, the pruned kernels of BOTH families come out with
// another instruction schedule (the order in which the compiler emits the inline helpers the two share changes with what else the unit
// instantiates, and the optimiser's result follows it): one unit keeps every kernel's code what the measurements were taken on.
#include "kde_sweep_f16.inc"
// ... and so is the f16 screen of the pruned d = 8 sweep: it counts into this unit's g_sweep_visit / g_sweep_tiles
#include "kde_screen_d8.inc"
// ... and the far pass behind it (round 16)
#include "kde_far32_d8.inc"

void launch_pack(const PackArgs& a, int dtype, hipStream_t st) {
    const int64_t npad = a.ntiles * 16;
    if (npad == 0) return;
    dim3 grid((unsigned)ceil_div(npad, 256)), block(256);
    if (use_f16x2(dtype)) {
        hipLaunchKernelGGL(pack_rows_f16_kernel, grid, block, 0, st, a);
        HIP_CHECK(hipGetLastError());
        return;
    }
    launch_pack_classic(a, dtype, st);
}

void launch_sweep(const SweepArgs& a_in, int dtype, int KS, bool cond, int nsplit, hipStream_t st) {
    SweepArgs a = a_in;
    a.nsplit_grid = nsplit;
    dim3 grid((unsigned)ceil_div(a.nqtiles, 4 * sweep_qg(dtype, cond, KS, a.prune != 0)), (unsigned)nsplit);
    if (use_f16x2(dtype)) {  // KS carries the number of 32-slot f16 MFMAs
        if (cond) launch_sweep_f16<true>(a, KS, grid, st); else launch_sweep_f16<false>(a, KS, grid, st);
        return;
    }
    if (dtype == PBN_F64) {
        if (cond) launch_sweep_t<double, true>(a, KS, grid, st); else launch_sweep_t<double, false>(a, KS, grid, st);
    } else {
        if (cond) launch_sweep_t<float, true>(a, KS, grid, st); else launch_sweep_t<float, false>(a, KS, grid, st);
    }
}

// fold: d mod 4 != 0 (norm in a free K slot); wmul: d mod 4 == 0 (norms as weights) - the two pruned plain fp64 shapes
void launch_sweep_grouped(const GSweepArgs& g, int dtype, int KS, hipStream_t st) {
    if (g.total_wg == 0) return;
    if (g.total_wg > 0x7fffffffll) throw invalid_error("grouped sweeps: grid too large");
    const dim3 grid((unsigned)g.total_wg), block(sweep_block_threads(true));
    if (use_f16x2(dtype)) {   // KS carries the number of 32-slot f16 MFMAs
        if (KS == 1 && g.w32) { ++g_w32_launches; hipLaunchKernelGGL((kde_sweep_f16_w32p_group_kernel<1>), grid, block, 0, st, g); }
        else if (KS == 1) hipLaunchKernelGGL((kde_sweep_f16_group_kernel<1>), grid, block, 0, st, g);
        else if (KS == 2) hipLaunchKernelGGL((kde_sweep_f16_group_kernel<2>), grid, block, 0, st, g);
        else throw invalid_error("grouped fp32 sweeps: at most 10 whitened dimensions");
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (dtype != PBN_F64 || KS < 1 || KS > 2 || (g.fold != 0) == (g.wmul != 0)) throw invalid_error("grouped sweeps: fp64 / fp32 on the f16 cores, at most 8 whitened dimensions");
#ifndef PBN_EXPERIMENTS
    if (!g.group_masks) throw invalid_error("grouped fp64 sweeps are compiled for per-group masks");   // (kde_sweep_body: gmasks)
#endif
    constexpr int QGP = PBN_QG_PRUNE;
    if (g.fold) {
        if (g.moments && (KS != 1 || !g.group_masks)) throw invalid_error("grouped sweeps: the moment pass stands beside one- and two-variable units with per-group masks");
        if (KS == 1 && g.moments) hipLaunchKernelGGL((kde_sweep_group_kernel<double, 1, QGP, true, false, true>), grid, block, 0, st, g);
        else if (KS == 1) hipLaunchKernelGGL((kde_sweep_group_kernel<double, 1, QGP, true, false>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((kde_sweep_group_kernel<double, 2, QGP, true, false>), grid, block, 0, st, g);
    } else {
        if (KS == 1) hipLaunchKernelGGL((kde_sweep_group_kernel<double, 1, QGP, false, true>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((kde_sweep_group_kernel<double, 2, QGP, false, true>), grid, block, 0, st, g);
    }
    HIP_CHECK(hipGetLastError());
}

}  // namespace pbn

// measurement aid like pbn_debug_sweep_visits: blocks the d = 8 screen kept / blocks it tested (those that pass the box test)
extern "C" void pbn_debug_d8_screen(unsigned long long* kept, unsigned long long* tested, int reset) {
    unsigned long long z = 0;
    if (kept) (void)hipMemcpyFromSymbol(kept, HIP_SYMBOL(pbn::g_screen_kept), sizeof z);
    if (tested) (void)hipMemcpyFromSymbol(tested, HIP_SYMBOL(pbn::g_screen_tested), sizeof z);
    if (reset) { (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_screen_kept), &z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_screen_tested), &z, sizeof z); }
}
// ... and, of the kept blocks, those it marked far for kde_sweep_far32_d8_kernel (counted like the two above: PBN_SWEEP_COUNT_REDO)
extern "C" void pbn_debug_d8_screen_far(unsigned long long* far, int reset) {
    unsigned long long z = 0;
    if (far) (void)hipMemcpyFromSymbol(far, HIP_SYMBOL(pbn::g_screen_far), sizeof z);
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_screen_far), &z, sizeof z);
}
extern "C" void pbn_debug_w32_launches(unsigned long long* n, int reset) {
    if (n) *n = pbn::g_w32_launches.load();
    if (reset) pbn::g_w32_launches.store(0);
}
extern "C" void pbn_debug_sweep_redo(unsigned long long* redo, unsigned long long* units, int reset) {
    unsigned long long z = 0;
    if (redo) (void)hipMemcpyFromSymbol(redo, HIP_SYMBOL(pbn::g_sweep_redo), sizeof z);
    if (units) (void)hipMemcpyFromSymbol(units, HIP_SYMBOL(pbn::g_sweep_units), sizeof z);
    if (reset) { (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_sweep_redo), &z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_sweep_units), &z, sizeof z); }
}
// measurement aid like the above: tiles visited / tiles offered to the waves of the pruned sweeps since the last reset
extern "C" void pbn_debug_sweep_visits(unsigned long long* visited, unsigned long long* tiles, int reset) {
    unsigned long long z = 0;
    if (visited) (void)hipMemcpyFromSymbol(visited, HIP_SYMBOL(pbn::g_sweep_visit), sizeof z);
    if (tiles) (void)hipMemcpyFromSymbol(tiles, HIP_SYMBOL(pbn::g_sweep_tiles), sizeof z);
    if (reset) { (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_sweep_visit), &z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_sweep_tiles), &z, sizeof z); }
}


// test aids, not part of the C ABI header: the rule's numbers (eps at ncap, theta for n rows) and the far pass's launches since the last reset
extern "C" void pbn_debug_far32_rule(double ncap, long long n_train, double* eps, double* theta) {
    if (eps) *eps = pbn::far32_term_error(ncap);
    if (theta) *theta = pbn::far32_theta(n_train);
}
extern "C" void pbn_debug_far32_launches(unsigned long long* n, int reset) {
    if (n) *n = pbn::g_far32_launches.load();
    if (reset) pbn::g_far32_launches.store(0);
}
