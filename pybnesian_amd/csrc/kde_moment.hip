// The tile-moment pass beside the grouped fp64 sum-only sweeps of one- and two-variable units (kde_group.hip), and its counters.
#include "common.hpp"
#include "kde_kernels.hpp"
#include "kde_group.hpp"
#include "kde_device.hpp"

namespace pbn {

// measurement aids, not part of the C ABI header
// moment pass (PBN_SWEEP_COUNT_REDO): pairs taken / (batch, group) passes made
__device__ unsigned long long g_mom_pairs = 0, g_mom_batches = 0, g_mom_visits = 0, g_mom_left = 0;
// always on: (tile, group) pairs the moment pass took, by dimension - one atomic per wave (pbn_debug_moment_totals)
__device__ unsigned long long g_mom_taken[2] = {0, 0};

// The moment pass of a grouped fp64 sum-only sweep of D = 1 or 2 dimensions (round 5).  Same flat grid and the same (unit, query block,
// split) mapping as kde_sweep_group_kernel, a wave owns the same 16-query groups - but here LANE = TILE: per 64-tile batch every lane with a
// pair loads the record of its own tile (structure of arrays: 47 | 10 coalesced loads, once per batch and group that has a pair in it), and the
// 16 queries of the group are taken one after the other - their coordinates and offsets are uniform (v_readlane from the lanes that hold
// them), the tile's coefficients per-lane registers.  Per (tile, query): 2 D + ~19 instructions + 44 | 8 FMAs of the Horner scheme, i.e. ~65
// fp64 issue slots per pair at D = 2 when all 64 lanes hold a pair (measured ~85 cycles at 56-62 busy lanes) against ~180 for the sweep's MFMA +
// 2^f form - and a lane idles only where ITS tile is not this group's (the first forms of this kernel - lane = query with the records through
// scalar loads, then 4 tile slots x 16 queries with per-lane record loads - paid for the union of the wave's groups' tiles resp. for 23 vector
// loads per four tiles: no faster than the sweep).  The exponent of the common factor is split as in the sweep (biased, integer offset from the
// prepass bound) and 2^x takes the sweep's own form (2^f of the fraction on the fp32 unit: the budget's first entry covers it; with the fp64
// polynomial the pass differed from the sweep by the fp32 unit's MEAN error, 1.3e-9 per term).  Running sums per (query, lane) in LDS, one
// cross-lane reduction per group; partials go behind the sweep's own (GSweepUnit::part_mom).
__device__ __forceinline__ double readlane_f64(double v, int l) {   // lane l's value, uniform (two v_readlane_b32 into scalar registers)
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
#ifndef PBN_MOM_WAVES2
#define PBN_MOM_WAVES2 2   // D = 2: 45 coefficients per lane - 3 waves / SIMD (168 VGPRs) spill them
#endif
#ifndef PBN_MOM_UNROLL
#define PBN_MOM_UNROLL 16
#endif
#ifndef PBN_MOM_EXP_F32
#define PBN_MOM_EXP_F32 1
#endif
template <int D>
__global__ __launch_bounds__(64, D == 2 ? PBN_MOM_WAVES2 : 3) void kde_moment_group_kernel(GSweepArgs g) {
    // per (group, query, lane) running sums: in LDS - QG x 16 x 64 doubles per wave (as registers they cost the D = 2 kernel 4 %: 256 VGPRs and
    // scratch, profiles/r6/moment_probes.txt)
    __shared__ double accs[PBN_QG_PRUNE * 16][64];
    const int u = g.wg_unit[blockIdx.x >> 6];
    const GSweepUnit& su = g.units[u];
    const unsigned bid = (unsigned)((int64_t)blockIdx.x - su.wg0);
    if (bid >= (unsigned)su.nwg) return;
    constexpr int QG = PBN_QG_PRUNE;
    constexpr int NC = pbn_mom_coefs(D);
    const int lane = threadIdx.x & 63;
    const unsigned Gq = (unsigned)((su.nqtiles + QG - 1) / QG), Gs = (unsigned)su.nsplit;
    const unsigned kk = bid / Gq;
    const int qx = (int)(bid % Gq);
    const int split = (kk & 1u) ? (int)(Gs - 1 - (kk >> 1)) : (int)(kk >> 1);   // pruned_block's order
    const int64_t qt0 = (int64_t)qx * QG;
    if (qt0 >= su.nqtiles) return;
    const int64_t t0 = (int64_t)split * su.tps;
    const int64_t t1 = (t0 + su.tps < su.ntiles) ? t0 + su.tps : su.ntiles;
    const int pd = su.pdims;
    const int64_t ms = su.mom_stride;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)su.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)su.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)su.qtile_thr;
    const PBN_GLOBAL double* __restrict__ QLp = (const PBN_GLOBAL double*)su.qlb;
    const PBN_GLOBAL float* __restrict__ R2p = (const PBN_GLOBAL float*)su.tile_rad2;
    const PBN_GLOBAL double* __restrict__ MOp = (const PBN_GLOBAL double*)su.tile_mom;
    const PBN_GLOBAL double* __restrict__ ZQp = (const PBN_GLOBAL double*)su.zq;
    const double margin = g.prune_margin > 0.0 ? g.prune_margin : (double)su.margin;
    PBN_GLOBAL double* part = (PBN_GLOBAL double*)su.part_mom;

    // Round 6: the wave's QG query groups share ONE walk over the tiles - a batch's boxes are tested for every group, the records of the lanes
    // that have a pair with ANY of them are loaded once (47 | 10 coalesced loads) and each group's 16 queries run against them: half the record
    // loads and half the exposed load latency per pair at QG = 2 (the kernel spent 28 % of its wave time in s_waitcnt).  Every (query, lane) sum
    // still meets its batches in ascending order: the partials are the ones of the group-by-group form, bit for bit.
    // The groups' 16 queries live in lanes 0..15 (copies in the other lanes): coordinates and the exponent offset - the prepass's lower bound of
    // the query's largest exponent, an integer as in the sweep.  A padding row (bound -inf) gets an offset that kills its terms.
    // (the exponents carry the magic constant of the sweep beside this pass: the same 2^x, exp2_magic - x below is that accumulator form)
    constexpr bool MOMM = PBN_MOM_EXP_F32 && PBN_EXP2_MAGIC && PBN_MAGIC_PRUNED && PBN_EXP2_F32 && PBN_EXP2_DEGREE <= 7;
    constexpr double MOMC = MOMM ? PBN_MAGIC_C : 0.0;
    double mqv[QG], cmv[QG], zv[QG][D], thr[QG];
    bool gok[QG], chk[QG];
#pragma unroll
    for (int gi = 0; gi < QG; ++gi) {
        gok[gi] = qt0 + gi < su.nqtiles;
        const int64_t qg = gok[gi] ? qt0 + gi : qt0;
        const int64_t q = qg * 16 + (lane & 15);
        const double lb = __builtin_ceil(QLp[q]);
        const bool qok = (lb < 0.0 ? -lb : lb) < 0x1p50;
        mqv[gi] = qok ? lb : 0.0;
        cmv[gi] = qok ? (Tr<double>::bias() + MOMC) - lb : -0x1p60;
        // x = -d2 / 2 + cmv <= cmv: a group none of whose queries can reach 900 exponent units (the prepass bound of its largest exponent lies
        // within ~870 units of 0: every query with a training row within 41 bandwidths) runs its 16 queries without the overflow test - one
        // basic block of 16 independent Horner schemes instead of 16 blocks with a branch between them
        chk[gi] = __any(cmv[gi] > 900.0 + MOMC) != 0;
#pragma unroll
        for (int k = 0; k < D; ++k) zv[gi][k] = qok ? ZQp[q * D + k] : 0.0;
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) accs[gi * 16 + qi][lane] = 0.0;
        thr[gi] = QTp[qg];
    }
    unsigned long long taken = 0;
    for (int64_t sb = t0; sb < t1; sb += 4096) {
        // (the sweep's two levels: 64 batches classified at once, lane = batch, then the batches in reach)
        const int64_t bt = sb + 64 * lane;
        unsigned long long bm[QG], bmu = 0;
#pragma unroll
        for (int gi = 0; gi < QG; ++gi) {
            if (su.batch_box) {
                const PBN_GLOBAL double* bb = (const PBN_GLOBAL double*)su.batch_box + ((int64_t)split * su.nbps + ((bt - t0) >> 6)) * 2 * pd;
                bm[gi] = __ballot(gok[gi] && bt < t1 && batch_in_reach<PBN_PRUNE_PD_NARROW>(bb, QBp + (qt0 + (gok[gi] ? gi : 0)) * 2 * pd, pd, thr[gi] - margin));
            } else {
                bm[gi] = __ballot(gok[gi] && bt < t1);
            }
            bmu |= bm[gi];
        }
        while (bmu) {
            const int bj = __builtin_ctzll(bmu);
            const int64_t tb = sb + 64 * (int64_t)bj;
            bmu &= bmu - 1;
            unsigned long long m[QG], mu = 0;
#pragma unroll
            for (int gi = 0; gi < QG; ++gi) {
                m[gi] = 0;
                if ((bm[gi] >> bj) & 1ull) {
                    unsigned long long nr;
                    if (g.count_redo && lane == 0) atomicAdd(&g_mom_visits, 1ull);
                    const unsigned long long kept = prune_group_mask3<PBN_PRUNE_PD_NARROW>(TBp, QBp + (qt0 + gi) * 2 * pd, R2p, pd, tb, t1, thr[gi] - margin,
                                                                      g.far_span > 0.0 ? thr[gi] - (margin - g.far_span) : -INFINITY,
                                                                      thr[gi] - (margin + PBN_MOM_EXTRA), lane, nr, m[gi]);
                    if (g.count_redo && lane == 0 && (kept & ~m[gi])) atomicAdd(&g_mom_left, 1ull);
                    if (g.count_redo && lane == 0 && m[gi]) { atomicAdd(&g_mom_pairs, (unsigned long long)__builtin_popcountll(m[gi])); atomicAdd(&g_mom_batches, 1ull); }
                }
                mu |= m[gi];
                taken += (unsigned long long)__builtin_popcountll(m[gi]);
            }
            if (!mu) continue;
            // my tile's record; a lane without a pair keeps zero coefficients and a centroid 10^10 units away: its polynomial is 0 and its
            // exponent -5e19, whose 2^x is an exact 0 (v_fract_f64 of an integer, the saturated v_cvt_i32_f64, v_ldexp_f64): it adds nothing,
            // without a select per query
            double c[D], cf[NC];
#pragma unroll
            for (int k = 0; k < D; ++k) c[k] = 1e10;
#pragma unroll
            for (int k = 0; k < NC; ++k) cf[k] = 0.0;
            if ((mu >> lane) & 1ull) {
                const PBN_GLOBAL double* __restrict__ rec = MOp + (tb + lane);
#pragma unroll
                for (int k = 0; k < D; ++k) c[k] = rec[(int64_t)k * ms];
#pragma unroll
                for (int k = 0; k < NC; ++k) cf[k] = rec[(int64_t)(D + k) * ms];
            }
#pragma unroll
            for (int gi = 0; gi < QG; ++gi) {
                if (!m[gi]) continue;
                const bool act = (m[gi] >> lane) & 1ull;
                // MASK: some lane holds a record for ANOTHER group of the wave and no pair with this one - its exponent is forced to -5e19 as
                // well (a select per query; not needed while the groups' masks agree, the common case for neighbouring groups)
                auto run = [&](auto checked, auto masked) {
                    constexpr bool CHECK = decltype(checked)::value, MASK = decltype(masked)::value;
#pragma unroll PBN_MOM_UNROLL
                    for (int qi = 0; qi < 16; ++qi) {
                        const double ux = readlane_f64(zv[gi][0], qi) - c[0];
                        double d2 = ux * ux, uy = 0.0;
                        if constexpr (D == 2) { uy = readlane_f64(zv[gi][1], qi) - c[1]; d2 = __builtin_fma(uy, uy, d2); }
                        double x = __builtin_fma(-0.5, d2, readlane_f64(cmv[gi], qi));
                        if constexpr (MASK) x = act ? x : -5e19;
                        if constexpr (CHECK) {
                            while (__builtin_expect(__any(x > 900.0 + MOMC), 0)) {
                                // the offset is a LOWER bound of the query's largest exponent: a far-out query (heavy tails) can sit thousands of
                                // units below a row its short neighbour scan missed.  Rebase the query (uniform: every lane's sum for it, and the
                                // offset it lives with from here on) by a fixed integer number of units
                                accs[gi * 16 + qi][lane] *= 0x1p-512;
                                if ((lane & 15) == qi) { cmv[gi] -= 512.0; mqv[gi] += 512.0; }
                                x = act ? x - 512.0 : -5e19;
                            }
                        }
                        // 2^x as in the sweep this pass stands in for: 2^f of the fraction on the fp32 unit (<= 1.4e-7 of the pair's contribution,
                        // the budget's first entry); x >= 0 for every pair that matters (the biased offset), a negative x comes out <= 2x too large
                        const double e = MOMM ? exp2_magic<true>(x) : PBN_MOM_EXP_F32 ? exp2_f64_fract<true>(x, 0.0) : Tr<double>::ex2_hi(x);
                        double pv;
                        if constexpr (D == 1) {
                            pv = cf[0];
#pragma unroll
                            for (int i = 1; i <= PBN_MOM_ORDER; ++i) pv = __builtin_fma(pv, ux, cf[i]);
                        } else {
                            int k = 0;
                            pv = 0.0;
#pragma unroll
                            for (int j = PBN_MOM_ORDER; j >= 0; --j) {
                                double qj = cf[k++];
#pragma unroll
                                for (int i = PBN_MOM_ORDER - j - 1; i >= 0; --i) qj = __builtin_fma(qj, ux, cf[k++]);
                                pv = __builtin_fma(pv, uy, qj);
                            }
                        }
                        accs[gi * 16 + qi][lane] = __builtin_fma(e, pv, accs[gi * 16 + qi][lane]);
                    }
                };
                if (chk[gi]) run(std::true_type{}, std::true_type{});
                else if (m[gi] != mu) run(std::false_type{}, std::true_type{});
                else run(std::false_type{}, std::false_type{});
            }
        }
    }
    if (lane == 0 && taken) atomicAdd(&g_mom_taken[D - 1], taken);
    // the groups' sums: add the 64 lanes' (tiles') parts per query, lane qi writes query qi
#pragma unroll
    for (int gi = 0; gi < QG; ++gi) {
        if (!gok[gi]) continue;
        double mine = 0.0;
#pragma unroll
        for (int qi = 0; qi < 16; ++qi) {
            double v = accs[gi * 16 + qi][lane];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            if (lane == qi) mine = v;
        }
        if (lane < 16) {
            const int64_t q = (qt0 + gi) * 16 + lane;
            PBN_GLOBAL double* o = part + ((int64_t)split * su.nqtiles * 16 + q) * 2;
            o[0] = mqv[gi] - Tr<double>::bias();   // the sums carry 2^bias, as the sweep's
            o[1] = mine;
        }
    }
}

void launch_moment_grouped(const GSweepArgs& g, int d, hipStream_t st) {
    if (g.total_wg == 0) return;
    const dim3 grid((unsigned)g.total_wg), block(64);
    if (d == 1) hipLaunchKernelGGL(kde_moment_group_kernel<1>, grid, block, 0, st, g);
    else if (d == 2) hipLaunchKernelGGL(kde_moment_group_kernel<2>, grid, block, 0, st, g);
    else throw invalid_error("moment pass: one or two dimensions");
    HIP_CHECK(hipGetLastError());
}

}  // namespace pbn

extern "C" void pbn_debug_moment_visits(unsigned long long* visits) {
    if (visits) (void)hipMemcpyFromSymbol(visits, HIP_SYMBOL(pbn::g_mom_visits), sizeof(unsigned long long));
}
extern "C" void pbn_debug_moment_left(unsigned long long* left, int reset) {
    unsigned long long z = 0;
    if (left) (void)hipMemcpyFromSymbol(left, HIP_SYMBOL(pbn::g_mom_left), sizeof z);
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_mom_left), &z, sizeof z);
}
extern "C" void pbn_debug_moment_totals(unsigned long long* pairs_d1, unsigned long long* pairs_d2, int reset) {
    unsigned long long v[2] = {0, 0}, z[2] = {0, 0};
    (void)hipMemcpyFromSymbol(v, HIP_SYMBOL(pbn::g_mom_taken), sizeof v);
    if (pairs_d1) *pairs_d1 = v[0];
    if (pairs_d2) *pairs_d2 = v[1];
    if (reset) (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_mom_taken), z, sizeof z);
}
extern "C" void pbn_debug_moment_pairs(unsigned long long* pairs, unsigned long long* batches, int reset) {
    unsigned long long z = 0;
    if (pairs) (void)hipMemcpyFromSymbol(pairs, HIP_SYMBOL(pbn::g_mom_pairs), sizeof z);
    if (batches) (void)hipMemcpyFromSymbol(batches, HIP_SYMBOL(pbn::g_mom_batches), sizeof z);
    if (reset) { (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_mom_pairs), &z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_mom_batches), &z, sizeof z); (void)hipMemcpyToSymbol(HIP_SYMBOL(pbn::g_mom_visits), &z, sizeof z); }
}
