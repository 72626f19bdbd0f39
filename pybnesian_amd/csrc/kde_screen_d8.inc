// The f16 screen of the pruned sum-only d = 8 sweep (round 11; part of kde_kernels.hip's translation unit: the sweep counters stay one pair in
// one unit).  kde_sweep_pruned_d8_kernel visits every (tile, group) block whose BOXES come within the group's drop threshold; on the bench table
// 36 % of those blocks hold no pair above the threshold at all - boxes over eight dimensions are wide.  kde_screen_d8_kernel walks the same
// boxes first and looks at the distances themselves, approximately: one v_mfma_f32_32x32x16_f16 gives the exponents of 32 training rows x 32
// queries - two tiles x the wave's two groups, four blocks - in 8 passes, against the 2 x 16 passes per block of the fp64 MFMAs.  A block ALL
// of whose 256 approximate exponents lie below the threshold by more than their error bound is taken out of the mask the sweep then reads
// (SweepArgs::live_mask) instead of testing boxes itself.
//
// Operands (32 B per row, the K = 16 slots of the MFMA; training row t against query q):
//   slot      0..7          8        9        10       11   12       13       14       15
//   training  f16(z_t,k)    nt_hi    nt_lo    et       0    1        1        1        0
//   query     f16(z_q,k)    1        1        1        0    nq_hi    nq_lo    eq       0
// nt = -1/2|z_t|^2 as hi = f16(nt), lo = f16(nt - hi); et, eq = the row's share of the error bound, rounded UP to f16.  The accumulator is
//   s~ + E,   s~ ~ s = z_t.z_q - 1/2|z_t|^2 - 1/2|z_q|^2 (the pair's exponent, base-2 units),   E = et + eq >= |s~ - s|:
// a pair is dead when that is < thr = the group's sum bound less the margin - what the box test compares -1/2 dist^2 of the boxes against.
// Round 14: with SweepArgs::qrow_thr a column is compared against ITS query's sum bound less the margin instead - at or above the group's, which
// is the smallest of the sixteen - and a block is dropped when every column lies below its own.  The budget argument is per query (a dropped
// term is below 2^-margin of its own query's sum); the box tests of phase 1 keep the group's number.
//
// The bound.  u = 2^-11 + 2^-24 (f16, round to nearest, a conversion by way of fp32 included), h = 2^-14 (the pack writes 0 for |x| < 2^-14:
// no f16 subnormal reaches the matrix core, whatever it does with them), v = 2^-23 (one fp32 rounding, truncation included), R = |z|_2,
// N = 1/2 R^2, |z|_1 <= sqrt(8) R, R_t R_q <= N_t + N_q:
//   coordinates  |d a_k| <= u |z_tk| + h, |a_k| <= (1 + u)|z_tk|, the same for b:
//                |z_t.z_q - a.b| <= (2u + u^2) R_t R_q + h (1 + u)(|z_t|_1 + |z_q|_1) + 8 h^2 <= (2u + u^2)(N_t + N_q) + 3 h (1 + u)(R_t + R_q) + 8 h^2
//   norms        |nt - hi - lo| <= u |nt - hi| + h <= u^2 N_t + h  (hi is finite: rows with N > 60000 are flagged, below)
//   fp32 sum     the 16 products are exact in fp32 (11 x 11 bits); adding them to C = 0 in any order errs by at most ((1 + v)^16 - 1) T <= 17 v T,
//                T = sum of their magnitudes <= (1 + u)^2 R_t R_q + (1 + u^2)(N_t + N_q) + et16 + eq16 <= 2.02 (N_t + N_q) + 1.01 (R_t + R_q) 2^-12 + 2^-12
//   together     E <= et + eq,   e = KAPPA N + LAMBDA R + MU,   KAPPA = 2^-10 + 2^-20 + 35 2^-23 = 9.82e-4, LAMBDA = 2^-12, MU = 2^-13
// (2u + 2u^2 <= 2^-10 + 2^-22 + 2^-21 < 2^-10 + 2^-20;  3h (1 + u) + 17 v 1.01 2^-12 < 2^-12;  4 h^2 + h + 17 v 2^-13 < 2^-13 per side.)
// tests/test_prune_d8_screen_cpu.py restates s~ and E in numpy and holds |s~ - s| <= E on adversarial rows.  Typical rows of the bench table
// (N = 67, R = 11.6 by the bandwidth rule) carry E = 0.14 exponent units.
// Rows that the f16 operands cannot hold - a NaN or infinite coordinate, |z_k| > 65504, N > 60000 - are FLAGGED: coordinates 0 and +inf in the
// norm's hi slot, so every exponent of theirs is +inf (no slot of the other side is negative or non-finite but a flagged row's own +inf):
// never a NaN, and the block is kept.  That matters to the serial kernel alone, whose fmaxf (v_max3_f32) would lose a NaN; the block maximum
// of kde_screen_d8_kernel (v_maximum3_f32) hands a NaN on, and `!(max < thr)` then keeps the block as well.  The comparison keeps on a NaN
// threshold too.  Padding rows (beyond the table) carry nt = -60000: they have no term.
#define PBN_SCREEN_KAPPA (0x1p-10 + 0x1p-20 + 35.0 * 0x1p-23)
#define PBN_SCREEN_LAMBDA 0x1p-12
#define PBN_SCREEN_MU 0x1p-13

typedef float f16acc __attribute__((ext_vector_type(16)));

// measurement aid, not part of the C ABI header: (tile, group) blocks the screen kept / blocks it tested (= the blocks that pass the box test)
__device__ unsigned long long g_screen_kept = 0, g_screen_tested = 0;
// ... and the kept blocks it handed to the far pass (round 16)
__device__ unsigned long long g_screen_far = 0;

// The far rule (round 16), one helper for the three kernels below: they must write the same far words.  A live block of a plain tile
// (SweepArgs::tile_plain) is FAR when every one of its 256 values s~ + E - each at or above the pair's true exponent - lies below its own
// column's thr_far = qrow_thr[q] - far_theta, rounded down to fp32 as the live rule's threshold is: every pair of the block is then proven
// far_theta bits below its own query's sum bound, which is what kde_far32_d8.inc's error bound needs.  A column whose query the fp32 pass does
// not take - 1/2|z_q|^2 above PBN_FAR32_NCAP or NaN, a bound that is NaN or beyond 4 PBN_FAR32_NCAP in magnitude (the pass's offset) - carries
// thr_far = -inf: nothing compares below it, and no block with that column is far.
__device__ __forceinline__ float screen_far_thr(const SweepArgs& a, int64_t q) {
    const double lb = ((const PBN_GLOBAL double*)a.qrow_thr)[q], nq = -((const PBN_GLOBAL double*)a.nypack)[q];
    if (!(nq <= PBN_FAR32_NCAP && __builtin_fabs(lb) <= 4.0 * PBN_FAR32_NCAP)) return -INFINITY;   // (a NaN on either side)
    const double thrd = lb - a.far_theta;
    float tf = (float)thrd;
    if ((double)tf > thrd) tf = __builtin_fmaf(-__builtin_fabsf(tf), 0x1p-23f, tf) - 0x1p-126f;   // at least one ulp down
    return tf;
}
__device__ __forceinline__ bool screen_not_far(float colmax, float thr_far) { return !(colmax < thr_far); }
// the plain bits of the 64 tiles from tile t on (a batch of a split starts at any tile: two words of the table-wide bitmap)
__device__ __forceinline__ unsigned long long screen_plain_word(const SweepArgs& a, int64_t t) {
    const PBN_GLOBAL unsigned long long* P = (const PBN_GLOBAL unsigned long long*)a.tile_plain + (t >> 6);
    const unsigned s = (unsigned)(t & 63);
    return s ? (P[0] >> s) | (P[1] << (64u - s)) : P[0];
}

__device__ __forceinline__ _Float16 f16_up(double x) {   // the smallest f16 >= x, x >= 0 and far below the format's top
    _Float16 hv = (_Float16)x;
    if ((double)hv < x) {
        unsigned short b = __builtin_bit_cast(unsigned short, hv);
        hv = __builtin_bit_cast(_Float16, (unsigned short)(b + 1));
    }
    return hv;
}

// one thread per padded row: z [n][8] (logical order; perm: sorted position -> logical row, null = z is sorted) -> out [ntiles * 16][2] hf8
__global__ __launch_bounds__(256) void kde_screen_pack_kernel(const double* __restrict__ z, const int32_t* __restrict__ perm, int64_t n, int64_t npad,
                                                             int is_query, hf8* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= npad) return;
    const _Float16 one = (_Float16)1.0f, zero = (_Float16)0.0f;
    hf8 c, k;
#pragma unroll
    for (int j = 0; j < 8; ++j) { c[j] = zero; k[j] = zero; }
    double hi = -60000.0, lo = 0.0, e = 0.0;
    if (r < n) {
        const double* zr = z + (perm ? (int64_t)perm[r] : r) * 8;
        double n2 = 0.0;
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double v = zr[j];
            ok = ok && __builtin_fabs(v) <= 65504.0;   // (false for a NaN)
            n2 = __builtin_fma(v, v, n2);
        }
        const double N = 0.5 * n2;
        ok = ok && N <= 60000.0;
        if (ok) {
#pragma unroll
            for (int j = 0; j < 8; ++j) c[j] = h_piece((float)zr[j]);
            hi = (double)h_piece((float)-N);
            lo = (double)h_piece((float)(-N - hi));
            e = PBN_SCREEN_KAPPA * N + PBN_SCREEN_LAMBDA * __builtin_sqrt(n2) + PBN_SCREEN_MU;
        } else {
            hi = INFINITY;
        }
    }
    const _Float16 e16 = f16_up(e);
    if (is_query) { k[0] = one; k[1] = one; k[2] = one; k[4] = (_Float16)hi; k[5] = (_Float16)lo; k[6] = e16; }
    else { k[0] = (_Float16)hi; k[1] = (_Float16)lo; k[2] = e16; k[4] = one; k[5] = one; k[6] = one; }
    out[r * 2] = c;
    out[r * 2 + 1] = k;
}

// Grid and block placement of kde_sweep_pruned_d8_kernel (pruned_block): wave (qx, split) here prepares the masks of wave (qx, split) there.
// live_mask[((qx * nsplit + split) * batches_per_split + batch) * QG + g]: bit b = tile 64 batch + b of the split passes group g's box test AND
// holds a pair the screen could not prove dead; every batch of the split is written (0 = out of reach).  box_mask (test aid, nullable): the box
// masks alone.
#ifndef PBN_SCREEN_WAVES
#define PBN_SCREEN_WAVES 4   // waves per SIMD the screen is compiled for (128 VGPRs: the joint box test of two groups over eight dimensions spills at 5 and more)
#endif
// Round 11's kernel, kept for one release as the A/B leg and the yardstick of mask equality (PBN_D8_SCREEN_STREAM=0): box tests and MFMAs
// interleaved batch by batch, one fragment load in flight per wave.  kde_screen_d8_kernel, below, writes the same words.
template <bool FAR>
__device__ __forceinline__ void screen_d8_serial_body(const SweepArgs& a) {
    constexpr int QG = PBN_QG_PRUNE, PD = PBN_PRUNE_PD;
    static_assert(QG == 2, "two groups = the 32 columns of the MFMA");
    const int lane = threadIdx.x & 63;
    int qx, split;
    pruned_block(a, QG, blockIdx.x, qx, split);
    const int64_t qt0 = (int64_t)qx * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL hf8* __restrict__ SA = (const PBN_GLOBAL hf8*)a.scr_train;
    const PBN_GLOBAL hf8* __restrict__ SQ = (const PBN_GLOBAL hf8*)a.scr_query;
    // the groups' boxes and thresholds in LDS, as the sweep keeps them (kde_sweep_body: QLDS) - the same words into the same box tests
    __shared__ double qbs[QG * (2 * PD + 1)];
    if (lane < QG * 2 * PD) {
        const int g = lane / (2 * PD);
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        qbs[lane] = QBp[qt * 2 * PD + (lane - g * 2 * PD)];
    } else if (lane < QG * 2 * PD + QG) {
        const int g = lane - QG * 2 * PD;
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        qbs[lane] = QTp[qt] - a.prune_margin;
    }
    asm volatile("" ::: "memory");   // (one wave per workgroup, LDS in order: no barrier)
    const int r = lane & 31, h = lane >> 5, gl = r >> 4;   // my column's group
    const int64_t qtl = qt0 + gl < a.nqtiles ? qt0 + gl : a.nqtiles - 1;
    const hf8 bq = SQ[(qtl * 16 + (r & 15)) * 2 + h];
    // my column's threshold - its own query's bound less the margin (SweepArgs::qrow_thr), the group's without one - as a float not above it
    // (a NaN stays a NaN: nothing compares below it)
    const PBN_GLOBAL double* __restrict__ QRp = (const PBN_GLOBAL double*)a.qrow_thr;
    const double thrd = QRp ? QRp[qtl * 16 + (r & 15)] - a.prune_margin : qbs[QG * 2 * PD + gl];
    float thrf = (float)thrd;
    if ((double)thrf > thrd) thrf = __builtin_fmaf(-__builtin_fabsf(thrf), 0x1p-23f, thrf) - 0x1p-126f;   // at least one ulp down
    float thrfar = -INFINITY;
    if constexpr (FAR) thrfar = screen_far_thr(a, qtl * 16 + (r & 15));
    const unsigned long long G0 = 0x0000ffff0000ffffull;   // the lanes that hold group 0's columns
    const bool count = a.count_redo != 0;
    if (count && lane == 0) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0) * QG);
    PBN_GLOBAL unsigned long long* LM = (PBN_GLOBAL unsigned long long*)a.live_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG;
    PBN_GLOBAL unsigned long long* BM = a.box_mask ? (PBN_GLOBAL unsigned long long*)a.box_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG : nullptr;
    PBN_GLOBAL unsigned long long* FM = FAR ? (PBN_GLOBAL unsigned long long*)a.far_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG : nullptr;
    auto frag = [&](int64_t tb, int bA, int bB) -> hf8 {
        const int64_t t = tb + (r < 16 ? bA : bB);
        return SA[(t * 16 + (r & 15)) * 2 + h];
    };
    for (int64_t sb = t0; sb < t1; sb += 4096) {
        const int64_t bt = sb + 64 * lane;   // my batch's first tile
        const PBN_GLOBAL double* bb = (const PBN_GLOBAL double*)a.batch_box + ((int64_t)split * a.batches_per_split + ((bt - t0) >> 6)) * 2 * PD;
        unsigned long long bmg[QG], bm = 0;
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            bmg[g] = __ballot(bt < t1 && batch_in_reach<PD>(bb, (const double*)&qbs[g * 2 * PD], PD, qbs[QG * 2 * PD + g]));
            bm |= bmg[g];
        }
        unsigned long long my_live[QG] = {0, 0}, my_box[QG] = {0, 0};   // of MY batch (lane = batch)
        unsigned long long my_far[QG] = {0, 0};
        while (bm) {
            const int j = __builtin_ctzll(bm);
            bm &= bm - 1;
            const int64_t tb = sb + 64 * (int64_t)j;
            const unsigned gsel = (unsigned)((bmg[0] >> j) & 1ull) | ((unsigned)((bmg[1] >> j) & 1ull) << 1);
            unsigned long long gm[QG];
            if (gsel == 3u) {
                const double* qb[QG] = {(const double*)&qbs[0], (const double*)&qbs[2 * PD]};
                const double thr[QG] = {qbs[QG * 2 * PD], qbs[QG * 2 * PD + 1]};
                prune_group_masks_joint<PD, QG>(TBp, qb, PD, tb, t1, thr, lane, gm);
            } else {
#pragma unroll
                for (int g = 0; g < QG; ++g)
                    gm[g] = ((gsel >> g) & 1u) ? prune_group_mask<PD>(TBp, (const double*)&qbs[g * 2 * PD], PD, tb, t1, qbs[QG * 2 * PD + g], lane) : 0ull;
            }
            unsigned long long mask = gm[0] | gm[1];
            if (!mask) continue;
            unsigned long long lm0 = 0, lm1 = 0, nf0 = 0, nf1 = 0;   // live; FAR: not far
            int bA = __builtin_ctzll(mask);
            mask &= mask - 1;
            int bB = mask ? __builtin_ctzll(mask) : bA;   // an odd number of tiles: the last MFMA takes its tile twice
            mask &= mask - 1;
            hf8 af = frag(tb, bA, bB);
            for (;;) {
                const bool more = mask != 0;
                int nA = bA, nB = bB;
                if (more) {
                    nA = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    nB = mask ? __builtin_ctzll(mask) : nA;
                    mask &= mask - 1;
                }
                const hf8 an = frag(tb, nA, nB);   // (unconditional, like the sweep's prefetch: after the last pair it is loaded again)
                f16acc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bq, acc, 0, 0, 0);
                // rows 0..15 of the product (tile A) sit in registers 0..7, rows 16..31 (tile B) in 8..15; the column - the query - is the lane
                const float mA = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(acc[0], acc[1]), __builtin_fmaxf(acc[2], acc[3])),
                                                 __builtin_fmaxf(__builtin_fmaxf(acc[4], acc[5]), __builtin_fmaxf(acc[6], acc[7])));
                const float mB = __builtin_fmaxf(__builtin_fmaxf(__builtin_fmaxf(acc[8], acc[9]), __builtin_fmaxf(acc[10], acc[11])),
                                                 __builtin_fmaxf(__builtin_fmaxf(acc[12], acc[13]), __builtin_fmaxf(acc[14], acc[15])));
                const unsigned long long kA = __ballot(!(mA < thrf)), kB = __ballot(!(mB < thrf));
                lm0 |= ((kA & G0) ? 1ull << bA : 0ull) | ((kB & G0) ? 1ull << bB : 0ull);
                lm1 |= ((kA & ~G0) ? 1ull << bA : 0ull) | ((kB & ~G0) ? 1ull << bB : 0ull);
                if constexpr (FAR) {
                    const unsigned long long fA = __ballot(screen_not_far(mA, thrfar)), fB = __ballot(screen_not_far(mB, thrfar));
                    nf0 |= ((fA & G0) ? 1ull << bA : 0ull) | ((fB & G0) ? 1ull << bB : 0ull);
                    nf1 |= ((fA & ~G0) ? 1ull << bA : 0ull) | ((fB & ~G0) ? 1ull << bB : 0ull);
                }
                if (!more) break;
                af = an; bA = nA; bB = nB;
            }
            lm0 &= gm[0];
            lm1 &= gm[1];
            if (count && lane == 0) {
                atomicAdd(&g_sweep_visit, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
                atomicAdd(&g_screen_tested, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
                atomicAdd(&g_screen_kept, (unsigned long long)(__builtin_popcountll(lm0) + __builtin_popcountll(lm1)));
            }
            if (lane == j) { my_live[0] = lm0; my_live[1] = lm1; my_box[0] = gm[0]; my_box[1] = gm[1]; }
            if constexpr (FAR) { if (lane == j) { my_far[0] = lm0 & ~nf0; my_far[1] = lm1 & ~nf1; } }
        }
        if (bt < t1) {
            const int64_t jb = (bt - t0) >> 6;
            LM[jb * QG] = my_live[0];
            LM[jb * QG + 1] = my_live[1];
            if (BM) { BM[jb * QG] = my_box[0]; BM[jb * QG + 1] = my_box[1]; }
            if constexpr (FAR) {
                const unsigned long long pw = screen_plain_word(a, bt);
                const unsigned long long f0 = my_far[0] & pw, f1 = my_far[1] & pw;
                FM[jb * QG] = f0;
                FM[jb * QG + 1] = f1;
                if (count && (f0 | f1)) atomicAdd(&g_screen_far, (unsigned long long)(__builtin_popcountll(f0) + __builtin_popcountll(f1)));
            }
        }
    }
    // the batch slots past the table's end in a short last split hold nothing: written too, so that no word of a launch's masks is left as
    // an earlier launch had it (the sweep never reads them; pbn_debug_d8_masks copies them)
    for (int64_t jb = ((t1 - t0 + 63) >> 6) + lane; jb < a.batches_per_split; jb += 64) {
        LM[jb * QG] = 0;
        LM[jb * QG + 1] = 0;
        if (BM) { BM[jb * QG] = 0; BM[jb * QG + 1] = 0; }
        if constexpr (FAR) { FM[jb * QG] = 0; FM[jb * QG + 1] = 0; }
    }
}

// The screen in two phases per wave (round 12).  The serial kernel's listing shows every MFMA behind `s_waitcnt vmcnt(0)` on a load issued a few
// scalar instructions earlier (the compiler rotated the source's prefetch away): one memory round trip per MFMA, one load in flight per wave.
// Phase 1 walks the super-batch's boxes exactly as before - batch_in_reach, prune_group_masks_joint, prune_group_mask on the same words - and
// parks the box words in LDS, issuing no MFMA.  Phase 2 walks the flat list of tile pairs those words define (batch order, pairs inside a batch
// as before: an odd count takes its last tile twice, no pair straddles batches) with PBN_SCREEN_RING fragments in flight: a prologue of R loads,
// then turns of R slots - MFMA, block maximum, two compares and ballots, the result ORed into the batch's live words in LDS, the load of the
// pair R ahead into the register the MFMA just read.  The loads are unconditional (a conditional load costs a vmcnt(0): run_batch in
// kde_kernels.hip): past the end of the list the last pair is loaded and screened again, which ORs the same bits.  Nothing else in the loop
// counts on vmcnt - the mask words leave through LDS and are stored after it - so each slot waits with vmcnt(R - 1)
// (tests/test_isa_screen_cpu.py).  A tile's bit depends on its own 16 rows alone: the words are the serial kernel's, bit for bit.
// The block maximum is __builtin_elementwise_maximum: 8 v_maximum3_f32 for the two tiles where fmaxf quiets every input first (19 v_max_f32 +
// 4 v_max3_f32).  On accumulators without a NaN - all of them, by the operands' design - the two maxima are equal; a NaN it PROPAGATES,
// and `!(max < thr)` then keeps the block instead of losing it.
#ifndef PBN_SCREEN_RING
#define PBN_SCREEN_RING 4   // fragments in flight per wave (4 VGPRs each)
#endif
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_serial_kernel(SweepArgs a) { screen_d8_serial_body<false>(a); }
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_serial_far_kernel(SweepArgs a) { screen_d8_serial_body<true>(a); }

template <bool FAR>
__device__ __forceinline__ void screen_d8_ring_body(const SweepArgs& a) {
    constexpr int QG = PBN_QG_PRUNE, PD = PBN_PRUNE_PD, R = PBN_SCREEN_RING;
    constexpr int MW = FAR ? 6 : 4;   // words per batch in msk: box, live; FAR: not far
    static_assert(QG == 2, "two groups = the 32 columns of the MFMA");
    static_assert(R >= 1 && R <= 16, "ring depth");
    const int lane = threadIdx.x & 63;
    int qx, split;
    pruned_block(a, QG, blockIdx.x, qx, split);
    const int64_t qt0 = (int64_t)qx * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL char* __restrict__ SAc = (const PBN_GLOBAL char*)a.scr_train;
    const PBN_GLOBAL hf8* __restrict__ SQ = (const PBN_GLOBAL hf8*)a.scr_query;
    __shared__ double qbs[QG * (2 * PD + 1)];            // the groups' boxes and thresholds, as in the serial kernel
    __shared__ unsigned long long msk[64 * MW];          // per batch of the super-batch: the box words of its groups, then the live words
    if (lane < QG * 2 * PD) {
        const int g = lane / (2 * PD);
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        qbs[lane] = QBp[qt * 2 * PD + (lane - g * 2 * PD)];
    } else if (lane < QG * 2 * PD + QG) {
        const int g = lane - QG * 2 * PD;
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        qbs[lane] = QTp[qt] - a.prune_margin;
    }
    asm volatile("" ::: "memory");   // (one wave per workgroup, LDS in order: no barrier)
    const bool count = a.count_redo != 0;
    if (count && lane == 0) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0) * QG);
    PBN_GLOBAL unsigned long long* LM = (PBN_GLOBAL unsigned long long*)a.live_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG;
    PBN_GLOBAL unsigned long long* BM = a.box_mask ? (PBN_GLOBAL unsigned long long*)a.box_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG : nullptr;
    PBN_GLOBAL unsigned long long* FM = FAR ? (PBN_GLOBAL unsigned long long*)a.far_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG : nullptr;
    for (int64_t sb = t0; sb < t1; sb += 4096) {
        // ---- phase 1: the box words of the super-batch's batches (lane = batch)
        const int64_t bt = sb + 64 * lane;   // my batch's first tile
        const PBN_GLOBAL double* bb = (const PBN_GLOBAL double*)a.batch_box + ((int64_t)split * a.batches_per_split + ((bt - t0) >> 6)) * 2 * PD;
        unsigned long long bmg[QG], bm = 0;
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            bmg[g] = __ballot(bt < t1 && batch_in_reach<PD>(bb, (const double*)&qbs[g * 2 * PD], PD, qbs[QG * 2 * PD + g]));
            bm |= bmg[g];
        }
        unsigned long long my_box[QG] = {0, 0};
        while (bm) {
            const int j = __builtin_ctzll(bm);
            bm &= bm - 1;
            const int64_t tb = sb + 64 * (int64_t)j;
            const unsigned gsel = (unsigned)((bmg[0] >> j) & 1ull) | ((unsigned)((bmg[1] >> j) & 1ull) << 1);
            unsigned long long gm[QG];
            if (gsel == 3u) {
                const double* qb[QG] = {(const double*)&qbs[0], (const double*)&qbs[2 * PD]};
                const double thr[QG] = {qbs[QG * 2 * PD], qbs[QG * 2 * PD + 1]};
                prune_group_masks_joint<PD, QG>(TBp, qb, PD, tb, t1, thr, lane, gm);
            } else {
#pragma unroll
                for (int g = 0; g < QG; ++g)
                    gm[g] = ((gsel >> g) & 1u) ? prune_group_mask<PD>(TBp, (const double*)&qbs[g * 2 * PD], PD, tb, t1, qbs[QG * 2 * PD + g], lane) : 0ull;
            }
            if (count && lane == 0 && (gm[0] | gm[1])) {
                atomicAdd(&g_sweep_visit, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
                atomicAdd(&g_screen_tested, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
            }
            if (lane == j) { my_box[0] = gm[0]; my_box[1] = gm[1]; }
        }
        msk[lane * MW] = my_box[0];
        msk[lane * MW + 1] = my_box[1];
#pragma unroll
        for (int k = 2; k < MW; ++k) msk[lane * MW + k] = 0;
        asm volatile("" ::: "memory");
        // ---- phase 2: the pairs of the parked words through the ring.  Everything that names a pair is scalar.
        const unsigned long long tiles = my_box[0] | my_box[1];
        unsigned long long todo = __ballot(tiles != 0);   // batches whose pairs are still to be listed
        if (todo) {
            // what only the MFMAs need is set up here, from a lane number the compiler cannot hoist it by: the joint box test of phase 1 fills
            // the 128 registers on its own (the queries' operands alone are four)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const int r = ln & 31, h = ln >> 5, gl = r >> 4;   // my column's group
            const int64_t qtl = qt0 + gl < a.nqtiles ? qt0 + gl : a.nqtiles - 1;
            const hf8 bq = SQ[(qtl * 16 + (r & 15)) * 2 + h];
            // my column's threshold - its own query's bound less the margin (SweepArgs::qrow_thr), the group's without one - as a float not above
            // it (a NaN stays a NaN: nothing compares below it)
            const PBN_GLOBAL double* __restrict__ QRp = (const PBN_GLOBAL double*)a.qrow_thr;
            const double thrd = QRp ? QRp[qtl * 16 + (r & 15)] - a.prune_margin : qbs[QG * 2 * PD + gl];
            float thrf = (float)thrd;
            if ((double)thrf > thrd) thrf = __builtin_fmaf(-__builtin_fabsf(thrf), 0x1p-23f, thrf) - 0x1p-126f;   // at least one ulp down
            float thrfar = -INFINITY;
            if constexpr (FAR) thrfar = screen_far_thr(a, qtl * 16 + (r & 15));
            // my 16 bytes of a training row's operands: rows 0..15 of the product come from the pair's first tile, 16..31 from its second
            const unsigned loff = (unsigned)((r & 15) * 32 + h * 16), second = r < 16 ? 0u : 1u;
            const int tiles_lo = (int)(unsigned)tiles, tiles_hi = (int)(unsigned)(tiles >> 32);
            const PBN_GLOBAL char* sbp = SAc + sb * 512;   // 512 B of operands per tile
            struct Pair { unsigned j, a, b; };   // batch of the super-batch, first and second tile of the batch
            Pair cur = {0u, 0u, 0u};       // the pair last listed
            unsigned long long left = 0;   // tiles of batch cur.j not yet in a pair
            auto next = [&]() -> bool {    // lists the next pair; false past the end (cur stays: that pair is loaded again)
                if (left == 0 && todo != 0) {
                    cur.j = (unsigned)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    left = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(tiles_lo, (int)cur.j) |
                           ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(tiles_hi, (int)cur.j) << 32);
                }
                if (left == 0) return false;
                cur.a = (unsigned)__builtin_ctzll(left);
                left &= left - 1;
                cur.b = left ? (unsigned)__builtin_ctzll(left) : cur.a;   // an odd number of tiles: the last MFMA takes its tile twice
                left &= left - 1;
                return true;
            };
            // A scalar base per pair and a 32-bit lane offset.  The base goes through an empty asm: where the compiler can see that a slot past the
            // end reloads the previous slot's pair it makes the load conditional - a copy of that slot's registers behind a vmcnt(0) - and the
            // ring drains in every slot.
            auto frag = [&](const Pair& d) -> hf8 {
                unsigned base = (d.j * 64u + d.a) * 512u;
                asm volatile("" : "+s"(base));
                const PBN_GLOBAL char* p = sbp + (uint64_t)base;
                return *(const PBN_GLOBAL hf8*)(p + (uint64_t)(loff + second * ((d.b - d.a) * 512u)));
            };
            auto slot = [&](const Pair& d, const hf8& af) {
                f16acc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bq, acc, 0, 0, 0);
                // rows 0..15 of the product (tile A) sit in registers 0..7, rows 16..31 (tile B) in 8..15; the column - the query - is the lane
                auto mx = [](float x, float y) { return __builtin_elementwise_maximum(x, y); };
                const float mA = mx(mx(mx(mx(acc[0], acc[1]), acc[2]), mx(mx(acc[3], acc[4]), acc[5])), mx(acc[6], acc[7]));
                const float mB = mx(mx(mx(mx(acc[8], acc[9]), acc[10]), mx(mx(acc[11], acc[12]), acc[13])), mx(acc[14], acc[15]));
                const unsigned long long kA = __ballot(!(mA < thrf)), kB = __ballot(!(mB < thrf));
                // group 0's columns are lanes 0..15 and 32..47: the halves of a ballot folded, its low 16 bits; group 1's the high 16
                const unsigned fA = (unsigned)kA | (unsigned)(kA >> 32), fB = (unsigned)kB | (unsigned)(kB >> 32);
                const unsigned long long l0 = ((fA & 0xffffu) ? 1ull << d.a : 0ull) | ((fB & 0xffffu) ? 1ull << d.b : 0ull);
                const unsigned long long l1 = ((fA >> 16) ? 1ull << d.a : 0ull) | ((fB >> 16) ? 1ull << d.b : 0ull);
                if constexpr (FAR) {
                    const unsigned long long gA = __ballot(screen_not_far(mA, thrfar)), gB = __ballot(screen_not_far(mB, thrfar));
                    const unsigned hA = (unsigned)gA | (unsigned)(gA >> 32), hB = (unsigned)gB | (unsigned)(gB >> 32);
                    const unsigned long long n0 = ((hA & 0xffffu) ? 1ull << d.a : 0ull) | ((hB & 0xffffu) ? 1ull << d.b : 0ull);
                    const unsigned long long n1 = ((hA >> 16) ? 1ull << d.a : 0ull) | ((hB >> 16) ? 1ull << d.b : 0ull);
                    if (lane < 2 * QG) __hip_atomic_fetch_or(&msk[d.j * (unsigned)MW + 2u + (unsigned)lane], lane == 0 ? l0 : lane == 1 ? l1 : lane == 2 ? n0 : n1,
                                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                } else {
                    if (lane < QG) __hip_atomic_fetch_or(&msk[d.j * 4u + 2u + (unsigned)lane], lane ? l1 : l0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            };
            Pair dq[R];
            hf8 fq[R];
            bool go = true;
#pragma unroll
            for (int i = 0; i < R; ++i) {
                next();
                dq[i] = cur;
                fq[i] = frag(cur);
            }
            do {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    slot(dq[i], fq[i]);
                    const bool more = next();
                    if (i == 0) go = more;   // the next turn's first pair exists
                    dq[i] = cur;
                    fq[i] = frag(cur);
                }
            } while (go);
        }
        asm volatile("" ::: "memory");
        if (bt < t1) {
            const int64_t jb = (bt - t0) >> 6;
            const unsigned long long lv0 = msk[lane * MW + 2] & my_box[0], lv1 = msk[lane * MW + 3] & my_box[1];
            LM[jb * QG] = lv0;
            LM[jb * QG + 1] = lv1;
            if (BM) { BM[jb * QG] = msk[lane * MW]; BM[jb * QG + 1] = msk[lane * MW + 1]; }
            if (count && (lv0 | lv1)) atomicAdd(&g_screen_kept, (unsigned long long)(__builtin_popcountll(lv0) + __builtin_popcountll(lv1)));
            if constexpr (FAR) {
                const unsigned long long pw = screen_plain_word(a, bt);
                const unsigned long long f0 = lv0 & ~msk[lane * MW + 4] & pw, f1 = lv1 & ~msk[lane * MW + 5] & pw;
                FM[jb * QG] = f0;
                FM[jb * QG + 1] = f1;
                if (count && (f0 | f1)) atomicAdd(&g_screen_far, (unsigned long long)(__builtin_popcountll(f0) + __builtin_popcountll(f1)));
            }
        }
        asm volatile("" ::: "memory");   // (the next super-batch parks its words where these were read)
    }
    // the batch slots past the table's end in a short last split hold nothing: written too (see the serial kernel)
    for (int64_t jb = ((t1 - t0 + 63) >> 6) + lane; jb < a.batches_per_split; jb += 64) {
        LM[jb * QG] = 0;
        LM[jb * QG + 1] = 0;
        if (BM) { BM[jb * QG] = 0; BM[jb * QG + 1] = 0; }
        if constexpr (FAR) { FM[jb * QG] = 0; FM[jb * QG + 1] = 0; }
    }
}

// The screen without a pair list (round 13).  The ring's slot is 87 instructions, most of them scalar and in dependent chains - find-first-bit,
// clear, readlane, the shifts that make a pair and its address, the masks of the LDS OR - and all of that walks a list that is not sparse: inside
// a batch in reach 47 of the 64 tiles pass a box test (profiles/r13/step0.txt).  This kernel screens CONSECUTIVE tile pairs (2p, 2p + 1) instead,
// in units of four pairs = 4 KiB of operands: from the unit of the first set bit of the batch's box words to the unit of the last.  A unit is one
// scalar base, four loads at immediate offsets 0 .. 3 KiB, four MFMAs per served sweep wave, and the eight result bits of a wave land at
// compile-time positions of a byte per lane, which one 64-bit shift by 8 x unit puts into the lane's word of the batch.  Behind a batch's last
// unit the words are ORed over each group's 32 lanes (four DPP steps inside a row of 16, the rows by readlane: lanes 0-15 and 32-47 hold
// group 0's columns) and kept by lane = batch.  A tile's bit depends on its own 16 rows and the group's 16 queries only - an MFMA output element
// does not depend on what else shares the instruction - and live = screened AND box, so bits of tiles that fail the box test, which the list
// never screened, change nothing: the words are the serial kernel's, bit for bit (tests/test_prune_d8_screen_dense_gpu.py).
// Two units of loads (8 fragments) are in flight: the list of (batch, unit) runs two units ahead of the MFMAs, across batches, and past its end
// the last unit is loaded again (unconditional loads, counted vmcnt waits) and its bits are shifted out.  A unit that would read beyond the
// table's last tile is moved back by whole tiles and its byte shifted right by as many: no tile at or beyond ntiles is read (ntiles >= 8:
// launch_screen_d8 hands smaller tables to the ring).
// NW = sweep waves served by one screen wave (NW x 2 query groups against one stream of fragments): phase 1 runs per served wave in turn, a
// batch's units run the MFMAs of the served waves in reach of it.
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_kernel(SweepArgs a) { screen_d8_ring_body<false>(a); }
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_far_kernel(SweepArgs a) { screen_d8_ring_body<true>(a); }

template <int NW, bool FAR>
__device__ __forceinline__ void screen_d8_dense_body(const SweepArgs& a) {
    constexpr int QG = PBN_QG_PRUNE, PD = PBN_PRUNE_PD, QW = QG * (2 * PD + 1);
    static_assert(QG == 2, "two groups = the 32 columns of the MFMA");
    static_assert(NW == 1 || NW == 2, "sweep waves per screen wave");
    const int lane = threadIdx.x & 63;
    int qxs, split;
    pruned_block(a, QG * NW, blockIdx.x, qxs, split);
    if ((int64_t)qxs * NW * QG >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL char* __restrict__ SAc = (const PBN_GLOBAL char*)a.scr_train;
    const PBN_GLOBAL hf8* __restrict__ SQ = (const PBN_GLOBAL hf8*)a.scr_query;
    __shared__ double qbs[NW * QW];                       // per served wave: the groups' boxes and thresholds, as in the serial kernel
    __shared__ unsigned long long msk[NW * 64 * QG];      // per served wave and batch of the super-batch: the box words of its groups
    for (int w = 0; w < NW; ++w) {
        const int64_t qt0 = ((int64_t)qxs * NW + w) * QG;
        if (lane < QG * 2 * PD) {
            const int g = lane / (2 * PD);
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            qbs[w * QW + lane] = QBp[qt * 2 * PD + (lane - g * 2 * PD)];
        } else if (lane < QW) {
            const int g = lane - QG * 2 * PD;
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            qbs[w * QW + lane] = QTp[qt] - a.prune_margin;
        }
    }
    asm volatile("" ::: "memory");   // (one wave per workgroup, LDS in order: no barrier)
    const bool count = a.count_redo != 0;
    const int64_t wave_words = (int64_t)a.nsplit_grid * a.batches_per_split * QG;   // of one sweep wave in live_mask / box_mask
    const int64_t word0 = ((int64_t)qxs * NW * a.nsplit_grid + split) * a.batches_per_split * QG;
    PBN_GLOBAL unsigned long long* LM = (PBN_GLOBAL unsigned long long*)a.live_mask + word0;
    PBN_GLOBAL unsigned long long* BM = a.box_mask ? (PBN_GLOBAL unsigned long long*)a.box_mask + word0 : nullptr;
    PBN_GLOBAL unsigned long long* FM = FAR ? (PBN_GLOBAL unsigned long long*)a.far_mask + word0 : nullptr;
    if (count && lane == 0)   // once per served sweep wave, as the ring and the serial kernel count
        for (int w = 0; w < NW && ((int64_t)qxs * NW + w) * QG < a.nqtiles; ++w) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0) * QG);
    for (int64_t sb = t0; sb < t1; sb += 4096) {
        // ---- phase 1: the box words of the super-batch's batches (lane = batch), one served sweep wave after the other
        const int64_t bt = sb + 64 * lane;   // my batch's first tile
        const PBN_GLOBAL double* bb = (const PBN_GLOBAL double*)a.batch_box + ((int64_t)split * a.batches_per_split + ((bt - t0) >> 6)) * 2 * PD;
        unsigned long long tiles = 0;        // of my batch: in reach of any served wave
        unsigned served = 0;                 // of my batch: the served waves in reach
#pragma unroll 1
        for (int w = 0; w < NW; ++w) {
            const double* qw = (const double*)&qbs[w * QW];
            unsigned long long my_box[QG] = {0, 0};
            if (((int64_t)qxs * NW + w) * QG < a.nqtiles) {
                unsigned long long bmg[QG], bm = 0;
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    bmg[g] = __ballot(bt < t1 && batch_in_reach<PD>(bb, qw + g * 2 * PD, PD, qw[QG * 2 * PD + g]));
                    bm |= bmg[g];
                }
                while (bm) {
                    const int j = __builtin_ctzll(bm);
                    bm &= bm - 1;
                    const int64_t tb = sb + 64 * (int64_t)j;
                    const unsigned gsel = (unsigned)((bmg[0] >> j) & 1ull) | ((unsigned)((bmg[1] >> j) & 1ull) << 1);
                    unsigned long long gm[QG];
                    if (gsel == 3u) {
                        const double* qb[QG] = {qw, qw + 2 * PD};
                        const double thr[QG] = {qw[QG * 2 * PD], qw[QG * 2 * PD + 1]};
                        prune_group_masks_joint<PD, QG>(TBp, qb, PD, tb, t1, thr, lane, gm);
                    } else {
#pragma unroll
                        for (int g = 0; g < QG; ++g)
                            gm[g] = ((gsel >> g) & 1u) ? prune_group_mask<PD>(TBp, qw + g * 2 * PD, PD, tb, t1, qw[QG * 2 * PD + g], lane) : 0ull;
                    }
                    if (count && lane == 0 && (gm[0] | gm[1])) {
                        atomicAdd(&g_sweep_visit, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
                        atomicAdd(&g_screen_tested, (unsigned long long)(__builtin_popcountll(gm[0]) + __builtin_popcountll(gm[1])));
                    }
                    if (lane == j) { my_box[0] = gm[0]; my_box[1] = gm[1]; }
                }
            }
            msk[(w * 64 + lane) * QG] = my_box[0];
            msk[(w * 64 + lane) * QG + 1] = my_box[1];
            tiles |= my_box[0] | my_box[1];
            served |= (my_box[0] | my_box[1]) ? 1u << w : 0u;
        }
        asm volatile("" ::: "memory");
        // ---- phase 2: the units of the batches in reach, two units of loads ahead of the MFMAs.  Everything that names a unit is scalar.
        unsigned long long my_scr[NW][QG];   // of MY batch (lane = batch): the tiles the screen could not prove dead, per served wave and group
#pragma unroll
        for (int w = 0; w < NW; ++w) { my_scr[w][0] = 0; my_scr[w][1] = 0; }
        unsigned long long my_nf[FAR ? NW : 1][QG];    // FAR: ... and the tiles with a column at or above its far threshold
#pragma unroll
        for (int w = 0; w < (FAR ? NW : 1); ++w) { my_nf[w][0] = 0; my_nf[w][1] = 0; }
        unsigned long long todo = __ballot(tiles != 0);   // batches whose units are still to be listed
        if (todo) {
            // what only the MFMAs need is set up here, from a lane number the compiler cannot hoist it by (see kde_screen_d8_kernel)
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const int r = ln & 31, h = ln >> 5, gl = r >> 4;   // my column's group
            hf8 bq[NW];
            float thrf[NW], thrfar[FAR ? NW : 1];
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int64_t qt0 = ((int64_t)qxs * NW + w) * QG;
                const int64_t qtl = qt0 + gl < a.nqtiles ? qt0 + gl : a.nqtiles - 1;
                bq[w] = SQ[(qtl * 16 + (r & 15)) * 2 + h];
                // my column's threshold - its own query's bound less the margin (SweepArgs::qrow_thr), the group's without one - as a float not
                // above it (a NaN stays a NaN: nothing compares below it)
                const PBN_GLOBAL double* __restrict__ QRp = (const PBN_GLOBAL double*)a.qrow_thr;
                const double thrd = QRp ? QRp[qtl * 16 + (r & 15)] - a.prune_margin : qbs[w * QW + QG * 2 * PD + gl];
                float tf = (float)thrd;
                if ((double)tf > thrd) tf = __builtin_fmaf(-__builtin_fabsf(tf), 0x1p-23f, tf) - 0x1p-126f;   // at least one ulp down
                thrf[w] = tf;
                if constexpr (FAR) thrfar[w] = screen_far_thr(a, qtl * 16 + (r & 15));
            }
            // my 16 bytes of a pair's KiB: rows 0..15 of the product come from tile 2p, 16..31 from tile 2p + 1
            const unsigned loff = (unsigned)(r * 32 + h * 16);
            const int tiles_lo = (int)(unsigned)tiles, tiles_hi = (int)(unsigned)(tiles >> 32);
            const int served_v = (int)served;
            const PBN_GLOBAL char* sbp = SAc + sb * 512;                                           // the super-batch's operands
            const int left = (int)(a.ntiles - sb < 8192 ? a.ntiles - sb : 8192);                   // tiles of the table from the super-batch's first
            // batch of the super-batch, unit of the batch, tiles the loads are moved back by, tiles the byte is shifted by (the same; 8 = not a
            // unit, every bit shifted out), served waves in reach, the batch's last unit
            struct Unit { unsigned j, u, back, sh, sel; bool last; };
            unsigned cj = 0, cu = 0, ce = 0, csel = 0;   // the list's cursor: batch, unit, the batch's last unit, its served waves
            bool started = false;
            auto next = [&]() -> Unit {   // lists the next unit; past the end the last one again, as no unit
                bool ok = true;
                if (started && cu < ce) ++cu;
                else if (todo != 0) {
                    started = true;
                    cj = (unsigned)__builtin_ctzll(todo);
                    todo &= todo - 1;
                    const unsigned long long t = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(tiles_lo, (int)cj) |
                                                 ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(tiles_hi, (int)cj) << 32);
                    cu = (unsigned)__builtin_ctzll(t) >> 3;
                    ce = (63u - (unsigned)__builtin_clzll(t)) >> 3;
                    csel = NW == 1 ? 1u : (unsigned)__builtin_amdgcn_readlane(served_v, (int)cj);
                } else ok = false;
                const int over = (int)(64u * cj + 8u * cu + 8u) - left;   // tiles of the unit beyond the table (< 8: its first tile is inside)
                const unsigned back = over > 0 ? (unsigned)over : 0u;
                Unit d = {cj, cu, back, back, csel, cu == ce};
                if (!ok) { d.sh = 8u; d.last = false; }
                return d;
            };
            // A scalar base per unit and a 32-bit lane offset; the base goes through an empty asm, so that the compiler cannot see a unit past the end
            // reload the previous one's bytes (it would make the load conditional behind a vmcnt(0): kde_screen_d8_kernel)
            auto load = [&](const Unit& d, hf8 (&f)[4]) {
                // the unit's first tile, from the super-batch's: NEGATIVE where a split of fewer than 8 tiles ends the table and the unit is moved
                // back in front of it
                int tile = (int)(64u * d.j + 8u * d.u) - (int)d.back;
                asm volatile("" : "+s"(tile));
                const PBN_GLOBAL char* p = sbp + (int64_t)tile * 512;   // (512 B of operands per tile)
#pragma unroll
                for (int i = 0; i < 4; ++i) f[i] = *(const PBN_GLOBAL hf8*)(p + (uint64_t)loff + i * 1024);
            };
            unsigned long long word[NW];   // per lane: the bits of my column's group in the batch being screened
#pragma unroll
            for (int w = 0; w < NW; ++w) word[w] = 0;
            unsigned long long wordf[FAR ? NW : 1];   // FAR: the same for "not far"
#pragma unroll
            for (int w = 0; w < (FAR ? NW : 1); ++w) wordf[w] = 0;
            auto row_or = [](unsigned x) -> unsigned {   // OR over my row of 16 lanes, in every lane of it
                x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true);    // quad_perm [1, 0, 3, 2]
                x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, true);    // quad_perm [2, 3, 0, 1]
                x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x124, 0xf, 0xf, true);   // row_ror:4
                x |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, 0x128, 0xf, 0xf, true);   // row_ror:8
                return x;
            };
            auto unit = [&](const Unit& d, const hf8 (&f)[4]) {
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    if (NW > 1 && !((d.sel >> w) & 1u)) continue;   // (uniform)
                    unsigned b = 0, bf = 0;
                    const f16acc zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                    // the next pair's MFMA is issued before this pair's maxima, which then run beside it (two accumulators in turn)
                    f16acc acc[4];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[0], bq[w], zero, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (i + 1 < 4) acc[i + 1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[i + 1], bq[w], zero, 0, 0, 0);
                        // rows 0..15 of the product (tile 2p) sit in registers 0..7, rows 16..31 (tile 2p + 1) in 8..15; the column - the query - is the lane
                        auto mx = [](float x, float y) { return __builtin_elementwise_maximum(x, y); };
                        const f16acc& c = acc[i];
                        const float mA = mx(mx(mx(mx(c[0], c[1]), c[2]), mx(mx(c[3], c[4]), c[5])), mx(c[6], c[7]));
                        const float mB = mx(mx(mx(mx(c[8], c[9]), c[10]), mx(mx(c[11], c[12]), c[13])), mx(c[14], c[15]));
                        b |= (!(mA < thrf[w]) ? 1u << (2 * i) : 0u) | (!(mB < thrf[w]) ? 2u << (2 * i) : 0u);
                        if constexpr (FAR) bf |= (screen_not_far(mA, thrfar[w]) ? 1u << (2 * i) : 0u) | (screen_not_far(mB, thrfar[w]) ? 2u << (2 * i) : 0u);
                    }
                    word[w] |= (unsigned long long)(b >> d.sh) << (8u * d.u);
                    if constexpr (FAR) wordf[w] |= (unsigned long long)(bf >> d.sh) << (8u * d.u);
                }
                if (d.last) {   // (uniform) the batch is through: its words over each group's lanes, kept by lane = batch
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        const unsigned lo = row_or((unsigned)word[w]), hi = row_or((unsigned)(word[w] >> 32));
                        unsigned long long g[QG];
#pragma unroll
                        for (int q = 0; q < QG; ++q)
                            g[q] = (unsigned long long)((unsigned)__builtin_amdgcn_readlane((int)lo, 16 * q) | (unsigned)__builtin_amdgcn_readlane((int)lo, 32 + 16 * q)) |
                                   ((unsigned long long)((unsigned)__builtin_amdgcn_readlane((int)hi, 16 * q) | (unsigned)__builtin_amdgcn_readlane((int)hi, 32 + 16 * q)) << 32);
                        if (lane == (int)d.j) { my_scr[w][0] = g[0]; my_scr[w][1] = g[1]; }
                        word[w] = 0;
                        if constexpr (FAR) {
                            const unsigned flo = row_or((unsigned)wordf[w]), fhi = row_or((unsigned)(wordf[w] >> 32));
                            unsigned long long nf[QG];
#pragma unroll
                            for (int q = 0; q < QG; ++q)
                                nf[q] = (unsigned long long)((unsigned)__builtin_amdgcn_readlane((int)flo, 16 * q) | (unsigned)__builtin_amdgcn_readlane((int)flo, 32 + 16 * q)) |
                                        ((unsigned long long)((unsigned)__builtin_amdgcn_readlane((int)fhi, 16 * q) | (unsigned)__builtin_amdgcn_readlane((int)fhi, 32 + 16 * q)) << 32);
                            if (lane == (int)d.j) { my_nf[w][0] = nf[0]; my_nf[w][1] = nf[1]; }
                            wordf[w] = 0;
                        }
                    }
                }
            };
            Unit dq[2];
            hf8 fq[2][4];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                dq[k] = next();
                load(dq[k], fq[k]);
            }
            do {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    unit(dq[k], fq[k]);
                    dq[k] = next();
                    load(dq[k], fq[k]);
                }
            } while (dq[0].sh != 8u);   // the next turn's first unit exists
        }
        if (bt < t1) {
            const int64_t jb = (bt - t0) >> 6;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                if (((int64_t)qxs * NW + w) * QG >= a.nqtiles) break;
                const unsigned long long bx0 = msk[(w * 64 + lane) * QG], bx1 = msk[(w * 64 + lane) * QG + 1];
                const unsigned long long lv0 = my_scr[w][0] & bx0, lv1 = my_scr[w][1] & bx1;
                LM[w * wave_words + jb * QG] = lv0;
                LM[w * wave_words + jb * QG + 1] = lv1;
                if (BM) { BM[w * wave_words + jb * QG] = bx0; BM[w * wave_words + jb * QG + 1] = bx1; }
                if (count && (lv0 | lv1)) atomicAdd(&g_screen_kept, (unsigned long long)(__builtin_popcountll(lv0) + __builtin_popcountll(lv1)));
                if constexpr (FAR) {
                    const unsigned long long pw = screen_plain_word(a, bt);
                    const unsigned long long f0 = lv0 & ~my_nf[w][0] & pw, f1 = lv1 & ~my_nf[w][1] & pw;
                    FM[w * wave_words + jb * QG] = f0;
                    FM[w * wave_words + jb * QG + 1] = f1;
                    if (count && (f0 | f1)) atomicAdd(&g_screen_far, (unsigned long long)(__builtin_popcountll(f0) + __builtin_popcountll(f1)));
                }
            }
        }
        asm volatile("" ::: "memory");   // (the next super-batch parks its words where these were read)
    }
    // the batch slots past the table's end in a short last split hold nothing: written too (see the serial kernel)
    for (int w = 0; w < NW; ++w) {
        if (((int64_t)qxs * NW + w) * QG >= a.nqtiles) break;
        for (int64_t jb = ((t1 - t0 + 63) >> 6) + lane; jb < a.batches_per_split; jb += 64) {
            LM[w * wave_words + jb * QG] = 0;
            LM[w * wave_words + jb * QG + 1] = 0;
            if (BM) { BM[w * wave_words + jb * QG] = 0; BM[w * wave_words + jb * QG + 1] = 0; }
            if constexpr (FAR) { FM[w * wave_words + jb * QG] = 0; FM[w * wave_words + jb * QG + 1] = 0; }
        }
    }
}
template <int NW>
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_dense_kernel(SweepArgs a) { screen_d8_dense_body<NW, false>(a); }
template <int NW>
__global__ __launch_bounds__(64, PBN_SCREEN_WAVES) void kde_screen_d8_dense_far_kernel(SweepArgs a) { screen_d8_dense_body<NW, true>(a); }

void launch_screen_pack(const double* z, const int32_t* perm, int64_t n, int64_t ntiles, bool is_query, void* out, hipStream_t st) {
    const int64_t npad = ntiles * 16;
    if (npad == 0) return;
    hipLaunchKernelGGL(kde_screen_pack_kernel, dim3((unsigned)ceil_div(npad, 256)), dim3(256), 0, st, z, perm, n, npad, is_query ? 1 : 0, (hf8*)out);
    HIP_CHECK(hipGetLastError());
}

// which: PBN_D8_SCREEN_STREAM - 0 the serial kernel, 1 the ring, anything else the dense kernel (the default).  The three write the same words.
#ifndef PBN_SCREEN_NW
#define PBN_SCREEN_NW 2   // sweep waves served by one wave of the dense kernel (2: each fragment load feeds two MFMAs; profiles/r13/c2_bench.txt)
#endif
void launch_screen_d8(const SweepArgs& a_in, int nsplit, int which, hipStream_t st) {
    SweepArgs a = a_in;
    a.nsplit_grid = nsplit;
    if (!a.scr_train || !a.scr_query || !a.live_mask || !a.batch_box || a.pdims != PBN_PRUNE_PD) throw invalid_error("KDE: the d = 8 screen needs its operands, masks and batch boxes");
    const int64_t nwaves = ceil_div(a.nqtiles, PBN_QG_PRUNE);
    const dim3 grid((unsigned)(nwaves * nsplit)), block(64);
    const bool far = a.far_mask != nullptr;   // (the far forms are kernels of their own: without far words the launch is the one it was)
    if (far && (!a.qrow_thr || !a.tile_plain || !a.nypack)) throw invalid_error("KDE: the d = 8 screen's far words need per-query bounds and the plain bits");
    if (which == 0) {
        if (far) hipLaunchKernelGGL(kde_screen_d8_serial_far_kernel, grid, block, 0, st, a);
        else hipLaunchKernelGGL(kde_screen_d8_serial_kernel, grid, block, 0, st, a);
    } else if (which == 1 || a.ntiles < 8) {   // (a unit of the dense kernel is 8 tiles of operands)
        if (far) hipLaunchKernelGGL(kde_screen_d8_far_kernel, grid, block, 0, st, a);
        else hipLaunchKernelGGL(kde_screen_d8_kernel, grid, block, 0, st, a);
    } else {
        // the shipped NW alone is instantiated; an EXPERIMENTS build has both and PBN_SCREEN_NW (the environment) picks
        const int nw = PBN_TUNE(SCREEN_NW, PBN_SCREEN_NW) == 2 ? 2 : 1;
        const dim3 dgrid((unsigned)(ceil_div(nwaves, (int64_t)nw) * nsplit));
#ifdef PBN_EXPERIMENTS
        if (far && nw == 2) hipLaunchKernelGGL(kde_screen_d8_dense_far_kernel<2>, dgrid, block, 0, st, a);
        else if (far) hipLaunchKernelGGL(kde_screen_d8_dense_far_kernel<1>, dgrid, block, 0, st, a);
        else if (nw == 2) hipLaunchKernelGGL(kde_screen_d8_dense_kernel<2>, dgrid, block, 0, st, a);
        else hipLaunchKernelGGL(kde_screen_d8_dense_kernel<1>, dgrid, block, 0, st, a);
#else
        if (far) hipLaunchKernelGGL(kde_screen_d8_dense_far_kernel<PBN_SCREEN_NW>, dgrid, block, 0, st, a);
        else hipLaunchKernelGGL(kde_screen_d8_dense_kernel<PBN_SCREEN_NW>, dgrid, block, 0, st, a);
#endif
    }
    HIP_CHECK(hipGetLastError());
}
