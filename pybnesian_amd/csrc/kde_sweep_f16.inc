// fp32 tables on the 16-bit matrix cores: the f16x2 pack, the four sweep bodies (16x16, grouped, W32, W32P), the far-query fix and their
// launchers.  Included by kde_kernels.hip, inside namespace pbn, after the fp64 sweeps (see there for why it is no unit of its own).

// ------------------------------------------------------------------------------------------------
// fp32 path on the 16-bit matrix cores ("f16x2", round 6; rounds 1-5: "bf16x3"): v_mfma_f32_16x16x4_f32 runs on the same FMA units as
// the VALU (measured: no overlap, tools/microbench.hip), v_mfma_f32_16x16x32_f16 does not (a 16-cycle MFMA costs the VALU ~8 issue
// cycles).  Round 6 measured the f16x2 sweep POWER-bound (profiles/r6/f32_power_bound.txt: 19 % fewer cycles bought a 19 % lower
// clock; 2.0 PFLOP/s of dense bf16 MFMA work): what a pair value costs in wall time is its matrix work, so the contraction is halved -
// every whitened coordinate is split into TWO f16 pieces z^ = a1 + a2 (a1 = f16(z), a2 = f16(z - a1): 22 mantissa bits, |z - z^| <=
// max(2^-22 |z|, 2^-20) - the floor is h_piece's flush rule: a low piece below 2^-20 is stored as zero, so the error is absolute wherever
// |z - a1| < 2^-20, which values next to an f16 value meet up to |z| ~ 4), the three products with weight >= 2^-11 (a1 b1, a1 b2, a2 b1)
// are exact in the f32 accumulator, the fourth (a2 b2,
// <= 2^-22 |a||b|) is dropped, and the norms are taken from the REPRESENTED z^: what the sweep evaluates is -1/2 |z^_t - z^_q|^2 up to
// the dropped products - an input perturbation of 2^-22 relative (fp32 inputs carry 2^-24 themselves) plus <= 2^-22 sum |a2 b2|, where
// bf16x3 paid 2^-24 |z|^2 of cancellation error with its norms from the unsplit z.  K = 3 d + 3 slots instead of 6 d + 3: ONE 32-slot
// MFMA per tile pair up to 9 dimensions (two before), two up to 20.
// f16 has 5 exponent bits: pieces are kept out of its subnormal range and inside its finite range by power-of-two slot scales -
//   coordinate k, slots 3k ... 3k+2:   training (a1, a1 2^-6, a2 2^6)   x   query (b1, b2 2^6, b1 2^-6);
//   a scalar that rides in slots (the training norm -1/2|z^_t|^2, the CKDE / W32 query offsets) is cut by split3s into three pieces
//   x = 2^15 p1 + 2^5 p2 + 2^-6 p3 against the constants (2^15, 2^5, 2^-6) on the other side: |x| <= 2^31, residual <= max(2^-33 |x|, 2^-20);
//   a piece that would be subnormal is stored as zero (its value stays in the residual the next piece takes - the LAST piece's stays
//   unrepresented: the absolute floors 2^-20 above), so the result does not depend on whether the matrix cores flush f16 subnormals.
//   The scaled roles a1 2^-6 and a2 go through the same rule: a1 2^-6 is zero for |a1| < 2^-8 and a2 for |a2| < 2^-14, and the products
//   they carry (|a1 b2| < 2^-19 |b|, |a2 b2| < 2^-25 max(|a|, |b|)) are then missing from the sweeps' exponents - below 2^-22 |z|^2 from
//   |z| = 8 on and below 2^-16 per coordinate under it.  (tests/f16_restatement.py proves the bounds, tests/test_f16_restatement_cpu.py
//   and tests/test_f16_stages_gpu.py assert them.)
// Query coordinates beyond +-65504 (54 000 bandwidths from the centre of the training set) are clamped and counted (PackArgs::far_count).
// Slot s of a row: s = 3 k + r (dimension k, role r) for s < 3 dm, then the three norm pieces; slot s lives in MFMA s / 32, lane group
// (s % 32) / 8, element s % 8.   Fragment arrays: [tile][NB][64 lanes][8 f16].  The query side -1/2|z^_q|^2 - m_q is the MFMA's C operand
// (a persistent register quad), so the VALU does nothing but v_exp_f32 and the sums.
// CKDE: one extra MFMA whose slots are the extra coordinate (0-2), its training norm against the constants (3-5) and the constants against
// the query norm + (m_marg - m_joint) (8-10, rewritten by the lanes of group 1 when an offset is raised).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack_rows_f16_kernel(PackArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t npad = a.ntiles * 16;
    if (r >= npad) return;
    const int64_t tile = r >> 4;
    const int idx = (int)(r & 15);
    const int d = a.d, dm = a.dm;
    const int NB = a.KS;  // number of 32-slot MFMAs of the main contraction
    const bool valid = r < a.n;

    double xc[PBN_MAX_D];
    if (valid) {
        const int64_t rr = a.perm ? (int64_t)a.perm[a.perm_stride > 1 ? r * a.perm_stride : r] : r;
        const int64_t lr = rr < a.n0 ? a.row0 + rr : a.row1 + (rr - a.n0);
        const int64_t src = a.rows ? (int64_t)a.rows[lr] : lr;
        for (int j = 0; j < d; ++j) {
            const float* col = (const float*)a.base + (int64_t)a.cols[j] * a.ld;
            xc[j] = (double)col[src] - a.mu[j];
        }
    }
    hpiece p1[PBN_MAX_D], p2[PBN_MAX_D];
    double nrm = 0.0;
    bool far = false;
    for (int i = 0; i < dm; ++i) {
        double z = 0.0;
        if (valid) {
            const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)i * d;
            for (int j = 0; j <= i; ++j) z = __builtin_fma(w[j], xc[j], z);
        }
        bool cl;
        const double zr = split2(z, p1[i], p2[i], cl);
        far = far || cl;
        nrm = __builtin_fma(zr, zr, nrm);
    }
    float nv = (float)(-0.5 * nrm);
    if (!valid) nv = a.is_query ? 0.0f : (float)PBN_PAD_NORM;
    const hpiece zero = (hpiece)0.0f, c1 = (hpiece)PBN_H_C1, c2 = (hpiece)PBN_H_C2, c3 = (hpiece)PBN_H_C3;
    f16x2_store_row((hf8*)a.pack, NB, tile, idx, dm, p1, p2, nv, a.is_query != 0);
    if (a.is_query) ((float*)a.npack)[tile * 16 + idx] = nv;
    if (a.xpack) {
        double z = 0.0;
        if (valid) {
            const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)dm * d;
            for (int j = 0; j <= dm; ++j) z = __builtin_fma(w[j], xc[j], z);
        }
        hpiece e1, e2, h1, h2, h3;
        bool cl;
        const double zr = split2(z, e1, e2, cl);
        far = far || cl;
        const float hn = (float)(-0.5 * zr * zr);
        split3s(hn, h1, h2, h3);
        const hpiece e1s = h_piece((float)e1 * (1.0f / PBN_H_LO));
        hf8* xp = (hf8*)a.xpack;
        hf8 g0, g1, gz;
#pragma unroll
        for (int j = 0; j < 8; ++j) gz[j] = zero;
        g0 = gz; g1 = gz;
        if (!a.is_query) {
            g0[0] = e1; g0[1] = e1s; g0[2] = e2; g0[3] = h1; g0[4] = h2; g0[5] = h3;
            g1[0] = c1; g1[1] = c2; g1[2] = c3;
        } else {
            g0[0] = e1; g0[1] = e2; g0[2] = e1s; g0[3] = c1; g0[4] = c2; g0[5] = c3;
            g1[0] = h1; g1[1] = h2; g1[2] = h3;
            ((float*)a.xnorm)[tile * 16 + idx] = hn;  // base of the rewritable slots 8..10
        }
        xp[tile * 64 + 0 * 16 + idx] = g0;
        xp[tile * 64 + 1 * 16 + idx] = g1;
        xp[tile * 64 + 2 * 16 + idx] = gz;
        xp[tile * 64 + 3 * 16 + idx] = gz;
    }
    if (a.is_query && a.far_flag) a.far_flag[r] = (far && valid) ? 1 : 0;
}

// Queries beyond the f16 range (PackArgs::far_flag; tens of thousands of bandwidths from the training set): one 256-thread block per query tile;
// a flagged query is evaluated in fp64 against every training row DECODED from the fragments (a1 + a2 - the values the sweeps use), its
// coordinates recomputed unclamped from the table, and its partials are replaced: split 0 gets (max exponent, sum), the others (the same
// offset, 0).  Nothing but a flag test when no query is flagged.
template <bool COND>
__global__ __launch_bounds__(256) void kde_far_fix_kernel(PackArgs a, const hf8* __restrict__ Apack, const hf8* __restrict__ Axpack, int NB, int64_t n_train,
                                                          int64_t ntiles, double* __restrict__ part, int nsplit, int64_t nqtiles) {
    constexpr int P = COND ? 4 : 2;
    __shared__ double zq[PBN_MAX_D + 1];
    __shared__ double red[4][4];
    const int64_t qtile = blockIdx.x;
    for (int qi = 0; qi < 16; ++qi) {
        const int64_t r = qtile * 16 + qi;
        if (r >= a.n || !a.far_flag[r]) continue;   // (uniform over the block)
        const int d = a.d, dm = a.dm;
        __syncthreads();
        if (threadIdx.x == 0) {
            const int64_t rr = a.perm ? (int64_t)a.perm[a.perm_stride > 1 ? r * a.perm_stride : r] : r;
            const int64_t lr = rr < a.n0 ? a.row0 + rr : a.row1 + (rr - a.n0);
            const int64_t src = a.rows ? (int64_t)a.rows[lr] : lr;
            double xc[PBN_MAX_D];
            for (int j = 0; j < d; ++j) xc[j] = (double)((const float*)a.base + (int64_t)a.cols[j] * a.ld)[src] - a.mu[j];
            for (int i = 0; i < d; ++i) {
                const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)i * d;
                double z = 0.0;
                for (int j = 0; j <= i; ++j) z = __builtin_fma(w[j], xc[j], z);
                zq[i] = z;
            }
        }
        __syncthreads();
        double m = -INFINITY, s = 0.0, mj = -INFINITY, sj = 0.0;
        const int spd = f16x2_spd(dm);
        for (int64_t t = threadIdx.x; t < n_train; t += 256) {
            const int64_t tile = t >> 4;
            const int idx = (int)(t & 15);
            double e = 0.0;
            for (int k = 0; k < dm; ++k) {
                const int s1 = spd * k, s2 = spd * k + 2;
                const double a1 = (double)(float)Apack[(tile * NB + (s1 >> 5)) * 64 + ((s1 & 31) >> 3) * 16 + idx][s1 & 7];
                const double a2 = (double)(float)Apack[(tile * NB + (s2 >> 5)) * 64 + ((s2 & 31) >> 3) * 16 + idx][s2 & 7];
                const double df = a1 + a2 * (1.0 / (double)PBN_H_LO) - zq[k];
                e = __builtin_fma(-0.5 * df, df, e);
            }
            if (e > m) { s = s * exp2(m - e) + 1.0; m = e; } else s += exp2(e - m);
            if (COND) {
                const double x1 = (double)(float)Axpack[tile * 64 + idx][0], x2 = (double)(float)Axpack[tile * 64 + idx][2];
                const double df = x1 + x2 * (1.0 / (double)PBN_H_LO) - zq[dm];
                const double ej = __builtin_fma(-0.5 * df, df, e);
                if (ej > mj) { sj = sj * exp2(mj - ej) + 1.0; mj = ej; } else sj += exp2(ej - mj);
            }
        }
        auto merge = [](double& m1, double& s1, double m2, double s2) {
            if (m2 > m1) { s1 = s1 * exp2(m1 - m2) + s2; m1 = m2; } else if (m2 > -INFINITY) s1 += s2 * exp2(m2 - m1);
        };
        for (int off = 32; off >= 1; off >>= 1) {
            merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
            if (COND) merge(mj, sj, __shfl_xor(mj, off), __shfl_xor(sj, off));
        }
        if ((threadIdx.x & 63) == 0) { double* o = red[threadIdx.x >> 6]; o[0] = m; o[1] = s; o[2] = mj; o[3] = sj; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < 4; ++w) {
                merge(m, s, red[w][0], red[w][1]);
                if (COND) merge(mj, sj, red[w][2], red[w][3]);
            }
            for (int sp = 0; sp < nsplit; ++sp) {
                double* o = part + ((int64_t)sp * nqtiles * 16 + r) * P;
                o[0] = m; o[1] = sp == 0 ? s : 0.0;
                if (COND) { o[2] = mj; o[3] = sp == 0 ? sj : 0.0; }
            }
        }
    }
}

// waves per SIMD the pruned fp32 sweeps are compiled for: 4 (<= 128 VGPRs; the fused CKDE shape needs 180 unconstrained and
// spills a few prologue / rare-path values to scratch, none in the tile loop).  One-wave workgroups walking irregular tile
// lists are latency-bound: 2 -> 4 resident waves is worth 12 % of C5's hill-climb and 12-14 % on the fp32 handles;
// 5 (96 VGPRs) spills inside the loop.
#ifndef PBN_F16_PRUNE_WAVES
#define PBN_F16_PRUNE_WAVES 4
#endif
#ifndef PBN_F16_WAVES
#define PBN_F16_WAVES 2   // the same for the unpruned fp32 sweeps of up to 10 dimensions (4 waves per workgroup: workgroups per CU)
#endif
// (Measured again in round 3 and dropped again: the tile sums of 8 / 16 consecutive tiles added in fp32 before they join the fp64 sums -
//  one v_add_f32 instead of v_cvt_f64_f32 + v_add_f64 per (tile, group).  The allocator answers with +35 VGPRs (138 -> 173: two
//  waves per SIMD instead of three): fp32 headline 14.5 -> 17.7 ms, 16.2 ms when held to three waves; tools/f32_variants.sh.)
#ifndef PBN_F16_PAIRSUM
#define PBN_F16_PAIRSUM 1
#endif
#ifndef PBN_F16_BLIND
#define PBN_F16_BLIND 1   // plain fp32 sweeps: batches / chunks of tiles without the per-tile overflow test, checked once at their end
#endif
// Measured (tools/lib_variants.sh, profiles/r3/bf16_blind_probe.txt): pruned fp32 slice sweeps -5...6 % (C5 9.25 -> 9.04 s), unpruned sweeps
// with one MFMA per tile pair -3.6 %; with two (d = 8 headline) +3 %: an unpruned split starts from the offsets of its own first tile, a near
// row later in the split overflows against them (whitened squared distances differ by hundreds), and every such chunk is swept twice - chunks
// of 256 / 1024 tiles 16.3 / 23.9 ms against 13.7.  So: always for the pruned sweeps (offsets from the prepass bounds: nothing to redo), chunks
// of 64 tiles for the unpruned sweeps - the two-MFMA ones only since their offsets look at 16 tiles spread over the split (PBN_F16_PROBES).
#ifndef PBN_F16_PROBES
#define PBN_F16_PROBES 16   // with them the two-MFMA unpruned sweep gains from the blind chunks too: d = 8 headline 13.89 -> 13.56 ms (4 probes: 13.82)
#endif
#ifndef PBN_F16_FSUM
#define PBN_F16_FSUM 1
#endif
#ifndef PBN_F16_PRUNE_SCHED
#define PBN_F16_PRUNE_SCHED 1   // pruned blind form: the (tile, 4 groups) stream placed by sched_group_barrier (process_tile)
#endif
#ifndef PBN_F16_BLIND_CHUNK
#define PBN_F16_BLIND_CHUNK 64
#endif
#ifndef PBN_F16_BLIND_NB2
#define PBN_F16_BLIND_NB2 1   // (0 without the probe tiles of PBN_F16_PROBES: see above)
#endif
template <int NB, bool COND, int QG, bool PRUNE>
__device__ __forceinline__ void kde_sweep_f16_body(const SweepArgs& a, const unsigned bid) {
    using V = f4;
    constexpr int WPB = sweep_block_threads(PRUNE) / 64;   // pruned: one wave per workgroup (see kde_sweep_kernel)
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lg = lane >> 4;
    int qx, split;
    if (PRUNE) pruned_block(a, WPB * QG, bid, qx, split); else xcd_block(qx, split);
    const int64_t qt0 = ((int64_t)qx * WPB + wave) * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;

    const PBN_GLOBAL hf8* __restrict__ Ap = (const PBN_GLOBAL hf8*)a.Apack;
    const PBN_GLOBAL hf8* __restrict__ Xp = (const PBN_GLOBAL hf8*)a.Axpack;
    const PBN_GLOBAL hf8* __restrict__ Bp = (const PBN_GLOBAL hf8*)a.Bpack;
    const PBN_GLOBAL float* __restrict__ NYp = (const PBN_GLOBAL float*)a.nypack;
    const PBN_GLOBAL hf8* __restrict__ BXp = (const PBN_GLOBAL hf8*)a.Bxpack;
    const PBN_GLOBAL float* __restrict__ XNp = (const PBN_GLOBAL float*)a.Bxnorm;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL double* __restrict__ QLp = (const PBN_GLOBAL double*)a.qlb;

    hf8 b[QG][NB];
    float ny[QG], m[QG];
    V cmv[QG];
    double sum[QG];
    hf8 bx[QG];
    float xn[QG], mj[QG];
    double sumj[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) b[g][mb] = Bp[(qt * NB + mb) * 64 + lane];
        ny[g] = NYp[qt * 16 + (lane & 15)];
        sum[g] = 0.0;
        if (COND) { bx[g] = BXp[qt * 64 + lane]; xn[g] = XNp[qt * 16 + (lane & 15)]; sumj[g] = 0.0; }
    }
    // tile pruning, as in kde_sweep_kernel
    double wlo[PBN_PRUNE_PD_NARROW] = {}, whi[PBN_PRUNE_PD_NARROW] = {}, wthr = 0;
    const int pd = PRUNE ? a.pdims : 0;
    if (PRUNE) {
        wthr = INFINITY;
#pragma unroll
        for (int k = 0; k < PBN_PRUNE_PD_NARROW; ++k) { wlo[k] = INFINITY; whi[k] = -INFINITY; }
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
            const double th = QTp[qt];
            wthr = th < wthr ? th : wthr;
#pragma unroll
            for (int k = 0; k < PBN_PRUNE_PD_NARROW; ++k)
                if (k < pd) {
                    const double l = QBp[qt * 2 * pd + k], h = QBp[qt * 2 * pd + pd + k];
                    wlo[k] = l < wlo[k] ? l : wlo[k];
                    whi[k] = h > whi[k] ? h : whi[k];
                }
        }
        wthr -= a.prune_margin;
    }
    auto set_bx = [&](int g) {  // slots 8..10 (lane group 1, elements 0..2) <- split3s(xn + m - mj)
        if (lg == 1) {
            hpiece q1, q2, q3;
            split3s(xn[g] + (m[g] - mj[g]), q1, q2, q3);
            bx[g][0] = q1; bx[g][1] = q2; bx[g][2] = q3;
        }
    };
    auto load_tile = [&](int64_t t, hf8 (&f)[NB], hf8& x) {
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) f[mb] = Ap[(t * NB + mb) * 64 + lane];
        if (COND) x = Xp[t * 64 + lane];
    };
    auto mfma_main = [&](const hf8 (&f)[NB], int g, V c) {
#pragma unroll
        for (int mb = 0; mb < NB; ++mb) c = __builtin_amdgcn_mfma_f32_16x16x32_f16(f[mb], b[g][mb], c, 0, 0, 0);
        return c;
    };

    // ---- prologue: offsets from the first tile ------------------------------------------------------------
    {
        hf8 f[NB], x;
        load_tile(t0, f, x);
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            const V c0 = {ny[g], ny[g], ny[g], ny[g]};
            V acc = mfma_main(f, g, c0);
            const float mx = colmax<float>(max4<float>(acc));
            m[g] = mx;
            const float cm = ny[g] - mx;
            cmv[g] = V{cm, cm, cm, cm};
            if (COND) {
                V accj = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, bx[g], acc, 0, 0, 0);  // slots 8..10 hold xn (m = mj = 0)
                mj[g] = colmax<float>(max4<float>(accj));
                set_bx(g);
            }
        }
        // plain unpruned sweeps: the offsets also look at PBN_F16_PROBES - 1 more tiles spread over the split - a split whose first 16
        // rows all lie far from a query otherwise meets rows hundreds of exponent units above its offset, and every such tile takes the
        // rescue path (or, in a blind chunk, costs the chunk a second pass)
        if constexpr (!COND && !PRUNE && PBN_F16_PROBES > 1) {
#pragma unroll 1
            for (int pz = 1; pz < PBN_F16_PROBES; ++pz) {
                load_tile(t0 + (t1 - t0) * pz / PBN_F16_PROBES, f, x);
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    const V c0 = {ny[g], ny[g], ny[g], ny[g]};
                    const V acc = mfma_main(f, g, c0);
                    const float mx = colmax<float>(max4<float>(acc));
                    if (mx > m[g]) {
                        m[g] = mx;
                        const float cm = ny[g] - mx;
                        cmv[g] = V{cm, cm, cm, cm};
                    }
                }
            }
        }
    }

    // pruned sweeps: offsets from the prepass bounds where they lie above the first tile's maximum (see kde_sweep_kernel)
    bool lbm[QG], lbmj[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) lbm[g] = lbmj[g] = false;
    if constexpr (PRUNE) {
        if (a.qlb) {
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
                const float lb = (float)QLp[qt * 16 + (lane & 15)];
                // a bound so large that fp32 cannot hold it to a fraction of a unit (a query ~2000 bandwidths out) is not used:
                // the first tile's offset comes with a term that is known to survive the rounding, the bound does not
                const bool fin = __builtin_fabsf(lb) < 0x1p22f;
                lbm[g] = fin && lb > m[g];
                if (lbm[g]) {
                    m[g] = lb;
                    const float cm = ny[g] - lb;
                    cmv[g] = V{cm, cm, cm, cm};
                }
                if (COND) {
                    lbmj[g] = fin && lb > mj[g];
                    if (lbmj[g]) mj[g] = lb;
                    set_bx(g);
                }
            }
        }
    }

    // Plain unpruned sweeps (the else branch): all groups' MFMAs are issued before the first exponential so that the matrix pipe works under the
    // VALU's exponentials, one overflow test per tile, the rare path redoes a group (C2 fp32: 15.2 -> 14.1 ms).  The
    // fused CKDE sweep and the pruned sweeps keep the group-by-group form: with two accumulator sets per group in flight,
    // or one wave per SIMD less, the other form loses (C5's sweeps 33 -> 40 s; pruned d = 1 plain sweep 8.3 -> 10.2 ms).
    // plain unpruned sweeps (PBN_F16_PAIRSUM): the sums of the two tiles of a loop iteration are added in fp32 and join the fp64 sums
    // together - one v_cvt_f64_f32 + v_add_f64 per group and TWO tiles
    constexpr bool PAIRSUM = !COND && !PRUNE && PBN_F16_PAIRSUM;
    float pend[PAIRSUM ? QG : 1];
#pragma unroll
    for (int g = 0; g < (PAIRSUM ? QG : 1); ++g) pend[g] = 0.f;
    // PBN_F16_FSUM (round 4): inside a BLIND batch / chunk (at most 64 tiles, looked at once at its end) the tile sums are added in fp32 and
    // join the fp64 sums once per batch - the v_cvt_f64_f32 + v_add_f64 per (tile, group) were 8 of the ~60 issue slots of a tile's four
    // groups.  At most 64 fp32 additions of positive terms: <= 4e-6 relative on a sum, against the fp32 bar of 1e-3.
    constexpr bool FSUM = !COND && PBN_F16_BLIND && PBN_F16_FSUM;
    float fs[FSUM ? QG : 1];
#pragma unroll
    for (int g = 0; g < (FSUM ? QG : 1); ++g) fs[g] = 0.f;
    auto flush_fs = [&]() {
        if constexpr (FSUM) {
#pragma unroll
            for (int g = 0; g < QG; ++g) { sum[g] += (double)fs[g]; fs[g] = 0.f; }
        }
    };
    // `blind` (plain sweeps, PBN_F16_BLIND): no overflow test and no rescue path - the caller looks at the fp64 sums once per batch / chunk
    // of tiles and redoes it checked if one of them went bad (as the fp64 sweeps do).  An exponent overflows only 128 units above its
    // query's offset, and the offsets start from the prepass bounds (pruned) or from a tile of the split itself.
    auto process_tile = [&](const hf8 (&f)[NB], const hf8& x, const int bit = 0, const bool flush = true, auto blind = std::false_type{}) {
        constexpr bool BLIND = decltype(blind)::value;
        if constexpr (COND || PRUNE) {
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                V acc = mfma_main(f, g, cmv[g]);
                V accj;
                if (COND) accj = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, bx[g], acc, 0, 0, 0);
                float e0 = Tr<float>::ex2(acc[0]), e1 = Tr<float>::ex2(acc[1]), e2 = Tr<float>::ex2(acc[2]), e3 = Tr<float>::ex2(acc[3]);
                float ts = (e0 + e1) + (e2 + e3);
                float tsj = 0;
                bool bad = BLIND ? false : !(ts < Tr<float>::big());
                if (COND) {
                    float j0 = Tr<float>::ex2(accj[0]), j1 = Tr<float>::ex2(accj[1]), j2 = Tr<float>::ex2(accj[2]), j3 = Tr<float>::ex2(accj[3]);
                    tsj = (j0 + j1) + (j2 + j3);
                    bad = bad || !(tsj < Tr<float>::big());
                }
                if (!BLIND && __builtin_expect(__any(bad), 0)) {
                    float mx = colmax<float>(max4<float>(acc));
                    if (mx > 0.f) {
                        m[g] += mx;
                        const float cm = ny[g] - m[g];
                        cmv[g] = V{cm, cm, cm, cm};
                        sum[g] *= exp2(-(double)mx);
                        acc -= mx;
                    }
                    e0 = Tr<float>::ex2(acc[0]); e1 = Tr<float>::ex2(acc[1]); e2 = Tr<float>::ex2(acc[2]); e3 = Tr<float>::ex2(acc[3]);
                    ts = (e0 + e1) + (e2 + e3);
                    if (COND) {
                        float mxj = colmax<float>(max4<float>(accj));
                        if (mxj > 0.f) {
                            mj[g] += mxj;
                            sumj[g] *= exp2(-(double)mxj);
                            accj -= mxj;
                        }
                        set_bx(g);
                        float j0 = Tr<float>::ex2(accj[0]), j1 = Tr<float>::ex2(accj[1]), j2 = Tr<float>::ex2(accj[2]), j3 = Tr<float>::ex2(accj[3]);
                        tsj = (j0 + j1) + (j2 + j3);
                    }
                }
                if constexpr (BLIND && FSUM) fs[g] += ts;
                else sum[g] += (double)ts;
                if (COND) sumj[g] += (double)tsj;
            }
#if PBN_F16_PRUNE_SCHED
            // Round 6: the blind pruned form's stream placed - M0 M1 [E0] M2 [E1] M3 [E2] [E3], E = the four exponentials and four additions of a
            // group: no exponential reads an accumulator younger than one group's work, the MFMAs issue between the VALU blocks instead of four
            // in a row followed by the hazard's s_nops
            if constexpr (BLIND && !COND && NB == 1 && QG == 4) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x400, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x400, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x400, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x400, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
            }
#endif
        } else {
            V acc[QG], accj[QG];
            float ts[QG], tsj[QG];
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                acc[g] = mfma_main(f, g, cmv[g]);
                if (COND) accj[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, bx[g], acc[g], 0, 0, 0);
            }
            bool bad = false;
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                const float e0 = Tr<float>::ex2(acc[g][0]), e1 = Tr<float>::ex2(acc[g][1]), e2 = Tr<float>::ex2(acc[g][2]), e3 = Tr<float>::ex2(acc[g][3]);
                ts[g] = (e0 + e1) + (e2 + e3);
                tsj[g] = 0;
                if constexpr (!BLIND) bad = bad || !(ts[g] < Tr<float>::big());
                if (COND) {
                    const float j0 = Tr<float>::ex2(accj[g][0]), j1 = Tr<float>::ex2(accj[g][1]), j2 = Tr<float>::ex2(accj[g][2]), j3 = Tr<float>::ex2(accj[g][3]);
                    tsj[g] = (j0 + j1) + (j2 + j3);
                    bad = bad || !(tsj[g] < Tr<float>::big());
                }
            }
            if (!BLIND && __builtin_expect(__any(bad), 0)) {
#pragma unroll
                for (int g = 0; g < QG; ++g) {
                    bool badg = !(ts[g] < Tr<float>::big());
                    if (COND) badg = badg || !(tsj[g] < Tr<float>::big());
                    if (!__any(badg)) continue;
                    float mx = colmax<float>(max4<float>(acc[g]));
                    if (mx > 0.f) {
                        m[g] += mx;
                        const float cm = ny[g] - m[g];
                        cmv[g] = V{cm, cm, cm, cm};
                        if constexpr (PAIRSUM) { sum[g] += (double)pend[g]; pend[g] = 0.f; }
                        sum[g] *= exp2(-(double)mx);
                        acc[g] -= mx;
                    }
                    const float e0 = Tr<float>::ex2(acc[g][0]), e1 = Tr<float>::ex2(acc[g][1]), e2 = Tr<float>::ex2(acc[g][2]), e3 = Tr<float>::ex2(acc[g][3]);
                    ts[g] = (e0 + e1) + (e2 + e3);
                    if (COND) {
                        float mxj = colmax<float>(max4<float>(accj[g]));
                        if (mxj > 0.f) {
                            mj[g] += mxj;
                            sumj[g] *= exp2(-(double)mxj);
                            accj[g] -= mxj;
                        }
                        set_bx(g);
                        const float j0 = Tr<float>::ex2(accj[g][0]), j1 = Tr<float>::ex2(accj[g][1]), j2 = Tr<float>::ex2(accj[g][2]), j3 = Tr<float>::ex2(accj[g][3]);
                        tsj[g] = (j0 + j1) + (j2 + j3);
                    }
                }
            }
#pragma unroll
            for (int g = 0; g < QG; ++g) {
                if constexpr (BLIND && FSUM) {
                    fs[g] += ts[g];
                } else if constexpr (PAIRSUM) {
                    if (flush) { sum[g] += (double)(pend[g] + ts[g]); pend[g] = 0.f; } else pend[g] = ts[g];
                } else {
                    sum[g] += (double)ts[g];
                }
                if (COND) sumj[g] += (double)tsj[g];
            }
        }
    };

    hf8 fA[NB], fB[NB], xA, xB;
    // (Measured and dropped, profiles/r3/prune_stream_probe.txt: the visit masks of the whole split taken first - lane w keeping the mask of
    //  batch w - and the kept tiles then walked as ONE stream across the batches through a ring of 3 or 4 tile fragments, the next set bit
    //  coming from scalar code on a v_readlane'd word.  The fp32 slice sweeps ran 9-12 % SLOWER (1.92 against 1.71 ms at 720 000 x 80 000,
    //  d = 2), C5 9.67 against 9.36 s, with 3 waves per SIMD 10.7 s: the loop is not waiting for its tiles - four waves per SIMD cover the
    //  one tile of prefetch - and the ring's 8-12 registers push the 128-register kernel into scratch.)
    if constexpr (PRUNE) {
        if (a.count_redo && lane == 0) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0));
        for (int64_t tb = t0; tb < t1; tb += 64) {   // see kde_sweep_kernel
            // (one mask per WAVE here: per-group masks as in the fp64 kernel - prune_group_mask - were measured and dropped for the
            //  fp32 kernels, which live on occupancy and straight-line issue: 1e6 x 1e5 handles +15...20 %, C5 15.8 -> 16.4 s)
            const unsigned long long mask = prune_visit_mask(TBp, pd, tb, t1, wlo, whi, wthr, lane);
            if (!mask) continue;
            if (a.count_redo && lane == 0) atomicAdd(&g_sweep_visit, (unsigned long long)__builtin_popcountll(mask));
            auto run_batch = [&](unsigned long long mk, auto blind) {
                // unconditional prefetch of the next kept tile (see kde_sweep_body: a conditional one costs a vmcnt(0) per tile)
                int b = __builtin_ctzll(mk);
                mk &= mk - 1;
                load_tile(tb + b, fA, xA);
                for (;;) {
                    const bool more = mk != 0;
                    const int b2 = more ? __builtin_ctzll(mk) : b;
                    mk &= mk - 1;
                    load_tile(tb + b2, fB, xB);
                    process_tile(fA, xA, b, true, blind);
                    if (!more) break;
                    const bool more2 = mk != 0;
                    const int b3 = more2 ? __builtin_ctzll(mk) : b2;
                    mk &= mk - 1;
                    load_tile(tb + b3, fA, xA);
                    process_tile(fB, xB, b2, true, blind);
                    if (!more2) break;
                    b = b3;
                }
            };
            if constexpr (!COND && PBN_F16_BLIND) {
                double saved[QG];
#pragma unroll
                for (int g = 0; g < QG; ++g) saved[g] = sum[g];
                run_batch(mask, std::true_type{});
                flush_fs();
                bool bad = false;
#pragma unroll
                for (int g = 0; g < QG; ++g) bad = bad || !(sum[g] < 0x1p1000);
                if (__builtin_expect(__any(bad), 0)) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) sum[g] = saved[g];
                    run_batch(mask, std::false_type{});
                }
            } else {
                run_batch(mask, std::false_type{});
            }
        }
    } else {
        auto run_range = [&](int64_t c0, int64_t c1, auto blind) {
            load_tile(c0, fA, xA);
            for (int64_t t = c0; t < c1; t += 2) {
                const bool second = t + 1 < c1;
                load_tile(second ? t + 1 : t, fB, xB);
                process_tile(fA, xA, 0, !second, blind);          // PAIRSUM: the first tile's sums wait for the second one's
                load_tile(t + 2 < c1 ? t + 2 : t, fA, xA);
                if (second) process_tile(fB, xB, 0, true, blind);
            }
        };
        if constexpr (!COND && PBN_F16_BLIND && (NB == 1 || PBN_F16_BLIND_NB2)) {
            constexpr int64_t CHUNK = PBN_F16_BLIND_CHUNK;   // tiles (an even number: the pair sums are flushed at its end)
            for (int64_t c0 = t0; c0 < t1; c0 += CHUNK) {
                const int64_t c1 = c0 + CHUNK < t1 ? c0 + CHUNK : t1;
                double saved[QG];
#pragma unroll
                for (int g = 0; g < QG; ++g) saved[g] = sum[g];
                run_range(c0, c1, std::true_type{});
                flush_fs();
                bool bad = false;
#pragma unroll
                for (int g = 0; g < QG; ++g) bad = bad || !(sum[g] < 0x1p1000);
                if (__builtin_expect(__any(bad), 0)) {
#pragma unroll
                    for (int g = 0; g < QG; ++g) sum[g] = saved[g];
                    run_range(c0, c1, std::false_type{});
                }
            }
        } else {
            run_range(t0, t1, std::false_type{});
        }
    }

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
        // The offsets are exponents of pairs of this split's first tile.  When the exponents are so large that their fp32
        // rounding (ulp(|e|) >> 1: queries ~10^6 bandwidths away) makes the second evaluation of that tile underflow, the
        // sum can come out empty although it holds at least the offset's own term: count that term.  (A split whose tiles
        // were all pruned gets the same term: below 2^-64 of the query's sum by the pruning rule.)
        // (not when the offset is a prepass bound: no term of this split stands behind it, an empty sum is empty)
        if (s == 0.0 && (m[g] - m[g]) == 0.f && !lbm[g]) s = 1.0;
        if (COND && sj == 0.0 && (mj[g] - mj[g]) == 0.f && !lbmj[g]) sj = 1.0;
        if (lg == 0 && qt0 + g < a.nqtiles) {
            PBN_GLOBAL double* o = part + ((int64_t)split * a.nqtiles * 16 + (qt0 + g) * 16 + lane) * P;
            o[0] = (double)m[g];
            o[1] = s;
            if (COND) { o[2] = (double)mj[g]; o[3] = sj; }
        }
    }
}

template <int NB, bool COND, int QG, bool PRUNE>
__global__ __launch_bounds__(sweep_block_threads(PRUNE), PRUNE ? PBN_F16_PRUNE_WAVES : (NB <= 2 ? PBN_F16_WAVES : 2)) void kde_sweep_f16_kernel(SweepArgs a) {
    kde_sweep_f16_body<NB, COND, QG, PRUNE>(a, blockIdx.x);
}

// grouped launch of the pruned plain fp32 sweeps (see kde_sweep_group_kernel)
template <int NB>
__global__ __launch_bounds__(sweep_block_threads(true), PBN_F16_PRUNE_WAVES) void kde_sweep_f16_group_kernel(GSweepArgs g) {
    const int u = g.wg_unit[blockIdx.x >> 6];
    const GSweepUnit& su = g.units[u];
    const unsigned bid = (unsigned)((int64_t)blockIdx.x - su.wg0);
    if (bid >= (unsigned)su.nwg) return;
    SweepArgs a;
    a.Apack = su.Apack; a.nxpack = su.nxpack; a.Axpack = nullptr;
    a.Bpack = su.Bpack; a.nypack = su.nypack; a.Bxpack = nullptr; a.Bxnorm = nullptr;
    a.ntiles = su.ntiles; a.nqtiles = su.nqtiles; a.tiles_per_split = su.tps;
    a.fold = 0; a.count_redo = g.count_redo; a.wmul = 0;
    a.prune = 1; a.pdims = su.pdims; a.prune_margin = g.prune_margin > 0.0 ? g.prune_margin : (double)su.margin;
    a.tile_box = su.tile_box; a.qtile_box = su.qtile_box; a.qtile_thr = su.qtile_thr; a.qlb = su.qlb;
    a.nsplit_grid = su.nsplit; a.part = su.part; a.group_masks = 0;
    kde_sweep_f16_body<NB, false, PBN_F16_QG_PRUNE, true>(a, bid);
}

// ------------------------------------------------------------------------------------------------
// W32 form of the plain unpruned fp32 sweep (round 6): the SAME packed f16x2 fragments contracted by v_mfma_f32_32x32x16_f16 -
// 32 training rows x 32 queries per accumulator, 16 pair values per lane and MFMA chain instead of 4.  An MFMA holds the SIMD's vector
// issue for 8 cycles whatever its shape (MI355X_MICROARCH.md, "vector-instruction ISSUE cost"), so the matrix side of a pair value
// costs 2 issue cycles at two 32-slot blocks (d = 5...9) instead of 4: the instruction-count bound of the d = 8 headline falls from
// 64 to 56 issue cycles per 256 pair values (v_exp_f32 8 + v_add_f32 4 per value, + the MFMAs).  Round 4 measured this shape
// compiler-scheduled and dropped it (14.1 against 13.05 ms: the four dependent 32-cycle MFMAs of a super-group are a longer chain than
// the wave's own exponentials cover).  Here the stream is PLACED: the loop is software-pipelined by one super-group - the chain of
// (tile pair, super-group s) issues while the 16 exponentials and 16 additions of the previous chain's accumulator run -, and
// __builtin_amdgcn_sched_group_barrier pins the order [MFMA, 4 x v_exp_f32, 4 x v_add_f32] x 4 per phase, so that no MFMA waits for
// its predecessor and no v_exp_f32 reads an accumulator younger than one phase.
//   * lane l: query column l % 32 of the super-group, half h = l / 32.  MFMA j of a chain takes slots 16 j + 8 h ... + 7 = block j / 2,
//     lane group 2 (j % 2) + h of the 16x16x32 fragment layout: the fragment arrays are read through another index map, nothing is repacked.
//     A training tile PAIR (rows 0-15 from one 16-row tile, 16-31 from another) feeds the A operand: lanes with (l % 32) < 16 read the first.
//   * the query side -1/2|z_q|^2 - m_q cannot be the C operand (16 registers per super-group): it rides in the three LAST slots of the
//     contraction (32 NB - 3 ...: split3 on the query side, rewritten when an offset moves; ones on the training side, written by
//     pack_rows_f16_kernel when 6 dm + 6 <= 32 NB - the 16x16 kernels meet zeros on the query side there), and C is the inline constant 0.
//   * accumulator row of register r: 8 (r / 4) + 4 h + r % 4 - registers 8...15 are the second tile of the pair (dropped for an odd tail).
//   * blind chunks of 64 tiles with fp32 tile sums, offsets from 16 probe tile pairs, checked redo: as kde_sweep_f16_body.
// Replaces kde/opencl_kernels/KDE.cl.src:115-121,143-170 for fp32 tables of 5...9 whitened dimensions.
// ------------------------------------------------------------------------------------------------
typedef float f16v __attribute__((ext_vector_type(16)));
#ifndef PBN_F16_W32_WAVES
#define PBN_F16_W32_WAVES 2
#endif
#ifndef PBN_F16_W32_SCHED
#define PBN_F16_W32_SCHED 1
#endif

template <int NB>
__global__ __launch_bounds__(256, PBN_F16_W32_WAVES) void kde_sweep_f16_w32_kernel(SweepArgs a) {
    constexpr int NJ = 2 * NB;   // MFMAs per chain
    constexpr int S = 2;         // super-groups of 32 queries per wave (= the 4 x 16 queries of the 16x16 kernel's wave: same grid)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, col = lane & 31, sub = col >> 4, idx = col & 15;
    int qx, split;
    xcd_block(qx, split);
    const int64_t qt0 = ((int64_t)qx * 4 + wave) * (2 * S);
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;

    const PBN_GLOBAL hf8* __restrict__ Ap = (const PBN_GLOBAL hf8*)a.Apack;
    const PBN_GLOBAL hf8* __restrict__ Bp = (const PBN_GLOBAL hf8*)a.Bpack;
    const PBN_GLOBAL float* __restrict__ NYp = (const PBN_GLOBAL float*)a.nypack;
    const int loff = half * 16 + idx;   // lane's place inside a (tile, block, j % 2) group of 32 fragment lanes

    hf8 b[S][NJ];
    float ny[S], m[S];
    double sum[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        int64_t qt = qt0 + 2 * s + sub;
        qt = qt < a.nqtiles ? qt : a.nqtiles - 1;
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[s][j] = Bp[(qt * NB + (j >> 1)) * 64 + (j & 1) * 32 + loff];
        ny[s] = NYp[qt * 16 + idx];
        m[s] = 0.f;
        sum[s] = 0.0;
    }
    auto set_off = [&](int s) {   // slots 32 NB - 3 ... of the query side <- split3(-1/2|z_q|^2 - m_q)
        hpiece q1, q2, q3;
        split3s(ny[s] - m[s], q1, q2, q3);
        if (half == 1) { b[s][NJ - 1][5] = q1; b[s][NJ - 1][6] = q2; b[s][NJ - 1][7] = q3; }
    };
    auto load_pair = [&](int64_t ta, int64_t tb, hf8 (&f)[NJ]) {
        const int64_t t = sub ? tb : ta;
#pragma unroll
        for (int j = 0; j < NJ; ++j) f[j] = Ap[(t * NB + (j >> 1)) * 64 + (j & 1) * 32 + loff];
    };
    auto chain = [&](const hf8 (&f)[NJ], int s) {
        f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[j], b[s][j], c, 0, 0, 0);
        return c;
    };
    auto colmax32 = [&](const f16v& v, int nr) {   // largest of the lane's first nr registers, then over the two halves of the column
        float mx = v[0];
#pragma unroll
        for (int r = 1; r < 16; ++r)
            if (r < nr) mx = v[r] > mx ? v[r] : mx;
        const float o = __shfl_xor(mx, 32);
        return mx > o ? mx : o;
    };

    // ---- offsets: the largest exponent of PBN_F16_PROBES tile pairs spread over the split (see kde_sweep_f16_body) ----
    {
#pragma unroll
        for (int s = 0; s < S; ++s) set_off(s);   // m = 0
        float mm[S];
#pragma unroll 1
        for (int pz = 0; pz < PBN_F16_PROBES; ++pz) {
            const int64_t ta = t0 + (t1 - t0) * pz / PBN_F16_PROBES;
            const int64_t tb = ta + 1 < t1 ? ta + 1 : ta;
            hf8 f[NJ];
            load_pair(ta, tb, f);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float mx = colmax32(chain(f, s), 16);
                mm[s] = (pz == 0 || mx > mm[s]) ? mx : mm[s];
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) { m[s] = mm[s]; set_off(s); }
    }

    // ---- checked form (the redo of a chunk whose sums overflowed, and the odd tail): one tile pair, super-group by super-group ----
    auto checked_pair = [&](int64_t ta, int64_t tb, const bool second) {
        hf8 f[NJ];
        load_pair(ta, tb, f);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            f16v acc = chain(f, s);
            const int nr = second ? 16 : 8;
            auto tile_sum = [&]() {
                float ts = 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (r < nr) ts += Tr<float>::ex2(acc[r]);
                return ts;
            };
            float ts = tile_sum();
            if (__builtin_expect(__any(!(ts < Tr<float>::big())), 0)) {
                const float mx = colmax32(acc, nr);
                if (mx > 0.f) {
                    m[s] += mx;
                    set_off(s);
                    sum[s] *= exp2(-(double)mx);
                    acc -= mx;
                }
                ts = tile_sum();
            }
            sum[s] += (double)ts;
        }
    };

    // ---- blind run of nbody x 4 tiles from c0: software-pipelined by one super-group, the stream placed by hand ----
    float fs[S];
    auto expsum = [&](const f16v& v) {   // 16 v_exp_f32 + 15 v_add_f32: four quads (e0 + e1) + (e2 + e3), added in order
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e0 = Tr<float>::ex2(v[4 * k]), e1 = Tr<float>::ex2(v[4 * k + 1]), e2 = Tr<float>::ex2(v[4 * k + 2]), e3 = Tr<float>::ex2(v[4 * k + 3]);
            q[k] = (e0 + e1) + (e2 + e3);
        }
        return ((q[0] + q[1]) + q[2]) + q[3];
    };
    auto place = [&]() {   // [MFMA, 4 trans, 4 VALU] x NJ
#if PBN_F16_W32_SCHED
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 16 / NJ, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 16 / NJ, 0);
        }
#endif
    };
    // contiguous tile pairs: the lane's byte offset inside a pair is fixed, the pair's base is wave-uniform (scalar address arithmetic)
    const uint32_t lane_b = (uint32_t)((sub * NB * 64 + loff) * 16);
    auto load_run = [&](int64_t t, hf8 (&f)[NJ]) {
        const PBN_GLOBAL char* base = (const PBN_GLOBAL char*)Ap + t * (int64_t)(NB * 64 * 16);
#pragma unroll
        for (int j = 0; j < NJ; ++j) f[j] = *(const PBN_GLOBAL hf8*)(base + lane_b + (uint32_t)(((j >> 1) * 64 + (j & 1) * 32) * 16));
    };
    auto blind_run = [&](int64_t c0, int nbody) {
        hf8 fA[NJ], fB[NJ];
        f16v acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] = -1000.f;   // the pipeline's first exponentials: 2^-1000 = 0
        load_run(c0, fA);
        int64_t t = c0;
#pragma unroll 1
        for (int i = 0; i < nbody; ++i, t += 4) {
            load_run(t + 2, fB);
            acc0 = chain(fA, 0);
            fs[1] += expsum(acc1);
            place();
            acc1 = chain(fA, 1);
            fs[0] += expsum(acc0);
            place();
            load_run(i + 1 < nbody ? t + 4 : t, fA);   // the last body's prefetch stays inside the run
            acc0 = chain(fB, 0);
            fs[1] += expsum(acc1);
            place();
            acc1 = chain(fB, 1);
            fs[0] += expsum(acc0);
            place();
        }
        fs[1] += expsum(acc1);
    };

    for (int64_t c0 = t0; c0 < t1; c0 += PBN_F16_BLIND_CHUNK) {
        const int64_t c1 = c0 + PBN_F16_BLIND_CHUNK < t1 ? c0 + PBN_F16_BLIND_CHUNK : t1;
        const int nbody = (int)((c1 - c0) >> 2);
        const int64_t cb = c0 + 4 * (int64_t)nbody;   // [cb, c1): at most three tiles, checked
        if (nbody) {
#pragma unroll
            for (int s = 0; s < S; ++s) fs[s] = 0.f;
            blind_run(c0, nbody);
            bool bad = false;
#pragma unroll
            for (int s = 0; s < S; ++s) bad = bad || !(fs[s] < Tr<float>::big());
            if (__builtin_expect(__any(bad), 0)) {
#pragma unroll 1
                for (int64_t t = c0; t < cb; t += 2) checked_pair(t, t + 1, true);
            } else {
#pragma unroll
                for (int s = 0; s < S; ++s) sum[s] += (double)fs[s];
            }
        }
#pragma unroll 1
        for (int64_t t = cb; t < c1; t += 2) checked_pair(t, t + 1 < c1 ? t + 1 : t, t + 1 < c1);
    }

    PBN_GLOBAL double* part = (PBN_GLOBAL double*)a.part;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double v = sum[s];
        v += __shfl_xor(v, 32);
        if (v == 0.0 && (m[s] - m[s]) == 0.f) v = 1.0;   // an empty sum holds at least the offset's own term (see kde_sweep_f16_body)
        const int64_t qt = qt0 + 2 * s + sub;
        if (half == 0 && qt < a.nqtiles) {
            PBN_GLOBAL double* o = part + ((int64_t)split * a.nqtiles * 16 + qt * 16 + idx) * 2;
            o[0] = (double)m[s];
            o[1] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// W32 form of the PRUNED plain fp32 sweeps (round 6; stand-alone handles and the grouped launches of the score engine: C5).  The kept tiles of
// a split - whatever batch they come from - are taken two at a time as the A operand of v_mfma_f32_32x32x16_f16 (any two 16-row tiles make a
// 32-row operand: lanes with (lane % 32) < 16 read the first), the wave's four 16-query groups are its two 32-query super-groups: per 2 048
// pair values 4 MFMAs instead of 8 (4 issue cycles per 256 values instead of 8), the stream software-pipelined by one super-group and placed as
// in kde_sweep_f16_w32_kernel.  The whole split is ONE blind region (fp32 tile sums: at most a few hundred pair sums per split, <= 3e-5
// relative, against the fp32 bar of 1e-3; offsets from the prepass bounds: an overflow is rare) - a wave whose sums came out bad walks its kept
// tiles again through the checked form.  An odd kept tile goes through the checked form too.  Visit masks: one per wave and 64-tile batch, as
// in kde_sweep_f16_body.
// ------------------------------------------------------------------------------------------------
#ifndef PBN_F16_W32P
#define PBN_F16_W32P 1
#endif
template <int NB>
__device__ __forceinline__ void kde_sweep_f16_w32p_body(const SweepArgs& a, const unsigned bid) {
    constexpr int NJ = 2 * NB, S = 2, QG = PBN_F16_QG_PRUNE;
    static_assert(QG == 2 * S, "the wave's query groups are its two 32-query super-groups");
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5, col = lane & 31, sub = col >> 4, idx = col & 15;
    int qx, split;
    pruned_block(a, QG, bid, qx, split);
    const int64_t qt0 = (int64_t)qx * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL hf8* __restrict__ Ap = (const PBN_GLOBAL hf8*)a.Apack;
    const PBN_GLOBAL hf8* __restrict__ Bp = (const PBN_GLOBAL hf8*)a.Bpack;
    const PBN_GLOBAL float* __restrict__ NYp = (const PBN_GLOBAL float*)a.nypack;
    const PBN_GLOBAL double* __restrict__ TBp = (const PBN_GLOBAL double*)a.tile_box;
    const PBN_GLOBAL double* __restrict__ QBp = (const PBN_GLOBAL double*)a.qtile_box;
    const PBN_GLOBAL double* __restrict__ QTp = (const PBN_GLOBAL double*)a.qtile_thr;
    const PBN_GLOBAL double* __restrict__ QLp = (const PBN_GLOBAL double*)a.qlb;
    const int loff = half * 16 + idx;

    hf8 b[S][NJ];
    float ny[S], m[S];
    double sum[S];
    bool lbm[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        int64_t qt = qt0 + 2 * s + sub;
        qt = qt < a.nqtiles ? qt : a.nqtiles - 1;
#pragma unroll
        for (int j = 0; j < NJ; ++j) b[s][j] = Bp[(qt * NB + (j >> 1)) * 64 + (j & 1) * 32 + loff];
        ny[s] = NYp[qt * 16 + idx];
        m[s] = 0.f;
        sum[s] = 0.0;
        lbm[s] = false;
    }
    // the wave's query box and threshold (as kde_sweep_f16_body)
    double wlo[PBN_PRUNE_PD_NARROW], whi[PBN_PRUNE_PD_NARROW], wthr = INFINITY;
    const int pd = a.pdims;
#pragma unroll
    for (int k = 0; k < PBN_PRUNE_PD_NARROW; ++k) { wlo[k] = INFINITY; whi[k] = -INFINITY; }
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        const double th = QTp[qt];
        wthr = th < wthr ? th : wthr;
#pragma unroll
        for (int k = 0; k < PBN_PRUNE_PD_NARROW; ++k)
            if (k < pd) {
                const double l = QBp[qt * 2 * pd + k], h = QBp[qt * 2 * pd + pd + k];
                wlo[k] = l < wlo[k] ? l : wlo[k];
                whi[k] = h > whi[k] ? h : whi[k];
            }
    }
    wthr -= a.prune_margin;

    auto set_off = [&](int s) {   // slots 32 NB - 3 ... of the query side <- split3s(-1/2|z_q|^2 - m_q)
        hpiece q1, q2, q3;
        split3s(ny[s] - m[s], q1, q2, q3);
        if (half == 1) { b[s][NJ - 1][5] = q1; b[s][NJ - 1][6] = q2; b[s][NJ - 1][7] = q3; }
    };
    auto load_pair = [&](int64_t ta, int64_t tb, hf8 (&f)[NJ]) {
        const int64_t t = sub ? tb : ta;
#pragma unroll
        for (int j = 0; j < NJ; ++j) f[j] = Ap[(t * NB + (j >> 1)) * 64 + (j & 1) * 32 + loff];
    };
    auto chain = [&](const hf8 (&f)[NJ], int s) {
        f16v c = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) c = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[j], b[s][j], c, 0, 0, 0);
        return c;
    };
    auto colmax32 = [&](const f16v& v, int nr) {
        float mx = v[0];
#pragma unroll
        for (int r = 1; r < 16; ++r)
            if (r < nr) mx = v[r] > mx ? v[r] : mx;
        const float o = __shfl_xor(mx, 32);
        return mx > o ? mx : o;
    };
    // ---- offsets: the first tile pair of the split, then the prepass bounds where they lie above (see kde_sweep_f16_body) ----
    {
#pragma unroll
        for (int s = 0; s < S; ++s) set_off(s);   // m = 0
        hf8 f[NJ];
        load_pair(t0, t0 + 1 < t1 ? t0 + 1 : t0, f);
#pragma unroll
        for (int s = 0; s < S; ++s) m[s] = colmax32(chain(f, s), 16);
        if (a.qlb) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                int64_t qt = qt0 + 2 * s + sub;
                qt = qt < a.nqtiles ? qt : a.nqtiles - 1;
                const float lb = (float)QLp[qt * 16 + idx];
                const bool fin = __builtin_fabsf(lb) < 0x1p22f;   // (a bound fp32 cannot hold to a fraction of a unit is not used)
                lbm[s] = fin && lb > m[s];
                if (lbm[s]) m[s] = lb;
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) set_off(s);
    }
    if (a.count_redo && lane == 0) atomicAdd(&g_sweep_tiles, (unsigned long long)(t1 - t0));

    // ---- the kept tiles of the split, in order: one visit mask per 64-tile batch (uniform control flow: every lane tests its own tile) ----
    int64_t wtb = t0 - 64;
    unsigned long long wmask = 0;
    auto rewind = [&]() { wtb = t0 - 64; wmask = 0; };
    auto next_tile = [&]() -> int64_t {
        while (!wmask) {
            wtb += 64;
            if (wtb >= t1) return -1;
            wmask = prune_visit_mask(TBp, pd, wtb, t1, wlo, whi, wthr, lane);
            if (a.count_redo && lane == 0 && wmask) atomicAdd(&g_sweep_visit, (unsigned long long)__builtin_popcountll(wmask));
        }
        const int bit = __builtin_ctzll(wmask);
        wmask &= wmask - 1;
        return wtb + bit;
    };

    // ---- checked form: ONE tile (rows 0-15 of the pair's accumulator), super-group by super-group ----
    auto checked_single = [&](int64_t t) {
        hf8 f[NJ];
        load_pair(t, t, f);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            f16v acc = chain(f, s);
            auto tile_sum = [&]() {
                float ts = 0.f;
#pragma unroll
                for (int r = 0; r < 8; ++r) ts += Tr<float>::ex2(acc[r]);
                return ts;
            };
            float ts = tile_sum();
            if (__builtin_expect(__any(!(ts < Tr<float>::big())), 0)) {
                const float mx = colmax32(acc, 8);
                if (mx > 0.f) {
                    m[s] += mx;
                    set_off(s);
                    sum[s] *= exp2(-(double)mx);
                    acc -= mx;
                }
                ts = tile_sum();
            }
            sum[s] += (double)ts;
        }
    };

    // ---- blind walk: pairs of kept tiles, software-pipelined by one super-group ----
    float fs[S];
#pragma unroll
    for (int s = 0; s < S; ++s) fs[s] = 0.f;
    auto expsum = [&](const f16v& v) {
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e0 = Tr<float>::ex2(v[4 * k]), e1 = Tr<float>::ex2(v[4 * k + 1]), e2 = Tr<float>::ex2(v[4 * k + 2]), e3 = Tr<float>::ex2(v[4 * k + 3]);
            q[k] = (e0 + e1) + (e2 + e3);
        }
        return ((q[0] + q[1]) + q[2]) + q[3];
    };
    auto place = [&]() {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 16 / NJ, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 16 / NJ, 0);
        }
    };
    int64_t single = -1;
    {
        hf8 fA[NJ], fB[NJ];
        f16v acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] = -1000.f;
        int64_t pa = next_tile(), pb = pa >= 0 ? next_tile() : -1;
        bool have = pb >= 0;
        if (!have) single = pa;
        if (have) load_pair(pa, pb, fA);
        while (have) {
            // the next pair (unconditional prefetch: a conditional load costs a vmcnt(0) per pair - see kde_sweep_f16_body)
            int64_t na = next_tile(), nb = na >= 0 ? next_tile() : -1;
            const bool more = nb >= 0;
            if (!more) single = na;
            load_pair(more ? na : pa, more ? nb : pb, fB);
            acc0 = chain(fA, 0);
            fs[1] += expsum(acc1);
            place();
            acc1 = chain(fA, 1);
            fs[0] += expsum(acc0);
            place();
            if (!more) break;
            pa = next_tile();
            pb = pa >= 0 ? next_tile() : -1;
            have = pb >= 0;
            if (!have) single = pa;
            load_pair(have ? pa : na, have ? pb : nb, fA);
            acc0 = chain(fB, 0);
            fs[1] += expsum(acc1);
            place();
            acc1 = chain(fB, 1);
            fs[0] += expsum(acc0);
            place();
        }
        fs[1] += expsum(acc1);
    }
    bool bad = false;
#pragma unroll
    for (int s = 0; s < S; ++s) bad = bad || !(fs[s] < Tr<float>::big());
    if (__builtin_expect(__any(bad), 0)) {   // the split again, tile by tile, checked (the odd tile included)
        rewind();
#pragma unroll 1
        for (int64_t t = next_tile(); t >= 0; t = next_tile()) checked_single(t);
    } else {
#pragma unroll
        for (int s = 0; s < S; ++s) sum[s] += (double)fs[s];
        if (single >= 0) checked_single(single);
    }

    PBN_GLOBAL double* part = (PBN_GLOBAL double*)a.part;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        double v = sum[s];
        v += __shfl_xor(v, 32);
        if (v == 0.0 && (m[s] - m[s]) == 0.f && !lbm[s]) v = 1.0;   // (see kde_sweep_f16_body: not when the offset is a prepass bound)
        const int64_t qt = qt0 + 2 * s + sub;
        if (half == 0 && qt < a.nqtiles) {
            PBN_GLOBAL double* o = part + ((int64_t)split * a.nqtiles * 16 + qt * 16 + idx) * 2;
            o[0] = (double)m[s];
            o[1] = v;
        }
    }
}

template <int NB>
__global__ __launch_bounds__(sweep_block_threads(true), PBN_F16_PRUNE_WAVES) void kde_sweep_f16_w32p_kernel(SweepArgs a) {
    kde_sweep_f16_w32p_body<NB>(a, blockIdx.x);
}
template <int NB>
__global__ __launch_bounds__(sweep_block_threads(true), PBN_F16_PRUNE_WAVES) void kde_sweep_f16_w32p_group_kernel(GSweepArgs g) {
    const int u = g.wg_unit[blockIdx.x >> 6];
    const GSweepUnit& su = g.units[u];
    const unsigned bid = (unsigned)((int64_t)blockIdx.x - su.wg0);
    if (bid >= (unsigned)su.nwg) return;
    SweepArgs a;
    a.Apack = su.Apack; a.nxpack = su.nxpack; a.Axpack = nullptr;
    a.Bpack = su.Bpack; a.nypack = su.nypack; a.Bxpack = nullptr; a.Bxnorm = nullptr;
    a.ntiles = su.ntiles; a.nqtiles = su.nqtiles; a.tiles_per_split = su.tps;
    a.fold = 0; a.count_redo = g.count_redo; a.wmul = 0;
    a.prune = 1; a.pdims = su.pdims; a.prune_margin = g.prune_margin > 0.0 ? g.prune_margin : (double)su.margin;
    a.tile_box = su.tile_box; a.qtile_box = su.qtile_box; a.qtile_thr = su.qtile_thr; a.qlb = su.qlb;
    a.nsplit_grid = su.nsplit; a.part = su.part; a.group_masks = 0;
    kde_sweep_f16_w32p_body<NB>(a, bid);
}

void launch_far_fix(const PackArgs& q, const void* Apack, const void* Axpack, int NB, int64_t n_train, int64_t ntiles, double* part, int nsplit, int64_t nqtiles,
                    bool cond, hipStream_t st) {
    if (!q.far_flag || nqtiles == 0) return;
    const dim3 grid((unsigned)nqtiles), block(256);
    if (cond) hipLaunchKernelGGL(kde_far_fix_kernel<true>, grid, block, 0, st, q, (const hf8*)Apack, (const hf8*)Axpack, NB, n_train, ntiles, part, nsplit, nqtiles);
    else hipLaunchKernelGGL(kde_far_fix_kernel<false>, grid, block, 0, st, q, (const hf8*)Apack, (const hf8*)Axpack, NB, n_train, ntiles, part, nsplit, nqtiles);
    HIP_CHECK(hipGetLastError());
}

// the W32 form of the plain unpruned fp32 sweep: one or two 32-slot blocks whose last three slots are free (up to 8 / 19 whitened dimensions)
bool f16x2_w32(int dm, int NB) {
    return knob_int("PBN_F32_W32", 1) != 0 && (NB == 1 || NB == 2) && f16x2_spd(dm) * dm + 6 <= 32 * NB;   // read per call: tests compare the two forms in one process
}

// ... and of the pruned plain fp32 sweeps (stand-alone handles, grouped launches): one 32-slot block whose last three slots are free
bool f16x2_w32p(int dm, int NB) {
    return PBN_F16_W32P != 0 && knob_int("PBN_F32_W32", 1) != 0 && NB == 1 && f16x2_spd(dm) * dm + 6 <= 32;
}

static std::atomic<unsigned long long> g_w32_launches{0};   // measurement aid (pbn_debug_w32_launches): launches of the W32 form
template <bool COND>
static void launch_sweep_f16(const SweepArgs& a, int NB, dim3 grid, hipStream_t st) {
    dim3 block(256);
    if (a.prune) {   // at most 6 marginal dimensions: 27 f16 slots, one MFMA (two are kept instantiated)
        block = dim3(sweep_block_threads(true));
        constexpr int QGP = PBN_F16_QG_PRUNE;
        grid = dim3((unsigned)(ceil_div(a.nqtiles, QGP) * a.nsplit_grid));   // one wave (QGP query groups) per workgroup, placed by pruned_block
        if constexpr (!COND) {
            if (a.w32 && NB == 1) {   // paired kept tiles on 32x32x16 MFMAs (kde_sweep_f16_w32p_body)
                ++g_w32_launches;
                hipLaunchKernelGGL((kde_sweep_f16_w32p_kernel<1>), grid, block, 0, st, a);
                HIP_CHECK(hipGetLastError());
                return;
            }
        }
        if (NB == 1) hipLaunchKernelGGL((kde_sweep_f16_kernel<1, COND, QGP, true>), grid, block, 0, st, a);
        else if (NB == 2) hipLaunchKernelGGL((kde_sweep_f16_kernel<2, COND, QGP, true>), grid, block, 0, st, a);
        else throw invalid_error("KDE: pruned fp32 sweeps cover at most 10 whitened dimensions");
        HIP_CHECK(hipGetLastError());
        return;
    }
    if constexpr (!COND) {
        if (a.w32 && (NB == 1 || NB == 2)) {   // same grid: a wave's four 16-query groups are its two 32-query super-groups
            ++g_w32_launches;
            if (NB == 1) hipLaunchKernelGGL((kde_sweep_f16_w32_kernel<1>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((kde_sweep_f16_w32_kernel<2>), grid, block, 0, st, a);
            HIP_CHECK(hipGetLastError());
            return;
        }
    }
    switch (NB) {
        case 1: hipLaunchKernelGGL((kde_sweep_f16_kernel<1, COND, 4, false>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((kde_sweep_f16_kernel<2, COND, 4, false>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((kde_sweep_f16_kernel<3, COND, 4, false>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((kde_sweep_f16_kernel<4, COND, 4, false>), grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL((kde_sweep_f16_kernel<5, COND, 2, false>), grid, block, 0, st, a); break;   // 21-32 dimensions (sweep_qg: 2)
        case 6: hipLaunchKernelGGL((kde_sweep_f16_kernel<6, COND, 2, false>), grid, block, 0, st, a); break;
        case 7: hipLaunchKernelGGL((kde_sweep_f16_kernel<7, COND, 2, false>), grid, block, 0, st, a); break;
        default: throw invalid_error("KDE: more than 32 whitened dimensions per sweep are not supported");
    }
    HIP_CHECK(hipGetLastError());
}
