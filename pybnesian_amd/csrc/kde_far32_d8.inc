// The far pass of the pruned sum-only d = 8 sweep (round 16): kde_sweep_far32_d8_kernel evaluates in fp32, on v_mfma_f32_16x16x4_f32 and
// v_exp_f32, the blocks the f16 screen proved FAR (kde_screen_d8.inc: screen_far_thr) - every pair of such a block lies theta bits below its
// own query's sum bound, so its term may carry 2^theta times the relative error a near term may.  Part of kde_kernels.hip's translation unit, like the screen
// (the unit's flags: no SLP vectoriser, whose packed fp32 adds beside MFMAs are an anti-lever on gfx950).
//
// What a far block computes, for training row t and query q of the same sorted fragments the fp64 sweep reads (Apack, nxpack, Bpack, nypack):
//   off   = ceil(qrow_thr[q])                                 integer, the offset of q's far partial sums: |off| <= 4 NCAP + 1 (screen_far_thr)
//   cq    = f32(ny_q - off + BIAS)                            ny_q = -1/2|z_q|^2 >= -NCAP; computed in fp64, rounded once
//   c     = f32(cq + f32(nt))                                 nt = -1/2|z_t|^2 >= -NCAP (plain tiles only)
//   x32   = c + sum_k f32(z_tk) f32(z_qk)                     two v_mfma_f32_16x16x4_f32: eight products into c
//   term  = v_exp_f32(x32),   x = z_t.z_q + nt + ny_q - off + BIAS the exact exponent
// and the terms are added in fp32 per lane (four rows of a column per tile) and carried into a double after at most 128 of them.
//
// The bound.  u = 2^-24 (one fp32 rounding to nearest), v = 2^-23 (one operation of the matrix core, whatever its rounding), C = NCAP,
// B = BIAS, K = 5 C + B + 1 >= |ny_q - off + B|, R_t R_q = 2 sqrt(N_t N_q) <= 2 C:
//   operands    |sum f32(z_tk) f32(z_qk) - z_t.z_q| <= (2u + u^2) R_t R_q <= (2u + u^2) 2C
//               (an operand below 2^-126 may be flushed: at most 8 x 2^-126 x sqrt(2C) more, which the last line's rounding up covers)
//   constants   |f32(nt) - nt| <= u C,  |cq - (ny_q - off + B)| <= u K,  the fp32 sum of the two <= u (1 + u)(C + K)
//   MFMAs       eight products and c in any order, every product and every addition rounded by at most v: each of the nine addends passes at
//               most ten such operations, so the error is at most ((1 + v)^10 - 1) T,  T = (1 + u)^2 2C + (1 + u)^2 (C + K) the addends' magnitudes
//   together    |x32 - x| <= delta(C) = (2u + u^2) 2C + u C + u K + u (1 + u)(C + K) + ((1 + v)^10 - 1)(1 + u)^2 (3C + K)
// delta(256) = 2.78e-3 exponent units (B = 64); nine tenths of it is the MFMA line, which prices the matrix core's additions at twice a rounding
// to nearest because its rounding is not documented.  A term's relative error is then at most
//   eps(C) = 2^delta (1 + v)(1 + u)^255 - 1                   v: v_exp_f32's 1 ulp;  (1 + u)^255: an fp32 sum of at most 256 addends (the kernel adds 128)
// = 1.94e-3 at C = 256 (far32_term_error).  x - B < -theta for every far pair, so x32 < B - theta + delta: no overflow; a term below 2^-126
// comes out 0: it lay 126 + B - 1 bits below its query's sum bound, 2^-146 of what the pruning margin drops anyway.
// theta: n far terms of at most 2^-theta of their query's sum each, wrong by eps each, move the sum by at most n 2^-theta eps; at 10^6 rows
// theta = the smallest integer with 10^6 2^-theta eps <= 8e-8 (PBN_FAR32_BUDGET, DESIGN.md 4 "fp32 far tail") = 35, and for n rows
// theta + log2(n / 10^6) as the pruning margin moves (far32_theta): the same 8e-8 at every size.  tests/test_far32_bound_cpu.py restates x32
// in numpy and holds |x32 - x| <= delta on rows built against it.
//
// Layouts.  The A and B operands have the f64 MFMA's layout (row / column = lane & 15, k = lane >> 4: the same for both MFMAs).  The
// ACCUMULATORS differ: register i of lane group lg = lane >> 4 is row 4 lg + i of the fp32 MFMA's product where the fp64 MFMA's is row
// 4 i + lg - far_pack_kernel reorders the norms.  The training side is read from fp32 copies made once per fit (SweepArgs::far_pack), the
// query side is converted in the prologue.
// Grid, (query wave, split) mapping and block order are the sweep's (pruned_block); a super-batch's far words are loaded by lane = batch as
// the sweep loads its live words, and their tiles run through a ring of loads as ONE list (see the kernel).
// Output: partial rows nsplit + split of SweepArgs::part, (off - B, sum); a (split, query) without a far block writes (-1e300, 0), which
// kde_finish_kernel's maximum and sum pass over.
typedef float f32x4 __attribute__((ext_vector_type(4)));

// measurement aid, not part of the C ABI header: launches of the far pass (tests: with the knob at 0 none runs)
static std::atomic<unsigned long long> g_far32_launches{0};

__global__ __launch_bounds__(64) void far_plain_kernel(const double* __restrict__ norms, int64_t ntiles, unsigned long long* __restrict__ out) {
    // one wave per word, lane = tile: the tile's 16 norms (-1/2|z|^2; padding rows PBN_PAD_NORM, a NaN row NaN) all at or above -NCAP
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 64 + lane;
    bool plain = t < ntiles;
    if (plain) {
#pragma unroll
        for (int i = 0; i < 16; ++i) plain = plain && norms[t * 16 + i] >= -PBN_FAR32_NCAP;   // (false for a NaN)
    }
    const unsigned long long w = __ballot(plain);
    if (lane == 0) out[blockIdx.x] = w;
}

// The far pass's own copy of the training fragments, written once per fit: per tile 768 bytes - per lane the two fp32 operands of its row
// (k = lane >> 4 and 4 + (lane >> 4): one 8-byte load), then the 16 norms in the fp32 MFMA's row order (register i of lane group lg = row
// 4 lg + i: one 16-byte load per lane).  f32(z) and f32(nt) of the bound above are these conversions.  Converting the fp64 fragments in the
// kernel instead cost six quarter-rate conversions and six loads per tile (profiles/r16/step_kernels.txt, "first form").
#define PBN_FAR32_TILE_BYTES 768
__global__ __launch_bounds__(64) void far_pack_kernel(const double* __restrict__ Ap, const double* __restrict__ Np, char* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = blockIdx.x;
    float* o = (float*)(out + t * PBN_FAR32_TILE_BYTES);
    o[lane * 2] = (float)Ap[(t * 2) * 64 + lane];
    o[lane * 2 + 1] = (float)Ap[(t * 2 + 1) * 64 + lane];
    if (lane < 16) o[128 + lane] = (float)Np[t * 16 + (lane & 3) * 4 + (lane >> 2)];   // row `lane`; pack_rows_kernel stores row 4 i + lg at lg * 4 + i
}

void launch_far_plain(const double* norms, int64_t ntiles, unsigned long long* out, hipStream_t st) {
    const int64_t words = ceil_div(ntiles, 64) + 1;   // (the last word is all zero: screen_plain_word reads two)
    hipLaunchKernelGGL(far_plain_kernel, dim3((unsigned)words), dim3(64), 0, st, norms, ntiles, out);
    HIP_CHECK(hipGetLastError());
}

void launch_far_pack(const void* Apack, const void* nxpack, int64_t ntiles, void* out, hipStream_t st) {
    if (ntiles == 0) return;
    hipLaunchKernelGGL(far_pack_kernel, dim3((unsigned)ntiles), dim3(64), 0, st, (const double*)Apack, (const double*)nxpack, (char*)out);
    HIP_CHECK(hipGetLastError());
}

#ifndef PBN_FAR32_RING
#define PBN_FAR32_RING 4   // tiles of loads in flight per wave (6 VGPRs each)
#endif
__global__ __launch_bounds__(64, 4) void kde_sweep_far32_d8_kernel(SweepArgs a) {
    constexpr int QG = PBN_QG_PRUNE, R = PBN_FAR32_RING;
    static_assert(QG == 2, "the screen's two groups per wave");
    const int lane = threadIdx.x & 63, lg = lane >> 4;
    int qx, split;
    pruned_block(a, QG, blockIdx.x, qx, split);
    const int64_t qt0 = (int64_t)qx * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL char* __restrict__ FPp = (const PBN_GLOBAL char*)a.far_pack;
    const PBN_GLOBAL double* __restrict__ Bp = (const PBN_GLOBAL double*)a.Bpack;
    const PBN_GLOBAL double* __restrict__ NYp = (const PBN_GLOBAL double*)a.nypack;
    const PBN_GLOBAL double* __restrict__ QRp = (const PBN_GLOBAL double*)a.qrow_thr;
    const PBN_GLOBAL unsigned long long* __restrict__ FMp =
        (const PBN_GLOBAL unsigned long long*)a.far_mask + ((int64_t)qx * a.nsplit_grid + split) * a.batches_per_split * QG;
    // ---- the query side in fp32: fragments, the columns' constants and offsets
    float b[QG][2], cq[QG], fs[QG];
    double off[QG], sum[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        const int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) b[g][ks] = (float)Bp[(qt * 2 + ks) * 64 + lane];
        const double lb = QRp[qt * 16 + (lane & 15)];
        const bool fin = __builtin_fabs(lb) <= 4.0 * PBN_FAR32_NCAP;   // (what screen_far_thr asks of a far block's columns; false for a NaN)
        off[g] = fin ? __builtin_ceil(lb) : 0.0;
        cq[g] = (float)(NYp[qt * 16 + (lane & 15)] - off[g] + PBN_FAR32_BIAS);
        fs[g] = 0.f;
        sum[g] = 0.0;
    }
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const unsigned loff = (unsigned)lane * 8u, noff = 512u + (unsigned)lg * 16u;
    auto block = [&](const f32x2& f, const f32x4& n, unsigned gsel) {
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            if (!((gsel >> g) & 1u)) continue;   // (uniform)
            f32x4 acc = {cq[g] + n[0], cq[g] + n[1], cq[g] + n[2], cq[g] + n[3]};
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f[0], b[g][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(f[1], b[g][1], acc, 0, 0, 0);
            const float e0 = __builtin_amdgcn_exp2f(acc[0]), e1 = __builtin_amdgcn_exp2f(acc[1]);
            const float e2 = __builtin_amdgcn_exp2f(acc[2]), e3 = __builtin_amdgcn_exp2f(acc[3]);
            fs[g] += (e0 + e1) + (e2 + e3);
        }
    };
    for (int64_t sb = t0; sb < t1; sb += 4096) {
        const int64_t bt = sb + 64 * lane;   // my batch's first tile
        unsigned long long fw[QG] = {0, 0};
        if (bt < t1) {
            const PBN_GLOBAL unsigned long long* fp = FMp + ((bt - t0) >> 6) * QG;
            fw[0] = fp[0];
            fw[1] = fp[1];
        }
        unsigned long long todo = __ballot((fw[0] | fw[1]) != 0);   // batches whose far tiles are still to be listed
        if (!todo) continue;
        // The far tiles of the super-batch as ONE list - batch after batch, bit after bit, everything that names a tile scalar - through a ring of R
        // tiles of loads: unconditional (past the end the last tile is loaded again, with no group to evaluate) and waited for by count, as in
        // kde_screen_d8_kernel; a walk that drained at every batch's end left the wave waiting for memory most of its time.
        const int w0lo = (int)(unsigned)fw[0], w0hi = (int)(unsigned)(fw[0] >> 32), w1lo = (int)(unsigned)fw[1], w1hi = (int)(unsigned)(fw[1] >> 32);
        const PBN_GLOBAL char* sbp = FPp + sb * PBN_FAR32_TILE_BYTES;
        struct Item { unsigned t, g; };   // tile of the super-batch, groups to evaluate (bit g)
        Item cur = {0u, 0u};
        unsigned cj = 0;
        unsigned long long gm0 = 0, gm1 = 0, left = 0;
        auto next = [&]() -> Item {
            if (left == 0 && todo != 0) {
                cj = (unsigned)__builtin_ctzll(todo);
                todo &= todo - 1;
                gm0 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(w0lo, (int)cj) | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(w0hi, (int)cj) << 32);
                gm1 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane(w1lo, (int)cj) | ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(w1hi, (int)cj) << 32);
                left = gm0 | gm1;
            }
            if (left == 0) return Item{cur.t, 0u};
            const unsigned c = (unsigned)__builtin_ctzll(left);
            left &= left - 1;
            cur.t = 64u * cj + c;
            cur.g = (unsigned)((gm0 >> c) & 1ull) | ((unsigned)((gm1 >> c) & 1ull) << 1);
            return cur;
        };
        auto load = [&](const Item& d, f32x2& f, f32x4& n) {
            unsigned base = d.t * (unsigned)PBN_FAR32_TILE_BYTES;
            asm volatile("" : "+s"(base));   // (so that a reload past the end stays a load: kde_screen_d8_kernel)
            const PBN_GLOBAL char* p = sbp + (uint64_t)base;
            f = *(const PBN_GLOBAL f32x2*)(p + loff);
            n = *(const PBN_GLOBAL f32x4*)(p + noff);
        };
        Item dq[R];
        f32x2 fq[R];
        f32x4 nq[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            dq[i] = next();
            load(dq[i], fq[i], nq[i]);
        }
        bool go = true;
        unsigned turn = 0;
        do {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                block(fq[i], nq[i], dq[i].g);
                dq[i] = next();
                if (i == 0) go = dq[i].g != 0;   // the next turn's first tile exists
                load(dq[i], fq[i], nq[i]);
            }
            if ((++turn & 7u) == 0u) {   // at most 8 R tiles x 4 rows = 128 fp32 addends, then into the double
#pragma unroll
                for (int g = 0; g < QG; ++g) { sum[g] += (double)fs[g]; fs[g] = 0.f; }
            }
        } while (go);
#pragma unroll
        for (int g = 0; g < QG; ++g) { sum[g] += (double)fs[g]; fs[g] = 0.f; }
    }
    // ---- the four row-lanes of each column, then (offset, sum) behind the sweep's partial rows
    PBN_GLOBAL double* part = (PBN_GLOBAL double*)a.part;
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        double s = sum[g];
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        if (lg == 0 && qt0 + g < a.nqtiles) {
            PBN_GLOBAL double* o = part + ((int64_t)(a.nsplit_grid + split) * a.nqtiles * 16 + (qt0 + g) * 16 + lane) * 2;
            o[0] = s > 0.0 ? off[g] - PBN_FAR32_BIAS : -1e300;
            o[1] = s > 0.0 ? s : 0.0;
        }
    }
}

void launch_sweep_far32_d8(const SweepArgs& a_in, int nsplit, hipStream_t st) {
    SweepArgs a = a_in;
    a.nsplit_grid = nsplit;
    if (!a.far_mask || !a.far_pack || !a.qrow_thr || !a.part || a.pdims != PBN_PRUNE_PD) throw invalid_error("KDE: the far pass needs the screen's far words and per-query bounds");
    const dim3 grid((unsigned)(ceil_div(a.nqtiles, PBN_QG_PRUNE) * nsplit)), block(64);
    hipLaunchKernelGGL(kde_sweep_far32_d8_kernel, grid, block, 0, st, a);
    HIP_CHECK(hipGetLastError());
    ++g_far32_launches;
}

double far32_term_error(double C) {
    const double u = 0x1p-24, v = 0x1p-23, B = PBN_FAR32_BIAS, K = 5.0 * C + B + 1.0;
    const double delta = (2.0 * u + u * u) * 2.0 * C + u * C + u * K + u * (1.0 + u) * (C + K) + (std::pow(1.0 + v, 10.0) - 1.0) * (1.0 + u) * (1.0 + u) * (3.0 * C + K);
    return std::exp2(delta) * (1.0 + v) * std::pow(1.0 + u, 255.0) - 1.0;
}

double far32_theta(int64_t n_train) {
    const double at1e6 = std::ceil(std::log2(1e6 * far32_term_error(PBN_FAR32_NCAP) / PBN_FAR32_BUDGET));
    return at1e6 + std::log2((double)n_train / 1e6);
}
