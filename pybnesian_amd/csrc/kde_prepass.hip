// What runs before a sweep: the classic pack (pack_rows), the generic pack and sweep of wide models, and the spatial sort keys, tile / batch
// boxes and exponent bounds of the pruned sweeps.  See kde_kernels.hip for the pipeline.
#include "common.hpp"
#include "kde_kernels.hpp"
#include "kde_device.hpp"

#include <algorithm>
#include <cmath>

namespace pbn {

// ------------------------------------------------------------------------------------------------
// pack_rows: one thread per (padded) row.
//   main components c < dm   -> pack[(tile*KS + c/4)*64 + (c%4)*16 + idx]   (A and B fragment order
//                               coincide: element [idx = lane&15][k = lane>>4])
//   norm  -1/2 sum_{c<dm} z^2 -> npack: training side in C-row order [tile][lg][i], query side [tile][idx]
//   extra component (CKDE)   -> xpack[tile*64 + k*16 + idx]:
//        training: k0 z_e, k1 -1/2 z_e^2, k2 1, k3 0      query: k0 z_e, k1 1, k2 -1/2 z_e^2, k3 0
// ------------------------------------------------------------------------------------------------
// T = fragment type, TS = element type of the table (float under double fragments: PackArgs::src_f32)
template <typename T, typename TS = T>
__global__ __launch_bounds__(256) void pack_rows_kernel(PackArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t npad = a.ntiles * 16;
    if (r >= npad) return;
    const int64_t tile = r >> 4;
    const int idx = (int)(r & 15);
    const int d = a.d, dm = a.dm, KS = a.KS;
    T* pack = (T*)a.pack;
    T* npack = (T*)a.npack;
    T* xpack = (T*)a.xpack;
    const bool valid = r < a.n;

    double xc[PBN_MAX_D];
    if (valid) {
        const int64_t rr = a.perm ? (int64_t)a.perm[a.perm_stride > 1 ? r * a.perm_stride : r] : r;
        const int64_t lr = rr < a.n0 ? a.row0 + rr : a.row1 + (rr - a.n0);
        const int64_t src = a.rows ? (int64_t)a.rows[lr] : lr;
        for (int j = 0; j < d; ++j) {
            const TS* col = (const TS*)a.base + (int64_t)a.cols[j] * a.ld;
            xc[j] = (double)col[src] - a.mu[j];
        }
    }
    double nrm = 0.0;
    for (int i = 0; i < KS * 4; ++i) {
        double z = 0.0;
        if (valid && i < dm) {
            const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)i * d;
            const int jn = a.wfull ? d : i + 1;   // a rotated whitening matrix (KdeModel::wfull) is full
            for (int j = 0; j < jn; ++j) z = __builtin_fma(w[j], xc[j], z);
        }
        const T zt = (T)z;
        // the norm is taken from the ROUNDED coordinate so that s2(t,t) == 0 up to one rounding
        nrm = __builtin_fma((double)zt, (double)zt, nrm);
        pack[(tile * KS + (i >> 2)) * 64 + (i & 3) * 16 + idx] = zt;
    }
    double nv = -0.5 * nrm;
    if (!valid) nv = a.is_query ? 0.0 : PBN_PAD_NORM;
    if (a.fold_norm && dm < KS * 4) pack[(tile * KS + (dm >> 2)) * 64 + (dm & 3) * 16 + idx] = a.is_query ? (T)1 : (T)nv;
    if (a.is_query) {
        npack[tile * 16 + idx] = (T)nv;
    } else {
        // idx -> (lg, i) with crow(lg, i) == idx
        int lg, i;
        if (sizeof(T) == 8) { lg = idx & 3; i = idx >> 2; } else { lg = idx >> 2; i = idx & 3; }
        npack[tile * 16 + lg * 4 + i] = (T)nv;
        // weights of the WMUL sweep behind the norms: 2^norm; NaN where it would lose bits (the sweep then takes its
        // classic path for that tile), 0 for padding
        if (a.write_w) npack[a.ntiles * 16 + tile * 16 + lg * 4 + i] = !valid ? (T)0 : (nv < -1000.0 ? (T)NAN : (T)exp2(nv));
        if constexpr (sizeof(T) == 8) {
            if (a.write_r) {   // the tile's radius: sqrt(max -norm) over its 16 rows (consecutive lanes), +inf with a padding row
                double rr = (valid && nv == nv) ? -nv : INFINITY;   // (a NaN row closes its chunk: the clamped form keeps the NaN)
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) { const double v = __shfl_xor(rr, o); rr = v > rr ? v : rr; }
                if (idx == 0) ((double*)npack)[a.ntiles * 32 + tile] = __builtin_sqrt(rr);
            }
        }
    }
    if (a.upack) {  // CKDE::cdf: standardised "x - b.e" of the row, in the norm's layout
        double u = 0.0;
        if (valid)
            for (int j = 0; j < d; ++j) u = __builtin_fma(a.wu[j], xc[j], u);
        T* up = (T*)a.upack;
        if (a.is_query) {
            up[tile * 16 + idx] = (T)u;
        } else {
            int lg, i;
            if (sizeof(T) == 8) { lg = idx & 3; i = idx >> 2; } else { lg = idx >> 2; i = idx & 3; }
            up[tile * 16 + lg * 4 + i] = (T)u;
        }
    }
    if (xpack) {
        double z = 0.0;
        if (valid) {
            const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)dm * d;
            for (int j = 0; j <= dm; ++j) z = __builtin_fma(w[j], xc[j], z);
        }
        const T zt = (T)z;
        const T hn = (T)(-0.5 * (double)zt * (double)zt);
        T* xp = xpack + tile * 64 + idx;
        xp[0] = zt;
        if (a.is_query) { xp[16] = (T)1; xp[32] = hn; } else { xp[16] = hn; xp[32] = (T)1; }
        xp[48] = (T)0;
    }
}

// ------------------------------------------------------------------------------------------------
// Tile pruning support (SweepArgs::prune): whitened coordinates + Morton keys of the logical rows, bounding boxes of the
// sorted 16-row tiles, and per query tile a lower bound of its queries' largest exponents.
// ------------------------------------------------------------------------------------------------
// (key cells: prune_key_bits / prune_key_cell in kde_kernels.hpp)

#define PBN_PRUNE_WINDOW 32     // training rows scanned on either side of a query's Morton position
// terms below 2^-52 of their query's largest known term are dropped: at most N * 2^-52 of a sum (2.2e-10 at 10^6 rows), a
// tenth of the error bound of the 2^x polynomial the kept terms go through.  (Round 1 and the first half of round 2 used
// 2^-64: C3's first iteration 28.2 s instead of 26.4 s, a pruned d = 2 sweep at 10^6 x 10^5 rows 15.0 ms instead of 13.6;
// 2^-44 would give 24.9 s / 12.5 ms at a worst case of 6e-8.)  PBN_PRUNE_MARGIN overrides at run time.  Since round 3 the value is
// the margin at 10^6 training rows and follows log2(n / 10^6) (prune_margin below): the BOUND is what is held constant.
#ifndef PBN_PRUNE_MARGIN
#define PBN_PRUNE_MARGIN 52.0
#endif
// fp32 (f16x2) sweeps: 2^-40.  What is dropped is at most N * 2^-40 of a sum (9e-7 at 10^6 rows, against the fp32 bar of
// 1e-3 and fp32's own 6e-8 per term); the support shrinks from 9.4 to 7.4 bandwidths per axis (a third of the tiles at 2-3
// dimensions).
#ifndef PBN_PRUNE_MARGIN_F32
#define PBN_PRUNE_MARGIN_F32 36.0   // round 4 (40 until then): N * 2^-36 = 1.5e-5 of a sum at 10^6 rows - the size of the fp32 Gram form's own error
#endif
#ifndef PBN_PRUNE_MARGIN_SUM
#define PBN_PRUNE_MARGIN_SUM 43.0   // fp64 sweeps whose result is a sum: 1.1e-7 of a sum at 10^6 rows, beside the 1.4e-7 of their 2^f (prune_margin)
#endif

// largest |z|^2 of the whitened rows (all d coordinates): one atomic max per block on the bits of a non-negative double
template <typename TS>
__global__ __launch_bounds__(256) void max_norm2_kernel(PackArgs a, unsigned long long* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double nrm = 0.0;
    if (r < a.n) {
        const int d = a.d;
        const int64_t lr = r < a.n0 ? a.row0 + r : a.row1 + (r - a.n0);
        const int64_t src = a.rows ? (int64_t)a.rows[lr] : lr;
        double xc[PBN_MAX_D];
        for (int j = 0; j < d; ++j) xc[j] = (double)((const TS*)a.base + (int64_t)a.cols[j] * a.ld)[src] - a.mu[j];
        for (int i = 0; i < d; ++i) {
            double z = 0.0;
            const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)i * d;
            const int jn = a.wfull ? d : i + 1;
            for (int j = 0; j < jn; ++j) z = __builtin_fma(w[j], xc[j], z);
            nrm = __builtin_fma(z, z, nrm);
        }
        if (!(nrm == nrm)) nrm = INFINITY;   // a NaN row: as far out as it gets
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(nrm, off);
        nrm = o > nrm ? o : nrm;
    }
    __shared__ double wmax[4];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = nrm;
    __syncthreads();
    if (threadIdx.x == 0) {
        double m = wmax[0];
        for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(m);
        if (bits > *(volatile unsigned long long*)out) atomicMax(out, bits);   // (see group_pack_train_kernel)
    }
}

// T = fragment type (the rounding the keys see), TS = element type of the table
template <typename T, typename TS = T>
__global__ __launch_bounds__(256) void prune_keys_kernel(PackArgs a, int zd, int kd, double* __restrict__ zrow, uint32_t* __restrict__ keys,
                                                         int32_t* __restrict__ iota, double inv_cell, int hilbert_nd) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.n) return;
    const int d = a.d;
    const int64_t lr = r < a.n0 ? a.row0 + r : a.row1 + (r - a.n0);
    const int64_t src = a.rows ? (int64_t)a.rows[lr] : lr;
    double xc[PBN_MAX_D];
    for (int j = 0; j < d; ++j) xc[j] = (double)((const TS*)a.base + (int64_t)a.cols[j] * a.ld)[src] - a.mu[j];
    uint32_t key = 0;
    uint32_t cells[4] = {0, 0, 0, 0};
    const int bits = prune_key_bits(kd);
    const bool curve = kd == 2 || (hilbert_nd && (kd == 3 || kd == 4));
    for (int i = 0; i < zd; ++i) {
        double z = 0.0;
        const double* w = (a.Wdev ? a.Wdev : a.W) + (size_t)i * d;
        const int jn = a.wfull ? d : i + 1;
        for (int j = 0; j < jn; ++j) z = __builtin_fma(w[j], xc[j], z);
        z = (double)(T)z;   // the rounding the pack applies
        zrow[r * zd + i] = z;
        if (i < kd) {
            const double half = (double)(1 << (bits - 1)), top = (double)((1 << bits) - 1);
            double c = __builtin_floor(z * inv_cell) + half;
            c = c < 0.0 ? 0.0 : (c > top ? top : c);
            const uint32_t cell = (uint32_t)c;
            if (curve) cells[i] = cell;
            else for (int b = 0; b < bits; ++b) key |= ((cell >> b) & 1u) << (b * kd + i);   // Morton interleave
        }
    }
    if (kd == 2) {   // two key dimensions: position along the Hilbert curve (see kde_group.hip group_keys_kernel); 16 bits per axis
        uint32_t x = cells[0], y = cells[1];
        const uint32_t n1 = (1u << bits) - 1u;
        for (uint32_t sq = 1u << (bits - 1); sq > 0; sq >>= 1) {
            const uint32_t rx = (x & sq) ? 1u : 0u, ry = (y & sq) ? 1u : 0u;
            key += sq * sq * ((3u * rx) ^ ry);
            if (ry == 0) {
                if (rx == 1) { x = n1 - x; y = n1 - y; }
                const uint32_t tmp = x; x = y; y = tmp;
            }
        }
    }
    if (curve && kd > 2) key = hilbert_key(cells, kd, bits);   // three / four key dimensions: the n-dimensional form of the same curve
    keys[r] = key;
    iota[r] = (int32_t)r;
}

__global__ __launch_bounds__(256) void tile_box_kernel(const double* __restrict__ zrow, const int32_t* __restrict__ perm, int64_t n, int zd, int pd,
                                                       double* __restrict__ box, double* __restrict__ zsorted) {
    // one thread per sorted row, 16 lanes per tile (one thread per TILE walked its 16 gathered rows in sequence: 57 us for the
    // 90 000 rows of a cv64 fold, next to a 250 us sweep)
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = r < n;
    double lo[PBN_PRUNE_PD], hi[PBN_PRUNE_PD];
#pragma unroll
    for (int k = 0; k < PBN_PRUNE_PD; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    if (valid) {
        const double* z = zrow + (int64_t)perm[r] * zd;
        for (int k = 0; k < zd; ++k) {
            const double v = z[k];
            zsorted[r * zd + k] = v;
#pragma unroll
            for (int j = 0; j < PBN_PRUNE_PD; ++j)
                if (j == k && j < pd && v == v) { lo[j] = v; hi[j] = v; }   // a NaN leaves the box alone, as the comparisons of the serial form did
        }
    }
    for (int off = 1; off < 16; off <<= 1) {
#pragma unroll
        for (int k = 0; k < PBN_PRUNE_PD; ++k) {
            const double l = __shfl_xor(lo[k], off), h = __shfl_xor(hi[k], off);
            lo[k] = l < lo[k] ? l : lo[k];
            hi[k] = h > hi[k] ? h : hi[k];
        }
    }
    if (valid && (threadIdx.x & 15) == 0) {
        const int64_t tile = r >> 4;
        for (int k = 0; k < pd; ++k) { box[tile * 2 * pd + k] = lo[k]; box[tile * 2 * pd + pd + k] = hi[k]; }
    }
}

// one thread per (sorted) query: largest exponent against the training rows around its Morton position - a valid lower
// bound of its largest term whatever those rows are - then per 16-query tile the smallest of those bounds and the box
__global__ __launch_bounds__(256) void query_prepass_kernel(const double* __restrict__ zq_row, const int32_t* __restrict__ qperm, int64_t nq,
                                                            const uint32_t* __restrict__ qkeys, const double* __restrict__ zt,
                                                            const uint32_t* __restrict__ tkeys, int64_t n, int zd, int pd,
                                                            double* __restrict__ qbox, double* __restrict__ qthr, double* __restrict__ qlb,
                                                            const double* __restrict__ subpart, int P, int which, double log2_nsub, double sub_abs,
                                                            double sub_rel, int sum_bound, const double* __restrict__ tile_box, int tile_window,
                                                            int64_t* __restrict__ qtpos) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = q < nq;
    double z[PBN_MAX_D];
    double best = -INFINITY;
    double sumb = -INFINITY;   // lower bound of log2 of the query's WHOLE sum: the part of it that has been looked at
    int64_t tpos_ = 0;   // the query's position in the (Morton-sorted) training order
    if (valid) {
        const double* zp = zq_row + (int64_t)qperm[q] * zd;
        for (int k = 0; k < zd; ++k) z[k] = zp[k];
        const uint32_t key = qkeys[q];
        int64_t lo = 0, hi = n;
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (tkeys[mid] < key) lo = mid + 1; else hi = mid; }
        tpos_ = lo;
        const int64_t b = lo - PBN_PRUNE_WINDOW > 0 ? lo - PBN_PRUNE_WINDOW : 0, e = lo + PBN_PRUNE_WINDOW < n ? lo + PBN_PRUNE_WINDOW : n;
        double acc = 0.0;
        auto term = [&](double ex) {   // the rows' terms are added up in the order of the rows
            if (ex > best) { acc = acc * exp2(best - ex) + 1.0; best = ex; }
            else acc += exp2(ex - best);
        };
        if (zd == 8) {
            // Round 15: with zd a run-time number every coordinate of every row was a load of its own behind the one before - a chain of
            // 64 x 8 load latencies per thread, and the kernel lasts as long as one thread does.  Eight dimensions (the bench's model): the
            // coordinates by constant index, and the exponents of four rows - 32 loads in flight - before their terms are added up.  The
            // same operations on the same numbers in the same order as the loop below: the same bits.
            double z8[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) z8[k] = zp[k];
            for (int64_t t = b; t < e; t += 4) {
                double ex[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double* r = zt + (t + i < e ? t + i : e - 1) * 8;   // (past the end: the last row once more, not used)
                    double d2 = 0.0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) { const double dd = r[k] - z8[k]; d2 = __builtin_fma(dd, dd, d2); }
                    ex[i] = -0.5 * d2;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (t + i < e) term(ex[i]);
            }
        } else {
            for (int64_t t = b; t < e; ++t) {
                double d2 = 0.0;
                for (int k = 0; k < zd; ++k) { const double dd = zt[t * zd + k] - z[k]; d2 = __builtin_fma(dd, dd, d2); }
                term(-0.5 * d2);
            }
        }
        if (acc > 0.0) sumb = best + log2(acc);
        // Neighbours in Morton order are neighbours in the keyed (<= 3) dimensions only: with more dimensions than that the
        // scan above finds rows that are close in 3 coordinates and anywhere in the others - a loose bound (d = 4: 6 % of the
        // tiles pruned where 70 % could be).  The sweep over a stratified subsample of the training rows bounds the largest
        // exponent whatever the dimension: max_t s2 >= log2(sum over the subsample of 2^s2) - log2(size of the subsample).
        if (subpart) {
            const double* sp = subpart + q * P + which;
            // log2 of the sum over the subsample: a part of the whole sum - AS THE SWEEP COMPUTED IT.  Where the subsample holds the one row that
            // makes up a query's whole sum (a query far from every row), the sweep's own error put the "part" above the whole (3.2e-9 units:
            // the 2^x polynomial; tests/test_prune_stages_gpu.py, ckde-d5), so its error budget comes off first (prune_subsample_slack)
            const double lr = sp[0] + log2(sp[1]);
            const double ls = lr - (sub_abs + sub_rel * __builtin_fabs(lr));
            const double lb = ls - log2_nsub;        // ... and its mean term: a lower bound of the LARGEST term
            best = lb > best ? lb : best;
            sumb = ls > sumb ? ls : sumb;
        }
    }
    // The pruning threshold stands on the bound of the query's SUM (the scanned neighbours' terms added up, or the subsample's sum -
    // log2(nsub) = up to 12 units above its mean term): what a skipped tile could add is then below 2^-margin of the sum itself, not
    // merely of its largest term - the same "at most N 2^-margin of a sum" as before, with a radius that is 5-10 % smaller per axis.
    // (PBN_GROUP_SUM_BOUND=0 restores the largest-term threshold, here and in the grouped evaluation.)
    // reduce over the 16 lanes of a query tile
    double thr = valid ? ((sum_bound && sumb > best) ? sumb : best) : INFINITY;
    double lob[PBN_PRUNE_PD], hib[PBN_PRUNE_PD];
    for (int k = 0; k < PBN_PRUNE_PD; ++k) { lob[k] = (valid && k < pd) ? z[k] : INFINITY; hib[k] = (valid && k < pd) ? z[k] : -INFINITY; }
    for (int off = 1; off < 16; off <<= 1) {
        const double o = __shfl_xor(thr, off);
        thr = o < thr ? o : thr;
        for (int k = 0; k < PBN_PRUNE_PD; ++k) {
            const double l = __shfl_xor(lob[k], off), h = __shfl_xor(hib[k], off);
            lob[k] = l < lob[k] ? l : lob[k];
            hib[k] = h > hib[k] ? h : hib[k];
        }
    }
    // Round 4: the boxes of the training tiles around the queries' position bound their sums from below, too (see group_prepass_kernel):
    // only where the boxes cover every dimension (pd == zd)
    if (tile_box && tile_window > 0 && sum_bound && pd == zd) {
        const int l16 = threadIdx.x & 15;
        const int64_t tp0 = __shfl(valid ? tpos_ : (int64_t)0, 0, 16);
        const int64_t full = n >> 4, tt = tp0 >> 4;
        const int64_t t_lo = tt - tile_window > 0 ? tt - tile_window : 0, t_hi = tt + tile_window < full ? tt + tile_window : full;
        double bmax = -INFINITY, bacc = 0.0;
        auto corner = [&](double ex) {
            if (!(ex == ex)) return;
            if (ex > bmax) { bacc = bacc * exp2(bmax - ex) + 1.0; bmax = ex; }
            else bacc += exp2(ex - bmax);
        };
        if (lob[0] <= hib[0]) {
            // (round 15, as the scan above: at eight dimensions a box's sixteen numbers by constant index, their loads in flight together;
            // the same bits)
            if (pd == PBN_PRUNE_PD) {
                for (int64_t t = t_lo + l16; t < t_hi; t += 16) {
                    const double* bx = tile_box + t * 2 * PBN_PRUNE_PD;
                    double d2 = 0.0;
#pragma unroll
                    for (int k = 0; k < PBN_PRUNE_PD; ++k) {
                        const double a1 = bx[PBN_PRUNE_PD + k] - lob[k], a2 = hib[k] - bx[k];
                        const double a = a1 > a2 ? a1 : a2;
                        d2 = __builtin_fma(a, a, d2);
                    }
                    corner(-0.5 * d2);
                }
            } else {
                for (int64_t t = t_lo + l16; t < t_hi; t += 16) {
                    const double* bx = tile_box + t * 2 * pd;
                    double d2 = 0.0;
                    for (int k = 0; k < pd; ++k) {
                        const double a1 = bx[pd + k] - lob[k], a2 = hib[k] - bx[k];
                        const double a = a1 > a2 ? a1 : a2;
                        d2 = __builtin_fma(a, a, d2);
                    }
                    corner(-0.5 * d2);
                }
            }
        }
        for (int off = 1; off < 16; off <<= 1) {
            const double om = __shfl_xor(bmax, off), oa = __shfl_xor(bacc, off);
            if (om > bmax) { bacc = bacc * exp2(bmax - om) + oa; bmax = om; }
            else if (om > -INFINITY) bacc += oa * exp2(om - bmax);
        }
        if (bacc > 0.0) {
            const double tb = bmax + log2(bacc) + 4.0;
            if (tb > thr && thr < INFINITY) thr = tb;
            if (valid && bmax > best) best = bmax;
        }
    }
    if (qlb && q < (nq + 15) / 16 * 16) qlb[q] = valid ? best : -INFINITY;   // per query: the sweep's starting offset
    if (valid && (threadIdx.x & 15) == 0) {
        const int64_t tile = q >> 4;
        if (qtpos) qtpos[tile] = tpos_;   // the tile's first query's training position: the centre of query_window_kernel's window
        qthr[tile] = thr;
        for (int k = 0; k < pd; ++k) { qbox[tile * 2 * pd + k] = lob[k]; qbox[tile * 2 * pd + pd + k] = hib[k]; }
    }
}

// Window-sum bound (sum-only pruned sweeps of the rotated d = 7, 8 models, kde_prune_rotates): one wave per 16-query tile adds up the EXACT
// terms of its queries against the 2 W training tiles around the tile's position in the sorted order (qtpos, from query_prepass_kernel),
// with the sweep's own fp64 MFMA exponents (fold: the norm rides in a K slot; otherwise the norms are added).  In 8 dimensions the prepass's
// 64 neighbours and tile-box corners sit a median 13 log2 units below a query's true sum; the window recovers most of that
// (tools/prune_window_estimate.py).  Any subset of a query's terms is a lower bound of its whole sum, so
//   lb = log2(window sum) - PBN_WINDOW_SLACK <= log2(whole sum):
// the exponents x are exact to ~1e-12 units; the per-lane offset mx is an integer >= every x seen, so 2^(x - mx) <= 1 goes through v_exp_f32
// on (float)(x - mx): the cast errs by at most |x - mx| 2^-24 <= 150 2^-24 units where the term is not below fp32's range (smaller terms
// may flush to 0 - a smaller sum, still a bound), v_exp_f32 by 1 ulp, and the four terms of a tile are added in fp32 (2 roundings) before
// the fp64 running sum: each term at most 1.0001e-5 too large, the sum likewise, log2 of it at most 1.5e-5 units too large - far inside
// the slack of 2^-8.  Rescaling by 2^(integer) is exact (or underflows: smaller).  Padding rows (row >= n_train) and NaN exponents are
// left out, and queries that are NaN or beyond nq do not enter the tile's minimum.
// Per query tile the smallest lb of its valid queries raises qthr where it is larger; per query the largest window exponent raises qlb
// where it is larger (an exponent of a real term: a lower bound of the query's largest).  The window's terms are NOT added to any sum.
// qrow_thr (nullable; round 14, the d = 8 screen's per-column thresholds): with T = the tile's bound as this kernel leaves it, a valid query
// whose own lb lies above T gets lb - a lower bound of ITS whole sum, which is all the budget argument asks of it - and every other column
// of the tile (padding, NaN queries, lb <= T) gets T.  A NaN T stays a NaN in all sixteen.
// dbg (nullable, pbn_debug_sum_window): lb per query in the sorted order, -inf where there is none.
#define PBN_WINDOW_SLACK 0x1p-8
// Round 15: how the pass runs.  One wave serves PBN_WINDOW_NQ neighbouring query tiles against ONE stream of training fragments, as the sweep
// serves its groups: neighbouring tiles sit ~10 training tiles apart in the sorted order, their windows overlap by 98 %, and a wave per tile
// streamed its own copy with one tile of loads in flight (0.80 ms at 1e6 x 1e5 rows, two thirds of its wave cycles waiting: profiles/r15/).
// The walk covers the hull of the served tiles' windows and every tile adds up the terms of its OWN window only (a uniform test per tile and
// fragment): the terms of every sum are the ones they were, so the thresholds - and with them the blocks the sweep visits, which
// tests/test_prune_d8_sweep_gpu.py pins to the block - move in their last bits at most.  Where the hull is longer than 2.5 W tiles (few
// queries, far apart) the wave walks each tile's own window in turn instead, so that no wave walks a table's length for a handful of
// queries.  PBN_WINDOW_RING tiles of fragments rotate through registers: two tiles of loads are in flight beyond the one being used,
// unconditional (past the end the last tile is loaded again) and waited for by count.  The padding test runs on the table's last tile
// only, a NaN exponent becomes -inf in the maximum that takes it.
// A walk is cut into `nparts` equal parts, one wave each, chosen by the host so that the CUs get the same number of workgroups to within
// one (window_parts); a part leaves (offset, sum, largest exponent) per query, and query_window_finish_kernel combines the parts in the
// order of their number - the same bits in every run - and writes qthr, qlb, qrow_thr and dbg by the rules above.
#define PBN_WINDOW_NQ 4
#define PBN_WINDOW_RING 3

// the walk of one wave: G query tiles qt[0..G) against the training tiles [t0, t1); partials to part[(k * nq16) + query], k = 0 offset, 1 sum, 2 top
template <bool FOLD, int G>
__device__ __forceinline__ void window_walk(const double* __restrict__ Ap, const double* __restrict__ Np, const double* __restrict__ Bp,
                                            const double* __restrict__ NYp, const int64_t (&qt)[G], const bool (&mine)[G], const int64_t (&lo)[G],
                                            const int64_t (&hi)[G], int64_t t0, int64_t t1, int64_t n_train, int64_t nq16,
                                            double* __restrict__ part, int lane) {
    constexpr int KS = 2, R = PBN_WINDOW_RING;
    using V = Tr<double>::vec4;
    const int lg = lane >> 4, col = lane & 15;
    double b[G][KS], ny[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) b[g][ks] = Bp[(qt[g] * KS + ks) * 64 + lane];
        ny[g] = NYp[qt[g] * 16 + col];
    }
    double mx[G], s[G], top[G];   // integer offset, sum of 2^(x - mx), largest x
#pragma unroll
    for (int g = 0; g < G; ++g) { mx[g] = -1e300; s[g] = 0.0; top[g] = -INFINITY; }
    // one tile of fragments against the G query tiles.  PAD (a constant at every call): the table's padded last tile, whose rows beyond
    // n_train are left out; the walk's loop never sees it.  fmax() drops a NaN exponent: -inf.
    auto tile = [&](double c0, double c1, V n, int64_t t, bool PAD) {
        V acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = FOLD ? V{ny[g], ny[g], ny[g], ny[g]} : n + ny[g];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = Tr<double>::mfma(c0, b[g][0], acc[g]);
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = Tr<double>::mfma(c1, b[g][1], acc[g]);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (G > 1 && !(t >= lo[g] && t < hi[g])) continue;   // (uniform) outside this query tile's own window
            double x[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                x[i] = __builtin_fmax(acc[g][i], -INFINITY);
                if (PAD) x[i] = t * 16 + Tr<double>::crow(lg, i) < n_train ? x[i] : -INFINITY;
            }
            const double tm = __builtin_fmax(__builtin_fmax(x[0], x[1]), __builtin_fmax(x[2], x[3]));
            // The offset is the largest ceil(tm) so far - an integer, -1e300 before the first term, so that x - mx is never inf - inf.  Where
            // no lane's offset rises (uniform test; all but the first few tiles of a walk) nothing is rescaled; where one does, every lane
            // rescales its sum by 2^(old - new offset): by 2^0 where its own stays, to 0 where it rises by 4000 or more (the first term: the
            // sum is 0 anyway).  ceil, the conversion and ldexp are quarter-rate instructions: 48 cycles a block where they run.
            if (__any(tm > mx[g])) {
                const double nm = __builtin_fmax(mx[g], __builtin_ceil(tm));
                s[g] = __builtin_ldexp(s[g], (int)__builtin_fmax(mx[g] - nm, -4000.0));
                top[g] = tm > mx[g] ? tm : top[g];   // (the term that set the offset: within one unit of the largest)
                mx[g] = nm;
            }
            const double nm = mx[g];
            const float f0 = __builtin_amdgcn_exp2f((float)(x[0] - nm)), f1 = __builtin_amdgcn_exp2f((float)(x[1] - nm));
            const float f2 = __builtin_amdgcn_exp2f((float)(x[2] - nm)), f3 = __builtin_amdgcn_exp2f((float)(x[3] - nm));
            s[g] += (double)((f0 + f1) + (f2 + f3));
        }
    };
    const int64_t nfull = n_train >> 4;                    // tiles without a padding row
    const int64_t te = t1 < nfull ? t1 : nfull;            // the loop's end
    if (t0 < te) {
        double a0[R], a1[R];
        V nx[R];
        const int64_t tl = te - 1;
        auto load = [&](int r, int64_t t) {
            t = t < tl ? t : tl;
            a0[r] = Ap[(t * KS) * 64 + lane];
            a1[r] = Ap[(t * KS + 1) * 64 + lane];
            if (!FOLD) nx[r] = *(const V*)(Np + t * 16 + lg * 4);
        };
#pragma unroll
        for (int r = 0; r < R - 1; ++r) load(r, t0 + r);
        for (int64_t tb = t0; tb < te; tb += R) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t t = tb + r;
                load((r + R - 1) % R, t + R - 1);   // into the registers the tile before this one has just left
                if (t < te) tile(a0[r], a1[r], nx[r], t, false);   // (uniform)
            }
        }
    }
    if (t0 <= nfull && nfull < t1) {   // (uniform) the padded last tile is this walk's
        V n = {};
        if (!FOLD) n = *(const V*)(Np + nfull * 16 + lg * 4);
        tile(Ap[(nfull * KS) * 64 + lane], Ap[(nfull * KS + 1) * 64 + lane], n, nfull, true);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!(s[g] > 0.0)) mx[g] = -INFINITY;   // no term: no offset (a term leaves at least 0.5 in the sum at the offset it set or met)
        // the four lanes of a query column (lg = 0..3)
        for (int off = 16; off < 64; off <<= 1) {
            const double om = __shfl_xor(mx[g], off), os = __shfl_xor(s[g], off), ot = __shfl_xor(top[g], off);
            top[g] = ot > top[g] ? ot : top[g];
            if (om > mx[g]) {
                const double sh = mx[g] - om;
                s[g] = (sh < -2000.0 ? 0.0 : __builtin_ldexp(s[g], (int)sh)) + os;
                mx[g] = om;
            } else if (om > -INFINITY) {
                const double sh = om - mx[g];
                s[g] += sh < -2000.0 ? 0.0 : __builtin_ldexp(os, (int)sh);
            }
        }
        if (mine[g] && lg == 0) {
            double* o = part + qt[g] * 16 + col;
            o[0] = mx[g];
            o[nq16] = s[g];
            o[2 * nq16] = top[g];
        }
    }
}

template <bool FOLD>
__global__ __launch_bounds__(256, 2) void query_window_kernel(const double* __restrict__ Ap, const double* __restrict__ Np, const double* __restrict__ Bp,
                                                           const double* __restrict__ NYp, int64_t ntiles, int64_t n_train, int64_t nqtiles,
                                                           const int64_t* __restrict__ qtpos, int window, int nparts, double* __restrict__ part) {
    constexpr int G = PBN_WINDOW_NQ;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform: what names a tile is scalar
    const int64_t grp = w / nparts;
    const int p = (int)(w - grp * nparts);
    if (grp * G >= nqtiles) return;   // (wave-uniform; no barriers)
    const int64_t nq16 = nqtiles * 16;
    double* mypart = part + (int64_t)p * 3 * nq16;
    int64_t qt[G], lo[G], hi[G];
    bool mine[G];
    int64_t hlo = ntiles, hhi = 0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        mine[g] = grp * G + g < nqtiles;   // a partner tile that does not exist: the last tile once more, nothing stored
        qt[g] = mine[g] ? grp * G + g : nqtiles - 1;
        const int64_t tt = qtpos[qt[g]] >> 4;
        lo[g] = tt - window > 0 ? tt - window : 0;
        hi[g] = tt + window < ntiles ? tt + window : ntiles;
        hlo = lo[g] < hlo ? lo[g] : hlo;
        hhi = hi[g] > hhi ? hi[g] : hhi;
    }
    auto cut = [&](int64_t a, int64_t e, int64_t& t0, int64_t& t1) {   // part p of [a, e)
        const int64_t len = e > a ? (e - a + nparts - 1) / nparts : 0;
        t0 = a + p * len < e ? a + p * len : e;
        t1 = t0 + len < e ? t0 + len : e;
    };
    if (hhi - hlo <= 2 * (int64_t)window + window / 2) {
        int64_t t0, t1;
        cut(hlo, hhi, t0, t1);
        window_walk<FOLD, G>(Ap, Np, Bp, NYp, qt, mine, lo, hi, t0, t1, n_train, nq16, mypart, lane);
    } else {
#pragma unroll 1
        for (int g = 0; g < G; ++g) {
            int64_t q1[1], l1[1] = {0}, h1[1] = {0}, t0, t1;
            bool m1[1];
#pragma unroll
            for (int k = 0; k < G; ++k)
                if (k == g) { q1[0] = qt[k]; m1[0] = mine[k]; l1[0] = lo[k]; h1[0] = hi[k]; }
            if (!m1[0]) break;
            cut(l1[0], h1[0], t0, t1);
            window_walk<FOLD, 1>(Ap, Np, Bp, NYp, q1, m1, l1, h1, t0, t1, n_train, nq16, mypart, lane);
        }
    }
}

// one thread per query column: the parts of its walk in the order of their number, then the rules of the header comment
__global__ __launch_bounds__(256) void query_window_finish_kernel(const double* __restrict__ part, int nparts, const double* __restrict__ NYp,
                                                                  int64_t nqtiles, int64_t nq, double* __restrict__ qthr, double* __restrict__ qlb,
                                                                  double* __restrict__ qrow_thr, double* __restrict__ dbg) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, nq16 = nqtiles * 16;
    if (q >= nq16) return;   // (whole query tiles: the 16 lanes of a tile stay together)
    double mx = -INFINITY, s = 0.0, top = -INFINITY;
    for (int p = 0; p < nparts; ++p) {
        const double* o = part + (int64_t)p * 3 * nq16 + q;
        const double om = o[0], os = o[nq16], ot = o[2 * nq16];
        top = ot > top ? ot : top;
        if (om > mx) {
            const double sh = mx - om;
            s = (sh < -2000.0 ? 0.0 : __builtin_ldexp(s, (int)sh)) + os;
            mx = om;
        } else if (om > -INFINITY) {
            const double sh = om - mx;
            s += sh < -2000.0 ? 0.0 : __builtin_ldexp(os, (int)sh);
        }
    }
    const int64_t qt = q >> 4;
    const double ny = NYp[q];
    const bool valid = q < nq && ny == ny;
    const double lb = (valid && s > 0.0) ? mx + log2(s) - PBN_WINDOW_SLACK : -INFINITY;
    if (dbg && q < nq) dbg[q] = lb;
    if (qlb && valid && top > qlb[q]) qlb[q] = top;
    double g = valid ? lb : INFINITY;
    for (int off = 1; off < 16; off <<= 1) { const double o = __shfl_xor(g, off); g = o < g ? o : g; }
    const double told = qthr[qt];   // (every lane reads it before lane 0's store below: one wave, program order)
    const bool raise = g < INFINITY && g > told;
    if (qrow_thr) {
        const double T = raise ? g : told;
        qrow_thr[q] = (valid && lb > T) ? lb : T;
    }
    if ((q & 15) == 0 && raise) qthr[qt] = g;
}

void launch_pack_classic(const PackArgs& a, int dtype, hipStream_t st) {
    const int64_t npad = a.ntiles * 16;
    if (npad == 0) return;
    dim3 grid((unsigned)ceil_div(npad, 256)), block(256);
    if (dtype == PBN_F64 && a.src_f32) hipLaunchKernelGGL((pack_rows_kernel<double, float>), grid, block, 0, st, a);
    else if (dtype == PBN_F64) hipLaunchKernelGGL(pack_rows_kernel<double>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(pack_rows_kernel<float>, grid, block, 0, st, a);
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// Wide models (more than 32 whitened dimensions): generic pack and sweep, see kde_kernels.hpp
// ------------------------------------------------------------------------------------------------
template <typename TS>
__global__ __launch_bounds__(256) void pack_rows_wide_kernel(WidePackArgs a) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= a.ntiles * 16) return;
    const int64_t tile = r >> 4;
    const int idx = (int)(r & 15);
    const int d = a.d, KS = a.KS;
    const bool valid = r < a.n;
    int64_t src = 0;
    if (valid) {
        const int64_t lr = r < a.n0 ? a.row0 + r : a.row1 + (r - a.n0);
        src = a.rows ? (int64_t)a.rows[lr] : lr;
    }
    double nrm = 0.0;
    for (int i = 0; i < KS * 4; ++i) {
        double z = 0.0;
        if (valid && i < a.dm) {
            // z_i = sum_{j <= i} W[i][j] (x_j - mu_j): the row's coordinates are re-read per i (L1 / L2 hits) instead of living in a
            // per-thread array of unknown size
            const double* w = a.W + (size_t)i * a.ldw;
            for (int j = 0; j <= i; ++j) {
                const double x = (double)((const TS*)a.base + (int64_t)a.cols[j] * a.ld)[src] - a.mu[j];
                z = __builtin_fma(w[j], x, z);
            }
        }
        nrm = __builtin_fma(z, z, nrm);
        a.pack[(tile * KS + (i >> 2)) * 64 + (i & 3) * 16 + idx] = z;
    }
    double nv = -0.5 * nrm;
    if (!valid) nv = a.is_query ? 0.0 : PBN_PAD_NORM;
    if (a.is_query) {
        a.npack[tile * 16 + idx] = nv;
    } else {
        const int lg = idx & 3, i = idx >> 2;   // f64 C-row order: crow(lg, i) == idx
        a.npack[tile * 16 + lg * 4 + i] = nv;
    }
    if (a.upack) {   // CKDE::cdf: standardised "x - b.e" of the row, in the norm's layout
        double u = 0.0;
        if (valid)
            for (int j = 0; j < d; ++j) u = __builtin_fma(a.wu[j], (double)((const TS*)a.base + (int64_t)a.cols[j] * a.ld)[src] - a.mu[j], u);
        if (a.is_query) a.upack[tile * 16 + idx] = u;
        else a.upack[tile * 16 + (idx & 3) * 4 + (idx >> 2)] = u;
    }
}

void launch_pack_wide(const WidePackArgs& a, hipStream_t st) {
    const int64_t npad = a.ntiles * 16;
    if (npad == 0) return;
    dim3 grid((unsigned)ceil_div(npad, 256)), block(256);
    if (a.src_f32) hipLaunchKernelGGL(pack_rows_wide_kernel<float>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(pack_rows_wide_kernel<double>, grid, block, 0, st, a);
    HIP_CHECK(hipGetLastError());
}

// one wave = one group of 16 queries; the B fragments come from memory at every K step (the wave's 16 queries are the same for all
// tiles: L1 hits), the offset is raised tile by tile (online logsumexp, integer offsets), 2^x by the degree-8 polynomial
__global__ __launch_bounds__(256) void kde_sweep_wide_kernel(SweepArgs a, int KS) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane >> 4;
    const int64_t qt = (int64_t)blockIdx.x * 4 + wave;
    const int split = blockIdx.y;
    if (qt >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const PBN_GLOBAL double* __restrict__ Ap = (const PBN_GLOBAL double*)a.Apack;
    const PBN_GLOBAL double* __restrict__ Np = (const PBN_GLOBAL double*)a.nxpack;
    const PBN_GLOBAL double* __restrict__ Bp = (const PBN_GLOBAL double*)a.Bpack + qt * KS * 64 + lane;
    const double ny = ((const PBN_GLOBAL double*)a.nypack)[qt * 16 + (lane & 15)];
    double m = -INFINITY, sum = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        d4 acc = *(const PBN_GLOBAL d4*)(Np + t * 16 + lg * 4) + ny;
        const PBN_GLOBAL double* __restrict__ At = Ap + t * KS * 64 + lane;
        for (int ks = 0; ks < KS; ++ks) acc = Tr<double>::mfma(At[ks * 64], Bp[ks * 64], acc);
        const double vmax = colmax<double>(max4<double>(acc));   // uniform over the four lanes of a query column
        if (vmax > m) {
            const double nm = __builtin_ceil(vmax);
            sum *= exp2(m - nm);   // m = -inf: the sum is still 0
            m = nm;
        }
        sum += (Tr<double>::ex2_hi(acc[0] - m) + Tr<double>::ex2_hi(acc[1] - m)) + (Tr<double>::ex2_hi(acc[2] - m) + Tr<double>::ex2_hi(acc[3] - m));
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    if (lg == 0) {
        PBN_GLOBAL double* o = (PBN_GLOBAL double*)a.part + ((int64_t)split * a.nqtiles * 16 + qt * 16 + lane) * 2;
        o[0] = m;
        o[1] = sum;
    }
}

void launch_sweep_wide(const SweepArgs& a, int KS, int nsplit, hipStream_t st) {
    if (a.nqtiles == 0) return;
    dim3 grid((unsigned)ceil_div(a.nqtiles, 4), (unsigned)nsplit), block(256);
    hipLaunchKernelGGL(kde_sweep_wide_kernel, grid, block, 0, st, a, KS);
    HIP_CHECK(hipGetLastError());
}

void launch_max_norm2(const PackArgs& a, int src_dtype, double* dev_out, hipStream_t st) {
    if (a.n <= 0) return;
    dim3 grid((unsigned)ceil_div(a.n, 256)), block(256);
    if (src_dtype == PBN_F64) hipLaunchKernelGGL(max_norm2_kernel<double>, grid, block, 0, st, a, (unsigned long long*)dev_out);
    else hipLaunchKernelGGL(max_norm2_kernel<float>, grid, block, 0, st, a, (unsigned long long*)dev_out);
    HIP_CHECK(hipGetLastError());
}

// Exponent distance below the queries' sum bound beyond which a training tile is skipped.  PBN_PRUNE_MARGIN (fp64, 52) /
// PBN_PRUNE_MARGIN_F32 (fp32, 40) are the values AT 10^6 TRAINING ROWS; for n rows the margin is that + log2(n / 10^6), so that the
// bound of what pruning can drop - at most n terms of 2^-margin of the sum each - is the same fraction of the sum whatever the size
// of the training set: 10^6 x 2^-52 = 2.2e-10 (fp32: 10^6 x 2^-40 = 9.1e-7).  With a constant margin the bound grew linearly with n
// (and was needlessly tight for the 10^4-10^5-row folds and slices of the score engine: 90 000 rows -> 48.5, 450 000 -> 50.9;
// 4 x 10^6 -> 54).  PBN_PRUNE_MARGIN_ADAPT=0 keeps the constant.
// Round 4: sweeps whose result is a SUM over the test rows (slogl, the score engine's terms: `sum_only`) carry a per-term arithmetic
// error of 1.4e-7 anyway (2^f on the fp32 transcendental unit), fp32 tables one of ~1e-5 (2^-24 |z|^2): their margins are set so that
// the dropped-mass bound matches - fp64 sums 43 at 10^6 rows (1.1e-7 of a sum), fp32 36 (1.5e-5) - while per-row logl outputs keep 52
// (2.2e-10).  cv64 3.06 -> 2.74 s, C3's first iteration 14.1 -> 12.6 s, C5 9.1 -> 8.7 s with the same operator sequences
// (profiles/r4/margin_probe4.txt).  PBN_PRUNE_MARGIN pins the fp64 value for both kinds, PBN_PRUNE_MARGIN_SUM the sum-only one,
// PBN_PRUNE_MARGIN_F32 the fp32 one; read per call (a host getenv per sweep launch) so that tests can pin them inside one process.
double prune_margin(int dtype, int64_t n_train, bool sum_only) {
    const bool adapt = PBN_TUNE(PRUNE_MARGIN_ADAPT, 1) != 0;
    double base;
    if (use_f16x2(dtype)) base = knob_double("PBN_PRUNE_MARGIN_F32", (double)PBN_PRUNE_MARGIN_F32);
    else base = knob_double("PBN_PRUNE_MARGIN", sum_only ? knob_double("PBN_PRUNE_MARGIN_SUM", (double)PBN_PRUNE_MARGIN_SUM) : (double)PBN_PRUNE_MARGIN);
    if (!adapt || n_train <= 0) return base;
    const double m = base + std::log2((double)n_train / 1e6);
    return m < 8.0 ? 8.0 : m;
}

void launch_prune_keys(const PackArgs& a, int dtype, int zd, int kd, double* zrow, uint32_t* keys, int32_t* iota, hipStream_t st) {
    if (a.n == 0) return;
    const dim3 grid((unsigned)ceil_div(a.n, 256)), block(256);
    const double inv_cell = 1.0 / prune_key_cell(kd);
    static const int hnd = PBN_TUNE(PRUNE_HILBERT_ND, 1);   // Hilbert order at three / four key dimensions too (two: always)
    if (dtype == PBN_F64 && a.src_f32) hipLaunchKernelGGL((prune_keys_kernel<double, float>), grid, block, 0, st, a, zd, kd, zrow, keys, iota, inv_cell, hnd);
    else if (dtype == PBN_F64) hipLaunchKernelGGL(prune_keys_kernel<double>, grid, block, 0, st, a, zd, kd, zrow, keys, iota, inv_cell, hnd);
    else hipLaunchKernelGGL(prune_keys_kernel<float>, grid, block, 0, st, a, zd, kd, zrow, keys, iota, inv_cell, hnd);
    HIP_CHECK(hipGetLastError());
}
void launch_tile_boxes(const double* zrow, const int32_t* perm, int64_t n, int zd, int pd, double* box, double* zsorted, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(tile_box_kernel, dim3((unsigned)ceil_div(ceil_div(n, 16) * 16, 256)), dim3(256), 0, st, zrow, perm, n, zd, pd, box, zsorted);
    HIP_CHECK(hipGetLastError());
}
// one 64-lane block per (split, batch): the bounding box of up to 64 tile boxes (the first level of the pruned sweeps' tile walk)
__global__ __launch_bounds__(64) void batch_box_kernel(const double* __restrict__ tile_box, int pd, int64_t ntiles, int64_t tps, int nbps, double* __restrict__ out) {
    const int split = blockIdx.x / nbps, k = blockIdx.x - split * nbps;
    const int64_t t0 = (int64_t)split * tps, t1 = t0 + tps < ntiles ? t0 + tps : ntiles;
    const int64_t t = t0 + 64 * (int64_t)k + (int)threadIdx.x;
    double lo[PBN_PRUNE_PD], hi[PBN_PRUNE_PD];
#pragma unroll
    for (int i = 0; i < PBN_PRUNE_PD; ++i) { lo[i] = INFINITY; hi[i] = -INFINITY; }
    if (t < t1) {
        const double* bx = tile_box + t * 2 * pd;
#pragma unroll
        for (int i = 0; i < PBN_PRUNE_PD; ++i)
            if (i < pd) { lo[i] = bx[i]; hi[i] = bx[pd + i]; }
    }
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int i = 0; i < PBN_PRUNE_PD; ++i) {
            const double l = __shfl_xor(lo[i], off), h = __shfl_xor(hi[i], off);
            lo[i] = l < lo[i] ? l : lo[i];
            hi[i] = h > hi[i] ? h : hi[i];
        }
    }
    if (threadIdx.x == 0) {
        double* bb = out + (int64_t)blockIdx.x * 2 * pd;
        for (int i = 0; i < pd; ++i) { bb[i] = lo[i]; bb[pd + i] = hi[i]; }
    }
}
void launch_batch_boxes(const double* tile_box, int pd, int64_t ntiles, int64_t tiles_per_split, int nsplit, double* out, hipStream_t st) {
    const int nbps = (int)ceil_div(tiles_per_split, 64);
    if (ntiles == 0 || nsplit <= 0) return;
    hipLaunchKernelGGL(batch_box_kernel, dim3((unsigned)((int64_t)nsplit * nbps)), dim3(64), 0, st, tile_box, pd, ntiles, tiles_per_split, nbps, out);
    HIP_CHECK(hipGetLastError());
}
void launch_query_prepass(const double* zq_row, const int32_t* qperm, int64_t nq, const uint32_t* qkeys_sorted, const double* ztrain_sorted,
                          const uint32_t* tkeys_sorted, int64_t n, int zd, int pd, double* qbox, double* qthr, double* qlb, hipStream_t st,
                          const double* subpart, int P, int which, double log2_nsub, const double* tile_box, int64_t* qtpos, int sub_dtype) {
    if (nq == 0) return;
    double sub_abs, sub_rel;
    prune_subsample_slack(sub_dtype, sub_abs, sub_rel);
    static const int sum_bound = PBN_TUNE(GROUP_SUM_BOUND, 1);
    static const int tile_window = std::max(0, PBN_TUNE(GROUP_TILE_WINDOW, 256));
    hipLaunchKernelGGL(query_prepass_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, zq_row, qperm, nq, qkeys_sorted, ztrain_sorted,
                       tkeys_sorted, n, zd, pd, qbox, qthr, qlb, subpart, P, which, log2_nsub, sub_abs, sub_rel, sum_bound, tile_box, tile_window, qtpos);
    HIP_CHECK(hipGetLastError());
}

// parts a window walk is cut into (query_window_kernel): the number in 1..8 under which the most loaded CU carries the least work - workgroups
// of four waves are dealt to the CUs in turn, so the work of a CU is ceil(workgroups / CUs) walks of 1 / parts of a window each - and among
// numbers within 3 % of the best the smallest: 1e5 queries on 256 CUs: 1 563 groups, 5 parts, 1 954 workgroups, 8 on a CU at most for 7.6
int window_parts(int64_t nqtiles, int num_cus) {
    static const int fixed = PBN_TUNE(WINDOW_PARTS, 0);
    if (fixed > 0) return fixed < 64 ? fixed : 64;
    const int64_t groups = ceil_div(nqtiles, PBN_WINDOW_NQ), cus = num_cus > 0 ? num_cus : 1;
    double cost[9], best = INFINITY;
    for (int s = 1; s <= 8; ++s) {
        cost[s] = (double)ceil_div(ceil_div(groups * s, 4), cus) / s;
        best = cost[s] < best ? cost[s] : best;
    }
    for (int s = 1; s <= 8; ++s)
        if (cost[s] <= 1.03 * best) return s;
    return 8;
}
size_t window_part_bytes(int64_t nqtiles, int nparts) { return (size_t)nparts * 3 * (size_t)nqtiles * 16 * sizeof(double); }

void launch_query_window(const double* Apack, const double* nxpack, const double* Bpack, const double* nypack, int64_t ntiles, int64_t n_train,
                         int64_t nqtiles, int64_t nq, const int64_t* qtpos, int window, bool fold, double* qthr, double* qlb, double* qrow_thr, double* dbg,
                         int nparts, double* part, hipStream_t st) {
    if (nqtiles == 0 || window <= 0) return;
    const dim3 grid((unsigned)ceil_div(ceil_div(nqtiles, PBN_WINDOW_NQ) * nparts, 4));
    if (fold) hipLaunchKernelGGL(query_window_kernel<true>, grid, dim3(256), 0, st, Apack, nxpack, Bpack, nypack, ntiles, n_train, nqtiles, qtpos, window, nparts, part);
    else hipLaunchKernelGGL(query_window_kernel<false>, grid, dim3(256), 0, st, Apack, nxpack, Bpack, nypack, ntiles, n_train, nqtiles, qtpos, window, nparts, part);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(query_window_finish_kernel, dim3((unsigned)ceil_div(nqtiles * 16, 256)), dim3(256), 0, st, part, nparts, nypack, nqtiles, nq, qthr, qlb, qrow_thr, dbg);
    HIP_CHECK(hipGetLastError());
}

}  // namespace pbn
