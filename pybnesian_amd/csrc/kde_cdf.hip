// CKDE::cdf / sample and the UCV pair sums: weight kernels on the sweep's MFMA + offset machinery (see kde_kernels.hip).
#include "common.hpp"
#include "kde_kernels.hpp"
#include "kde_device.hpp"

namespace pbn {

// ------------------------------------------------------------------------------------------------
// kde_cdf: CKDE::cdf.  The reference (CKDE.hpp:560-735 + KDE.cl.src:376-468) materialises, per tile of 64 test rows,
// the N x 64 weight matrix W (marginal KDE terms), the N x 64 conditional means, their normal cdf, the element-wise
// product and two column sums.  Here: the weights are the marginal sweep's 2^(s2 - m) (same MFMA + offset machinery),
// the conditional mean is linear, (x_q - mu_t(e_q)) / sigma_c = u_q - u_t with u = (x - b.e) / sigma_c precomputed per
// row, so a pair costs one erfc; cdf_q = sum_t w_t Phi(u_q - u_t) / sum_t w_t.  No evidence: w_t = 1.
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T half_erfc(T x);
template <>
__device__ __forceinline__ double half_erfc<double>(double x) { return 0.5 * erfc(x); }

// 1/2 erfc(x) for the fp64 CKDE::cdf kernel, branch-free: erfc(|x|) = erfcx(|x|) exp(-x^2) with erfcx from a table of
// degree-7 polynomials on [i/8, (i+1)/8) (48 intervals up to 6, relative error 6.5e-14: tools/erfcx_table.py; beyond 6
// the exponential alone is below 2^-52), the table staged in LDS, the exponential by the sweep's own 2^x.  About a third
// of the instructions of the library erfc.
#define PBN_ERFCX_INTERVALS 48
__device__ const double ERFCX_TABLE[PBN_ERFCX_INTERVALS * 8] = {
#include "erfcx_table.inc"
};
__device__ __forceinline__ double half_erfc_table(double x, const double* __restrict__ tab) {
    const double a = __builtin_fabs(x);
    const double ac = __builtin_fmin(a, 5.999999999);
    int idx;
    const double scaled = ac * 8.0;
    asm("v_cvt_i32_f64 %0, %1" : "=v"(idx) : "v"(scaled));                 // truncation = floor: ac >= 0
    const double r = __builtin_fma((double)idx, -0.125, ac) - 0.0625;     // centred in the interval
    const double* c = tab + idx * 8;
    double p = c[7];
    p = __builtin_fma(p, r, c[6]);
    p = __builtin_fma(p, r, c[5]);
    p = __builtin_fma(p, r, c[4]);
    p = __builtin_fma(p, r, c[3]);
    p = __builtin_fma(p, r, c[2]);
    p = __builtin_fma(p, r, c[1]);
    p = __builtin_fma(p, r, c[0]);
    const double e = exp2_f64<8>(-(a * a) * 0x1.71547652b82fep+0);        // exp(-a^2)
    const double h = 0.5 * p * e;
    return x >= 0.0 ? h : 1.0 - h;
}
template <>
__device__ __forceinline__ float half_erfc<float>(float x) { return 0.5f * erfcf(x); }

// MODE 0: weights only (CKDE::sample), 1: weights x normal cdf (CKDE::cdf), 2: sum w and sum sqrt(w) with the offset
// pinned at 0 (UCV: K_2H = sqrt of the un-normalised K_H; self pairs keep every exponent <= 0)
template <typename T, int KS, int QG, int MODE>
__global__ __launch_bounds__(256, 2) void kde_cdf_kernel(CdfArgs a) {
    constexpr bool CDF = MODE == 1;
    // KS == 0: the number of K steps is a run-time value (more than 16 evidence variables / UCV dimensions): the fragments of both
    // sides are read at every step instead of living in registers
    constexpr bool RT = KS == 0;
    constexpr int KSR = RT ? 1 : KS;
    const int ksn = RT ? a.KS : KS;
    using V = typename Tr<T>::vec4;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int lg = lane >> 4;
    int qx, split;
    xcd_block(qx, split);
    constexpr bool TABLE = CDF && sizeof(T) == 8;
    __shared__ double etab[TABLE ? PBN_ERFCX_INTERVALS * 8 : 1];
    if (TABLE) {   // before any wave leaves: the barrier needs them all
        for (int e = threadIdx.x; e < PBN_ERFCX_INTERVALS * 8; e += 256) etab[e] = ERFCX_TABLE[e];
        __syncthreads();
    }
    const int64_t qt0 = ((int64_t)qx * 4 + wave) * QG;
    if (qt0 >= a.nqtiles) return;
    const int64_t t0 = (int64_t)split * a.tiles_per_split;
    const int64_t t1 = (t0 + a.tiles_per_split < a.ntiles) ? t0 + a.tiles_per_split : a.ntiles;
    const T* __restrict__ Ap = (const T*)a.Apack;
    const T* __restrict__ Np = (const T*)a.nxpack;
    const T* __restrict__ Up = (const T*)a.utrain;
    const T* __restrict__ Bp = (const T*)a.Bpack;
    const T* __restrict__ NYp = (const T*)a.nypack;
    const T* __restrict__ UQp = (const T*)a.uquery;

    T b[QG][KSR], ny[QG], cm[QG], m[QG], uq[QG];
    int64_t qtg[QG];
    double sw[QG], sc[QG];
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        int64_t qt = qt0 + g < a.nqtiles ? qt0 + g : a.nqtiles - 1;
        qtg[g] = qt;
        if constexpr (!RT) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) b[g][ks] = Bp[(qt * KS + ks) * 64 + lane];
        }
        ny[g] = NYp[qt * 16 + (lane & 15)];
        uq[g] = CDF ? UQp[qt * 16 + (lane & 15)] : (T)0;
        sw[g] = 0.0; sc[g] = 0.0;
    }
    {   // offsets from the first tile
        const V nx = *(const V*)(Np + t0 * 16 + lg * 4);
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            V acc = nx + ny[g];
            if constexpr (RT) {
                for (int ks = 0; ks < ksn; ++ks) acc = Tr<T>::mfma(Ap[(t0 * ksn + ks) * 64 + lane], Bp[(qtg[g] * ksn + ks) * 64 + lane], acc);
            } else {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = Tr<T>::mfma(Ap[(t0 * KS + ks) * 64 + lane], b[g][ks], acc);
            }
            m[g] = MODE == 2 ? (T)0 : colmax<T>(max4<T>(acc));
            cm[g] = ny[g] - m[g];
        }
    }
    for (int64_t t = t0; t < t1; ++t) {
        T af[KSR];
        if constexpr (!RT) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) af[ks] = Ap[(t * KS + ks) * 64 + lane];
        }
        const V nx = *(const V*)(Np + t * 16 + lg * 4);
        V ut = {0, 0, 0, 0};
        if (CDF) ut = *(const V*)(Up + t * 16 + lg * 4);
#pragma unroll
        for (int g = 0; g < QG; ++g) {
            V acc = nx + cm[g];
            if constexpr (RT) {
                for (int ks = 0; ks < ksn; ++ks) acc = Tr<T>::mfma(Ap[(t * ksn + ks) * 64 + lane], Bp[(qtg[g] * ksn + ks) * 64 + lane], acc);
            } else {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = Tr<T>::mfma(af[ks], b[g][ks], acc);
            }
            T w0 = Tr<T>::ex2_hi(acc[0]), w1 = Tr<T>::ex2_hi(acc[1]), w2 = Tr<T>::ex2_hi(acc[2]), w3 = Tr<T>::ex2_hi(acc[3]);
            T ts = (w0 + w1) + (w2 + w3);
            if (MODE != 2 && __builtin_expect(__any(!(ts < Tr<T>::big())), 0)) {
                const T mx = colmax<T>(max4<T>(acc));
                if (mx > (T)0) {
                    m[g] += mx;
                    cm[g] = ny[g] - m[g];
                    const double f = exp2(-(double)mx);
                    sw[g] *= f; sc[g] *= f;
                    acc -= mx;
                }
                w0 = Tr<T>::ex2_hi(acc[0]); w1 = Tr<T>::ex2_hi(acc[1]); w2 = Tr<T>::ex2_hi(acc[2]); w3 = Tr<T>::ex2_hi(acc[3]);
                ts = (w0 + w1) + (w2 + w3);
            }
            if constexpr (MODE == 2 && sizeof(T) == 4) {
                // UCV takes the N self pairs off the totals as N: a row against itself must weigh exactly 1.  The fp32 Gram form leaves
                // 1 + O(2^-24 |z|^2) there, which the K_H term multiplies by 2^(d/2 + 1) against the K_2H(0) the score starts from.
                if (t == qtg[g]) {
                    const int col = lane & 15;
                    w0 = Tr<T>::crow(lg, 0) == col ? (T)1 : w0; w1 = Tr<T>::crow(lg, 1) == col ? (T)1 : w1;
                    w2 = Tr<T>::crow(lg, 2) == col ? (T)1 : w2; w3 = Tr<T>::crow(lg, 3) == col ? (T)1 : w3;
                    ts = (w0 + w1) + (w2 + w3);
                }
            }
            // Phi((x_q - mu_t)/sigma_c) = 1/2 erfc((u_t - u_q)), u pre-divided by sqrt 2 (KDE.cl.src:448-456)
            sw[g] += (double)ts;
            if (MODE == 2) sc[g] += (double)((sqrt(w0) + sqrt(w1)) + (sqrt(w2) + sqrt(w3)));
            if (CDF) {
                auto phi = [&](T v) -> T {
                    if constexpr (TABLE) return (T)half_erfc_table((double)v, etab);
                    else return half_erfc<T>(v);
                };
                const T c = (w0 * phi(ut[0] - uq[g]) + w1 * phi(ut[1] - uq[g])) + (w2 * phi(ut[2] - uq[g]) + w3 * phi(ut[3] - uq[g]));
                sc[g] += (double)c;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < QG; ++g) {
        double s = sw[g], c = sc[g];
        s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
        c += __shfl_xor(c, 16); c += __shfl_xor(c, 32);
        if (lg == 0 && qt0 + g < a.nqtiles) {
            double* o = a.part + ((int64_t)split * a.nqtiles * 16 + (qt0 + g) * 16 + lane) * 4;
            o[0] = (double)m[g]; o[1] = s; o[2] = c; o[3] = 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void kde_cdf_finish_kernel(const double* __restrict__ part, int nsplit, int64_t nqtiles, int64_t nq,
                                                              double* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const double* p = part + q * 4;
    const int64_t stride = nqtiles * 16 * 4;
    double m = p[0], sw = p[1], sc = p[2];
    for (int sp = 1; sp < nsplit; ++sp) {
        const double* pp = p + sp * stride;
        const double M = m > pp[0] ? m : pp[0];
        const double f1 = exp2(m - M), f2 = exp2(pp[0] - M);
        sw = sw * f1 + pp[1] * f2;
        sc = sc * f1 + pp[2] * f2;
        m = M;
    }
    out[q] = sc / sw;
}

template <typename T, int CDF>
static void launch_cdf_t(const CdfArgs& a, int KS, dim3 grid, hipStream_t st) {
    dim3 block(256);
    switch (KS) {
        case 1: hipLaunchKernelGGL((kde_cdf_kernel<T, 1, 2, CDF>), grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL((kde_cdf_kernel<T, 2, 2, CDF>), grid, block, 0, st, a); break;
        case 3: hipLaunchKernelGGL((kde_cdf_kernel<T, 3, 2, CDF>), grid, block, 0, st, a); break;
        case 4: hipLaunchKernelGGL((kde_cdf_kernel<T, 4, 2, CDF>), grid, block, 0, st, a); break;
        default:
            if constexpr (sizeof(T) == 8) hipLaunchKernelGGL((kde_cdf_kernel<T, 0, 2, CDF>), grid, block, 0, st, a);   // runtime-sized (a.KS)
            else throw invalid_error("CKDE::cdf / sample / UCV: more than 16 dimensions take fp64 fragments");
    }
    HIP_CHECK(hipGetLastError());
}

// utrain == nullptr: weights only (sum w per split; used by CKDE::sample to locate the sampled instance).
void launch_cdf(const CdfArgs& a_in, int dtype, int KS, int nsplit, hipStream_t st) {
    CdfArgs a = a_in;
    a.KS = KS;
    dim3 grid((unsigned)ceil_div(a.nqtiles, 4 * 2), (unsigned)nsplit);
    const bool cdf = a.utrain != nullptr;
    if (dtype == PBN_F64) { if (cdf) launch_cdf_t<double, 1>(a, KS, grid, st); else launch_cdf_t<double, 0>(a, KS, grid, st); }
    else                  { if (cdf) launch_cdf_t<float, 1>(a, KS, grid, st); else launch_cdf_t<float, 0>(a, KS, grid, st); }
}

// UCV pair sums: part[split][query] = (0, sum_t w, sum_t sqrt w, 0) with w = 2^(s2(t, q)); then the two totals over the
// first nq queries and all splits, fixed order.
__global__ __launch_bounds__(256) void ucv_block_sums_kernel(const double* __restrict__ part, int nsplit, int64_t nqtiles, int64_t nq,
                                                              double* __restrict__ block_w, double* __restrict__ block_r) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double w = 0.0, r = 0.0;
    if (q < nq) {
        const int64_t stride = nqtiles * 16 * 4;
        for (int sp = 0; sp < nsplit; ++sp) {
            w += part[sp * stride + q * 4 + 1];
            r += part[sp * stride + q * 4 + 2];
        }
    }
    __shared__ double red[256];
    for (int pass = 0; pass < 2; ++pass) {
        red[threadIdx.x] = pass ? r : w;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) (pass ? block_r : block_w)[blockIdx.x] = red[0];
        __syncthreads();
    }
}

void launch_ucv(const CdfArgs& a_in, int dtype, int KS, int nsplit, int64_t nq, double* block_scratch, double* dev_out2, hipStream_t st) {
    CdfArgs a = a_in;
    a.KS = KS;
    dim3 grid((unsigned)ceil_div(a.nqtiles, 4 * 2), (unsigned)nsplit);
    if (dtype == PBN_F64) launch_cdf_t<double, 2>(a, KS, grid, st); else launch_cdf_t<float, 2>(a, KS, grid, st);
    const int64_t nblocks = ceil_div(nq, 256);
    hipLaunchKernelGGL(ucv_block_sums_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, a.part, nsplit, a.nqtiles, nq, block_scratch,
                       block_scratch + nblocks);
    HIP_CHECK(hipGetLastError());
    launch_reduce_final(block_scratch, nblocks, dev_out2, st);
    launch_reduce_final(block_scratch + nblocks, nblocks, dev_out2 + 1, st);
}

void launch_cdf_finish(const double* part, int nsplit, int64_t nqtiles, int64_t nq, double* dev_out, hipStream_t st) {
    if (nq == 0) return;
    hipLaunchKernelGGL(kde_cdf_finish_kernel, dim3((unsigned)ceil_div(nq, 256)), dim3(256), 0, st, part, nsplit, nqtiles, nq, dev_out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace pbn
