// The end of the KDE pipeline - kde_finish, the final reduction, the difference of two logl vectors - and the host predicates that pick a
// sweep's shape (shared by the launchers in kde_kernels.hip and the model code).
#include "common.hpp"
#include "kde_kernels.hpp"

namespace pbn {

// ------------------------------------------------------------------------------------------------
// kde_finish: per query merge the split partials (fixed order), logl = lognorm + ln2*(m + log2 sum)
// [CKDE: joint - marginal], optional logl store, deterministic block tree sum.
// ------------------------------------------------------------------------------------------------
template <bool COND>
__global__ __launch_bounds__(256) void kde_finish_kernel(FinishArgs a) {
    constexpr int P = COND ? 4 : 2;
    constexpr double LN2 = 0.693147180559945309417232121458;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double val = 0.0, val_marg = 0.0;
    if (q < a.nq) {
        const double* p = a.part + q * P;
        const int64_t stride = a.nqtiles * 16 * P;
        // two passes: the largest offset first, then the sums scaled to it in split order - one 2^x per partial and no
        // dependent chain (the running-rescale form cost two library exp2 per split in sequence: with the 157 splits of a
        // 90 000 x 10 000 sweep this kernel took 65 us against the sweep's 250).  Integer offsets (the fp64 sweeps' own) make every
        // factor an exact power of two, so the result is the one of the running form bit for bit.
        double m = p[0], mjj = COND ? p[2] : 0.0;
        for (int sp = 1; sp < a.nsplit; ++sp) {
            const double* pp = p + sp * stride;
            const double m2 = pp[0];
            m = m > m2 ? m : m2;
            if (COND) { const double m3 = pp[2]; mjj = mjj > m3 ? mjj : m3; }
        }
        double s = 0.0, sj = 0.0;
#pragma unroll 4
        for (int sp = 0; sp < a.nsplit; ++sp) {
            const double* pp = p + sp * stride;
            s += pp[1] * exp2(pp[0] - m);
            if (COND) sj += pp[3] * exp2(pp[2] - mjj);
        }
        double l = a.lognorm + LN2 * (m + log2(s));
        if (COND) {
            const double lj = a.lognorm + LN2 * (mjj + log2(sj)), lm = a.lognorm_marg + LN2 * (m + log2(s));
            l = lj - lm;
            if (a.block_sums_marg) { l = lj; val_marg = lm; }   // the two sums separately (score engine's set cache)
        }
        if (a.logl) a.logl[a.scatter ? (int64_t)a.scatter[q] : q] = l;
        val = l;
    }
    __shared__ double red[256];
    red[threadIdx.x] = val;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0 && a.block_sums) a.block_sums[blockIdx.x] = red[0];
    if (COND && a.block_sums_marg) {
        __syncthreads();
        red[threadIdx.x] = val_marg;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.block_sums_marg[blockIdx.x] = red[0];
    }
}

// Final fixed-order reduction of the per-block sums (replaces the multi-pass sum1d of
// opencl_config.hpp:344-397 with one launch).
__global__ __launch_bounds__(256) void reduce_final_kernel(const double* __restrict__ in, int64_t n, double* out) {
    __shared__ double red[256];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) v += in[i];
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

__global__ __launch_bounds__(256) void diff_kernel(double* __restrict__ out, const double* __restrict__ a, const double* __restrict__ b, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = a[i] - b[i];
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
void launch_diff(double* out, const double* a, const double* b, int64_t n, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(diff_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, out, a, b, n);
    HIP_CHECK(hipGetLastError());
}

void launch_reduce_final(const double* in, int64_t n, double* out, hipStream_t st) {
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(256), 0, st, in, n, out);
    HIP_CHECK(hipGetLastError());
}

bool use_f16x2(int dtype) {
    static const int v = PBN_TUNE(F32_F16X2, 1);   // (0: fp32 tables on the f32 MFMA kernels - the round-1 path, kept for comparisons)
    return v != 0 && dtype == PBN_F32;
}

int f16x2_mfmas(int dm) { return f16x2_blocks(dm); }   // f16x2: three (four where they fit) slots per dimension + the training norm

bool sweep_folds_norm(int dtype, bool cond, int KS, int dm) {
    static const int v = PBN_TUNE(SWEEP_FOLD, 1);
    return v != 0 && !use_f16x2(dtype) && dm % 4 != 0 && KS <= 4;   // more than 16 dimensions: one form only
}

bool sweep_weights_norm(int dtype, bool cond, int KS, int dm) {
    static const int v = PBN_TUNE(SWEEP_WMUL, 1);
    return v != 0 && dtype == PBN_F64 && !cond && dm % 4 == 0 && KS <= 2;   // KS 3, 4: 169 / 181 VGPRs, a wave per SIMD lost
}

int sweep_qg(int dtype, bool cond, int KS, bool prune) {
    if (prune && dtype == PBN_F64) return cond ? PBN_QG_PRUNE_COND : PBN_QG_PRUNE;
    if (prune && use_f16x2(dtype) && !cond) return PBN_F16_QG_PRUNE;   // (what the grids of the pruned launches - stand-alone and grouped - are sized with)
    if (KS > 4) return 2;   // more than 16 (fp32: 20) dimensions: two query groups per wave (fragment registers); KS = MFMAs per tile pair
    if (dtype == PBN_F64) return cond ? SweepQG<true, true>::value : SweepQG<true, false>::value;
    return cond ? SweepQG<false, true>::value : SweepQG<false, false>::value;
}

void launch_finish(const FinishArgs& a, bool cond, double* dev_sum_out, hipStream_t st, double* dev_sum_marg_out) {
    const int64_t nblocks = ceil_div(a.nq, 256);
    if (nblocks == 0) return;
    dim3 grid((unsigned)nblocks), block(256);
    if (cond)
        hipLaunchKernelGGL(kde_finish_kernel<true>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(kde_finish_kernel<false>, grid, block, 0, st, a);
    HIP_CHECK(hipGetLastError());
    if (dev_sum_out) launch_reduce_final(a.block_sums, nblocks, dev_sum_out, st);
    if (dev_sum_marg_out && a.block_sums_marg) launch_reduce_final(a.block_sums_marg, nblocks, dev_sum_marg_out, st);
}

}  // namespace pbn
