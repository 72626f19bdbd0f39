// The per-lane partial-correlation test of LinearCorrelation's device batch over tables with nulls (lincor_null_finish_kernel,
// lincor_null_batch.hip) as a __device__ function: the symmetric eigenproblem of one (k + 2)-variable covariance block, the
// pseudo-inverse and the Student-t tail.  It restates the body of lincor_batch_kernel (lincor_batch.hip) statement for statement.
// That kernel keeps its own text: moved into this function it computed the same operations (equal counts of every fp64 opcode) with
// other operands fused - its largest difference from the host routine went from 3.68e-11 to 5.26e-11, past the bound
// tests/test_lincor_batch_gpu.py measured for it - and what it computes is not this unit's to change.
#pragma once
#include "lincor.hpp"

namespace pbn {
namespace lincor {

template <int M>
struct Tri {   // upper triangle, row-major: (i, j) with i <= j
    static constexpr int SIZE = M * (M + 1) / 2;
    static constexpr __host__ __device__ int at(int i, int j) { return i <= j ? i * M - i * (i - 1) / 2 + (j - i) : j * M - j * (j - 1) / 2 + (i - j); }
};

#ifdef __HIPCC__
// p-value of the test whose covariance block is `a` (destroyed: it holds the rotated block afterwards) over `rows` rows.  redo: an
// eigenvalue lies within REDO_FACTOR of the pseudo-inverse threshold (or the block holds a NaN) - the caller recomputes the test with
// the host routine.  Every index into a, u0, u1 is a compile-time constant.
template <int M>
__device__ __forceinline__ double block_pvalue(double (&a)[Tri<M>::SIZE], long long rows, bool& redo) {
    if constexpr (M == 2) {   // cor_0cond
        double cor = 0;
        if (!(a[Tri<2>::at(0, 0)] < MACHINE_TOL || a[Tri<2>::at(1, 1)] < MACHINE_TOL))
            cor = fmin(1.0, fmax(-1.0, a[Tri<2>::at(0, 1)] / sqrt(a[Tri<2>::at(0, 0)] * a[Tri<2>::at(1, 1)])));
        redo = false;
        return cor_pvalue(cor, test_df(rows, 0));
    } else {
        double u0[M], u1[M];
#pragma unroll
        for (int i = 0; i < M; ++i) { u0[i] = i == 0 ? 1.0 : 0.0; u1[i] = i == 1 ? 1.0 : 0.0; }
        for (int sweep = 0; sweep < 64; ++sweep) {
            double off = 0.0, diag = 0.0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                diag += a[Tri<M>::at(i, i)] * a[Tri<M>::at(i, i)];
#pragma unroll
                for (int j = i + 1; j < M; ++j) off += a[Tri<M>::at(i, j)] * a[Tri<M>::at(i, j)];
            }
            if (off <= 1e-34 * diag || off == 0.0) break;
#pragma unroll
            for (int p = 0; p < M - 1; ++p)
#pragma unroll
                for (int q = p + 1; q < M; ++q) {
                    const double apq = a[Tri<M>::at(p, q)];
                    if (apq == 0.0) continue;
                    const double app = a[Tri<M>::at(p, p)], aqq = a[Tri<M>::at(q, q)];
                    const double theta = (aqq - app) / (2.0 * apq);
                    const double tt = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
                    for (int r = 0; r < M; ++r) {
                        if (r == p || r == q) continue;
                        const double arp = a[Tri<M>::at(r, p)], arq = a[Tri<M>::at(r, q)];
                        a[Tri<M>::at(r, p)] = c * arp - s * arq;
                        a[Tri<M>::at(r, q)] = s * arp + c * arq;
                    }
                    // the 2 x 2 block: columns p, q first, then rows p, q, as the host's two passes do
                    const double app1 = c * app - s * apq, apq1 = s * app + c * apq;
                    const double aqp1 = c * apq - s * aqq, aqq1 = s * apq + c * aqq;
                    a[Tri<M>::at(p, p)] = c * app1 - s * aqp1;
                    a[Tri<M>::at(p, q)] = c * apq1 - s * aqq1;
                    a[Tri<M>::at(q, q)] = s * apq1 + c * aqq1;
                    const double u0p = u0[p], u0q = u0[q], u1p = u1[p], u1q = u1[q];
                    u0[p] = c * u0p - s * u0q; u0[q] = s * u0p + c * u0q;
                    u1[p] = c * u1p - s * u1q; u1[q] = s * u1p + c * u1q;
                }
        }
        // cor_svd (linearcorrelation.hpp:29-47): partial correlation of the first two variables from the pseudo-inverse
        double dmax = a[Tri<M>::at(0, 0)], dmin = dmax;
#pragma unroll
        for (int i = 1; i < M; ++i) { dmax = fmax(dmax, a[Tri<M>::at(i, i)]); dmin = fmin(dmin, a[Tri<M>::at(i, i)]); }
        const double tol = M * dmax * 2.220446049250313e-16;
        double p11 = 0, p12 = 0, p22 = 0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const double d = a[Tri<M>::at(i, i)];
            if (d > tol) {
                const double inv = 1.0 / d;
                p11 += u0[i] * u0[i] * inv;
                p12 += u0[i] * u1[i] * inv;
                p22 += u1[i] * u1[i] * inv;
            }
        }
        double cor = 0;
        if (!(p11 < MACHINE_TOL || p22 < MACHINE_TOL)) cor = fmin(1.0, fmax(-1.0, -p12 / sqrt(p11 * p22)));
        redo = !(dmin >= REDO_FACTOR * tol);   // (a NaN block is flagged as well)
        return cor_pvalue(cor, test_df(rows, M - 2));
    }
}
#endif

}  // namespace lincor
}  // namespace pbn
