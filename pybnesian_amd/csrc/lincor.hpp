// LinearCorrelation's handle and the p-value arithmetic its host routine (lincor.hip) and its device batch
// (lincor_batch.hip) share: one text for both sides, so that they can differ by rounding only (hipcc contracts a * b + c
// into an FMA for the device; the host build has none).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "common.hpp"

struct pbn_lincor {
    int n = 0;
    int64_t rows = 0;
    std::vector<double> cov;  // n x n
    // handles made from a device table (pbn_lincor_create) keep the covariance on the device as well and remember their context;
    // handles from pbn_lincor_from_cov are host only (ctx null)
    pbn::ctx_ptr ctx;
    pbn::dev_buf<double> dcov;
    int64_t batch_threshold = 0;   // batches (per conditioning-set size) of fewer tests loop on the host; set by pbn_lincor_create
    int64_t device_tests = 0, host_tests = 0, host_redone = 0;   // pbn_lincor_batch_stats
    // grow-only staging of the batch function
    pbn::dev_buf<int> d_idx;
    pbn::dev_buf<double> d_out;
    pbn::dev_buf<unsigned char> d_flag;
};

namespace pbn {
namespace lincor {

// inlined into the kernels on the device (a call would park the lane's block across it); the host build is left as it was
#if defined(__HIP_DEVICE_COMPILE__)
#define PBN_HD __host__ __device__ __attribute__((always_inline)) inline
#else
#define PBN_HD __host__ __device__ inline
#endif

constexpr double MACHINE_TOL = 1.4901161193847656e-08;  // util/math_constants.hpp:30
// the device batch covers conditioning sets of 0 ... K_DEV variables (blocks of up to K_DEV + 2 = 8: the symmetric triangle and two
// rows of eigenvectors are 52 doubles per lane, 104 of the 128 registers that keep four waves per SIMD); larger sets loop on the host
constexpr int K_DEV = 6;
// a = df / 2 below this takes two lgamma() on the host; the device has the asymptotic series only, so such tests stay on the host
constexpr double LGAMMA_SERIES_MIN = 16.0;
// default of pbn_lincor_set_batch_threshold: the smallest measured batch from which the device wins for every k - at 1 000 tests
// k = 0 (no eigenproblem at all) is at 1.1 x the host loop and k = 6 at 20 x; at 500 k = 0 loses (profiles/r10/pc_timing.json)
constexpr int64_t LINCOR_BATCH_MIN_TESTS = 1000;
// an eigenvalue below REDO_FACTOR x the pseudo-inverse threshold makes the lane hand its test back to the host: next to the
// threshold one ulp decides whether the eigenvalue is dropped
constexpr double REDO_FACTOR = 8.0;

// log(Gamma(a + 1/2) / Gamma(a)) without the cancellation of two lgamma() of ~a log a each
PBN_HD double lgamma_ratio_half(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (a < LGAMMA_SERIES_MIN) return std::numeric_limits<double>::quiet_NaN();   // never dispatched to the device
#else
    if (a < LGAMMA_SERIES_MIN) return std::lgamma(a + 0.5) - std::lgamma(a);
#endif
    const double r = 1.0 / a;
    // Gamma(a+1/2)/Gamma(a) = sqrt(a) (1 - 1/(8a) + 1/(128a^2) + 5/(1024a^3) - 21/(32768a^4) - 399/(262144a^5) ...)
    const double s = 1.0 + r * (-1.0 / 8 + r * (1.0 / 128 + r * (5.0 / 1024 + r * (-21.0 / 32768 + r * (-399.0 / 262144 + r * (869.0 / 4194304))))));
    return 0.5 * std::log(a) + std::log(s);
}

// Regularised incomplete beta I_x(a, b) by the modified Lentz continued fraction; log_pref = log of x^a (1-x)^b / B(a,b).
PBN_HD double ibeta_cf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    double c = 1.0, d = 1.0 - (a + b) * x / (a + 1.0);
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m < 100000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((a + m2 - 1.0) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (a + b + m) * x / ((a + m2) * (a + m2 + 1.0));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < eps) break;
    }
    return h;
}

// 2 * P(T_df > |t|) = I_{df/(df+t^2)}(df/2, 1/2)   (linearcorrelation.cpp:9-13 with boost's students_t)
PBN_HD double two_sided_t_pvalue(double t, double df) {
    // Boost's students_t rejects df <= 0 (domain_error): fewer rows than variables + 2
    if (std::isnan(t) || !(df > 0)) return std::numeric_limits<double>::quiet_NaN();
    if (std::isinf(t)) return 0.0;
    const double t2 = t * t;
    if (t2 == 0.0) return 1.0;
    const double a = 0.5 * df, b = 0.5;
    const double x = df / (df + t2), y = t2 / (df + t2);  // y = 1 - x without cancellation
    // log B(a, 1/2) = lgamma(1/2) - log(Gamma(a + 1/2) / Gamma(a))
    const double lbeta = 0.5 * std::log(3.14159265358979323846264338327950288) - lgamma_ratio_half(a);
    const double lx = (t2 < df) ? std::log1p(-y) : std::log(x);
    const double ly = (t2 < df) ? std::log(y) : std::log1p(-x);
    const double log_pref = a * lx + b * ly - lbeta;
    if (x < (a + 1.0) / (a + b + 2.0)) {
        // tails below the smallest normal double are reported as 0: the power terms of Boost's / cephes' incomplete
        // beta underflow there, and exact zeros are what the tie-breaking of MMPC sees for such pairs
        const double p = std::exp(log_pref) * ibeta_cf(a, b, x) / a;
        return p < std::numeric_limits<double>::min() ? 0.0 : p;
    }
    return 1.0 - std::exp(log_pref) * ibeta_cf(b, a, y) / b;
}

PBN_HD double cor_pvalue(double cor, int64_t df) {
    const double statistic = cor * std::sqrt((double)df) / std::sqrt(1 - cor * cor);
    return two_sided_t_pvalue(std::fabs(statistic), (double)df);
}

// linearcorrelation.cpp:46,93: N - 2 without a conditioning set, N - 3 for one conditioning variable; the general overload builds a
// (k+2) matrix and uses N - 2 - (k + 2)
PBN_HD int64_t test_df(int64_t rows, int k) { return k == 0 ? rows - 2 : (k == 1 ? rows - 3 : rows - 2 - (k + 2)); }

#undef PBN_HD

// the scalar host test (lincor.hip): cor_0cond / cyclic Jacobi + pseudo-inverse, then cor_pvalue
double lincor_pvalue(const pbn_lincor* h, int v1, int v2, int k, const int* cond);

}  // namespace lincor
}  // namespace pbn
