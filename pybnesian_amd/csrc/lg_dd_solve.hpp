// Double-double arithmetic and the host solve of the ill-conditioned LinearGaussianCPD refit (lg_accurate.hip): from the RAW
// moments sum x_i, sum x_i x_j of [y, x1..xp] in double-double to beta, the unbiased variance and the rank.  Host code only,
// no HIP runtime: lg_accurate.hip includes it with PBN_DD_FN = __host__ __device__ inline (its Gram kernel accumulates with
// the same two_sum / two_prod / dd_add), tests/c/lg_dd_check.cpp includes it as plain C++.
//
// Centring.  C = (N G - S S^T) / N with the cancellation done exactly (dd_centred_times_n): G - S mu in double-double
// would add a few 2^-104 of the RAW moment to every entry, (mean / sigma)^2 times that of the centred one.
//
// Rank decision.  What exact centring cannot remove is the roundoff the raw moments arrive with: once the data carry more
// than about (104 - log2 n) / 2 bits the row sums round, an entry of G is good to a few 2^-104 of ITSELF, after centring
// that is a few 2^-104 (1 + (mean / sigma)^2) of the centred entry, and the eliminations of the pivoted Cholesky carry the
// noise of every column taken into the remaining diagonal.  A pivot is therefore taken as zero (dependent column,
// coefficient 0) when
//     pivot <= (eps min(n, d))^2 * first pivot                the square of ColPivHouseholderQR's default threshold, or
//     pivot <= 64 * 2^-104 * max(G_ii, C_ii * max_j G_jj / C_jj)   it does not rise above the centring noise
// (j over the parents that are not constant to roundoff, C_jj > 64 * 2^-104 G_jj; 64: a few units in the last place of each
// of up to 15 eliminations).  The first rule alone, about 1e-30 of the first pivot, is below the noise as soon as a column's
// mean is some 50 sigma away from zero: an exactly dependent parent then kept a pivot of pure noise and coefficients that
// nothing bounds.  A column the second rule drops has kappa^2 (1 + (mean / sigma)^2) >~ 2^98: no digit of its coefficient
// could have been right.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <numeric>
#include <utility>
#include <vector>

#ifndef PBN_DD_FN
#define PBN_DD_FN inline
#endif

// The error-free transformations below (TwoSum, TwoProd) are exact only if every operation is rounded exactly as
// written: hipcc's default for device code, -ffp-contract=fast, would fuse the product of TwoProd into the first addition of
// the following TwoSum (s = fma(x, y, acc) instead of acc + round(x y)) and silently turn the double-double accumulation
// back into plain double.
#pragma STDC FP_CONTRACT OFF

namespace pbn {
namespace score {

namespace {

struct dd {
    double hi, lo;
};
PBN_DD_FN dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
PBN_DD_FN dd quick_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}
PBN_DD_FN dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, __builtin_fma(a, b, -p)};
}
PBN_DD_FN dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = quick_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return quick_two_sum(s.hi, s.lo);
}
PBN_DD_FN dd dd_add_prod(dd acc, double a, double b) { return dd_add(acc, two_prod(a, b)); }
inline dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
inline dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
inline dd dd_mul(dd a, dd b) {
    dd p = two_prod(a.hi, b.hi);
    p.lo += a.hi * b.lo + a.lo * b.hi;
    return quick_two_sum(p.hi, p.lo);
}
inline dd dd_div(dd a, dd b) {
    const double q1 = a.hi / b.hi;
    dd r = dd_sub(a, dd_mul(b, {q1, 0.0}));
    const double q2 = r.hi / b.hi;
    r = dd_sub(r, dd_mul(b, {q2, 0.0}));
    const double q3 = r.hi / b.hi;
    dd q = quick_two_sum(q1, q2);
    return dd_add(q, {q3, 0.0});
}
inline dd dd_sqrt(dd a) {
    if (!(a.hi > 0.0)) return {0.0, 0.0};
    const double x = 1.0 / std::sqrt(a.hi), ax = a.hi * x;
    const dd diff = dd_sub(a, two_prod(ax, ax));
    return dd_add({ax, 0.0}, {diff.hi * (x * 0.5), 0.0});
}

// N g - s_i s_j, every bit of it: the twelve error-free partial products are added into a nonoverlapping expansion (Shewchuk's
// grow-expansion: TwoSum down the components, nothing is rounded away), which is then summed smallest first.  The cancellation of the
// centring - a factor 1 + (mean / sigma)^2 - happens exactly; only the final sum rounds, relative to the CENTRED value.
inline dd dd_centred_times_n(double N, dd g, dd si, dd sj) {
    const dd t[6] = {two_prod(N, g.hi),        two_prod(N, g.lo),        two_prod(-si.hi, sj.hi),
                     two_prod(-si.hi, sj.lo),  two_prod(-si.lo, sj.hi),  two_prod(-si.lo, sj.lo)};
    double e[12];
    int m = 0;
    for (const dd& term : t)
        for (const double b : {term.lo, term.hi}) {
            double q = b;
            for (int k = 0; k < m; ++k) {
                const dd s = two_sum(q, e[k]);
                e[k] = s.lo;
                q = s.hi;
            }
            e[m++] = q;
        }
    dd acc = {0.0, 0.0};
    for (int k = 0; k < m; ++k) acc = dd_add(acc, {e[k], 0.0});
    return acc;
}

constexpr double DD_NOISE = 64.0 * 4.930380657631324e-32;   // 64 * 2^-104

// S (d), G (d x d, column-major, symmetric): raw moments of [y, x1..xp] over n rows.  beta: d (intercept first); returns the
// unbiased variance RSS / (n - p - 1) (inf when n <= p + 1); *rank (nullable): the number of parents kept.
inline double lg_dd_solve(int64_t n, int d, const dd* S, const dd* G, double* beta, int* rank_out) {
    const int p = d - 1;
    // centred SSE and means
    const dd N = {(double)n, 0.0};
    std::vector<dd> C((size_t)d * d), mu(d);
    for (int i = 0; i < d; ++i) mu[i] = dd_div(S[i], N);
    for (int j = 0; j < d; ++j)
        for (int i = 0; i <= j; ++i)   // (N G - S S) / N with the cancellation done exactly: G - S mu in double-double loses (mean / sigma)^2
            C[i + (size_t)j * d] = C[j + (size_t)i * d] = dd_div(dd_centred_times_n((double)n, G[i + (size_t)j * d], S[i], S[j]), N);
    // diagonally pivoted Cholesky of the parents' block (indices 1..p), rank by the squared QR threshold and the centring noise
    std::vector<int> piv(p);
    std::iota(piv.begin(), piv.end(), 0);
    std::vector<dd> L((size_t)p * p, dd{0, 0}), diag(p);
    std::vector<double> floor_(p);
    double offset = 1.0;   // largest raw / centred second moment among the parents that are not constant to roundoff
    for (int i = 0; i < p; ++i) {
        diag[i] = C[(i + 1) + (size_t)(i + 1) * d];
        const double g = G[(i + 1) + (size_t)(i + 1) * d].hi;
        if (diag[i].hi > DD_NOISE * g) offset = std::max(offset, g / diag[i].hi);
    }
    for (int i = 0; i < p; ++i) floor_[i] = DD_NOISE * std::max(G[(i + 1) + (size_t)(i + 1) * d].hi, diag[i].hi * offset);
    const double thr = std::pow(2.220446049250313e-16 * (double)std::min<int64_t>(n, d), 2.0);
    int rank = 0;
    double first = 0.0;
    for (int k = 0; k < p; ++k) {
        int best = k;
        for (int j = k + 1; j < p; ++j)
            if (diag[piv[j]].hi > diag[piv[best]].hi) best = j;
        std::swap(piv[k], piv[best]);
        // rows of L follow the pivot order: swap the already computed parts
        for (int c2 = 0; c2 < k; ++c2) std::swap(L[k + (size_t)c2 * p], L[best + (size_t)c2 * p]);
        const dd pk = diag[piv[k]];
        if (k == 0) first = pk.hi;
        if (!(pk.hi > thr * first) || !(pk.hi > floor_[piv[k]]) || !std::isfinite(pk.hi)) break;
        const dd lkk = dd_sqrt(pk);
        L[k + (size_t)k * p] = lkk;
        for (int i = k + 1; i < p; ++i) {
            dd v = C[(piv[i] + 1) + (size_t)(piv[k] + 1) * d];
            for (int c2 = 0; c2 < k; ++c2) v = dd_sub(v, dd_mul(L[i + (size_t)c2 * p], L[k + (size_t)c2 * p]));
            v = dd_div(v, lkk);
            L[i + (size_t)k * p] = v;
            diag[piv[i]] = dd_sub(diag[piv[i]], dd_mul(v, v));
        }
        rank = k + 1;
    }
    // forward / backward solves on the leading `rank` pivots; RSS = C_yy - |w|^2
    std::vector<dd> w(rank), z(rank);
    dd rss = C[0];
    for (int i = 0; i < rank; ++i) {
        dd v = C[0 + (size_t)(piv[i] + 1) * d];
        for (int c2 = 0; c2 < i; ++c2) v = dd_sub(v, dd_mul(L[i + (size_t)c2 * p], w[c2]));
        w[i] = dd_div(v, L[i + (size_t)i * p]);
        rss = dd_sub(rss, dd_mul(w[i], w[i]));
    }
    for (int i = rank - 1; i >= 0; --i) {
        dd v = w[i];
        for (int c2 = i + 1; c2 < rank; ++c2) v = dd_sub(v, dd_mul(L[c2 + (size_t)i * p], z[c2]));
        z[i] = dd_div(v, L[i + (size_t)i * p]);
    }
    std::vector<dd> b(p, dd{0, 0});
    for (int i = 0; i < rank; ++i) b[piv[i]] = z[i];
    dd b0 = mu[0];
    for (int j = 0; j < p; ++j) b0 = dd_sub(b0, dd_mul(b[j], mu[j + 1]));
    beta[0] = b0.hi;
    for (int j = 0; j < p; ++j) beta[j + 1] = b[j].hi;
    if (rank_out) *rank_out = rank;
    if (n <= p + 1) return std::numeric_limits<double>::infinity();
    return std::max(rss.hi, 0.0) / ((double)n - p - 1);
}

}  // namespace
}  // namespace score
}  // namespace pbn
