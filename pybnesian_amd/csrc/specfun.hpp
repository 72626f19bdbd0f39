// Special functions shared by the host side of the independence tests (mi.hip, chisq.hip: chi-square p-values; rcot.hip: the gamma
// tails of the weighted chi-square sums).
#pragma once
#include <cmath>
#include <limits>

namespace pbn {

// ---- regularised upper incomplete gamma Q(a, x): chi-square survival function (boost chi_squared complement) --------
inline double gamma_q(double a, double x) {
    if (std::isnan(x) || std::isnan(a)) return std::numeric_limits<double>::quiet_NaN();
    if (x <= 0) return 1.0;
    if (std::isinf(x)) return 0.0;
    const double lg = std::lgamma(a);
    if (x < a + 1.0) {  // series for P, Q = 1 - P
        double ap = a, sum = 1.0 / a, del = sum;
        for (int n = 0; n < 100000; ++n) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (std::fabs(del) < std::fabs(sum) * 1e-17) break;
        }
        return 1.0 - sum * std::exp(-x + a * std::log(x) - lg);
    }
    // Lentz continued fraction for Q
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int i = 1; i < 100000; ++i) {
        const double an = -i * (i - a);
        b += 2.0;
        d = an * d + b; if (std::fabs(d) < tiny) d = tiny;
        c = b + an / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 1e-16) break;
    }
    const double q = std::exp(-x + a * std::log(x) - lg) * h;
    return q < std::numeric_limits<double>::min() ? 0.0 : q;
}

}  // namespace pbn
