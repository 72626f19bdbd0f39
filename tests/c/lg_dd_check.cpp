// Host check of pybnesian_amd/csrc/lg_dd_solve.hpp: the double-double solve of the ill-conditioned LinearGaussianCPD refit, without a GPU.
// Reads cases from the file named on the command line - per case: int64 n, int64 d, then the table, n x d doubles, column-major, column 0
// the response - accumulates the raw moments sum x_i, sum x_i x_j row by row in double-double (what gram_dd_kernel does in another order),
// calls lg_dd_solve and prints one line per case: rank, variance, beta[0..d), as hexadecimal floats.  Built and run by
// tests/test_lg_accurate_cpu.py (hipcc, host code only), which compares with exact rational least squares (tests/lg_exact.py).
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../pybnesian_amd/csrc/lg_dd_solve.hpp"

using pbn::score::dd;

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: lg_dd_check CASES\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t head[2];
    while (std::fread(head, sizeof(int64_t), 2, f) == 2) {
        const int64_t n = head[0];
        const int d = (int)head[1];
        if (n < 1 || d < 1 || d > 16) { std::fprintf(stderr, "bad case header\n"); return 2; }
        std::vector<double> x((size_t)n * d);
        if (std::fread(x.data(), sizeof(double), x.size(), f) != x.size()) { std::fprintf(stderr, "short case\n"); return 2; }
        std::vector<dd> S(d, dd{0, 0}), G((size_t)d * d, dd{0, 0});
        for (int64_t r = 0; r < n; ++r)
            for (int j = 0; j < d; ++j) {
                const double xj = x[(size_t)j * n + r];
                S[j] = pbn::score::dd_add(S[j], {xj, 0.0});
                for (int i = 0; i <= j; ++i) G[i + (size_t)j * d] = pbn::score::dd_add_prod(G[i + (size_t)j * d], x[(size_t)i * n + r], xj);
            }
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < j; ++i) G[j + (size_t)i * d] = G[i + (size_t)j * d];
        std::vector<double> beta(d);
        int rank = -1;
        const double variance = pbn::score::lg_dd_solve(n, d, S.data(), G.data(), beta.data(), &rank);
        std::printf("%d %a", rank, variance);
        for (int j = 0; j < d; ++j) std::printf(" %a", beta[j]);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}
