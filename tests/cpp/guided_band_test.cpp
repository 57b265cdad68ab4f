// guided_band_test -- csrc/guided_band.h as plain host C++ (no HIP, no GPU): reads cases from the file named on the command line and prints
// the band of each as rows of '0' / '1', for tests/test_guided_band.py to compare with numpy bit for bit.  Built with -ffp-contract=off and
// the address and undefined-behaviour sanitizers.
//
// File: any number of cases, each
//     K1 K2
//     thr2 and the 9 entries of F as hexadecimal floating-point literals (exact)
//     K1 lines "x y", then K2 lines "x y" (integers)
// Output per case: "case K1 K2", then K1 lines of K2 characters, once through gb_candidate and once through the per-point form the
// kernel uses (gb_line per point, gb_test per combination); the program fails if the two differ or if the transposed predicate differs.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../reconstructor_amd/csrc/guided_band.h"

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: guided_band_test CASES\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int K1, K2, n_cases = 0;
    while (std::fscanf(f, "%d %d", &K1, &K2) == 2) {
        if (K1 < 0 || K2 < 0) return 2;
        char word[64];
        double v[10];
        for (int k = 0; k < 10; ++k) {
            if (std::fscanf(f, "%63s", word) != 1) return 2;
            v[k] = std::strtod(word, nullptr);
        }
        const double thr2 = v[0], *F = v + 1;
        const double Ft[9] = {F[0], F[3], F[6], F[1], F[4], F[7], F[2], F[5], F[8]};
        std::vector<double> p1(2 * (size_t)K1), p2(2 * (size_t)K2);
        for (double &c : p1) { int i; if (std::fscanf(f, "%d", &i) != 1) return 2; c = i; }
        for (double &c : p2) { int i; if (std::fscanf(f, "%d", &i) != 1) return 2; c = i; }
        std::vector<GbLine> l1((size_t)K1), l2((size_t)K2);
        for (int q = 0; q < K1; ++q) l1[q] = gb_line(F, 0, p1[2 * q], p1[2 * q + 1], thr2);
        for (int t = 0; t < K2; ++t) l2[t] = gb_line(F, 1, p2[2 * t], p2[2 * t + 1], thr2);
        std::printf("case %d %d\n", K1, K2);
        std::string row((size_t)K2, '0');
        for (int q = 0; q < K1; ++q) {
            for (int t = 0; t < K2; ++t) {
                const bool c = gb_candidate(F, p1[2 * q], p1[2 * q + 1], p2[2 * t], p2[2 * t + 1], thr2);
                const bool k = gb_test(l1[q], p1[2 * q], p1[2 * q + 1], l2[t], p2[2 * t], p2[2 * t + 1]);
                const bool r = gb_candidate(Ft, p2[2 * t], p2[2 * t + 1], p1[2 * q], p1[2 * q + 1], thr2);
                if (c != k || c != r) { std::fprintf(stderr, "forms differ at case %d (%d, %d): %d %d %d\n", n_cases, q, t, c, k, r); return 1; }
                row[(size_t)t] = c ? '1' : '0';
            }
            std::printf("%s\n", row.c_str());
        }
        ++n_cases;
    }
    std::fclose(f);
    std::printf("%d cases done\n", n_cases);
    return 0;
}
