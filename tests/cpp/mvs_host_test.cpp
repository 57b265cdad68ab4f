// mvs_host_test.cpp -- csrc/mvs_geom.h evaluated by plain host C++ (tests/test_mvs_host.py builds this with g++, -ffp-contract=off and the
// address and undefined-behaviour sanitizers): the bodies of rcn_mvs_inv_depths and rcn_mvs_homographies and every other function of the
// header, on cases read from a file, results printed as hexadecimal doubles for a bit-for-bit comparison with tests/mvs_ref.py.
//
//   inv near far D                                  -> D doubles (or "bad")
//   hom nc ref S D | poses 12 nc | intr 6 nc | srcs S | inv D   -> S D 9 doubles (or "bad")
//   warp rows cols | H 9                            -> rows cols entries "qu qv" or "-"
//   sample rows cols qu qv | bytes                  -> the blend
//   cost n Sa Va Sb Sbb Sab                         -> the cost or "-"
//   refine cm c0 cp have_m have_p im i0 ip          -> the refined inverse depth
//   lift P 12 | K 4 | x y z                         -> 3 doubles
//   proj P 12 | K 4 | X 3                           -> u v z
//   dist K 6 | x y                                  -> u v
#include "../../reconstructor_amd/csrc/mvs_geom.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static FILE *g_in;

static bool word(std::string &w)
{
    char buf[128];
    if (std::fscanf(g_in, "%127s", buf) != 1) return false;
    w = buf;
    return true;
}

static double num()
{
    std::string w;
    if (!word(w)) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    return std::strtod(w.c_str(), nullptr);
}

static long long integer()
{
    std::string w;
    if (!word(w)) { std::fprintf(stderr, "short file\n"); std::exit(2); }
    return std::strtoll(w.c_str(), nullptr, 10);
}

static std::vector<double> nums(size_t n)
{
    std::vector<double> v(n);
    for (double &x : v) x = num();
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2 || !(g_in = std::fopen(argv[1], "r"))) { std::fprintf(stderr, "usage: mvs_host_test cases.txt\n"); return 2; }
    std::string cmd;
    int done = 0;
    while (word(cmd)) {
        if (cmd == "inv") {
            const double near_z = num(), far_z = num();
            const int D = (int)integer();
            std::vector<double> out((size_t)(D > 0 && D <= 4096 ? D : 1));
            if (!mg_inv_depths(near_z, far_z, D, 1024, out.data())) std::printf("bad\n");
            else { for (int k = 0; k < D; ++k) std::printf("%a ", out[(size_t)k]); std::printf("\n"); }
        } else if (cmd == "hom") {
            const int nc = (int)integer(), ref = (int)integer(), S = (int)integer(), D = (int)integer();
            const std::vector<double> P = nums(12 * (size_t)nc), K = nums(6 * (size_t)nc);
            std::vector<int32_t> srcs((size_t)S);
            for (int32_t &s : srcs) s = (int32_t)integer();
            const std::vector<double> inv = nums((size_t)D);
            std::vector<double> H((size_t)S * D * 9 + 1);
            if (!mg_homographies(P.data(), K.data(), ref, srcs.data(), S, inv.data(), D, 16, 1024, H.data())) std::printf("bad\n");
            else { for (size_t i = 0; i + 1 < H.size(); ++i) std::printf("%a ", H[i]); std::printf("\n"); }
        } else if (cmd == "warp") {
            const int rows = (int)integer(), cols = (int)integer();
            const std::vector<double> H = nums(9);
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < cols; ++x) {
                    int qu, qv;
                    if (mg_warp(H.data(), x, y, rows, cols, &qu, &qv)) std::printf("%d %d ", qu, qv);
                    else std::printf("- - ");
                }
            std::printf("\n");
        } else if (cmd == "sample") {
            const int rows = (int)integer(), cols = (int)integer(), qu = (int)integer(), qv = (int)integer();
            std::vector<uint8_t> img((size_t)rows * cols);
            for (uint8_t &b : img) b = (uint8_t)integer();
            std::printf("%d\n", mg_sample(img.data(), cols, 1, rows, cols, qu, qv));
        } else if (cmd == "cost") {
            const int n = (int)integer();
            const long long Sa = integer(), Va = integer(), Sb = integer(), Sbb = integer(), Sab = integer();
            double c;
            if (mg_cost(n, Sa, Va, Sb, Sbb, Sab, &c)) std::printf("%a\n", c);
            else std::printf("-\n");
        } else if (cmd == "refine") {
            const double cm = num(), c0 = num(), cp = num();
            const bool hm = integer() != 0, hp = integer() != 0;
            const double im = num(), i0 = num(), ip = num();
            std::printf("%a\n", mg_refine(cm, c0, cp, hm, hp, im, i0, ip));
        } else if (cmd == "lift") {
            const std::vector<double> P = nums(12), K = nums(4);
            const int x = (int)integer(), y = (int)integer();
            const double z = num();
            double X[3];
            mg_lift(P.data(), K.data(), x, y, z, X);
            std::printf("%a %a %a\n", X[0], X[1], X[2]);
        } else if (cmd == "proj") {
            const std::vector<double> P = nums(12), K = nums(4), X = nums(3);
            double u, v, z;
            mg_project(P.data(), K.data(), X.data(), &u, &v, &z);
            std::printf("%a %a %a\n", u, v, z);
        } else if (cmd == "dist") {
            const std::vector<double> K = nums(6);
            const int x = (int)integer(), y = (int)integer();
            double u, v;
            mg_distort(K.data(), x, y, &u, &v);
            std::printf("%a %a\n", u, v);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
        ++done;
    }
    std::fclose(g_in);
    std::printf("%d cases done\n", done);
    return 0;
}
