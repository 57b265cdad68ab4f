// GuidedMatcher::matchFeatures (reconstructor_amd/host/HipGuidedMatcher.h) on features with coordinates, for tests/test_guided_cpp.py.
//   guided_adapter_test in.bin out.bin
// in.bin: int32 K1, K2, D, cross_check; 9 doubles F; K1 x D and K2 x D floats; K1 x 2 and K2 x 2 int32 coordinates.
// out.bin: K1 int32, the train row of every query row or -1 (the map in dense form).
#include <cstdio>
#include <cstdlib>

#include "../../reconstructor_amd/host/HipGuidedMatcher.h"

using namespace reconstructor::Core;

static std::vector<FeaturePtr<>> features(const float *rows, const int32_t *xy, int K, int D)
{
    std::vector<FeaturePtr<>> f;
    for (int i = 0; i < K; ++i)
        f.push_back(std::make_shared<Feature<>>(FeatCoord<>(xy[2 * i], xy[2 * i + 1]), FeatDesc(rows + (size_t)i * D, rows + (size_t)(i + 1) * D)));
    return f;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t h[4];
    double F[9];
    if (std::fread(h, 4, 4, in) != 4 || h[0] < 0 || h[1] < 0 || h[2] <= 0 || std::fread(F, 8, 9, in) != 9) return 2;
    const int K1 = h[0], K2 = h[1], D = h[2];
    std::vector<float> q((size_t)K1 * D), t((size_t)K2 * D);
    std::vector<int32_t> xy1(2 * (size_t)K1), xy2(2 * (size_t)K2);
    if (std::fread(q.data(), 4, q.size(), in) != q.size() || std::fread(t.data(), 4, t.size(), in) != t.size() ||
        std::fread(xy1.data(), 4, xy1.size(), in) != xy1.size() || std::fread(xy2.data(), 4, xy2.size(), in) != xy2.size()) return 2;
    std::fclose(in);
    const std::vector<FeaturePtr<>> f1 = features(q.data(), xy1.data(), K1, D), f2 = features(t.data(), xy2.data(), K2, D);
    GuidedMatcher m(0);
    m.options.cross_check = h[3];
    std::map<int, int> matches;
    m.matchFeatures(f1, f2, F, matches);
    std::vector<int32_t> out((size_t)K1, -1);
    for (const auto &kv : matches) out[(size_t)kv.first] = kv.second;
    FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) return 2;
    std::fclose(o);
    bool threw = false;
    m.options.max_error_px = -1.f;                             // the library's refusal arrives as an exception
    try {
        std::map<int, int> none;
        m.matchFeatures(f1, f2, F, none);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    std::printf("matches %zu threw %d\n", matches.size(), threw ? 1 : 0);
    return 0;
}
