// HipHammingMatcher::matchFeatures (reconstructor_amd/host/HipFeatureMatcher.h) on rows of 32 floats, for tests/test_hamming_cpp.py.
//   hamming_adapter_test in.bin out.bin
// in.bin: int32 K1, K2, then K1 x 32 and K2 x 32 floats.  out.bin: K1 int32, the train row of every query row or -1 (the map in dense
// form).  Then the same call with 0.5 written into one value of a train row: it must throw std::invalid_argument, and stdout says so.
#include <cstdio>
#include <cstdlib>

#include "../../reconstructor_amd/host/HipFeatureMatcher.h"

using namespace reconstructor::Core;

static std::vector<FeaturePtr<>> features(const float *rows, int K)
{
    std::vector<FeaturePtr<>> f;
    for (int i = 0; i < K; ++i) f.push_back(std::make_shared<Feature<>>(FeatCoord<>(i, i), FeatDesc(rows + (size_t)i * 32, rows + (size_t)(i + 1) * 32)));
    return f;
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t K[2];
    if (std::fread(K, 4, 2, in) != 2 || K[0] < 0 || K[1] < 0) return 2;
    std::vector<float> q((size_t)K[0] * 32), t((size_t)K[1] * 32);
    if (std::fread(q.data(), 4, q.size(), in) != q.size() || std::fread(t.data(), 4, t.size(), in) != t.size()) return 2;
    std::fclose(in);
    std::vector<FeaturePtr<>> f1 = features(q.data(), K[0]), f2 = features(t.data(), K[1]);
    HipHammingMatcher m(0);
    FeatureMatcher &base = m;                                  // through the reference's interface
    std::map<int, int> matches;
    base.matchFeatures(f1, f2, matches, {0, 0}, {0, 0});
    std::vector<int32_t> out((size_t)K[0], -1);
    for (const auto &kv : matches) out[(size_t)kv.first] = kv.second;
    FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), 4, out.size(), o) != out.size()) return 2;
    std::fclose(o);
    bool threw = false;
    if (K[1] > 0) {
        f2[(size_t)K[1] / 2]->featDesc.desc[9] = 0.5f;
        std::map<int, int> none;
        try {
            base.matchFeatures(f1, f2, none, {0, 0}, {0, 0});
        } catch (const std::invalid_argument &) {
            threw = none.empty();
        }
    }
    std::printf("matches %zu threw %d\n", matches.size(), threw ? 1 : 0);
    return 0;
}
