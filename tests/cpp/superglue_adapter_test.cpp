// Driver of reconstructor_amd/host/HipSuperGlueMatcher.h for tests/test_superglue_cpp.py.
//   superglue_adapter_test IN OUT
// IN  (binary): int32 m, n, D; float descs1[D][m]; float descs2[D][n]       (the network's [descSize][featuresNum] layout)
// OUT (binary): int32 k; k x (int32 feature of image 1, feature of image 2): the std::map of matchFeatures in its own order;
//               then the batched form on two pairs -- the same pair, and its first m - 3 and n - 2 features --
//               int32 stride; int32 counts[2]; int32 table[2][stride]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reconstructor_amd/host/HipSuperGlueMatcher.h"

using namespace reconstructor::Core;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3) return 2;
    const int m = hdr[0], n = hdr[1], D = hdr[2];
    std::vector<float> h1((size_t)D * m), h2((size_t)D * n);
    if (std::fread(h1.data(), sizeof(float), h1.size(), f) != h1.size()) return 2;
    if (std::fread(h2.data(), sizeof(float), h2.size(), f) != h2.size()) return 2;
    std::fclose(f);
    const int stride = m + 5;
    float *d1 = nullptr, *d2 = nullptr;
    int32_t *mn = nullptr, *table = nullptr, *counts = nullptr;
    if (hipMalloc((void **)&d1, h1.size() * sizeof(float)) || hipMalloc((void **)&d2, h2.size() * sizeof(float)) ||
        hipMalloc((void **)&mn, 4 * sizeof(int32_t)) || hipMalloc((void **)&table, (size_t)2 * stride * sizeof(int32_t)) ||
        hipMalloc((void **)&counts, 2 * sizeof(int32_t))) return 3;
    const int32_t mn_host[4] = {m, m - 3, n, n - 2};
    if (hipMemcpy(d1, h1.data(), h1.size() * sizeof(float), FeatureMatcherSuperglueAssign::kMemcpyHostToDevice) ||
        hipMemcpy(d2, h2.data(), h2.size() * sizeof(float), FeatureMatcherSuperglueAssign::kMemcpyHostToDevice) ||
        hipMemcpy(mn, mn_host, sizeof(mn_host), FeatureMatcherSuperglueAssign::kMemcpyHostToDevice)) return 3;
    int rc = 0;
    try {
        FeatureMatcherSuperglueAssign matcher;
        std::map<int, int> matches;
        matcher.matchFeatures(d1, m, 1, m, d2, n, 1, n, D, matches);
        // both pairs of the batch read the same descriptors: pair stride 0
        matcher.matchFeaturesBatch(d1, 0, 1, m, d2, 0, 1, n, mn, mn + 2, 2, m, n, D, table, stride, counts);
        if (rcn_synchronize(matcher.ctx()) != RCN_OK) throw std::runtime_error(rcn_last_error(matcher.ctx()));
        std::vector<int32_t> th((size_t)2 * stride), ch(2);
        if (hipMemcpy(th.data(), table, th.size() * sizeof(int32_t), FeatureMatcherSuperglueAssign::kMemcpyDeviceToHost) ||
            hipMemcpy(ch.data(), counts, 2 * sizeof(int32_t), FeatureMatcherSuperglueAssign::kMemcpyDeviceToHost)) return 3;
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        const int32_t k = (int32_t)matches.size();
        std::fwrite(&k, sizeof(k), 1, o);
        for (const auto &qt : matches) {
            const int32_t e[2] = {qt.first, qt.second};
            std::fwrite(e, sizeof(int32_t), 2, o);
        }
        const int32_t s = stride;
        std::fwrite(&s, sizeof(s), 1, o);
        std::fwrite(ch.data(), sizeof(int32_t), 2, o);
        std::fwrite(th.data(), sizeof(int32_t), th.size(), o);
        std::fclose(o);
        std::printf("matches %d batch %d %d status %d\n", (int)k, (int)ch[0], (int)ch[1], matcher.lastStatus());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    for (void *p : {(void *)d1, (void *)d2, (void *)mn, (void *)table, (void *)counts}) (void)hipFree(p);
    return rc;
}
