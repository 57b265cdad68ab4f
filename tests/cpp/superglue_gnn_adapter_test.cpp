// Driver of FeatureMatcherSuperglueNet (reconstructor_amd/host/HipSuperGlueMatcher.h) for tests/test_superglue_gnn_cpp.py.
//   superglue_gnn_adapter_test IN OUT
// IN  (binary): int32 L, m, n, H1, W1, H2, W2; double bin_score; int32 layer_types[L]; int64 n_params; float params[n_params];
//               then per image: float xy[k][2] (pixels, integral), float conf[k], float desc[k][256]
// OUT (binary): int32 k; k x (int32 feature of image 1, feature of image 2): the std::map of matchFeatures in its own order;
//               then the batched form on two pairs -- the same pair, and its first m - 3 and n - 2 features --
//               int32 stride; int32 counts[2]; int32 table[2][stride]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reconstructor_amd/host/HipSuperGlueMatcher.h"

using namespace reconstructor::Core;

template <class T> static bool rd(FILE *f, T *p, size_t n) { return std::fread(p, sizeof(T), n, f) == n; }

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[7];
    double binScore;
    if (!rd(f, hdr, 7) || !rd(f, &binScore, 1)) return 2;
    const int L = hdr[0], m = hdr[1], n = hdr[2];
    std::vector<int32_t> types((size_t)L);
    int64_t nParams = 0;
    if (!rd(f, types.data(), types.size()) || !rd(f, &nParams, 1)) return 2;
    std::vector<float> params((size_t)nParams);
    if (!rd(f, params.data(), params.size())) return 2;
    std::vector<float> xy[2], conf[2], desc[2];
    std::vector<FeaturePtr<>> feats[2];
    for (int i = 0; i < 2; ++i) {
        const size_t k = i ? n : m;
        xy[i].resize(2 * k); conf[i].resize(k); desc[i].resize(256 * k);
        if (!rd(f, xy[i].data(), xy[i].size()) || !rd(f, conf[i].data(), k) || !rd(f, desc[i].data(), desc[i].size())) return 2;
        for (size_t j = 0; j < k; ++j)
            feats[i].push_back(std::make_shared<FeatureConf<>>(FeatCoordConf<>((int)xy[i][2 * j], (int)xy[i][2 * j + 1], (double)conf[i][j]),
                                                               FeatDesc(desc[i].begin() + 256 * j, desc[i].begin() + 256 * (j + 1))));
    }
    std::fclose(f);
    const int stride = m + 5;
    const size_t fl[2] = {(size_t)m * 259, (size_t)n * 259};
    float *in[2] = {nullptr, nullptr};
    int32_t *mn = nullptr, *shapes = nullptr, *table = nullptr, *counts = nullptr;
    if (hipMalloc((void **)&in[0], fl[0] * sizeof(float)) || hipMalloc((void **)&in[1], fl[1] * sizeof(float)) || hipMalloc((void **)&mn, 4 * sizeof(int32_t)) ||
        hipMalloc((void **)&shapes, 8 * sizeof(int32_t)) || hipMalloc((void **)&table, (size_t)2 * stride * sizeof(int32_t)) ||
        hipMalloc((void **)&counts, 2 * sizeof(int32_t))) return 3;
    const int H2D = 1, D2H = 2;      // hipMemcpyKind
    const int32_t mn_host[4] = {m, m - 3, n, n - 2}, sh_host[8] = {hdr[3], hdr[4], hdr[3], hdr[4], hdr[5], hdr[6], hdr[5], hdr[6]};
    for (int i = 0; i < 2; ++i) {
        const size_t k = i ? n : m;
        if (hipMemcpy(in[i], xy[i].data(), 2 * k * sizeof(float), H2D) || hipMemcpy(in[i] + 2 * k, conf[i].data(), k * sizeof(float), H2D) ||
            hipMemcpy(in[i] + 3 * k, desc[i].data(), 256 * k * sizeof(float), H2D)) return 3;
    }
    if (hipMemcpy(mn, mn_host, sizeof(mn_host), H2D) || hipMemcpy(shapes, sh_host, sizeof(sh_host), H2D)) return 3;
    int rc = 0;
    try {
        FeatureMatcherSuperglueNet matcher(types, params, binScore);
        std::map<int, int> matches;
        matcher.matchFeatures(feats[0], feats[1], matches, {hdr[3], hdr[4]}, {hdr[5], hdr[6]});
        // both pairs of the batch read the same arrays: pair stride 0 (the keypoints and confidences are [pairs][max] arrays, so
        // the second pair is given the same capacity and fewer features)
        std::vector<float> two;
        float *kp2[2] = {nullptr, nullptr};
        for (int i = 0; i < 2; ++i) {
            const size_t k = i ? n : m;
            if (hipMalloc((void **)&kp2[i], 2 * 3 * k * sizeof(float))) return 3;
            two.assign(2 * 3 * k, 0.f);
            for (int b = 0; b < 2; ++b) {
                std::copy(xy[i].begin(), xy[i].end(), two.begin() + b * 2 * k);
                std::copy(conf[i].begin(), conf[i].end(), two.begin() + 4 * k + b * k);
            }
            if (hipMemcpy(kp2[i], two.data(), two.size() * sizeof(float), H2D)) return 3;
        }
        matcher.matchFeaturesBatch(kp2[0], kp2[0] + 4 * (size_t)m, in[0] + 3 * (size_t)m, 0, 256, 1, kp2[1], kp2[1] + 4 * (size_t)n, in[1] + 3 * (size_t)n, 0, 256, 1,
                                   shapes, shapes + 4, mn, mn + 2, 2, m, n, table, stride, counts);
        if (rcn_synchronize(matcher.ctx()) != RCN_OK) throw std::runtime_error(rcn_last_error(matcher.ctx()));
        std::vector<int32_t> th((size_t)2 * stride), ch(2);
        if (hipMemcpy(th.data(), table, th.size() * sizeof(int32_t), D2H) || hipMemcpy(ch.data(), counts, 2 * sizeof(int32_t), D2H)) return 3;
        for (int i = 0; i < 2; ++i) (void)hipFree(kp2[i]);
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
    for (void *p : {(void *)in[0], (void *)in[1], (void *)mn, (void *)shapes, (void *)table, (void *)counts}) (void)hipFree(p);
    return rc;
}
