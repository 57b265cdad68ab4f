// Driver of reconstructor_amd/host/HipFeatureSuperPoint.h for tests/test_keypoints_cpp.py.
//   keypoint_adapter_test IN OUT [capacity]
// IN  (binary): int32 H, W; float logits[65][H/8][W/8]; float descriptors[256][H/8][W/8]
// OUT (binary): int32 m; then per keypoint of processKeypoints int32 x, y and float conf; int32 m2; then per feature of
//               detectPost int32 x, y, float conf and its 256 floats
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reconstructor_amd/host/HipFeatureSuperPoint.h"

using namespace reconstructor::Core;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hw[2];
    if (std::fread(hw, sizeof(int32_t), 2, f) != 2) return 2;
    const int H = hw[0], W = hw[1], Hc = H / 8, Wc = W / 8;
    std::vector<float> logits((size_t)65 * Hc * Wc), desc((size_t)256 * Hc * Wc);
    if (std::fread(logits.data(), sizeof(float), logits.size(), f) != logits.size()) return 2;
    if (std::fread(desc.data(), sizeof(float), desc.size(), f) != desc.size()) return 2;
    std::fclose(f);
    float *dl = nullptr, *dd = nullptr;
    if (hipMalloc((void **)&dl, logits.size() * sizeof(float)) || hipMalloc((void **)&dd, desc.size() * sizeof(float))) return 3;
    if (hipMemcpy(dl, logits.data(), logits.size() * sizeof(float), FeatureSuperPointPost::kMemcpyHostToDevice) ||
        hipMemcpy(dd, desc.data(), desc.size() * sizeof(float), FeatureSuperPointPost::kMemcpyHostToDevice)) return 3;
    int rc = 0;
    try {
        FeatureSuperPointPost post(nullptr, RCN_KP_HEAT_REFERENCE, 4, argc > 3 ? std::atoi(argv[3]) : 2048);
        const auto kps = post.processKeypoints(dl, (int64_t)Hc * Wc, Wc, 1, H, W, 0.015, 4);     // CONF_THRESH, BORDER_SIZE
        std::vector<FeaturePtr<>> features;
        post.detectPost(dl, (int64_t)Hc * Wc, Wc, 1, dd, (int64_t)Hc * Wc, Wc, 1, H, W, 0.015, 4, features);
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        int32_t m = (int32_t)kps.size();
        std::fwrite(&m, sizeof(m), 1, o);
        for (const auto &k : kps) {
            const int32_t xy[2] = {k.x, k.y};
            const float c = (float)k.conf;
            std::fwrite(xy, sizeof(int32_t), 2, o);
            std::fwrite(&c, sizeof(float), 1, o);
        }
        m = (int32_t)features.size();
        std::fwrite(&m, sizeof(m), 1, o);
        for (const auto &p : features) {
            const auto *fc = static_cast<const FeatureConf<> *>(p.get());
            const int32_t xy[2] = {fc->featCoord.x, fc->featCoord.y};
            const float c = (float)fc->conf;
            std::fwrite(xy, sizeof(int32_t), 2, o);
            std::fwrite(&c, sizeof(float), 1, o);
            if (fc->featDesc.desc.size() != 256) rc = 4;
            std::fwrite(fc->featDesc.desc.data(), sizeof(float), fc->featDesc.desc.size(), o);
        }
        std::fclose(o);
        std::printf("keypoints %d features %d rounds %d\n", (int)kps.size(), (int)features.size(), post.lastRounds());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    (void)hipFree(dl);
    (void)hipFree(dd);
    return rc;
}
