// Driver of FeatureSuperPointNet (reconstructor_amd/host/HipFeatureSuperPoint.h) for tests/test_superpoint_net_cpp.py.
//   superpoint_net_adapter_test IN OUT [capacity]
// IN  (binary): int32 H, W; int64 n_params; float params[n_params]; float image[H][W]; uint8 bytes[256]
// OUT (binary): int32 m; then per feature of detect int32 x, y, float conf and its 256 floats; float prepared[256] = prepImg(bytes)
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
    int64_t np = 0;
    if (std::fread(hw, sizeof(int32_t), 2, f) != 2 || std::fread(&np, sizeof(np), 1, f) != 1 || np < 0 || np > (1 << 24)) return 2;
    const int H = hw[0], W = hw[1];
    std::vector<float> params((size_t)np), img((size_t)H * W);
    std::vector<uint8_t> bytes(256);
    if (std::fread(params.data(), sizeof(float), params.size(), f) != params.size()) return 2;
    if (std::fread(img.data(), sizeof(float), img.size(), f) != img.size()) return 2;
    if (std::fread(bytes.data(), 1, bytes.size(), f) != bytes.size()) return 2;
    std::fclose(f);
    int rc = 0;
    try {
        FeatureSuperPointNet net(params.data(), np, nullptr, RCN_KP_HEAT_REFERENCE, 4, argc > 3 ? std::atoi(argv[3]) : 2048);
        std::vector<FeaturePtr<>> features;
        net.detect(img.data(), H, W, features);
        const std::vector<float> prepared = FeatureSuperPointNet::prepImg(bytes.data(), 16, 16);
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        const int32_t m = (int32_t)features.size();
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
        std::fwrite(prepared.data(), sizeof(float), prepared.size(), o);
        std::fclose(o);
        std::printf("features %d runs %d rounds %d\n", (int)features.size(), net.runs(), net.lastRounds());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    return rc;
}
