// Driver of FeatureClassic(Detector::Orb) (reconstructor_amd/host/HipFeatureClassic.h) for tests/test_orb_cpp.py.
//   orb_adapter_test IN OUT [capacity] [K] [pattern: 0 built-in, 1 the one in IN]
// IN  (binary): int32 n, H, W; uint8 images[n][H][W]; int8 pattern[1024]
// OUT (binary): per image of detect: int32 m, then per feature int32 x, y and its 32 floats; then detectBatch over all images with K:
//               int32 counts[n]; per image int32 emitted, int32 xy[emitted][2]; float rows[n][K][32] (read back from the device)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reconstructor_amd/host/HipFeatureClassic.h"

using namespace reconstructor::Core;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[3];
    if (std::fread(hdr, sizeof(int32_t), 3, f) != 3 || hdr[0] < 1 || hdr[0] > 64 || hdr[1] < 1 || hdr[2] < 1 || hdr[1] > 4096 || hdr[2] > 4096) return 2;
    const int n = hdr[0], H = hdr[1], W = hdr[2];
    const size_t px = (size_t)H * W;
    std::vector<uint8_t> images((size_t)n * px);
    std::vector<int8_t> pattern(1024);
    if (std::fread(images.data(), 1, images.size(), f) != images.size() || std::fread(pattern.data(), 1, 1024, f) != 1024) return 2;
    std::fclose(f);
    const int capacity = argc > 3 ? std::atoi(argv[3]) : 4096, K = argc > 4 ? std::atoi(argv[4]) : 64;
    const bool own = argc > 5 && std::atoi(argv[5]) != 0;
    int rc = 0;
    try {
        FeatureClassic det(FeatureClassic::Detector::Orb, nullptr, capacity);
        if (det.descriptorSize() != 32) return 4;
        if (own) det.setOrbPattern(pattern.data());
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        for (int i = 0; i < n; ++i) {
            GreyImage img;
            img.rows = H; img.cols = W;
            img.u8.assign(images.begin() + (size_t)i * px, images.begin() + (size_t)(i + 1) * px);
            std::vector<FeaturePtr<>> features;
            det.detect(det.prepImg(img), features);
            const int32_t m = (int32_t)features.size();
            std::fwrite(&m, sizeof(m), 1, o);
            for (const auto &p : features) {
                const int32_t xy[2] = {p->featCoord.x, p->featCoord.y};
                std::fwrite(xy, sizeof(int32_t), 2, o);
                if (p->featDesc.desc.size() != 32) rc = 4;
                std::fwrite(p->featDesc.desc.data(), sizeof(float), p->featDesc.desc.size(), o);
            }
        }
        const int runs = det.runs();
        uint8_t *dev = nullptr;
        float *rows = nullptr;
        const size_t nrows = (size_t)n * K * 32;
        if (hipMalloc((void **)&dev, images.size()) || hipMalloc((void **)&rows, nrows * sizeof(float)) ||
            hipMemcpy(dev, images.data(), images.size(), FeatureClassic::kMemcpyHostToDevice)) return 3;
        std::vector<std::vector<FeatCoord<>>> coords;
        std::vector<int> counts;
        det.detectBatch(dev, n, H, W, K, rows, coords, counts);
        for (int i = 0; i < n; ++i) { const int32_t c = counts[(size_t)i]; std::fwrite(&c, sizeof(c), 1, o); }
        for (int i = 0; i < n; ++i) {
            const int32_t m = (int32_t)coords[(size_t)i].size();
            std::fwrite(&m, sizeof(m), 1, o);
            for (const auto &c : coords[(size_t)i]) { const int32_t xy[2] = {c.x, c.y}; std::fwrite(xy, sizeof(int32_t), 2, o); }
        }
        std::vector<float> host(nrows);
        if (hipMemcpy(host.data(), rows, nrows * sizeof(float), FeatureClassic::kMemcpyDeviceToHost)) return 3;
        std::fwrite(host.data(), sizeof(float), host.size(), o);
        (void)hipFree(dev);
        (void)hipFree(rows);
        std::fclose(o);
        std::printf("images %d runs %d\n", n, runs);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    return rc;
}
