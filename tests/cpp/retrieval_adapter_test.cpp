// retrieval_adapter_test <in.bin> <out.bin> <topK> <nCentroids> <iterations>
// in.bin: int32 n, K, D, first id, id step; int32 counts[n]; float rows [n][K][D].  Image slot s gets id first + s * step and is
// inserted into `features` in descending order of id.  Runs HipImageMatcher::match, then matchDevice on the packed block.
// out.bin: per image in ascending id: int32 id, int32 m, int32 partners[m]; then int32 P and the P pairs of matchDevice.
#include <cstdio>
#include <cstdlib>
#include <fstream>

#include "../../reconstructor_amd/host/HipImageMatcher.h"

using namespace reconstructor::Core;

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int32_t hdr[5];
    in.read((char *)hdr, sizeof hdr);
    const int n = hdr[0], K = hdr[1], D = hdr[2], first = hdr[3], step = hdr[4];
    std::vector<int32_t> counts((size_t)n);
    std::vector<float> rows((size_t)n * K * D);
    in.read((char *)counts.data(), (std::streamsize)(counts.size() * 4));
    in.read((char *)rows.data(), (std::streamsize)(rows.size() * 4));
    if (!in) return 3;
    std::unordered_map<int, std::vector<FeaturePtr<>>> features;
    std::unordered_map<int, std::filesystem::path> paths;
    for (int s = n - 1; s >= 0; --s) {
        std::vector<FeaturePtr<>> f;
        for (int r = 0; r < counts[(size_t)s]; ++r) {
            const float *p = rows.data() + ((size_t)s * K + r) * D;
            f.push_back(std::make_shared<Feature<>>(FeatCoord<>(r, s), FeatDesc(p, p + D)));
        }
        features[first + s * step] = f;
        paths[first + s * step] = "image" + std::to_string(s) + ".png";
    }
    try {
        rcn_ctx *ctx = nullptr;
        if (rcn_create(0, &ctx) != RCN_OK) return 4;
        std::ofstream out(argv[2], std::ios::binary);
        {
            HipImageMatcher matcher(ctx, std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
            ImageMatcher &plugin = matcher;
            std::unordered_map<int, std::vector<int>> imgMatches;
            plugin.match(paths, features, imgMatches);
            if ((int)imgMatches.size() != n) return 5;
            for (int s = 0; s < n; ++s) {
                const std::vector<int> &m = imgMatches.at(first + s * step);
                const int32_t head[2] = {first + s * step, (int32_t)m.size()};
                out.write((const char *)head, sizeof head);
                out.write((const char *)m.data(), (std::streamsize)(m.size() * 4));
            }
            float *dev = nullptr;
            if (hipMalloc((void **)&dev, rows.size() * 4) || hipMemcpy(dev, rows.data(), rows.size() * 4, HipImageMatcher::kMemcpyHostToDevice)) return 6;
            int32_t *cdev = nullptr;
            if (hipMalloc((void **)&cdev, counts.size() * 4) || hipMemcpy(cdev, counts.data(), counts.size() * 4, HipImageMatcher::kMemcpyHostToDevice)) return 6;
            const std::vector<int32_t> pairs = matcher.matchDevice(dev, cdev, n, K, D, first);
            (void)hipFree(dev);
            (void)hipFree(cdev);
            const int32_t P = (int32_t)(pairs.size() / 2);
            out.write((const char *)&P, 4);
            out.write((const char *)pairs.data(), (std::streamsize)(pairs.size() * 4));
        }
        rcn_destroy(ctx);
        std::printf("images %d\n", n);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
