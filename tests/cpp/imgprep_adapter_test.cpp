// Driver of reconstructor::Utils::ImagePrep (reconstructor_amd/host/HipImagePrep.h) and of the colours HipTriangulator.h gives
// its landmarks, for tests/test_imgprep_cpp.py.
//   imgprep_adapter_test IN OUT PLY_PLAIN PLY_FLAGS
// IN  (binary): int32 n, H, W, maxSize, K, L, C; uint8 images[n][H][W][3] (BGR); int32 xy[n][K][2]; int32 counts[n];
//               int32 first_img[L], first_feat[L]; double xyz[L][3]; uint8 inlier[L]; double poses34[C][12]
// OUT (binary): per image of readImg (from a buffer with 5 bytes of row padding): int32 rows, cols; double factor;
//               uint8 rgb[rows][cols][3]; uint8 gray[rows][cols]; then per feature of extractFeatureColors int32 red, green, blue;
//               then reshapeImg of image 0 taken as RGB: int32 rows, cols; uint8 [rows][cols][3];
//               then int32 camera ids[C] in the iteration order of the pose map saveCloud walked
// PLY_PLAIN / PLY_FLAGS: saveCloud(landmarks, poses, path) and saveCloud(landmarks, poses, path, inliers); a landmark has the
// colour of feature first_feat of image first_img when both are in range, black otherwise.
// stdout: "landmarks N coloured M": a Triangulator batch of N accepted two-view tracks, M of them with their first feature's colour.
#include <cstdio>
#include <cstdlib>
#include <unordered_map>
#include <vector>

#include "../../reconstructor_amd/host/HipImagePrep.h"
#include "../../reconstructor_amd/host/HipTriangulator.h"

using namespace reconstructor::Core;
using reconstructor::Utils::ImagePrep;

template <class T> static bool readv(FILE *f, std::vector<T> &v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[7];
    if (std::fread(hdr, sizeof(int32_t), 7, f) != 7) return 2;
    const int n = hdr[0], H = hdr[1], W = hdr[2], maxSize = hdr[3], K = hdr[4], L = hdr[5], C = hdr[6];
    if (n < 1 || n > 64 || H < 1 || W < 1 || H > 4096 || W > 4096 || K < 1 || K > 4096 || L < 0 || L > 65536 || C < 1 || C > 64) return 2;
    const size_t px = (size_t)H * W * 3;
    std::vector<uint8_t> images((size_t)n * px), inlier((size_t)L);
    std::vector<int32_t> xy((size_t)n * K * 2), counts((size_t)n), firstImg((size_t)L), firstFeat((size_t)L);
    std::vector<double> xyz((size_t)L * 3), poses((size_t)C * 12);
    if (!readv(f, images) || !readv(f, xy) || !readv(f, counts) || !readv(f, firstImg) || !readv(f, firstFeat) || !readv(f, xyz) || !readv(f, inlier) ||
        !readv(f, poses)) return 2;
    std::fclose(f);
    int rc = 0;
    try {
        Triangulator tri;                       // one ctx for both adapters
        ImagePrep prep(tri.ctx());
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        std::unordered_map<int, std::vector<FeaturePtr<>>> features;
        for (int i = 0; i < n; ++i) {
            ColourImage img;
            img.rows = H; img.cols = W; img.channels = 3; img.step = (size_t)W * 3 + 5;
            img.data.assign((size_t)H * img.step, 0xCD);
            for (int y = 0; y < H; ++y) std::copy(images.begin() + (size_t)i * px + (size_t)y * W * 3, images.begin() + (size_t)i * px + (size_t)(y + 1) * W * 3,
                                                  img.data.begin() + (size_t)y * img.step);
            GreyImage gray;
            const double factor = prep.readImg(img, maxSize, &gray);
            const int32_t shape[2] = {img.rows, img.cols};
            std::fwrite(shape, sizeof(int32_t), 2, o);
            std::fwrite(&factor, sizeof(double), 1, o);
            std::fwrite(img.data.data(), 1, img.data.size(), o);
            std::fwrite(gray.u8.data(), 1, gray.u8.size(), o);
            if (gray.rows != img.rows || gray.cols != img.cols || img.step != 0 || img.data.size() != (size_t)img.rows * img.cols * 3) rc = 4;
            auto &fs = features[i];
            for (int k = 0; k < K && k < counts[(size_t)i]; ++k) {
                auto p = std::make_shared<Feature<>>();
                p->featCoord = FeatCoord<>(xy[((size_t)i * K + k) * 2], xy[((size_t)i * K + k) * 2 + 1]);
                fs.push_back(p);
            }
            prep.extractFeatureColors(fs, img);
            for (const auto &p : fs) {
                const int32_t col[3] = {p->featColor.red, p->featColor.green, p->featColor.blue};
                std::fwrite(col, sizeof(int32_t), 3, o);
            }
        }
        {
            ColourImage img;
            img.rows = H; img.cols = W; img.channels = 3;
            img.data.assign(images.begin(), images.begin() + px);
            prep.reshapeImg(img, maxSize);
            const int32_t shape[2] = {img.rows, img.cols};
            std::fwrite(shape, sizeof(int32_t), 2, o);
            std::fwrite(img.data.data(), 1, img.data.size(), o);
        }
        std::vector<Landmark> landmarks;
        std::vector<bool> flags;
        for (int l = 0; l < L; ++l) {
            const int i = firstImg[(size_t)l], k = firstFeat[(size_t)l];
            FeatColor c;
            if (i >= 0 && i < n && k >= 0 && k < (int)features[i].size()) c = features[i][(size_t)k]->featColor;
            landmarks.emplace_back(xyz[3 * (size_t)l], xyz[3 * (size_t)l + 1], xyz[3 * (size_t)l + 2], c.red, c.green, c.blue);
            flags.push_back(inlier[(size_t)l] != 0);
        }
        std::unordered_map<int, Mat4d> imgIdx2camPose;
        for (int c = 0; c < C; ++c) {
            Mat4d T;
            for (int r = 0; r < 3; ++r) for (int k = 0; k < 4; ++k) T(r, k) = poses[(size_t)c * 12 + 4 * r + k];
            imgIdx2camPose[7 * c + 3] = T;                                      // ids that do not iterate in insertion order
        }
        prep.saveCloud(landmarks, imgIdx2camPose, argv[3]);
        prep.saveCloud(landmarks, imgIdx2camPose, argv[4], flags);
        for (const auto &kv : imgIdx2camPose) { const int32_t id = (kv.first - 3) / 7; std::fwrite(&id, sizeof(int32_t), 1, o); }
        std::fclose(o);

        // two cameras one unit apart looking down z, a grid of points in front of them: every accepted track's landmark must carry
        // the colour of the track's FIRST feature, whichever image that is
        std::unordered_map<int, std::vector<FeaturePtr<>>> feats;
        std::unordered_map<int, Mat4d> camPose;
        std::unordered_map<int, PinholeCamera> camIntr;
        camPose[0] = Mat4d();
        camPose[1] = Mat4d();
        camPose[1](0, 3) = -1.0;
        camIntr[0] = PinholeCamera(480, 640, 500.0, 500.0);
        camIntr[1] = camIntr[0];
        std::vector<Triangulator::Track> batch;
        for (int j = 0; j < 24; ++j) {
            const double X = -1.0 + 0.13 * (j % 6), Y = -0.6 + 0.31 * (j / 6), Z = 4.0 + 0.2 * (j % 5);
            for (int cam = 0; cam < 2; ++cam) {
                const auto uv = camIntr[cam].project(X + camPose[cam](0, 3), Y, Z);
                auto p = std::make_shared<Feature<>>();
                p->featCoord = FeatCoord<>((int)uv.first, (int)uv.second);
                p->featColor = FeatColor(10 + j, 100 + cam, 200 - j);
                feats[cam].push_back(p);
            }
            if (j % 2) batch.push_back({{1, j}, {0, j}});
            else batch.push_back({{0, j}, {1, j}});
        }
        std::vector<Landmark> lms;
        tri.triangulateMultiView(batch, feats, lms, camPose, camIntr);
        int coloured = 0;
        for (const auto &lm : lms) {
            const auto &first = lm.triangulatedFeatures.front();
            const FeatColor &c = feats[first.imgIdx][(size_t)first.featIdx]->featColor;
            coloured += lm.red == c.red && lm.green == c.green && lm.blue == c.blue && lm.green == 100 + first.imgIdx;
        }
        std::printf("landmarks %d coloured %d\n", (int)lms.size(), coloured);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    return rc;
}
