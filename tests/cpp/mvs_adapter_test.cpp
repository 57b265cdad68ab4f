// Driver of reconstructor::Utils::DenseCloud (reconstructor_amd/host/HipDenseCloud.h) for tests/test_mvs_cpp.py.
//   mvs_adapter_test IN OUT PLY
// IN  (binary): int32 n, rows, cols, V, S, D, radius, min_sources, min_consistent, stride; double max_cost, rel_tol;
//               double poses34[n][12]; double intrinsics[n][6]; int32 views[V][1 + S] (camera indices, -1: none); double range[V][2];
//               uint8 gray[n][rows][cols]; uint8 rgb[n][rows][cols][3]
// OUT (binary): the adapter's vertices (16-byte records); PLY: saveDenseCloud's file.
// Camera i goes in under the image id 7 + 3 i, colour images with 5 bytes of row padding.  The driver repeats the whole chain in plain
// loops over csrc/mvs_geom.h -- every window summed by itself, no tiles, no separable sums -- and compares: stdout
// "vertices N plain M equal E maps E2 threw T" (E, E2: the adapter's vertices / depth maps equal the plain loop's byte for byte).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#if defined(__GNUC__) && !defined(__clang__)
#pragma GCC optimize("fp-contract=off")      // what csrc/mvs_geom.h asks of clang by pragma
#endif
#include "../../reconstructor_amd/csrc/mvs_geom.h"
#include "../../reconstructor_amd/host/HipDenseCloud.h"

using namespace reconstructor::Core;
using namespace reconstructor::Utils;

template <class T> static bool readv(FILE *f, std::vector<T> &v) { return v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(); }

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t h[10];
    double fo[2];
    if (std::fread(h, 4, 10, f) != 10 || std::fread(fo, 8, 2, f) != 2) return 2;
    const int n = h[0], rows = h[1], cols = h[2], V = h[3], S = h[4], D = h[5], R = h[6], minSources = h[7], minConsistent = h[8], stride = h[9];
    if (n < 2 || n > 64 || rows < 1 || cols < 1 || rows > 1024 || cols > 1024 || V < 1 || V > 64 || S < 1 || S > 16 || D < 1 || D > 1024 || R < 1 || R > 5 || stride < 1) return 2;
    const size_t px = (size_t)rows * cols;
    std::vector<double> P((size_t)n * 12), K((size_t)n * 6), range((size_t)V * 2);
    std::vector<int32_t> views((size_t)V * (1 + S));
    std::vector<uint8_t> gray(px * n), rgb(3 * px * n);
    if (!readv(f, P) || !readv(f, K) || !readv(f, views) || !readv(f, range) || !readv(f, gray) || !readv(f, rgb)) return 2;
    std::fclose(f);

    // ---- the plain loops
    std::vector<uint8_t> ug(px * n), uc(3 * px * n);
    for (int i = 0; i < n; ++i)
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols; ++x) {
                double u, v;
                int qu, qv;
                mg_distort(&K[6 * (size_t)i], x, y, &u, &v);
                const bool ok = mg_quantise(u, v, rows, cols, &qu, &qv);
                ug[px * i + (size_t)y * cols + x] = ok ? (uint8_t)((mg_sample(&gray[px * i], cols, 1, rows, cols, qu, qv) + 512) >> 10) : 0;
                for (int c = 0; c < 3; ++c)
                    uc[3 * (px * i + (size_t)y * cols + x) + c] = ok ? (uint8_t)((mg_sample(&rgb[3 * px * i + c], 3 * (int64_t)cols, 3, rows, cols, qu, qv) + 512) >> 10) : 0;
            }
    std::vector<int16_t> plane(px * V, -1);
    std::vector<float> depth(px * V, 0.f), cost(px * V, INFINITY);
    const int nwin = (2 * R + 1) * (2 * R + 1);
    for (int v = 0; v < V; ++v) {
        const int32_t *vw = &views[(size_t)v * (1 + S)];
        std::vector<double> inv((size_t)D), H((size_t)S * D * 9);
        if (!mg_inv_depths(range[2 * (size_t)v], range[2 * (size_t)v + 1], D, 1024, inv.data()) ||
            !mg_homographies(P.data(), K.data(), vw[0], vw + 1, S, inv.data(), D, 16, 1024, H.data())) return 2;
        const uint8_t *a = &ug[px * vw[0]];
        for (int y = R; y < rows - R; ++y)
            for (int x = R; x < cols - R; ++x) {
                int64_t Sa = 0, Saa = 0;
                for (int dy = -R; dy <= R; ++dy)
                    for (int dx = -R; dx <= R; ++dx) { const int64_t t = a[(size_t)(y + dy) * cols + x + dx]; Sa += t; Saa += t * t; }
                const int64_t Va = nwin * Saa - Sa * Sa;
                if (Va <= 0) continue;
                std::vector<double> costs((size_t)D, INFINITY);
                for (int k = 0; k < D; ++k) {
                    double sum = 0.0;
                    int cnt = 0;
                    for (int s = 0; s < S; ++s) {
                        if (vw[1 + s] < 0) continue;
                        const double *Hk = &H[((size_t)s * D + k) * 9];
                        int64_t Sb = 0, Sbb = 0, Sab = 0;
                        bool all = true;
                        for (int dy = -R; dy <= R && all; ++dy)
                            for (int dx = -R; dx <= R; ++dx) {
                                int qu, qv;
                                if (!mg_warp(Hk, x + dx, y + dy, rows, cols, &qu, &qv)) { all = false; break; }
                                const int64_t b = mg_sample(&ug[px * vw[1 + s]], cols, 1, rows, cols, qu, qv), t = a[(size_t)(y + dy) * cols + x + dx];
                                Sb += b; Sbb += b * b; Sab += t * b;
                            }
                        double c;
                        if (all && mg_cost(nwin, Sa, Va, Sb, Sbb, Sab, &c)) { sum += c; ++cnt; }
                    }
                    if (cnt >= minSources && cnt > 0) costs[(size_t)k] = sum / (double)cnt;
                }
                int bk = 0;
                for (int k = 1; k < D; ++k) if (costs[(size_t)k] < costs[(size_t)bk]) bk = k;
                if (!(costs[(size_t)bk] < INFINITY) || costs[(size_t)bk] > fo[0]) continue;
                const bool hm = bk > 0 && costs[(size_t)bk - 1] < INFINITY, hp = bk + 1 < D && costs[(size_t)bk + 1] < INFINITY;
                const double r = mg_refine(hm ? costs[(size_t)bk - 1] : 0.0, costs[(size_t)bk], hp ? costs[(size_t)bk + 1] : 0.0, hm, hp, hm ? inv[(size_t)bk - 1] : 0.0,
                                           inv[(size_t)bk], hp ? inv[(size_t)bk + 1] : 0.0);
                const size_t o = px * v + (size_t)y * cols + x;
                plane[o] = (int16_t)bk; depth[o] = (float)(1.0 / r); cost[o] = (float)costs[(size_t)bk];
            }
    }
    std::vector<int> viewOf((size_t)n, -1);
    for (int v = V - 1; v >= 0; --v) viewOf[(size_t)views[(size_t)v * (1 + S)]] = v;       // an image swept twice: its first map
    std::vector<DenseVertex> plain;
    for (int v = 0; v < V; ++v) {
        const int32_t *vw = &views[(size_t)v * (1 + S)];
        for (int y = 0; y < rows; y += stride)
            for (int x = 0; x < cols; x += stride) {
                const size_t o = px * v + (size_t)y * cols + x;
                if (plane[o] < 0) continue;
                double X[3];
                mg_lift(&P[12 * (size_t)vw[0]], &K[6 * (size_t)vw[0]], x, y, (double)depth[o], X);
                int agree = 0;
                for (int s = 0; s < S; ++s) {
                    const int src = vw[1 + s];
                    if (src < 0 || viewOf[(size_t)src] < 0) continue;
                    double u, w, z;
                    mg_project(&P[12 * (size_t)src], &K[6 * (size_t)src], X, &u, &w, &z);
                    const double fu = std::floor(u + 0.5), fv = std::floor(w + 0.5);
                    if (!(z > 0.0) || !(fu >= 0.0 && fu <= cols - 1 && fv >= 0.0 && fv <= rows - 1)) continue;
                    const size_t q = px * viewOf[(size_t)src] + (size_t)fv * cols + (size_t)fu;
                    if (plane[q] >= 0 && std::fabs(z - (double)depth[q]) <= fo[1] * z) ++agree;
                }
                if (agree < minConsistent) continue;
                const uint8_t *c = &uc[3 * (px * vw[0] + (size_t)y * cols + x)];
                plain.push_back(DenseVertex{(float)X[0], (float)X[1], (float)X[2], c[0], c[1], c[2], 255});
            }
    }

    // ---- the adapter, on the containers the pipeline holds
    std::map<int, Mat4d> poses;
    std::map<int, std::array<double, 6>> intr;
    std::map<int, GreyImage> grays;
    std::map<int, ColourImage> colours;
    for (int i = 0; i < n; ++i) {
        const int id = 7 + 3 * i;
        Mat4d M;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 4; ++c) M(r, c) = P[12 * (size_t)i + 4 * r + c];
        poses[id] = M;
        std::array<double, 6> k6;
        std::copy(K.begin() + 6 * i, K.begin() + 6 * i + 6, k6.begin());
        intr[id] = k6;
        GreyImage g;
        g.rows = rows; g.cols = cols; g.u8.assign(gray.begin() + px * i, gray.begin() + px * (i + 1));
        grays[id] = g;
        ColourImage ci;
        ci.rows = rows; ci.cols = cols; ci.channels = 3; ci.step = 3 * (size_t)cols + 5;
        ci.data.assign((size_t)rows * ci.step, 0xCD);
        for (int y = 0; y < rows; ++y) std::copy(rgb.begin() + 3 * (px * i + (size_t)y * cols), rgb.begin() + 3 * (px * i + (size_t)(y + 1) * cols), ci.data.begin() + (size_t)y * ci.step);
        colours[id] = ci;
    }
    std::vector<DenseView> dv((size_t)V);
    for (int v = 0; v < V; ++v) {
        dv[(size_t)v].refId = 7 + 3 * views[(size_t)v * (1 + S)];
        for (int s = 0; s < S; ++s) if (views[(size_t)v * (1 + S) + 1 + s] >= 0) dv[(size_t)v].sourceIds.push_back(7 + 3 * views[(size_t)v * (1 + S) + 1 + s]);
        dv[(size_t)v].nearDepth = range[2 * (size_t)v]; dv[(size_t)v].farDepth = range[2 * (size_t)v + 1];
    }
    int threw = 0, equal = 0, maps = 0;
    size_t nv = 0;
    try {
        DenseCloud dc;
        dc.numPlanes = D;
        dc.options.radius = R; dc.options.min_sources = minSources; dc.options.min_consistent = minConsistent; dc.options.stride = stride;
        dc.options.max_cost = fo[0]; dc.options.rel_tol = fo[1];
        const std::vector<DenseVertex> got = dc.denseCloud(poses, intr, grays, colours, dv);
        nv = got.size();
        equal = got.size() == plain.size() && dc.lastTotal == (int64_t)plain.size() && (got.empty() || std::memcmp(got.data(), plain.data(), 16 * got.size()) == 0);
        const DepthMaps m = dc.computeDepthMaps(poses, intr, grays, dv);
        maps = m.rows == rows && m.cols == cols && std::memcmp(m.plane.data(), plane.data(), 2 * px * V) == 0 && std::memcmp(m.depth.data(), depth.data(), 4 * px * V) == 0 &&
               std::memcmp(m.cost.data(), cost.data(), 4 * px * V) == 0;
        FILE *o = std::fopen(argv[2], "wb");
        if (!o) return 2;
        if (!got.empty()) std::fwrite(got.data(), 16, got.size(), o);
        std::fclose(o);
        if (dc.saveDenseCloud(poses, intr, grays, colours, dv, argv[3]) != nv) return 3;
        std::vector<DenseView> bad = dv;
        bad[0].sourceIds.push_back(bad[0].refId);          // its own source
        try { dc.denseCloud(poses, intr, grays, colours, bad); } catch (const std::runtime_error &) { ++threw; }
        bad = dv;
        bad[0].refId = 5;                                  // no such camera
        try { dc.denseCloud(poses, intr, grays, colours, bad); } catch (const std::runtime_error &) { ++threw; }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("vertices %zu plain %zu equal %d maps %d threw %d\n", nv, plain.size(), equal, maps, threw);
    return 0;
}
