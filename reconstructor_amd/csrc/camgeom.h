// camgeom.h -- camera geometry shared by the landmark kernels (validity.hip, triangulate.hip, pnp.hip).  gfx950.
//
// Every operation is a separately rounded IEEE double (contraction off) in one fixed order, so that every kernel that
// projects a landmark or measures a triangulation angle does it with the same bits.
#pragma once
#include "rcn_internal.h"

namespace {

// camera centre -R't of every camera, once (SequentialReconstructor.cpp:820)
__global__ void k_cam_centres(const double *__restrict__ poses, int n_cams, double *__restrict__ centres)
{
#pragma clang fp contract(off)
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_cams) return;
    const double *P = poses + 12 * (size_t)c;
    for (int i = 0; i < 3; ++i)
        centres[3 * (size_t)c + i] = ((-P[i]) * P[3] + (-P[4 + i]) * P[7]) + (-P[8 + i]) * P[11];
}

// L1 reprojection error |u - x| + |v - y| of the world point X seen at integer pixel (ox, oy) by the camera with rows of
// [R | t] P and intrinsics K = fx fy cx cy k1 k2: getLandmarkLocalCoords (:842-848), PinholeCamera::project
// (Camera.h:59-76), calcProjectionError (:852-867).  *depth: the camera-frame z.
__device__ __forceinline__ double reproj_l1(const double *P, const double *K, const double *X, int32_t ox, int32_t oy, double *depth)
{
#pragma clang fp contract(off)
    double l[3];
    for (int i = 0; i < 3; ++i) l[i] = ((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3];
    double x = l[0] / l[2], y = l[1] / l[2];
    const double radius = x * x + y * y;
    const double distortion = K[4] * radius + (K[5] * radius) * radius;
    x += distortion;
    y += distortion;
    const double u = K[0] * x + K[2], v = K[1] * y + K[3];
    *depth = l[2];
    return fabs(u - (double)ox) + fabs(v - (double)oy);
}

// The same projection with the squared L2 error (u - x)^2 + (v - y)^2: what cv::solvePnPRansac scores (pnp.hip).
__device__ __forceinline__ double reproj_sq(const double *P, const double *K, const double *X, int32_t ox, int32_t oy)
{
#pragma clang fp contract(off)
    double l[3];
    for (int i = 0; i < 3; ++i) l[i] = ((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3];
    double x = l[0] / l[2], y = l[1] / l[2];
    const double radius = x * x + y * y;
    const double distortion = K[4] * radius + (K[5] * radius) * radius;
    x += distortion;
    y += distortion;
    const double du = (K[0] * x + K[2]) - (double)ox, dv = (K[1] * y + K[3]) - (double)oy;
    return du * du + dv * dv;
}

// calcTriangulationAngle (:815-836): 180 acos(r1.r2 / (|r1| |r2|)) / 3.1415 for the rays from the camera centres c1, c2
// to X.  Symmetric in (c1, c2) bit for bit (the products commute, the sums run in the same order).
__device__ __forceinline__ double tri_angle(const double *X, const double *c1, const double *c2)
{
#pragma clang fp contract(off)
    const double r1[3] = {X[0] - c1[0], X[1] - c1[1], X[2] - c1[2]};
    const double r2[3] = {X[0] - c2[0], X[1] - c2[1], X[2] - c2[2]};
    const double n1 = sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]);
    const double n2 = sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]);
    const double dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
    return 180.0 * acos(dot / (n1 * n2)) / 3.1415;
}

}  // namespace
