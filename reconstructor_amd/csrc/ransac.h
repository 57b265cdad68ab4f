// ransac.h -- the scalars of OpenCV's RANSAC loop shared by fmat.hip, twoview.hip and pnp.hip.  gfx950.
//
// All three searches must sample and stop as the reference's cv:: loop does, bit for bit: one definition each.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace {

// cv::RNG: multiply with carry
__device__ __forceinline__ unsigned rng_next(unsigned long long &s)
{
    s = (unsigned long long)(unsigned)s * 4164903690U + (unsigned)(s >> 32);
    return (unsigned)s;
}

// cv::RANSACUpdateNumIters: every operation a separately rounded double; pow / log are the device library's
__device__ __forceinline__ int update_num_iters(double p, double ep, int model_points, int max_iters)
{
#pragma clang fp contract(off)
    p = fmax(p, 0.); p = fmin(p, 1.);
    ep = fmax(ep, 0.); ep = fmin(ep, 1.);
    double num = fmax(1. - p, DBL_MIN);
    double denom = 1. - pow(1. - ep, (double)model_points);
    if (denom < DBL_MIN) return 0;
    num = log(num);
    denom = log(denom);
    return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)lrint(num / denom);
}

__device__ __forceinline__ bool finite_d(double x) { return x - x == 0.0; }

}  // namespace
