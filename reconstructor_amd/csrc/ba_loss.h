// ba_loss.h -- the robust losses of the bundle adjuster: rho(s), rho'(s) and the row weight sqrt(rho'(s)) of
// one observation, s = r0^2 + r1^2 of its unweighted residual in pixels^2, a > 0 the scale in pixels, b = a * a.
//
//   kind                     rho(s)                                    rho'(s)
//   RCN_BA_LOSS_TRIVIAL 0    s                                         1
//   RCN_BA_LOSS_HUBER   1    s <= b: s,  else 2 a sqrt(s) - b          s <= b: 1,  else max(DBL_MIN, a / sqrt(s))
//   RCN_BA_LOSS_SOFT_L1 2    2 b (sqrt(1 + s/b) - 1)                   max(DBL_MIN, 1 / sqrt(1 + s/b))
//   RCN_BA_LOSS_CAUCHY  3    b log(1 + s/b)                            max(DBL_MIN, 1 / (1 + s/b))
//
// A restatement of ceres::HuberLoss / SoftLOneLoss / CauchyLoss from memory: parity with Ceres is unpinned.  All three have
// rho'' <= 0 everywhere, so Ceres' Corrector takes alpha = 0 and the corrected residual and Jacobian of an observation are the plain
// ones times w = sqrt(rho'(s)): nothing else.  Soft-L1 and Cauchy are evaluated in the forms that do not cancel at small s/b,
// 2 s / (sqrt(1 + s/b) + 1) and b log1p(s/b): the same functions.  A non-finite s gives a non-finite rho under every kind (a
// candidate with a non-finite residual is rejected by its cost); rho' is clamped from below and may then be finite.
// Plain C++: no HIP dependency, a host compiler takes this file alone (tests/cpp/ba_loss_test.cpp).
#pragma once

#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define RCN_LOSS_HD __host__ __device__ __forceinline__
#else
#define RCN_LOSS_HD inline
#endif

#define RCN_BA_LOSS_KIND_TRIVIAL 0
#define RCN_BA_LOSS_KIND_HUBER 1
#define RCN_BA_LOSS_KIND_SOFT_L1 2
#define RCN_BA_LOSS_KIND_CAUCHY 3

RCN_LOSS_HD double ba_loss_rho(int kind, double a, double b, double s)
{
    switch (kind) {
    case RCN_BA_LOSS_KIND_HUBER: return s <= b ? s : 2.0 * a * sqrt(s) - b;
    case RCN_BA_LOSS_KIND_SOFT_L1: return 2.0 * s / (sqrt(1.0 + s / b) + 1.0);
    case RCN_BA_LOSS_KIND_CAUCHY: return b * log1p(s / b);
    default: return s;
    }
}

RCN_LOSS_HD double ba_loss_clamp(double v) { return v > DBL_MIN ? v : DBL_MIN; }

RCN_LOSS_HD double ba_loss_drho(int kind, double a, double b, double s)
{
    switch (kind) {
    case RCN_BA_LOSS_KIND_HUBER: return s <= b ? 1.0 : ba_loss_clamp(a / sqrt(s));
    case RCN_BA_LOSS_KIND_SOFT_L1: return ba_loss_clamp(1.0 / sqrt(1.0 + s / b));
    case RCN_BA_LOSS_KIND_CAUCHY: return ba_loss_clamp(1.0 / (1.0 + s / b));
    default: return 1.0;
    }
}

// what the observation's row (26 Jacobian entries, 2 residuals) is multiplied by
RCN_LOSS_HD double ba_loss_weight(int kind, double a, double b, double s) { return sqrt(ba_loss_drho(kind, a, b, s)); }
