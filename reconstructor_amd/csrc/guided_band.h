// guided_band.h -- the epipolar band of guided matching, one text for the GPU kernels (guided.hip) and for plain
// host C++ (tests/cpp/guided_band_test.cpp).  No HIP header is needed: without a HIP compiler the qualifiers vanish.
//
// Pair (query image, train image), F row-major in the filter's convention: p1 the query point, p2 the train point, residual
// p2^T F p1.  With thr2 = max_error_px^2, every product and every sum an fp64 operation of its own (contraction off), in the order of
// epi_inlier9 (fmat.hip) and without its divisions:
//     a  = F0 x1 + F1 y1 + F2    b  = F3 x1 + F4 y1 + F5    c  = F6 x1 + F7 y1 + F8      the line of p1 in the train image
//     q2 = a a + b b             d2 = x2 a + y2 b + c       t2 = d2 d2
//     a' = F0 x2 + F3 y2 + F6    b' = F1 x2 + F4 y2 + F7    c' = F2 x2 + F5 y2 + F8      the line of p2 in the query image
//     q1 = a'a' + b'b'           d1 = x1 a' + y1 b' + c'    t1 = d1 d1
//     candidate = 0 < q1 < DBL_MAX  &&  0 < q2 < DBL_MAX  &&  t1 <= thr2 q1  &&  t2 <= thr2 q2
// A point's line depends on that point alone, so a kernel computes gb_line once per point and gb_test once per (query, train): the
// per-point limit GbLine::lim folds the range test of q into thr2 q (a squared residual is never <= -1, and a NaN one is <= nothing).
// Transposing F and swapping the two points swaps (a, b, c, q2, d2) with (a', b', c', q1, d1) term by term, so
// gb_candidate(F, p1, p2) == gb_candidate(F^T, p2, p1) bit for bit.
#pragma once
#include <float.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GB_FN __host__ __device__ inline
#else
#define GB_FN inline
#endif

struct GbLine { double a, b, c, lim; };      // the line of a point in the other image; lim = thr2 (a^2 + b^2), or -1: no candidates at all

// tr == 0: the line F p of a query point (a, b, c above); tr != 0: the line F^T p of a train point (a', b', c')
GB_FN GbLine gb_line(const double *F, int tr, double x, double y, double thr2)
{
#pragma clang fp contract(off)
    GbLine l;
    if (!tr) {
        l.a = F[0] * x + F[1] * y + F[2];
        l.b = F[3] * x + F[4] * y + F[5];
        l.c = F[6] * x + F[7] * y + F[8];
    } else {
        l.a = F[0] * x + F[3] * y + F[6];
        l.b = F[1] * x + F[4] * y + F[7];
        l.c = F[2] * x + F[5] * y + F[8];
    }
    const double q = l.a * l.a + l.b * l.b;
    l.lim = (q > 0 && q < DBL_MAX) ? thr2 * q : -1.0;
    return l;
}

// one side of the band: is the point (x, y) within the limit of the line l (of the other image's point)?
GB_FN bool gb_side(const GbLine &l, double x, double y)
{
#pragma clang fp contract(off)
    const double d = x * l.a + y * l.b + l.c;
    const double t = d * d;
    return t <= l.lim;
}

// l1: gb_line(F, 0, x1, y1), l2: gb_line(F, 1, x2, y2)
GB_FN bool gb_test(const GbLine &l1, double x1, double y1, const GbLine &l2, double x2, double y2)
{
    // both limits first: a degenerate line on either side (lim = -1) refuses the pair whatever the other side says
    return l1.lim >= 0 && l2.lim >= 0 && gb_side(l2, x1, y1) && gb_side(l1, x2, y2);
}

GB_FN bool gb_candidate(const double *F, double x1, double y1, double x2, double y2, double thr2)
{
    const GbLine l1 = gb_line(F, 0, x1, y1, thr2), l2 = gb_line(F, 1, x2, y2, thr2);
    return gb_test(l1, x1, y1, l2, x2, y2);
}
