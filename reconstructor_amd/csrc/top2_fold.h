// top2_fold.h -- the exact running top-2 of unsigned keys, folded two and four keys at a time.
//
// (m1, m2) is the sorted running pair, m1 <= m2.  After a call it holds the two smallest of the multiset {m1, m2, keys}: the
// same pair that med3 + min per key leaves behind, in fewer operations:
//   one key at a time   med3 + min per key                      2    operations per key
//   top2_fold2          med3, min3, min                         1.5
//   top2_fold4          2 med3, 3 min3                          1.25
// Why it holds: with a <= b, med3(a, u, v) is the second smallest of {a, u, v} -- the only member of that triple besides its
// minimum that can be among the two smallest of {a, b, u, v} -- so the new second is min(b, med3(a, u, v)).  Four keys chain
// the minimum through both pairs and take ONE min3 over b and the two medians.
// Nothing else lives here: the kernels (match.hip, coarse_i8.h) pack their keys and spread these operations over MFMA gaps.
#pragma once

#if defined(__HIPCC__)
#define RCN_TOP2_HD __host__ __device__ __forceinline__
#else
#define RCN_TOP2_HD inline
#endif

// min(min(a, b), c) is ONE v_min3_u32 on the device as long as the inner minimum has no second user
RCN_TOP2_HD unsigned umin3(unsigned a, unsigned b, unsigned c)
{
    const unsigned ab = a < b ? a : b;
    return ab < c ? ab : c;
}

// v_med3_u32.  Through asm on the device: a median spelled with min / max shares min(a, b) with a neighbouring umin3 of the
// same operands, and the shared node keeps v_min3_u32 from forming.
RCN_TOP2_HD unsigned umed3(unsigned a, unsigned b, unsigned c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
#else
    const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned t = hi < c ? hi : c;
    return lo > t ? lo : t;
#endif
}

// the first half of a fold: m1 <- min(m1, u, v), returns the key that may still become the second
RCN_TOP2_HD unsigned top2_fold_pair(unsigned &m1, unsigned u, unsigned v)
{
    const unsigned s = umed3(m1, u, v);
    m1 = umin3(m1, u, v);
    return s;
}

RCN_TOP2_HD void top2_fold2(unsigned &m1, unsigned &m2, unsigned u, unsigned v)
{
    const unsigned s = top2_fold_pair(m1, u, v);
    m2 = m2 < s ? m2 : s;
}

RCN_TOP2_HD void top2_fold4(unsigned &m1, unsigned &m2, unsigned u, unsigned v, unsigned w, unsigned x)
{
    const unsigned s1 = top2_fold_pair(m1, u, v);
    const unsigned s2 = top2_fold_pair(m1, w, x);
    m2 = umin3(m2, s1, s2);
}
