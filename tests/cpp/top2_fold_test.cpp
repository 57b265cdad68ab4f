// The batched top-2 fold (csrc/top2_fold.h) on the host, against a sort.  Stand-alone: includes that header alone.
//   1. top2_fold2 / top2_fold4 exhaustively on the values 0..5 (a <= b, duplicates and all-equal included);
//   2. 10^6 random 32-bit cases with 0xFFFFFFFF (the initial value and the key of a padded row) in every position;
//   3. chains of 32 keys folded four at a time, two at a time and one at a time: the same pair, and the sort's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../reconstructor_amd/csrc/top2_fold.h"

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++failures <= 20) { std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #c); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// the fold the kernels used before: med3 + min per key
static void fold1(unsigned &m1, unsigned &m2, unsigned u)
{
    m2 = umed3(m1, m2, u);
    m1 = m1 < u ? m1 : u;
}

static void two_smallest(std::vector<unsigned> v, unsigned &s1, unsigned &s2)
{
    std::sort(v.begin(), v.end());
    s1 = v[0]; s2 = v[1];
}

static void check2(unsigned a, unsigned b, unsigned u, unsigned v)
{
    unsigned s1, s2, m1 = a, m2 = b, n1 = a, n2 = b;
    two_smallest({a, b, u, v}, s1, s2);
    top2_fold2(m1, m2, u, v);
    fold1(n1, n2, u); fold1(n1, n2, v);
    CHECK(m1 == s1 && m2 == s2, "fold2(%u %u | %u %u) = %u %u, sort %u %u", a, b, u, v, m1, m2, s1, s2);
    CHECK(n1 == s1 && n2 == s2, "key by key (%u %u | %u %u) = %u %u, sort %u %u", a, b, u, v, n1, n2, s1, s2);
}

static void check4(unsigned a, unsigned b, unsigned u, unsigned v, unsigned w, unsigned x)
{
    unsigned s1, s2, m1 = a, m2 = b, n1 = a, n2 = b;
    two_smallest({a, b, u, v, w, x}, s1, s2);
    top2_fold4(m1, m2, u, v, w, x);
    fold1(n1, n2, u); fold1(n1, n2, v); fold1(n1, n2, w); fold1(n1, n2, x);
    CHECK(m1 == s1 && m2 == s2, "fold4(%u %u | %u %u %u %u) = %u %u, sort %u %u", a, b, u, v, w, x, m1, m2, s1, s2);
    CHECK(n1 == s1 && n2 == s2, "key by key (%u %u | %u %u %u %u) = %u %u, sort %u %u", a, b, u, v, w, x, n1, n2, s1, s2);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{   // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 16);
}

int main()
{
    // 1. exhaustive on 0..5
    long n_small = 0;
    for (unsigned a = 0; a < 6; ++a)
        for (unsigned b = a; b < 6; ++b)
            for (unsigned u = 0; u < 6; ++u)
                for (unsigned v = 0; v < 6; ++v) {
                    check2(a, b, u, v);
                    for (unsigned w = 0; w < 6; ++w)
                        for (unsigned x = 0; x < 6; ++x) { check4(a, b, u, v, w, x); ++n_small; }
                }
    // the median itself, all orders
    for (unsigned a = 0; a < 6; ++a)
        for (unsigned b = 0; b < 6; ++b)
            for (unsigned c = 0; c < 6; ++c) {
                unsigned s[3] = {a, b, c};
                std::sort(s, s + 3);
                CHECK(umed3(a, b, c) == s[1] && umin3(a, b, c) == s[0], "med3 / min3 of %u %u %u", a, b, c);
            }

    // 2. random 32-bit cases; case i has 0xFFFFFFFF in the positions its low six bits name, so every position (and every
    //    combination of positions) carries it many times
    const unsigned PAD = 0xFFFFFFFFu;
    long pad_seen[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 1000000; ++i) {
        unsigned k[6];
        for (int j = 0; j < 6; ++j) {
            k[j] = rnd();
            if ((i & 7) == 7) k[j] &= 0xFFFFF003u;          // keys of equal value part differ in the row bits only
            if ((i >> j) & 1) { k[j] = PAD; ++pad_seen[j]; }
        }
        if (k[0] > k[1]) std::swap(k[0], k[1]);
        check4(k[0], k[1], k[2], k[3], k[4], k[5]);
        check2(k[0], k[1], k[2], k[3]);
    }
    for (int j = 0; j < 6; ++j) CHECK(pad_seen[j] > 100000, "position %d saw the padded key %ld times", j, pad_seen[j]);

    // 3. chains of 32 keys from the initial pair
    for (int c = 0; c < 20000; ++c) {
        std::vector<unsigned> keys(32);
        for (auto &k : keys) {
            k = rnd();
            if (c % 3 == 1) k = (k & 0xFF000FFFu);           // many equal value parts
            if (c % 5 == 2 && (rnd() & 3) == 0) k = PAD;     // padded rows among them
        }
        if (c % 7 == 3) for (auto &k : keys) k = PAD;        // a pair of padded rows only
        unsigned a1 = PAD, a2 = PAD, b1 = PAD, b2 = PAD, c1 = PAD, c2 = PAD;
        for (int i = 0; i < 32; i += 4) top2_fold4(a1, a2, keys[i], keys[i + 1], keys[i + 2], keys[i + 3]);
        for (int i = 0; i < 32; i += 2) top2_fold2(b1, b2, keys[i], keys[i + 1]);
        for (int i = 0; i < 32; ++i) fold1(c1, c2, keys[i]);
        std::vector<unsigned> all(keys);
        all.push_back(PAD); all.push_back(PAD);
        unsigned s1, s2;
        two_smallest(all, s1, s2);
        CHECK(a1 == s1 && a2 == s2, "chain %d by four: %u %u, sort %u %u", c, a1, a2, s1, s2);
        CHECK(b1 == s1 && b2 == s2, "chain %d by two: %u %u, sort %u %u", c, b1, b2, s1, s2);
        CHECK(c1 == s1 && c2 == s2, "chain %d key by key: %u %u, sort %u %u", c, c1, c2, s1, s2);
        // the kernels' form: a pair closed per two keys, the median of the first pair parked until the second closes
        unsigned d1 = PAD, d2 = PAD;
        for (int i = 0; i < 32; i += 4) {
            const unsigned p = top2_fold_pair(d1, keys[i], keys[i + 1]);
            d2 = umin3(d2, p, top2_fold_pair(d1, keys[i + 2], keys[i + 3]));
        }
        CHECK(d1 == s1 && d2 == s2, "chain %d by pairs: %u %u, sort %u %u", c, d1, d2, s1, s2);
    }

    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("%ld exhaustive cases, 1000000 random cases, 20000 chains: all cases pass\n", n_small);
    return 0;
}
