// ba_loss_test -- csrc/ba_loss.h alone, on the host, against long double (tests/test_ba_loss.py builds this with the address and
// undefined-behaviour sanitizers).  What is checked, for Huber, soft-L1 and Cauchy at scales from 1e-3 to 1e150 and s from 0 to 1e12 b:
//   rho and rho' against the closed forms of the header's table, evaluated in long double: 8 u relative (rho: a square root or a
//     logarithm, a division and two or three more operations; no cancellation in the forms the header evaluates);
//   rho' against a centred difference of the long-double rho, h = 2^-20 s: the difference's own truncation error is
//     |rho'''| h^2 / 6 <= rho' (h / s)^2 for these three families, so 2^-38 relative is what the difference can tell;
//   Huber on both sides of s = b (b itself, its two neighbours), and rho(s) == s, rho' == 1, weight == 1 BITWISE for s <= b;
//   s = 0: rho == 0, rho' == 1; s = inf and s = NaN: rho not finite under every kind; rho' >= DBL_MIN everywhere (s = inf and
//     s = DBL_MAX included); the trivial kind: rho == s, rho' == 1.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../reconstructor_amd/csrc/ba_loss.h"

typedef long double ld;
static int g_bad = 0;
#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            if (++g_bad <= 20) { printf("FAIL %s:%d  ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                  \
    } while (0)

static ld rho_ld(int kind, ld a, ld b, ld s)
{
    switch (kind) {
    case 1: return s <= b ? s : 2 * a * sqrtl(s) - b;
    case 2: return 2 * s / (sqrtl(1 + s / b) + 1);      // = 2 b (sqrt(1 + s/b) - 1), which cancels at small s/b in any precision
    case 3: return b * log1pl(s / b);      // = b log(1 + s/b), without the rounding of 1 + s/b
    default: return s;
    }
}
static ld drho_ld(int kind, ld a, ld b, ld s)
{
    switch (kind) {
    case 1: return s <= b ? 1 : a / sqrtl(s);
    case 2: return 1 / sqrtl(1 + s / b);
    case 3: return 1 / (1 + s / b);
    default: return 1;
    }
}
static bool same_bits(double x, double y) { return memcmp(&x, &y, 8) == 0; }

int main()
{
    const double U = ldexp(1.0, -53);
    const double scales[] = {1e-3, 0.5, 1.0, 2.0, 3.7, 1e3, 1e150};
    const double ratios[] = {1e-12, 1e-6, 1e-3, 0.1, 0.5, 0.999, 1.001, 1.5, 2.0, 10.0, 1e3, 1e6, 1e12};
    long cases = 0;
    for (int kind = 1; kind <= 3; ++kind)
        for (double a : scales) {
            const double b = a * a;
            for (double q : ratios) {
                const double s = q * b;
                if (!std::isfinite(s)) continue;      // (the largest scale times the largest ratio; s = inf has its own check below)
                const double r = ba_loss_rho(kind, a, b, s), dr = ba_loss_drho(kind, a, b, s), w = ba_loss_weight(kind, a, b, s);
                const ld R = rho_ld(kind, a, b, s);
                const ld D = drho_ld(kind, a, b, s);
                CHECK(fabsl(r - R) <= 8 * U * fabsl(R), "rho kind %d a %g s/b %g: %.17g against %.21Lg", kind, a, q, r, R);
                CHECK(fabsl(dr - D) <= 8 * U * fabsl(D), "rho' kind %d a %g s/b %g: %.17g against %.21Lg", kind, a, q, dr, D);
                CHECK(fabsl((ld)w * w - dr) <= 4 * U * dr, "weight kind %d a %g s/b %g", kind, a, q);
                CHECK(dr >= DBL_MIN && dr <= 1.0, "rho' range kind %d a %g s/b %g: %g", kind, a, q, dr);
                // centred difference of the long-double rho (not across Huber's kink)
                const ld h = ldexpl((ld)s, -20);
                if (!(kind == 1 && (s - h <= b) != (s + h <= b))) {
                    const ld fd = (rho_ld(kind, a, b, s + h) - rho_ld(kind, a, b, s - h)) / (2 * h);
                    // besides the truncation, the difference carries the rounding of two long-double rho over 2 h: 2^-64 rho / (2^-20 s)
                    const ld tol = ldexpl(1.0L, -38) * fabsl(D) + ldexpl(1.0L, -41) * fabsl(R) / s;
                    CHECK(fabsl(fd - dr) <= tol, "rho' against the difference, kind %d a %g s/b %g: %.17g against %.21Lg", kind, a, q, dr, fd);
                }
                if (kind == 1 && s <= b) CHECK(same_bits(r, s) && same_bits(dr, 1.0) && same_bits(w, 1.0), "Huber below the scale is not the identity: a %g s/b %g", a, q);
                ++cases;
            }
            // Huber on both sides of s = b
            if (kind == 1) {
                const double lo = nextafter(b, 0.0), hi = nextafter(b, HUGE_VAL);
                for (double s : {lo, b}) CHECK(same_bits(ba_loss_rho(1, a, b, s), s) && same_bits(ba_loss_drho(1, a, b, s), 1.0) && same_bits(ba_loss_weight(1, a, b, s), 1.0), "Huber at the scale, a %g", a);
                const double r = ba_loss_rho(1, a, b, hi), dr = ba_loss_drho(1, a, b, hi);
                CHECK(fabsl(r - rho_ld(1, a, b, hi)) <= 8 * U * b && dr < 1.0 + 2 * U && dr > 1.0 - 4 * U, "Huber just above the scale, a %g: %.17g %.17g", a, r, dr);
            }
            // s = 0, inf, NaN, DBL_MAX
            CHECK(ba_loss_rho(kind, a, b, 0.0) == 0.0 && same_bits(ba_loss_drho(kind, a, b, 0.0), 1.0) && same_bits(ba_loss_weight(kind, a, b, 0.0), 1.0), "s = 0, kind %d a %g", kind, a);
            const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
            CHECK(!std::isfinite(ba_loss_rho(kind, a, b, inf)), "rho(inf) is finite, kind %d a %g", kind, a);
            CHECK(!std::isfinite(ba_loss_rho(kind, a, b, nan)), "rho(NaN) is finite, kind %d a %g", kind, a);
            for (double s : {inf, DBL_MAX, nan}) {
                const double dr = ba_loss_drho(kind, a, b, s);
                CHECK(dr >= DBL_MIN, "rho' below DBL_MIN at s = %g, kind %d a %g: %g", s, kind, a, dr);
            }
        }
    // the trivial kind
    for (double s : {0.0, 1e-300, 3.25, 1e300}) CHECK(same_bits(ba_loss_rho(0, 2.0, 4.0, s), s) && same_bits(ba_loss_drho(0, 2.0, 4.0, s), 1.0) && same_bits(ba_loss_weight(0, 2.0, 4.0, s), 1.0), "trivial kind at %g", s);
    CHECK(!std::isfinite(ba_loss_rho(0, 2.0, 4.0, std::numeric_limits<double>::quiet_NaN())), "trivial rho(NaN)");
    if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
    printf("all cases pass (%ld points)\n", cases);
    return 0;
}
