// Square root in BLS12-381 Fp and the y coordinate of a ZCash-compressed G1 point, shared by the gfx950 decoding kernel
// (decode.hip through point_decode.h, 32-bit limbs) and, through g++, by the CPU test build (tests/cpu_build/sqrt_check.cpp).
//
// p = 3 (mod 4), so a^((p+1)/4) is a square root of a whenever a is a square; whether it is one is read off the result:
// y^2 = a.  The exponent is a constant of 379 bits and is walked in 4-bit windows from the top: 14 products for the table
// a^2 .. a^15, then 4 squarings and at most one product per window -- 376 squarings and 91 window products, 481 field products
// in all against ~570 for the bit-by-bit loop.  Which windows multiply depends on the exponent alone: no branch on data.
#pragma once
#include "field.h"

namespace vsp {

// a^((p+1)/4), a in Montgomery form
template <class P> VSP_HD Mont<P> fp_pow_sqrt_exponent(const Mont<P> &a) {
    static_assert(P::N * sizeof(typename P::limb_t) == 48, "the exponent below is Fp's");
    const uint64_t e[6] = {0xee7fbfffffffeaabULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL,      // (p + 1) / 4, little-endian words
                           0xd91dd2e13ce144afULL, 0x92c6e9ed90d2eb35ULL, 0x0680447a8e5ff9a6ULL};
    Mont<P> tab[16];
    tab[0] = Mont<P>::one(); tab[1] = a;
    for (int d = 2; d < 16; d++) tab[d] = mul(tab[d - 1], a);
    Mont<P> acc = tab[(e[5] >> 56) & 15];                      // window 94, the highest non-zero one (6)
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int w = 93; w >= 0; w--) {
        acc = sqr(sqr(sqr(sqr(acc))));
        const unsigned d = (unsigned)(e[w >> 4] >> ((w & 15) * 4)) & 15u;
        if (d) acc = mul(acc, tab[d]);
    }
    return acc;
}
// y = a square root of a (Montgomery form both); false when a is not a square (y is then a root of -a).  sqrt(0) = 0.
template <class P> VSP_HD bool fp_sqrt(const Mont<P> &a, Mont<P> &y) {
    y = fp_pow_sqrt_exponent(a);
    return eq(sqr(y), a);
}
// a CANONICAL value above (p - 1) / 2: the "y is the larger of y and -y" rule of the compressed encoding (flag 0x20)
template <class P> VSP_HD bool fp_canon_above_half(const Mont<P> &canon) {
    using L = typename P::limb_t;
    constexpr int LB = sizeof(L) * 8, PER = 64 / LB;
    const uint64_t half[6] = {0xdcff7fffffffd555ULL, 0x0f55ffff58a9ffffULL, 0xb39869507b587b12ULL,   // (p - 1) / 2
                              0xb23ba5c279c2895fULL, 0x258dd3db21a5d66bULL, 0x0d0088f51cbff34dULL};
    bool lt = false, gt = false;
    for (int i = P::N - 1; i >= 0; i--) {
        const L h = (L)(half[i / PER] >> ((i % PER) * LB));
        gt = gt || (!lt && canon.l[i] > h);
        lt = lt || (!gt && canon.l[i] < h);
    }
    return gt;
}
// the y of the G1 point with abscissa x (Montgomery form) and sign flag `larger`: y^2 = x^3 + 4, y > (p - 1) / 2 iff larger.
// false when x^3 + 4 is not a square (no such point).
template <class P> VSP_HD bool g1_y_from_x(const Mont<P> &x, bool larger, Mont<P> &y) {
    const Mont<P> four = dbl(dbl(Mont<P>::one()));
    const Mont<P> rhs = add(mul(sqr(x), x), four);
    const bool on_curve = fp_sqrt(rhs, y);
    if (fp_canon_above_half(from_mont(y)) != larger) y = neg(y);
    return on_curve;
}

}  // namespace vsp
