// Square root in BLS12-381 Fp2 = Fp[u]/(u^2 + 1) and the y coordinate of a ZCash-compressed G2 point, shared by the gfx950 decoding
// kernel (decode.hip through point_decode.h, 32-bit limbs) and, through g++, by the CPU test build (tests/cpu_build/sqrt2_check.cpp).
//
// a = a0 + a1 u is a square in Fp2 exactly when its norm n = a0^2 + a1^2 is a square in Fp.  With s a root of n, one of
// d = (a0 + s) / 2 and d' = (a0 - s) / 2 is a square in Fp (d d' = -a1^2 / 4 and -1 is not a square: p = 3 mod 4), d + d' = a0, and
//     t^2 =  d:  (t + a1/(2t) u)^2 = d + d' + a1 u = a          t^2 = -d:  (a1/(2t) + t u)^2 = d' + d + a1 u = a
// Both Fp roots and the one inversion come out of ONE fixed chain w(z) = z^((p-3)/4):  z w = z^((p+1)/4) is the root candidate,
// z w^2 = z^((p-1)/2) = chi(z) is +-1 (0 for z = 0), and 1 / (z w) = chi(z) w.  So
//     s = n w(n)   (a is not a square iff s^2 != n)        t = d w(d),  chi = t w(d),  a1 / (2t) = chi a1 w(d) / 2
// With a1 = 0 the root s is +-a0 and d may come out 0; then d = a0 is taken (the formulas above hold with d' = 0), which also makes
// the argument 0 give 0.  The exponent is a constant of 379 bits walked in 4-bit windows from the top as fp_sqrt.h walks (p+1)/4:
// 14 products for the table, 376 squarings and 91 window products -- 481 field products per chain, no branch on data.  Per point:
// 2 (norm) + 481 + 2 (s, s^2) + 481 + 3 (t, chi, a1 w) = 969 products for the root; g2_y_from_x adds 5 for x^3 and 2 for the
// canonical form the sign rule reads: 976, against ~2 900 for the four generic square-and-multiply loops of the host function.
#pragma once
#include "fp_sqrt.h"

namespace vsp {

// a^((p-3)/4), a in Montgomery form.  One out-of-line copy in a kernel: the root calls it twice
template <class P> VSP_HD_CALL Mont<P> fp_pow_p_minus_3_over_4(const Mont<P> &a) {
    static_assert(P::N * sizeof(typename P::limb_t) == 48, "the exponent below is Fp's");
    const uint64_t e[6] = {0xee7fbfffffffeaaaULL, 0x07aaffffac54ffffULL, 0xd9cc34a83dac3d89ULL,      // (p - 3) / 4, little-endian words
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
// a / 2: the same limbs halve a canonical value and a Montgomery-form one
template <class P> VSP_HD Mont<P> fp_half(const Mont<P> &a) {
    using L = typename P::limb_t; using W = typename WideOf<L>::T;
    constexpr int N = P::N, LB = sizeof(L) * 8;
    const bool odd = (a.l[0] & 1) != 0;
    Mont<P> t; W c = 0;
    for (int i = 0; i < N; i++) { c += (W)a.l[i] + (odd ? P::MOD[i] : (L)0); t.l[i] = (L)c; c >>= LB; }      // a + p < 2^(bits): the spare top bit
    Mont<P> r;
    for (int i = 0; i < N; i++) r.l[i] = (L)(t.l[i] >> 1) | (i + 1 < N ? (L)(t.l[i + 1] << (LB - 1)) : (L)0);
    return r;
}
template <class P> VSP_HD Mont<P> fp_select(bool c, const Mont<P> &a, const Mont<P> &b) {
    Mont<P> r;
    for (int i = 0; i < P::N; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
// y = a square root of a (Montgomery form both); false exactly when a is not a square (y is then no root of anything).  sqrt(0) = 0.
template <class F> VSP_HD bool fp2_sqrt(const Fp2T<F> &a, Fp2T<F> &y) {
    const F n = add(sqr(a.c0), sqr(a.c1));
    const F s = mul(fp_pow_p_minus_3_over_4(n), n);
    const bool square = eq(sqr(s), n);
    F d = fp_half(add(a.c0, s));
    d = fp_select(is_zero(d), a.c0, d);
    const F w = fp_pow_p_minus_3_over_4(d);
    const F t = mul(w, d);
    const bool plus = eq(mul(t, w), F::one());                 // chi(d) = 1: t^2 = d; otherwise t^2 = -d (or d = 0: everything below is 0)
    const F o = fp_half(mul(a.c1, w));                         // chi a1 / (2t)
    y.c0 = fp_select(plus, t, neg(o));
    y.c1 = fp_select(plus, o, t);
    return square;
}
// a CANONICAL Fp2 value "larger" than its negation: its highest non-zero coefficient, c1 first and then c0, above (p - 1) / 2 -- the
// sign rule of the compressed encoding (flag 0x20) for G2
template <class F> VSP_HD bool fp2_canon_larger(const Fp2T<F> &canon) {
    return fp_canon_above_half(fp_select(is_zero(canon.c1), canon.c0, canon.c1));
}
// the y of the G2 point with abscissa x (Montgomery form) and sign flag `larger`: y^2 = x^3 + 4 (1 + u), y larger than -y iff
// larger.  false when x^3 + 4 (1 + u) is not a square (no such point).
template <class F> VSP_HD bool g2_y_from_x(const Fp2T<F> &x, bool larger, Fp2T<F> &y) {
    Fp2T<F> b; b.c0 = dbl(dbl(F::one())); b.c1 = b.c0;
    const bool on_curve = fp2_sqrt(add(mul(sqr(x), x), b), y);
    if (fp2_canon_larger(from_mont(y)) != larger) y = neg(y);
    return on_curve;
}

}  // namespace vsp
