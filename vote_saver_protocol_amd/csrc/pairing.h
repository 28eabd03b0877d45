// The optimal ate pairing on BLS12-381, shared by the gfx950 pairing kernels (pairing.hip, 32-bit limbs) and, through g++, by the CPU
// test build (tests/cpu_build/pairing_check.cpp, both limb types).
//
//     e(P, Q) = f_{|x|, Q}(P) ^ ((p^12 - 1) / r),   |x| = 0xd201000000010000,   P in G1,  Q in G2 (on the twist y^2 = x^3 + 4 (1 + u))
//
// CONVENTION.  The curve parameter x is negative, and the usual definition conjugates the Miller value for it (f_{x,Q} = 1 / f_{|x|,Q}
// up to factors the exponentiation removes).  This library does NOT: it computes the pairing of the test oracle (pairing.py), whose miller_loop
// walks |x| and whose final_exp raises to (p^12 - 1) / r -- the inverse of the value of libraries that conjugate.  Bilinearity and
// every product-is-one test are the same under either convention; the 576 bytes of a GT element are not.
// Miller values differ between implementations by factors from proper subfields (the projective line scaling below); only values after
// the final exponentiation are comparable.
//
// Miller loop.  Q is untwisted by (x, y) -> (x / w^2, y / w^3); the line through untwisted points with slope m' / w (m' the slope on
// the twist), evaluated at P = (xP, yP) and multiplied by w^3 (an element of Fp4, removed by the final exponentiation), is
//     l = (yT - m' xT) + m' xP v - yP v w                                      (v = w^2, v w = w^3)
// a value with three non-zero Fp2 coefficients of twelve (mul_by_014).  T runs in homogeneous projective coordinates (X : Y : Z),
// x = X / Z, y = Y / Z, so m' has a denominator in Fp2 that the line is multiplied through by: no inversion in the loop.
//   doubling (Costello-Lange-Naehrig), b' = 4 (1 + u):
//     A = X Y / 2, B = Y^2, C = Z^2, E = 3 b' C, F = 3 E, G = (B + F) / 2, H = (Y + Z)^2 - (B + C), J = X^2
//     X3 = A (B - F),  Y3 = G^2 - 3 E^2,  Z3 = B H          l = (E - B) + 3 J xP v - H yP v w            3 products + 6 squares + 4
//   mixed addition of the affine Q = (x2, y2):
//     th = Y - y2 Z, la = X - x2 Z, c = th^2, d = la^2, e = la d, f = Z c, g = X d, h = e + f - 2 g
//     X3 = la h,  Y3 = th (g - h) - e Y,  Z3 = Z e          l = (th x2 - la y2) - th xP v + la yP v w    11 products + 2 squares + 4
// 63 doublings and 5 additions (the set bits of |x| below the top one); per step an Fp12 square (36) and a line product (39).
//     field products: 63 (36 + 39 + 25) + 5 (39 + 41) = 6 700
//
// Final exponentiation.  Easy part f^((p^6 - 1)(p^2 + 1)): one Fp12 inversion, one conjugation, one Frobenius p^2, two products.
// Hard part, the EXACT exponent (p^4 - p^2 + 1) / r = (x - 1)^2 / 3 (x + p)(x^2 + p^2 - 1) + 1 (Hayashida-Hayasaka-Teruya), not a
// multiple of it: 3 divides x - 1, so with n = |x| and inverses by conjugation (the value is in the cyclotomic subgroup)
//     a = f^((n + 1) / 3),  b = a^(n + 1)              = f^((x - 1)^2 / 3)
//     c = b^p conj(b^n)                                = b^(x + p)
//     d = (c^n)^n c^(p^2) conj(c)                      = c^(x^2 + p^2 - 1)            result = d f
// five exponentiations by 62..64-bit constants with cyclotomic squares (18): 4 x (63 squares + 5 products) by n and 62 squares + 27
// products by (n + 1) / 3 = 0x460055555555aaab.
//     field products: 314 x 18 + (47 + 7) x 54 + 15 + 2 x 10 + 593 (the inversion: 4 Fp6 products, 33, and 488 for the one in Fp2) = 9 196
// 15 896 field products per pairing; a product of m pairings shares one final exponentiation.
#pragma once
#include "fp12.h"
#include "curve.h"

namespace vsp {

static constexpr uint64_t BLS_X_ABS = 0xd201000000010000ULL;          // |x|
static constexpr uint64_t BLS_X_ABS_PLUS_1_OVER_3 = 0x460055555555aaabULL;

template <class F> struct alignas(16) G2Proj { Fp2T<F> X, Y, Z; };

// The three Fp2 values of a line before xP and yP are multiplied in.  Doubling: a = E - B, b = 3 J, c = H, the line is
// a + b xP v - c yP v w.  Addition: a = j, b = th, c = la, the line is a - b xP v + c yP v w.  They depend on Q alone.
template <class F> struct alignas(16) LineCoeffs { Fp2T<F> a, b, c; };
static constexpr int MILLER_LINES = 68;                               // 63 doublings + 5 additions, in loop order

// T = 2 T and the coefficients of l_{T,T}
template <class F> VSP_HD_CALL void line_double(G2Proj<F> &T, LineCoeffs<F> &l) {
    const Fp2T<F> A = f2half(f2mul(T.X, T.Y)), B = f2sqr(T.Y), C = f2sqr(T.Z);
    const Fp2T<F> C4 = dbl(dbl(C)), bC = mul_xi(C4);                 // b' C = 4 (1 + u) C
    const Fp2T<F> E = add(dbl(bC), bC), Fv = add(dbl(E), E);
    const Fp2T<F> G = f2half(add(B, Fv)), H = sub(f2sqr(add(T.Y, T.Z)), add(B, C)), J = f2sqr(T.X);
    const Fp2T<F> E2 = f2sqr(E);
    T.X = f2mul(A, sub(B, Fv));
    T.Y = sub(f2sqr(G), add(dbl(E2), E2));
    T.Z = f2mul(B, H);
    l.a = sub(E, B); l.b = add(dbl(J), J); l.c = H;
}
// the coefficients of l_{T,Q} and T = T + Q.  T = +-Q does not occur for points of order r (the multiples of Q met are below |x| < r)
template <class F> VSP_HD_CALL void line_add(G2Proj<F> &T, const Affine<Fp2T<F>> &Q, LineCoeffs<F> &l) {
    const Fp2T<F> th = sub(T.Y, f2mul(Q.y, T.Z)), la = sub(T.X, f2mul(Q.x, T.Z));
    const Fp2T<F> c = f2sqr(th), d = f2sqr(la), e = f2mul(la, d), ff = f2mul(T.Z, c), g = f2mul(T.X, d);
    const Fp2T<F> h = sub(add(e, ff), dbl(g));
    l.a = sub(f2mul(th, Q.x), f2mul(la, Q.y));
    T.X = f2mul(la, h);
    T.Y = sub(f2mul(th, sub(g, h)), f2mul(e, T.Y));
    T.Z = f2mul(T.Z, e);
    l.b = th; l.c = la;
}
// f = f l for the line of a doubling / of an addition, evaluated at P = (xP, yP)
template <class F> VSP_HD void mul_line_double(Fp12T<F> &f, const LineCoeffs<F> &l, const F &xP, const F &yP) { f = mul_by_014(f, l.a, mul_fp(l.b, xP), neg(mul_fp(l.c, yP))); }
template <class F> VSP_HD void mul_line_add(Fp12T<F> &f, const LineCoeffs<F> &l, const F &xP, const F &yP) { f = mul_by_014(f, l.a, neg(mul_fp(l.b, xP)), mul_fp(l.c, yP)); }

// T = 2 T; f = f^2 l_{T,T}(P)
template <class F> VSP_HD_CALL void miller_double(Fp12T<F> &f, G2Proj<F> &T, const F &xP, const F &yP) {
    LineCoeffs<F> l;
    line_double(T, l);
    f = sqr(f);
    mul_line_double(f, l, xP, yP);
}
// f = f l_{T,Q}(P); T = T + Q
template <class F> VSP_HD_CALL void miller_add(Fp12T<F> &f, G2Proj<F> &T, const Affine<Fp2T<F>> &Q, const F &xP, const F &yP) {
    LineCoeffs<F> l;
    line_add(T, Q, l);
    mul_line_add(f, l, xP, yP);
}
// f_{|x|,Q}(P), P and Q affine in Montgomery form; one when either is infinity (x = y = 0).  No conjugation: see CONVENTION
template <class F> VSP_HD Fp12T<F> miller_loop(const Affine<F> &P, const Affine<Fp2T<F>> &Q) {
    Fp12T<F> f = Fp12T<F>::one();
    if (is_inf(P) || is_inf(Q)) return f;
    G2Proj<F> T; T.X = Q.x; T.Y = Q.y; T.Z = Fp2T<F>::one();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 62; i >= 0; i--) {
        miller_double(f, T, P.x, P.y);
        if ((BLS_X_ABS >> i) & 1) miller_add(f, T, Q, P.x, P.y);
    }
    return f;
}

// PREPARED ARGUMENTS.  The point arithmetic of the loop depends on Q alone: for a Q that is fixed (a key member) the 68 coefficient
// triples are computed once -- 68 x 3 x 96 = 19 584 bytes in Montgomery form -- and a pair with such a Q costs per step only the two
// products by xP, yP and the line product: 63 (4 + 39) + 5 (4 + 39) = 2 924 field products plus its share of the squarings.
// Q = infinity prepares to lines that are one (a = 1, b = c = 0): the pair contributes one.
template <class F> VSP_HD void prepare_g2(const Affine<Fp2T<F>> &Q, LineCoeffs<F> *out /* MILLER_LINES */) {
    if (is_inf(Q)) {
        for (int s = 0; s < MILLER_LINES; s++) { out[s].a = Fp2T<F>::one(); out[s].b = Fp2T<F>::zero(); out[s].c = Fp2T<F>::zero(); }
        return;
    }
    G2Proj<F> T; T.X = Q.x; T.Y = Q.y; T.Z = Fp2T<F>::one();
    int s = 0;
    for (int i = 62; i >= 0; i--) {
        line_double(T, out[s++]);
        if ((BLS_X_ABS >> i) & 1) line_add(T, Q, out[s++]);
    }
}
// The Miller value of a product of pairs with ONE squaring per step: (f1 f2)^2 l1 l2 = f1^2 l1 f2^2 l2, so the result is the product of
// the miller_loop values of the pairs, coefficient for coefficient.  g pairs with prepared arguments: pair j is P[j * p_stride] with the
// lines at lines[j * MILLER_LINES]; and, when Qv is not null, one more pair (*Pv, *Qv) whose point arithmetic runs here (more than one
// variable argument would want their T in an array: no caller has two).  A pair whose P is infinity contributes nothing, as does a
// variable pair whose Q is.
template <class F> VSP_HD Fp12T<F> miller_multi(const Affine<F> *P, size_t p_stride, const LineCoeffs<F> *lines, size_t g, const Affine<F> *Pv,
                                                const Affine<Fp2T<F>> *Qv) {
    Fp12T<F> f = Fp12T<F>::one();
    const bool var = Qv && !is_inf(*Pv) && !is_inf(*Qv);
    G2Proj<F> T;
    if (var) { T.X = Qv->x; T.Y = Qv->y; T.Z = Fp2T<F>::one(); }
    int s = 0;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = 62; i >= 0; i--) {
        const bool bit = (BLS_X_ABS >> i) & 1;
        f = sqr(f);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (size_t j = 0; j < g; j++) {
            const Affine<F> Pj = P[j * p_stride];
            if (is_inf(Pj)) continue;
            mul_line_double(f, lines[j * MILLER_LINES + s], Pj.x, Pj.y);
            if (bit) mul_line_add(f, lines[j * MILLER_LINES + s + 1], Pj.x, Pj.y);
        }
        if (var) {
            LineCoeffs<F> l;
            line_double(T, l);
            mul_line_double(f, l, Pv->x, Pv->y);
            if (bit) { line_add(T, *Qv, l); mul_line_add(f, l, Pv->x, Pv->y); }
        }
        s += bit ? 2 : 1;
    }
    return f;
}

// a^e for a in the cyclotomic subgroup, e a constant with its top bit at `top`
template <class F> VSP_HD_CALL Fp12T<F> cyclotomic_pow(const Fp12T<F> &a, uint64_t e, int top) {
    Fp12T<F> r = a;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = top - 1; i >= 0; i--) {
        r = cyclotomic_sqr(r);
        if ((e >> i) & 1) r = mul(r, a);
    }
    return r;
}
// f^((p^12 - 1) / r); f = 0 gives 0
template <class F> VSP_HD Fp12T<F> final_exp(const Fp12T<F> &f) {
    Fp12T<F> t = mul(conj(f), inv(f));                               // f^(p^6 - 1)
    t = mul(frobenius2(t), t);                                       // ^(p^2 + 1): in the cyclotomic subgroup from here on
    const Fp12T<F> a = cyclotomic_pow(t, BLS_X_ABS_PLUS_1_OVER_3, 62);
    const Fp12T<F> b = mul(cyclotomic_pow(a, BLS_X_ABS, 63), a);
    const Fp12T<F> c = mul(frobenius(b), conj(cyclotomic_pow(b, BLS_X_ABS, 63)));
    const Fp12T<F> cn = cyclotomic_pow(cyclotomic_pow(c, BLS_X_ABS, 63), BLS_X_ABS, 63);
    const Fp12T<F> d = mul(mul(cn, frobenius2(c)), conj(c));
    return mul(d, t);
}
// e(P, Q)
template <class F> VSP_HD Fp12T<F> pairing(const Affine<F> &P, const Affine<Fp2T<F>> &Q) { return final_exp(miller_loop(P, Q)); }

}  // namespace vsp
