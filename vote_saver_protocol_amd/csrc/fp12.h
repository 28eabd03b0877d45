// The tower over BLS12-381 Fp2 up to Fp12, shared by the gfx950 pairing kernels (pairing.hip, 32-bit limbs) and, through g++, by the
// CPU test build (tests/cpu_build/pairing_check.cpp, both limb types).
//
//     Fp2 = Fp[u] / (u^2 + 1)          Fp6 = Fp2[v] / (v^3 - xi),  xi = 1 + u          Fp12 = Fp6[w] / (w^2 - v)
//
// An Fp12T<F> is twelve F in memory, the coefficient of u^i v^j w^k at index (k * 3 + j) * 2 + i: the order of the 576-byte GT
// encoding (wire.hip, the test oracle's gt_to_tower_le).  Everything is in Montgomery form; no function branches or indexes memory on
// data.  Field products per operation (an Fp2 product is 3, an Fp2 square 2):
//     fp6 mul 18      fp12 mul 54      fp12 sqr 36      sparse line product 39      cyclotomic sqr 18      frobenius p: 15, p^2: 10
//     fp12 inv: 2 fp6 squares-as-products + fp6 inv (33 + 4) + 2 fp6 products, and ONE Fp inversion (a^(p-2) through the fixed chain of fp2_sqrt.h, 484)
// The products that a kernel calls many times are out-of-line (VSP_HD_CALL) and work on memory operands: an Fp12 value is 144 32-bit
// registers, so a lane keeps its tower values in scratch and only the Fp2 level lives in registers.
#pragma once
#include "fp2_sqrt.h"

namespace vsp {

template <class F> struct alignas(16) Fp6T {
    Fp2T<F> c0, c1, c2;
    VSP_HD static Fp6T zero() { Fp6T r; r.c0 = Fp2T<F>::zero(); r.c1 = r.c0; r.c2 = r.c0; return r; }
    VSP_HD static Fp6T one() { Fp6T r; r.c0 = Fp2T<F>::one(); r.c1 = Fp2T<F>::zero(); r.c2 = r.c1; return r; }
};
template <class F> struct alignas(16) Fp12T {
    Fp6T<F> c0, c1;
    VSP_HD static Fp12T zero() { Fp12T r; r.c0 = Fp6T<F>::zero(); r.c1 = r.c0; return r; }
    VSP_HD static Fp12T one() { Fp12T r; r.c0 = Fp6T<F>::one(); r.c1 = Fp6T<F>::zero(); return r; }
};

// a 384-bit constant given as six little-endian 64-bit words, as an element of either limb width (the Montgomery radix is 2^384 for both)
template <class F> VSP_HD F fp_from_words(const uint64_t *w) {
    using L = typename F::L;
    constexpr int LB = sizeof(L) * 8, PER = 64 / LB;
    F r;
    for (int i = 0; i < F::N; i++) r.l[i] = (L)(w[i / PER] >> ((i % PER) * LB));
    return r;
}
// 1 / a = a^(p-2) = (a^((p-3)/4))^4 a; 0 -> 0
template <class P> VSP_HD Mont<P> fp_inv_chain(const Mont<P> &a) { return mul(sqr(sqr(fp_pow_p_minus_3_over_4(a))), a); }

// ---------------------------------------------------------------- Fp2: the out-of-line products, xi, conjugation
template <class F> VSP_HD_CALL Fp2T<F> f2mul(const Fp2T<F> &a, const Fp2T<F> &b) { return mul(a, b); }
template <class F> VSP_HD_CALL Fp2T<F> f2sqr(const Fp2T<F> &a) { return sqr(a); }
template <class F> VSP_HD Fp2T<F> mul_xi(const Fp2T<F> &a) { Fp2T<F> r; r.c0 = sub(a.c0, a.c1); r.c1 = add(a.c0, a.c1); return r; }    // a (1 + u)
template <class F> VSP_HD Fp2T<F> conj(const Fp2T<F> &a) { Fp2T<F> r; r.c0 = a.c0; r.c1 = neg(a.c1); return r; }
template <class F> VSP_HD Fp2T<F> mul_fp(const Fp2T<F> &a, const F &k) { Fp2T<F> r; r.c0 = mul(a.c0, k); r.c1 = mul(a.c1, k); return r; }
template <class F> VSP_HD Fp2T<F> f2half(const Fp2T<F> &a) { Fp2T<F> r; r.c0 = fp_half(a.c0); r.c1 = fp_half(a.c1); return r; }
template <class F> VSP_HD Fp2T<F> f2inv(const Fp2T<F> &a) {
    const F n = fp_inv_chain(add(sqr(a.c0), sqr(a.c1)));
    Fp2T<F> r; r.c0 = mul(a.c0, n); r.c1 = neg(mul(a.c1, n)); return r;
}

// ---------------------------------------------------------------- Fp6
template <class F> VSP_HD bool is_zero(const Fp6T<F> &a) { return is_zero(a.c0) && is_zero(a.c1) && is_zero(a.c2); }
template <class F> VSP_HD bool eq(const Fp6T<F> &a, const Fp6T<F> &b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1) && eq(a.c2, b.c2); }
template <class F> VSP_HD Fp6T<F> add(const Fp6T<F> &a, const Fp6T<F> &b) { Fp6T<F> r; r.c0 = add(a.c0, b.c0); r.c1 = add(a.c1, b.c1); r.c2 = add(a.c2, b.c2); return r; }
template <class F> VSP_HD Fp6T<F> sub(const Fp6T<F> &a, const Fp6T<F> &b) { Fp6T<F> r; r.c0 = sub(a.c0, b.c0); r.c1 = sub(a.c1, b.c1); r.c2 = sub(a.c2, b.c2); return r; }
template <class F> VSP_HD Fp6T<F> neg(const Fp6T<F> &a) { Fp6T<F> r; r.c0 = neg(a.c0); r.c1 = neg(a.c1); r.c2 = neg(a.c2); return r; }
template <class F> VSP_HD Fp6T<F> mul_v(const Fp6T<F> &a) { Fp6T<F> r; r.c0 = mul_xi(a.c2); r.c1 = a.c0; r.c2 = a.c1; return r; }            // a v
// Karatsuba over the three coefficients: 6 Fp2 products
template <class F> VSP_HD_CALL Fp6T<F> mul(const Fp6T<F> &a, const Fp6T<F> &b) {
    const Fp2T<F> t0 = f2mul(a.c0, b.c0), t1 = f2mul(a.c1, b.c1), t2 = f2mul(a.c2, b.c2);
    Fp6T<F> r;
    r.c0 = add(t0, mul_xi(sub(sub(f2mul(add(a.c1, a.c2), add(b.c1, b.c2)), t1), t2)));
    r.c1 = add(sub(sub(f2mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1), mul_xi(t2));
    r.c2 = add(sub(sub(f2mul(add(a.c0, a.c2), add(b.c0, b.c2)), t0), t2), t1);
    return r;
}
// a (b0 + b1 v): 5 Fp2 products
template <class F> VSP_HD_CALL Fp6T<F> mul_by_01(const Fp6T<F> &a, const Fp2T<F> &b0, const Fp2T<F> &b1) {
    const Fp2T<F> t0 = f2mul(a.c0, b0), t1 = f2mul(a.c1, b1);
    Fp6T<F> r;
    r.c0 = add(t0, mul_xi(f2mul(a.c2, b1)));
    r.c1 = sub(sub(f2mul(add(a.c0, a.c1), add(b0, b1)), t0), t1);
    r.c2 = add(f2mul(a.c2, b0), t1);
    return r;
}
// a (b1 v): 3 Fp2 products
template <class F> VSP_HD_CALL Fp6T<F> mul_by_1(const Fp6T<F> &a, const Fp2T<F> &b1) {
    Fp6T<F> r;
    r.c0 = mul_xi(f2mul(a.c2, b1)); r.c1 = f2mul(a.c0, b1); r.c2 = f2mul(a.c1, b1);
    return r;
}
// 1 / a; 0 -> 0.  9 products, 3 squares, one Fp2 inversion
template <class F> VSP_HD_CALL Fp6T<F> inv(const Fp6T<F> &a) {
    const Fp2T<F> t0 = sub(f2sqr(a.c0), mul_xi(f2mul(a.c1, a.c2)));
    const Fp2T<F> t1 = sub(mul_xi(f2sqr(a.c2)), f2mul(a.c0, a.c1));
    const Fp2T<F> t2 = sub(f2sqr(a.c1), f2mul(a.c0, a.c2));
    const Fp2T<F> d = f2inv(add(f2mul(a.c0, t0), mul_xi(add(f2mul(a.c2, t1), f2mul(a.c1, t2)))));
    Fp6T<F> r; r.c0 = f2mul(t0, d); r.c1 = f2mul(t1, d); r.c2 = f2mul(t2, d); return r;
}

// ---------------------------------------------------------------- Fp12
template <class F> VSP_HD bool eq(const Fp12T<F> &a, const Fp12T<F> &b) { return eq(a.c0, b.c0) && eq(a.c1, b.c1); }
template <class F> VSP_HD bool is_one(const Fp12T<F> &a) { return eq(a.c0.c0, Fp2T<F>::one()) && is_zero(a.c0.c1) && is_zero(a.c0.c2) && is_zero(a.c1); }
template <class F> VSP_HD Fp12T<F> add(const Fp12T<F> &a, const Fp12T<F> &b) { Fp12T<F> r; r.c0 = add(a.c0, b.c0); r.c1 = add(a.c1, b.c1); return r; }
template <class F> VSP_HD Fp12T<F> sub(const Fp12T<F> &a, const Fp12T<F> &b) { Fp12T<F> r; r.c0 = sub(a.c0, b.c0); r.c1 = sub(a.c1, b.c1); return r; }
// a^(p^6): w -> -w.  The inverse of a value of norm one over Fp6 (everything after the easy part of the final exponentiation)
template <class F> VSP_HD Fp12T<F> conj(const Fp12T<F> &a) { Fp12T<F> r; r.c0 = a.c0; r.c1 = neg(a.c1); return r; }
template <class F> VSP_HD_CALL Fp12T<F> mul(const Fp12T<F> &a, const Fp12T<F> &b) {
    const Fp6T<F> t0 = mul(a.c0, b.c0), t1 = mul(a.c1, b.c1);
    Fp12T<F> r;
    r.c1 = sub(sub(mul(add(a.c0, a.c1), add(b.c0, b.c1)), t0), t1);
    r.c0 = add(t0, mul_v(t1));
    return r;
}
template <class F> VSP_HD_CALL Fp12T<F> sqr(const Fp12T<F> &a) {
    const Fp6T<F> ab = mul(a.c0, a.c1);
    Fp12T<F> r;
    r.c0 = sub(sub(mul(add(a.c0, a.c1), add(a.c0, mul_v(a.c1))), ab), mul_v(ab));
    r.c1 = add(ab, ab);
    return r;
}
// a (l0 + l1 v + l4 v w), the shape of a line value (pairing.h): 13 Fp2 products against 18
template <class F> VSP_HD_CALL Fp12T<F> mul_by_014(const Fp12T<F> &a, const Fp2T<F> &l0, const Fp2T<F> &l1, const Fp2T<F> &l4) {
    const Fp6T<F> t0 = mul_by_01(a.c0, l0, l1), t1 = mul_by_1(a.c1, l4);
    Fp12T<F> r;
    r.c1 = sub(sub(mul_by_01(add(a.c0, a.c1), l0, add(l1, l4)), t0), t1);
    r.c0 = add(t0, mul_v(t1));
    return r;
}
// 1 / a; 0 -> 0
template <class F> VSP_HD_CALL Fp12T<F> inv(const Fp12T<F> &a) {
    const Fp6T<F> d = inv(sub(mul(a.c0, a.c0), mul_v(mul(a.c1, a.c1))));
    Fp12T<F> r; r.c0 = mul(a.c0, d); r.c1 = neg(mul(a.c1, d)); return r;
}

// Frobenius: u^p = -u, and w^p = w gamma with gamma = xi^((p-1)/6), so the coefficient of v^j w^k = w^(2j+k) is conjugated and
// multiplied by gamma^(2j+k).  For p^2 there is no conjugation and gamma2 = xi^((p^2-1)/6) is a sixth root of unity in Fp.
// Constants in Montgomery form, little-endian 64-bit words.
template <class F> VSP_HD_CALL Fp12T<F> frobenius(const Fp12T<F> &a) {
    const uint64_t g[5][2][6] = {      // gamma^1 .. gamma^5 as c0, c1
        {{0x07089552b319d465ULL, 0xc6695f92b50a8313ULL, 0x97e83cccd117228fULL, 0xa35baecab2dc29eeULL, 0x1ce393ea5daace4dULL, 0x08f2220fb0fb66ebULL},
         {0xb2f66aad4ce5d646ULL, 0x5842a06bfc497cecULL, 0xcf4895d42599d394ULL, 0xc11b9cba40a8e8d0ULL, 0x2e3813cbe5a0de89ULL, 0x110eefda88847fafULL}},
        {{0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL},
         {0xcd03c9e48671f071ULL, 0x5dab22461fcda5d2ULL, 0x587042afd3851b95ULL, 0x8eb60ebe01bacb9eULL, 0x03f97d6e83d050d2ULL, 0x18f0206554638741ULL}},
        {{0x7bcfa7a25aa30fdaULL, 0xdc17dec12a927e7cULL, 0x2f088dd86b4ebef1ULL, 0xd1ca2087da74d4a7ULL, 0x2da2596696cebc1dULL, 0x0e2b7eedbbfd87d2ULL},
         {0x7bcfa7a25aa30fdaULL, 0xdc17dec12a927e7cULL, 0x2f088dd86b4ebef1ULL, 0xd1ca2087da74d4a7ULL, 0x2da2596696cebc1dULL, 0x0e2b7eedbbfd87d2ULL}},
        {{0x890dc9e4867545c3ULL, 0x2af322533285a5d5ULL, 0x50880866309b7e2cULL, 0xa20d1b8c7e881024ULL, 0x14e4f04fe2db9068ULL, 0x14e56d3f1564853aULL},
         {0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL, 0x0000000000000000ULL}},
        {{0x82d83cf50dbce43fULL, 0xa2813e53df9d018fULL, 0xc6f0caa53c65e181ULL, 0x7525cf528d50fe95ULL, 0x4a85ed50f4798a6bULL, 0x171da0fd6cf8eebdULL},
         {0x3726c30af242c66cULL, 0x7c2ac1aad1b6fe70ULL, 0xa04007fbba4b14a2ULL, 0xef517c3266341429ULL, 0x0095ba654ed2226bULL, 0x02e370eccc86f7ddULL}}};
    Fp2T<F> gk[5];
    for (int k = 0; k < 5; k++) { gk[k].c0 = fp_from_words<F>(g[k][0]); gk[k].c1 = fp_from_words<F>(g[k][1]); }
    Fp12T<F> r;
    r.c0.c0 = conj(a.c0.c0);
    r.c1.c0 = f2mul(conj(a.c1.c0), gk[0]);
    r.c0.c1 = f2mul(conj(a.c0.c1), gk[1]);
    r.c1.c1 = f2mul(conj(a.c1.c1), gk[2]);
    r.c0.c2 = f2mul(conj(a.c0.c2), gk[3]);
    r.c1.c2 = f2mul(conj(a.c1.c2), gk[4]);
    return r;
}
template <class F> VSP_HD_CALL Fp12T<F> frobenius2(const Fp12T<F> &a) {
    const uint64_t g[5][6] = {         // gamma2^1 .. gamma2^5
        {0xecfb361b798dba3aULL, 0xc100ddb891865a2cULL, 0x0ec08ff1232bda8eULL, 0xd5c13cc6f1ca4721ULL, 0x47222a47bf7b5c04ULL, 0x0110f184e51c5f59ULL},
        {0x30f1361b798a64e8ULL, 0xf3b8ddab7ece5a2aULL, 0x16a8ca3ac61577f7ULL, 0xc26a2ff874fd029bULL, 0x3636b76660701c6eULL, 0x051ba4ab241b6160ULL},
        {0x43f5fffffffcaaaeULL, 0x32b7fff2ed47fffdULL, 0x07e83a49a2e99d69ULL, 0xeca8f3318332bb7aULL, 0xef148d1ea0f4c069ULL, 0x040ab3263eff0206ULL},
        {0xcd03c9e48671f071ULL, 0x5dab22461fcda5d2ULL, 0x587042afd3851b95ULL, 0x8eb60ebe01bacb9eULL, 0x03f97d6e83d050d2ULL, 0x18f0206554638741ULL},
        {0x890dc9e4867545c3ULL, 0x2af322533285a5d5ULL, 0x50880866309b7e2cULL, 0xa20d1b8c7e881024ULL, 0x14e4f04fe2db9068ULL, 0x14e56d3f1564853aULL}};
    Fp12T<F> r;
    r.c0.c0 = a.c0.c0;
    r.c1.c0 = mul_fp(a.c1.c0, fp_from_words<F>(g[0]));
    r.c0.c1 = mul_fp(a.c0.c1, fp_from_words<F>(g[1]));
    r.c1.c1 = mul_fp(a.c1.c1, fp_from_words<F>(g[2]));
    r.c0.c2 = mul_fp(a.c0.c2, fp_from_words<F>(g[3]));
    r.c1.c2 = mul_fp(a.c1.c2, fp_from_words<F>(g[4]));
    return r;
}

// (a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi): 3 Fp2 squares
template <class F> VSP_HD void fp4_sqr(const Fp2T<F> &a, const Fp2T<F> &b, Fp2T<F> &c0, Fp2T<F> &c1) {
    const Fp2T<F> t0 = f2sqr(a), t1 = f2sqr(b);
    c0 = add(mul_xi(t1), t0);
    c1 = sub(sub(f2sqr(add(a, b)), t0), t1);
}
// a^2 for a in the cyclotomic subgroup (a^(p^6+1) = 1 and a^(p^4-p^2+1) = 1: everything after the easy part of the final
// exponentiation), Granger-Scott: three Fp4 squares, 18 field products against 36.  NOT a square of a general value.
template <class F> VSP_HD_CALL Fp12T<F> cyclotomic_sqr(const Fp12T<F> &a) {
    Fp2T<F> z0 = a.c0.c0, z4 = a.c0.c1, z3 = a.c0.c2, z2 = a.c1.c0, z1 = a.c1.c1, z5 = a.c1.c2, t0, t1, t2, t3;
    fp4_sqr(z0, z1, t0, t1);
    z0 = add(dbl(sub(t0, z0)), t0);
    z1 = add(dbl(add(t1, z1)), t1);
    fp4_sqr(z2, z3, t0, t1);
    fp4_sqr(z4, z5, t2, t3);
    z4 = add(dbl(sub(t0, z4)), t0);
    z5 = add(dbl(add(t1, z5)), t1);
    t0 = mul_xi(t3);
    z2 = add(dbl(add(t0, z2)), t0);
    z3 = add(dbl(sub(t2, z3)), t2);
    Fp12T<F> r;
    r.c0.c0 = z0; r.c0.c1 = z4; r.c0.c2 = z3; r.c1.c0 = z2; r.c1.c1 = z1; r.c1.c2 = z5;
    return r;
}

template <class F> VSP_HD Fp12T<F> to_mont(const Fp12T<F> &a) {
    Fp12T<F> r;
    r.c0.c0 = to_mont(a.c0.c0); r.c0.c1 = to_mont(a.c0.c1); r.c0.c2 = to_mont(a.c0.c2);
    r.c1.c0 = to_mont(a.c1.c0); r.c1.c1 = to_mont(a.c1.c1); r.c1.c2 = to_mont(a.c1.c2);
    return r;
}
template <class F> VSP_HD Fp12T<F> from_mont(const Fp12T<F> &a) {
    Fp12T<F> r;
    r.c0.c0 = from_mont(a.c0.c0); r.c0.c1 = from_mont(a.c0.c1); r.c0.c2 = from_mont(a.c0.c2);
    r.c1.c0 = from_mont(a.c1.c0); r.c1.c1 = from_mont(a.c1.c1); r.c1.c2 = from_mont(a.c1.c2);
    return r;
}

using Fp6 = Fp6T<Fp>;
using Fp12 = Fp12T<Fp>;
using HFp12 = Fp12T<HFp>;

}  // namespace vsp
