// CPU test build of the prepared G2 arguments and the shared-squaring Miller loop (pairing.h prepare_g2, miller_multi, compiled by g++
// with the 32-bit-limb type the pairing kernels use and with the host's 64-bit-limb type).  Test infrastructure only.  All arguments
// canonical little-endian u64 limbs: an Fp12 value is 72 words in tower order, a G1 point x | y (12 words), a G2 point x.c0 | x.c1 |
// y.c0 | y.c1 (24 words), all zero = infinity; a line triple is a | b | c (36 words).
// With -DPREPARED_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_prepared_pairing_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/pairing.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }
template <class F> static Affine<F> load_g1(const uint64_t *p) { Affine<F> P; P.x = to_mont(load<F>(p)); P.y = to_mont(load<F>(p + 6)); return P; }
template <class F> static Affine<Fp2T<F>> load_g2(const uint64_t *p) {
    Affine<Fp2T<F>> Q; Q.x = to_mont(load<Fp2T<F>>(p)); Q.y = to_mont(load<Fp2T<F>>(p + 12)); return Q;
}
template <class F> static void store_line(uint64_t *p, const LineCoeffs<F> &l) { store(p, from_mont(l.a)); store(p + 12, from_mont(l.b)); store(p + 24, from_mont(l.c)); }

// out_multi = miller_multi over the g pairs, pair `var` (or none: -1) with a variable Q and the others prepared;
// out_product = the Fp12 product of the miller_loop values of the same pairs.  No final exponentiation on either
template <class F> static void multi_and_product(const uint64_t *g1, const uint64_t *g2, size_t g, int var, uint64_t *out_multi, uint64_t *out_product) {
    std::vector<Affine<F>> P;
    std::vector<LineCoeffs<F>> lines;
    Affine<F> Pv; Affine<Fp2T<F>> Qv;
    Fp12T<F> prod = Fp12T<F>::one();
    for (size_t k = 0; k < g; k++) {
        const Affine<F> Pk = load_g1<F>(g1 + 12 * k);
        const Affine<Fp2T<F>> Qk = load_g2<F>(g2 + 24 * k);
        prod = mul(prod, miller_loop(Pk, Qk));
        if ((int)k == var) { Pv = Pk; Qv = Qk; continue; }
        P.push_back(Pk);
        lines.resize(lines.size() + MILLER_LINES);
        prepare_g2(Qk, lines.data() + lines.size() - MILLER_LINES);
    }
    const Fp12T<F> f = miller_multi<F>(P.data(), 1, lines.data(), P.size(), var >= 0 ? &Pv : nullptr, var >= 0 ? &Qv : nullptr);
    store(out_multi, from_mont(f));
    store(out_product, from_mont(prod));
}
// prepared[0], prepared[67] of Q, and the same two triples from the formulas of the unprepared step written out here: the first from the
// affine Q (T = (x, y, 1): B = y^2, E = 3 b', J = x^2, H = 2 y), the last from the T that the existing loop (miller_double / miller_add)
// reaches before its last doubling.  out: 4 x 36 words
template <class F> static void line_ends(const uint64_t *g2, uint64_t *out) {
    using T2 = Fp2T<F>;
    const Affine<T2> Q = load_g2<F>(g2);
    std::vector<LineCoeffs<F>> lines(MILLER_LINES);
    prepare_g2(Q, lines.data());
    store_line(out, lines[0]);
    store_line(out + 36, lines[MILLER_LINES - 1]);
    auto triple = [](const G2Proj<F> &T) {
        const T2 B = sqr(T.Y), C = sqr(T.Z), bC = mul_xi(dbl(dbl(C))), E = add(dbl(bC), bC), J = sqr(T.X);
        LineCoeffs<F> l;
        l.a = sub(E, B); l.b = add(dbl(J), J); l.c = sub(sqr(add(T.Y, T.Z)), add(B, C));
        return l;
    };
    G2Proj<F> T; T.X = Q.x; T.Y = Q.y; T.Z = T2::one();
    store_line(out + 72, triple(T));
    Fp12T<F> f = Fp12T<F>::one();
    const F one = F::one();
    for (int i = 62; i >= 1; i--) {
        miller_double(f, T, one, one);
        if ((BLS_X_ABS >> i) & 1) miller_add(f, T, Q, one, one);
    }
    store_line(out + 108, triple(T));
}

extern "C" {
void chk_multi_and_product(const uint64_t *g1, const uint64_t *g2, size_t g, int var, uint64_t *m, uint64_t *p) { multi_and_product<Fp>(g1, g2, g, var, m, p); }
void chk_hmulti_and_product(const uint64_t *g1, const uint64_t *g2, size_t g, int var, uint64_t *m, uint64_t *p) { multi_and_product<HFp>(g1, g2, g, var, m, p); }
void chk_line_ends(const uint64_t *g2, uint64_t *out) { line_ends<Fp>(g2, out); }
void chk_hline_ends(const uint64_t *g2, uint64_t *out) { line_ends<HFp>(g2, out); }
}

#ifdef PREPARED_CHECK_MAIN
#include <stdio.h>
// the generators, canonical
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                  0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                  0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                  0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
// three pairs made of the generators, their doubles and an infinity member: miller_multi equals the product of the loops with every
// pair prepared and with each one left variable, and the ends of the prepared lines are the unprepared steps' -- for both limb
// types, which must also agree on the bytes
template <class F> static int run(uint64_t *out_multi) {
    uint64_t g1[36] = {0}, g2[72] = {0}, prod[72], multi[72], ends[144];
    memcpy(g1, GEN1, sizeof GEN1); memcpy(g2, GEN2, sizeof GEN2);
    const Affine<F> P2 = xyzz_to_affine(xyzz_dbl(xyzz_from_affine(load_g1<F>(GEN1))));
    const Affine<Fp2T<F>> Q2 = xyzz_to_affine(xyzz_dbl(xyzz_from_affine(load_g2<F>(GEN2))));
    store(g1 + 12, from_mont(P2.x)); store(g1 + 18, from_mont(P2.y));
    store(g2 + 24, from_mont(Q2.x)); store(g2 + 36, from_mont(Q2.y));
    memcpy(g2 + 48, GEN2, sizeof GEN2);                              // third pair: P = infinity
    int bad = 0;
    for (int var = -1; var < 3; var++) {
        multi_and_product<F>(g1, g2, 3, var, multi, prod);
        bad |= memcmp(multi, prod, sizeof multi) != 0;
    }
    multi_and_product<F>(g1, g2, 2, -1, out_multi, prod);
    bad |= memcmp(out_multi, prod, sizeof prod) != 0;
    line_ends<F>(g2 + 24, ends);
    bad |= memcmp(ends, ends + 72, 72 * sizeof(uint64_t)) != 0;
    return bad;
}
int main() {
    uint64_t m32[72], m64[72];
    int bad = run<Fp>(m32) | run<HFp>(m64);
    bad |= memcmp(m32, m64, sizeof m32) != 0;
    printf(bad ? "prepared_check: FAILED\n" : "prepared_check: ok\n");
    return bad;
}
#endif
