// CPU test build of the tower arithmetic and the pairing (fp12.h, pairing.h compiled by g++ with the 32-bit-limb type the pairing
// kernels use, and with the host's 64-bit-limb type).  Test infrastructure only.  All arguments canonical little-endian u64 limbs: an
// Fp12 value is 72 words in tower order (the 576 bytes of the GT encoding), a G1 point x | y (12 words), a G2 point x.c0 | x.c1 |
// y.c0 | y.c1 (24 words), all zero = infinity.
// With -DPAIRING_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_pairing_cpu.py).
#include <string.h>
#include "../../vote_saver_protocol_amd/csrc/pairing.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }

template <class F> static void f12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using T = Fp12T<F>;
    const T x = to_mont(load<T>(a)), y = to_mont(load<T>(b));
    T r;
    switch (op) {
        case 0: r = mul(x, y); break;
        case 1: r = sqr(x); break;
        case 2: r = inv(x); break;
        case 3: r = conj(x); break;
        case 4: r = frobenius(x); break;
        case 5: r = frobenius2(x); break;
        case 6: r = cyclotomic_sqr(x); break;
        case 7: r = add(x, y); break;
        case 8: r = sub(x, y); break;
        default: r = final_exp(x); break;
    }
    store(out, from_mont(r));
}
// a (l0 + l1 v + l4 v w), the line coefficients as 36 words l0 | l1 | l4
template <class F> static void f12_sparse(const uint64_t *a, const uint64_t *l, uint64_t *out) {
    using T = Fp12T<F>; using T2 = Fp2T<F>;
    store(out, from_mont(mul_by_014(to_mont(load<T>(a)), to_mont(load<T2>(l)), to_mont(load<T2>(l + 12)), to_mont(load<T2>(l + 24)))));
}
template <class F> static Fp12T<F> miller_of(const uint64_t *g1, const uint64_t *g2) {
    Affine<F> P; P.x = to_mont(load<F>(g1)); P.y = to_mont(load<F>(g1 + 6));
    Affine<Fp2T<F>> Q; Q.x = to_mont(load<Fp2T<F>>(g2)); Q.y = to_mont(load<Fp2T<F>>(g2 + 12));
    return miller_loop(P, Q);
}
// out = fexp(prod_k ml(g1[k], g2[k])); returns 1 when it is one
template <class F> static int pairing_product(const uint64_t *g1, const uint64_t *g2, size_t m, uint64_t *out) {
    Fp12T<F> f = Fp12T<F>::one();
    for (size_t k = 0; k < m; k++) f = mul(f, miller_of<F>(g1 + 12 * k, g2 + 24 * k));
    f = final_exp(f);
    store(out, from_mont(f));
    return is_one(f) ? 1 : 0;
}

extern "C" {
void chk_f12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) { f12_op<Fp>(op, a, b, out); }
void chk_hf12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) { f12_op<HFp>(op, a, b, out); }
void chk_f12_sparse(const uint64_t *a, const uint64_t *l, uint64_t *out) { f12_sparse<Fp>(a, l, out); }
void chk_hf12_sparse(const uint64_t *a, const uint64_t *l, uint64_t *out) { f12_sparse<HFp>(a, l, out); }
int chk_pairing_product(const uint64_t *g1, const uint64_t *g2, size_t m, uint64_t *out) { return pairing_product<Fp>(g1, g2, m, out); }
int chk_hpairing_product(const uint64_t *g1, const uint64_t *g2, size_t m, uint64_t *out) { return pairing_product<HFp>(g1, g2, m, out); }
}

#ifdef PAIRING_CHECK_MAIN
#include <stdio.h>
// the generators, canonical
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                  0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                  0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                  0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
// e(G1, G2) is not one, e(G1, G2) e(-G1, G2) is, infinity gives one, and the tower operations agree with each other on e(G1, G2): for
// both limb types, which must also agree on the 576 bytes
template <class F> static int run(uint64_t *e_out) {
    uint64_t g1[24], g2[48], out[72], zero[72] = {0};
    memcpy(g1, GEN1, sizeof GEN1); memcpy(g2, GEN2, sizeof GEN2);
    int bad = 0;
    bad |= pairing_product<F>(g1, g2, 1, e_out) != 0;
    // -G1: y -> p - y
    Affine<F> P; P.x = to_mont(load<F>(GEN1)); P.y = neg(to_mont(load<F>(GEN1 + 6)));
    store(g1 + 12, from_mont(P.x)); store(g1 + 18, from_mont(P.y));
    memcpy(g2 + 24, GEN2, sizeof GEN2);
    bad |= pairing_product<F>(g1, g2, 2, out) != 1;
    bad |= pairing_product<F>(zero, g2, 1, out) != 1;
    bad |= pairing_product<F>(g1, zero, 1, out) != 1;
    const Fp12T<F> e = to_mont(load<Fp12T<F>>(e_out));
    bad |= !eq(sqr(e), mul(e, e));
    bad |= !eq(cyclotomic_sqr(e), sqr(e));
    bad |= !is_one(mul(e, inv(e)));
    bad |= !is_one(mul(e, conj(e)));
    bad |= !eq(frobenius(frobenius(e)), frobenius2(e));
    return bad;
}
int main() {
    uint64_t e32[72], e64[72];
    int bad = run<Fp>(e32) | run<HFp>(e64);
    bad |= memcmp(e32, e64, sizeof e32) != 0;
    printf(bad ? "pairing_check: FAILED\n" : "pairing_check: ok\n");
    return bad;
}
#endif
