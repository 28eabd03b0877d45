// CPU test build of the tower arithmetic and the pairing (fp12.h, pairing.h compiled by g++ with the 32-bit-limb type the pairing
// kernels use, and with the host's 64-bit-limb type).  Test infrastructure only.  All arguments canonical little-endian u64 limbs: an
// Fp12 value is 72 words in tower order (the 576 bytes of the GT encoding), a G1 point x | y (12 words), a G2 point x.c0 | x.c1 |
// y.c0 | y.c1 (24 words), all zero = infinity.
// With -DPAIRING_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_pairing_cpu.py).
#include <string.h>
#include "../../vote_saver_protocol_amd/csrc/gt_dlog.h"
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
// One operation of a level of the tower on n values, the (level, op) codes of vsp_selftest_tower (include/vsp.h): an element is
// 6 * level words, a, b and out alike.  Returns 0, or 1 for a level or an op there is none of
template <class F> static Fp6T<F> to_mont6(const Fp6T<F> &a) { Fp6T<F> r; r.c0 = to_mont(a.c0); r.c1 = to_mont(a.c1); r.c2 = to_mont(a.c2); return r; }
template <class F> static Fp6T<F> from_mont6(const Fp6T<F> &a) { Fp6T<F> r; r.c0 = from_mont(a.c0); r.c1 = from_mont(a.c1); r.c2 = from_mont(a.c2); return r; }
template <class F> static int tower2_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using T = Fp2T<F>;
    const T x = to_mont(load<T>(a)), y = to_mont(load<T>(b));
    T r;
    switch (op) {
        case 0: r = mul(x, y); break;
        case 1: r = sqr(x); break;
        case 2: r = inv(x); break;
        case 3: r = conj(x); break;
        case 4: r = f2inv(x); break;
        case 5: r = mul_xi(x); break;
        case 6: r = f2half(x); break;
        case 7: r = add(x, y); break;
        case 8: r = sub(x, y); break;
        case 9: r = mul_fp(x, y.c0); break;
        case 10: r = neg(x); break;
        case 11: r = dbl(x); break;
        case 12: r.c0 = fp_half(x.c0); r.c1 = fp_half(x.c1); break;
        case 13: r.c0 = fp_inv_chain(x.c0); r.c1 = fp_inv_chain(x.c1); break;
        default: return 1;
    }
    store(out, from_mont(r));
    return 0;
}
template <class F> static int tower6_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using T = Fp6T<F>;
    const T x = to_mont6(load<T>(a)), y = to_mont6(load<T>(b));
    T r;
    switch (op) {
        case 0: r = mul(x, y); break;
        case 1: r = mul_v(x); break;
        case 2: r = inv(x); break;
        case 3: r = mul_by_01(x, y.c0, y.c1); break;
        case 4: r = mul_by_1(x, y.c1); break;
        case 7: r = add(x, y); break;
        case 8: r = sub(x, y); break;
        default: return 1;
    }
    store(out, from_mont6(r));
    return 0;
}
template <class F> static int tower12_op(int op, const uint64_t *a, const uint64_t *b, uint64_t *out) {
    using T = Fp12T<F>;
    if (op >= 0 && op <= 9) { f12_op<F>(op, a, b, out); return 0; }
    const T x = to_mont(load<T>(a)), y = to_mont(load<T>(b));
    if (op == 10) store(out, from_mont(mul_by_014(x, y.c0.c0, y.c0.c1, y.c1.c1)));
    else if (op == 11) { memset(out, 0, sizeof(T)); out[0] = is_one(x) ? 1 : 0; }
    else if (op == 12) store(out, from_mont(gt_pow(x, b, 4)));
    else return 1;
    return 0;
}
template <class F> static int tower_op(int level, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    if (level != 2 && level != 6 && level != 12) return 1;
    const size_t w = 6 * (size_t)level;
    int bad = 0;
    for (size_t i = 0; i < n; i++)
        bad |= level == 2 ? tower2_op<F>(op, a + i * w, b + i * w, out + i * w)
             : level == 6 ? tower6_op<F>(op, a + i * w, b + i * w, out + i * w) : tower12_op<F>(op, a + i * w, b + i * w, out + i * w);
    return bad;
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
int chk_tower_op(int level, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) { return tower_op<Fp>(level, op, a, b, out, n); }
int chk_htower_op(int level, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) { return tower_op<HFp>(level, op, a, b, out, n); }
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
    // the (level, op) entry on e(G1, G2) and its parts, two values a call: every op of every level runs, a square is the product with
    // itself, a times its inverse is one, e^r is one, and an op or a level there is none of is refused
    uint64_t in[144], t1[144], t2[144];
    memcpy(in, e_out, 72 * sizeof(uint64_t)); store(in + 72, from_mont(conj(e)));
    const uint64_t r_words[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    for (int level : {2, 6, 12}) {
        const size_t w = 6 * (size_t)level, m = 144 / w;            // 12, 4 or 2 values of the level
        for (int op = 0; op < 14; op++) {
            const bool has = level == 2 || (level == 6 ? (op <= 4 || op == 7 || op == 8) : op <= 12);
            bad |= tower_op<F>(level, op, in, in, t1, m) != (has ? 0 : 1);
        }
        bad |= tower_op<F>(level, 0, in, in, t1, m) != 0;           // a a
        if (level != 6) { bad |= tower_op<F>(level, 1, in, in, t2, m) != 0; bad |= memcmp(t1, t2, sizeof t1) != 0; }
        bad |= tower_op<F>(level, 2, in, in, t1, m) | tower_op<F>(level, 0, in, t1, t2, m);      // a (1 / a)
        for (size_t k = 0; k < m; k++) {
            bad |= t2[k * w] != 1;
            for (size_t j = 1; j < w; j++) bad |= t2[k * w + j] != 0;
        }
    }
    memcpy(t1, r_words, sizeof r_words); memcpy(t1 + 72, r_words, sizeof r_words);
    bad |= tower_op<F>(12, 12, in, t1, t2, 2) | tower_op<F>(12, 11, t2, t2, t1, 2);
    bad |= t1[0] != 1 || t1[72] != 1;
    bad |= tower_op<F>(3, 0, in, in, t1, 1) != 1;
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
