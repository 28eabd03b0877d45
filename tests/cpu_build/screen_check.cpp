// CPU test build of the screened ballot check's arithmetic (vote_saver_protocol_amd/csrc/screen.h: screen_mul128 and the product tree,
// compiled by g++ with the 32-bit-limb type the kernels use and with the host's 64-bit-limb type).  Test infrastructure only.  All
// arguments canonical little-endian u64 limbs: a G1 point x | y (12 words, all zero = infinity), an Fp12 value 72 words in tower order.
// With -DSCREEN_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_screen_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/screen.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }

// out = (lo + 2^64 hi) P, through the steps the kernel takes
template <class F> static void mul128(const uint64_t *g1, uint64_t lo, uint64_t hi, uint64_t *out) {
    Affine<F> P; P.x = to_mont(load<F>(g1)); P.y = to_mont(load<F>(g1 + 6));
    XYZZ<F> acc;
    screen_mul128(acc, P, lo, hi, [](XYZZ<F> *a) { *a = xyzz_dbl(*a); }, [](XYZZ<F> *a, const Affine<F> *q) { xyzz_madd(*a, *q); });
    const Affine<F> r = xyzz_to_affine(acc);
    store(out, from_mont(r.x)); store(out + 6, from_mont(r.y));
}
// n values in ranges of len, lying back to back: out_tree[r] = the product of range r by the levels the host queues (one
// screen_segment_product per lane of k_screen_product), out_serial[r] = the same product by one chain
template <class F> static void tree_and_serial(const uint64_t *vals, size_t n, size_t len, uint64_t *out_tree, uint64_t *out_serial) {
    std::vector<Fp12T<F>> cur(n), nxt;
    for (size_t i = 0; i < n; i++) cur[i] = to_mont(load<Fp12T<F>>(vals + 72 * i));
    ScreenLevel lv = screen_first_level(n, len);
    const size_t R = lv.ranges;
    for (size_t r = 0; r < R; r++) {
        Fp12T<F> f = cur[r * len];
        for (size_t i = 1; i < lv.count(r); i++) f = mul(f, cur[r * len + i]);
        store(out_serial + 72 * r, from_mont(f));
    }
    auto mul_ = [](Fp12T<F> *f, const Fp12T<F> *g) { *f = mul(*f, *g); };
    while (lv.stride > 1) {
        const ScreenLevel nx = lv.next();
        nxt.assign(R * nx.stride, Fp12T<F>::zero());
        for (size_t r = 0; r < R; r++)
            for (size_t t = 0; t < screen_level_count(lv.count(r)); t++) nxt[r * nx.stride + t] = screen_segment_product(cur.data() + r * lv.stride, lv.count(r), t, mul_);
        cur.swap(nxt); lv = nx;
    }
    for (size_t r = 0; r < R; r++) store(out_tree + 72 * r, from_mont(cur[r]));
}

extern "C" {
void chk_mul128(const uint64_t *g1, uint64_t lo, uint64_t hi, uint64_t *out) { mul128<Fp>(g1, lo, hi, out); }
void chk_hmul128(const uint64_t *g1, uint64_t lo, uint64_t hi, uint64_t *out) { mul128<HFp>(g1, lo, hi, out); }
void chk_tree_and_serial(const uint64_t *vals, size_t n, size_t len, uint64_t *t, uint64_t *s) { tree_and_serial<Fp>(vals, n, len, t, s); }
void chk_htree_and_serial(const uint64_t *vals, size_t n, size_t len, uint64_t *t, uint64_t *s) { tree_and_serial<HFp>(vals, n, len, t, s); }
}

#ifdef SCREEN_CHECK_MAIN
#include <stdio.h>
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
// (2^128 - 1) G + G = 2^64 (2^64 G); 1 G = G; z infinity = infinity; trees of 1, 2, 63, 64, 65 values and of 65 in ranges of 17 against
// the chains, over values that are small powers of a fixed element -- for both limb types, which must agree on the bytes
template <class F> static int run(uint64_t *out) {
    uint64_t a[12], b[12], c[12], zero[12] = {0};
    int bad = 0;
    mul128<F>(GEN1, 1, 0, a);
    bad |= memcmp(a, GEN1, sizeof a) != 0;
    mul128<F>(GEN1, 0, 1, a); mul128<F>(a, 0, 1, b);                 // 2^128 G
    mul128<F>(GEN1, ~0ULL, ~0ULL, c);                                // (2^128 - 1) G
    Affine<F> C; C.x = to_mont(load<F>(c)); C.y = to_mont(load<F>(c + 6));
    Affine<F> G; G.x = to_mont(load<F>(GEN1)); G.y = to_mont(load<F>(GEN1 + 6));
    XYZZ<F> s = xyzz_from_affine(C); xyzz_madd(s, G);
    const Affine<F> S = xyzz_to_affine(s);
    store(c, from_mont(S.x)); store(c + 6, from_mont(S.y));
    bad |= memcmp(b, c, sizeof b) != 0;
    mul128<F>(zero, 5, 7, a);
    bad |= memcmp(a, zero, sizeof a) != 0;
    memcpy(out, b, sizeof b);
    // Fp12 values: v_i = g^(i + 1) for g = 2 + 3 w-ish (any element with every coefficient set)
    Fp12T<F> g;
    { uint64_t w[72] = {0}; for (int k = 0; k < 12; k++) w[6 * k] = 2 + k; g = to_mont(load<Fp12T<F>>(w)); }
    std::vector<uint64_t> vals(72 * 65), t(72 * 65), sr(72 * 65);
    Fp12T<F> v = g;
    for (size_t i = 0; i < 65; i++) { store(vals.data() + 72 * i, from_mont(v)); v = mul(v, g); }
    const size_t shapes[][2] = {{1, 1}, {2, 2}, {63, 63}, {64, 64}, {65, 65}, {65, 17}, {65, 1}};
    for (auto &sh : shapes) {
        tree_and_serial<F>(vals.data(), sh[0], sh[1], t.data(), sr.data());
        const size_t R = (sh[0] + sh[1] - 1) / sh[1];
        bad |= memcmp(t.data(), sr.data(), R * 72 * sizeof(uint64_t)) != 0;
    }
    memcpy(out + 12, t.data(), 72 * sizeof(uint64_t));
    return bad;
}
int main() {
    uint64_t m32[84], m64[84];
    int bad = run<Fp>(m32) | run<HFp>(m64);
    bad |= memcmp(m32, m64, sizeof m32) != 0;
    printf(bad ? "screen_check: FAILED\n" : "screen_check: ok\n");
    return bad;
}
#endif
