// CPU test build of the GT discrete-logarithm search (gt_dlog.h, compiled by g++ with the 32-bit-limb type the decryption kernels use and
// with the host's 64-bit-limb type).  Test infrastructure only.  A GT value is 72 canonical little-endian u64 words in tower order.
// The table is built and the giant range walked in runs of DLOG_RUN_STEPS, the way the kernels cut them over lanes.
// With -DDLOG_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_gt_dlog_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/gt_dlog.h"
using namespace vsp;

template <class F> static Fp12T<F> load_gt(const uint64_t *p) { Fp12T<F> t; memcpy(&t, p, sizeof t); return to_mont(t); }
template <class F> static void store_gt(uint64_t *p, const Fp12T<F> &t) { const Fp12T<F> c = from_mont(t); memcpy(p, &c, sizeof c); }

// keys, js: 2^b entries, sorted by fingerprint
template <class F> static void table(const uint64_t *base_w, unsigned b, unsigned fp_bits, uint64_t *keys, uint32_t *js) {
    const Fp12T<F> base = load_gt<F>(base_w);
    const uint64_t B = (uint64_t)1 << b;
    for (uint64_t j0 = 0; j0 < B; j0 += DLOG_RUN_STEPS)
        dlog_baby_run(base, j0, (unsigned)(B - j0 < DLOG_RUN_STEPS ? B - j0 : DLOG_RUN_STEPS), fp_bits, keys + j0);
    dlog_sort_table(keys, js, B);
}
// the m in [0, max_value] with base^m = value, or DLOG_NONE: every run of the giant range, the lowest result
template <class F> static uint64_t find(const uint64_t *value_w, const uint64_t *base_w, unsigned b, unsigned fp_bits, uint64_t max_value, const uint64_t *keys,
                                        const uint32_t *js) {
    const Fp12T<F> value = load_gt<F>(value_w), base = load_gt<F>(base_w), g = dlog_giant_stride(base, b);
    const uint64_t K = dlog_giant_steps(max_value, b);
    uint64_t found = DLOG_NONE;
    for (uint64_t k0 = 0; k0 < K; k0 += DLOG_RUN_STEPS) {
        const uint64_t m = dlog_giant_run(value, base, g, k0, (unsigned)(K - k0 < DLOG_RUN_STEPS ? K - k0 : DLOG_RUN_STEPS), keys, js, b, fp_bits, max_value);
        if (m < found) found = m;
    }
    return found;
}
// out = conj(base^B) base^B
template <class F> static void stride_times_power(const uint64_t *base_w, unsigned b, uint64_t *out) {
    const Fp12T<F> base = load_gt<F>(base_w);
    store_gt(out, mul(dlog_giant_stride(base, b), gt_pow_u64(base, (uint64_t)1 << b)));
}
template <class F> static void power(const uint64_t *base_w, const uint64_t *e4, uint64_t *out) { store_gt(out, gt_pow(load_gt<F>(base_w), e4, 4)); }
template <class F> static uint64_t fingerprint(const uint64_t *x_w, unsigned fp_bits) { return gt_fingerprint(load_gt<F>(x_w), fp_bits); }

extern "C" {
#define DLOG_EXPORTS(PRE, F)                                                                                                                                  \
    void PRE##table(const uint64_t *base, unsigned b, unsigned fp_bits, uint64_t *keys, uint32_t *js) { table<F>(base, b, fp_bits, keys, js); }              \
    uint64_t PRE##find(const uint64_t *value, const uint64_t *base, unsigned b, unsigned fp_bits, uint64_t max_value, const uint64_t *keys, const uint32_t *js) { \
        return find<F>(value, base, b, fp_bits, max_value, keys, js);                                                                                        \
    }                                                                                                                                                         \
    void PRE##stride_times_power(const uint64_t *base, unsigned b, uint64_t *out) { stride_times_power<F>(base, b, out); }                                   \
    void PRE##power(const uint64_t *base, const uint64_t *e4, uint64_t *out) { power<F>(base, e4, out); }                                                     \
    uint64_t PRE##fingerprint(const uint64_t *x, unsigned fp_bits) { return fingerprint<F>(x, fp_bits); }
DLOG_EXPORTS(chk_, Fp)
DLOG_EXPORTS(chk_h, HFp)
unsigned chk_auto_baby_bits(uint64_t max_value) { return dlog_auto_baby_bits(max_value); }
uint64_t chk_giant_steps(uint64_t max_value, unsigned b) { return dlog_giant_steps(max_value, b); }
unsigned chk_run_steps(void) { return DLOG_RUN_STEPS; }
uint64_t chk_launch_lanes(uint64_t items, uint64_t runs) { return dlog_launch_lanes(items, runs); }
}

#ifdef DLOG_CHECK_MAIN
#include <stdio.h>
// the generators, canonical
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                  0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                  0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                  0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
// base = e(G1, G2) of this header's own pairing; B = 8, max_value = 100 and a 4-bit fingerprint: every m in 0..100 found, 101..103
// refused though the last giant step reaches them; the table's keys must agree between the limb types
template <class F> static int run(uint64_t *keys_out) {
    Affine<F> P; Affine<Fp2T<F>> Q;
    { F t; memcpy(&t, GEN1, sizeof t); P.x = to_mont(t); memcpy(&t, GEN1 + 6, sizeof t); P.y = to_mont(t); }
    { Fp2T<F> t; memcpy(&t, GEN2, sizeof t); Q.x = to_mont(t); memcpy(&t, GEN2 + 12, sizeof t); Q.y = to_mont(t); }
    uint64_t base_w[72], value_w[72];
    const Fp12T<F> base = pairing(P, Q);
    store_gt(base_w, base);
    uint32_t js[8];
    table<F>(base_w, 3, 4, keys_out, js);
    int bad = 0;
    Fp12T<F> x = Fp12T<F>::one();
    for (uint64_t m = 0; m <= 103; m++) {
        store_gt(value_w, x);
        const uint64_t got = find<F>(value_w, base_w, 3, 4, 100, keys_out, js);
        bad |= got != (m <= 100 ? m : DLOG_NONE);
        x = mul(x, base);
    }
    stride_times_power<F>(base_w, 3, value_w);
    bad |= !is_one(load_gt<F>(value_w));
    return bad;
}
int main() {
    uint64_t k32[8], k64[8];
    int bad = run<Fp>(k32) | run<HFp>(k64);
    bad |= memcmp(k32, k64, sizeof k32) != 0;
    printf(bad ? "dlog_check: FAILED\n" : "dlog_check: ok\n");
    return bad;
}
#endif
