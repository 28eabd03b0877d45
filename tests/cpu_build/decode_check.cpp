// CPU test build of the decoding rules (point_decode.h decode_record compiled by g++ with the 32-bit-limb types the decoding kernel
// uses).  Test infrastructure only.  A record is 48 (G1) or 96 (G2) bytes as they travel; the point comes back canonical, little-endian
// u64 limbs: x | y (12 words) for G1, x.c0 | x.c1 | y.c0 | y.c1 (24 words) for G2, all zero for infinity and for a rejected record.
// With -DDECODE_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_tally_cpu.py).
#include <string.h>
#include "../../vote_saver_protocol_amd/csrc/point_decode.h"
using namespace vsp;

// returns decode_record's status
template <class F> static int decode(const uint8_t *rec, uint64_t *out) {
    uint32_t w[sizeof(F) / 4];                                       // the kernel reads whole words
    memcpy(w, rec, sizeof w);
    Affine<F> p;
    const uint32_t st = decode_record(w, p);
    p.x = from_mont(p.x); p.y = from_mont(p.y);
    memcpy(out, &p, sizeof p);
    return (int)st;
}
extern "C" {
int chk_decode_g1(const uint8_t *rec, uint64_t *out) { return decode<Fp>(rec, out); }
int chk_decode_g2(const uint8_t *rec, uint64_t *out) { return decode<Fp2>(rec, out); }
}

#ifdef DECODE_CHECK_MAIN
#include <stdio.h>
// the compressed generators (the y of both is the smaller one), canonical x | y and x.c0 | x.c1 | y.c0 | y.c1
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                  0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                  0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                  0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
// 6 little-endian words -> 48 big-endian bytes
static void be48(uint8_t *o, const uint64_t *l) { for (int i = 0; i < 6; i++) for (int b = 0; b < 8; b++) o[47 - (i * 8 + b)] = (uint8_t)(l[i] >> (8 * b)); }
static bool all_zero(const uint64_t *p, int n) { uint64_t o = 0; for (int i = 0; i < n; i++) o |= p[i]; return o == 0; }
// the generator of either group decodes to itself, infinity to zero, and the malformed and the pointless records are refused and zero
int main() {
    int bad = 0;
    uint8_t r1[48], r2[96];
    uint64_t o1[12], o2[24];
    be48(r1, GEN1); r1[0] |= 0x80;
    bad |= chk_decode_g1(r1, o1) != 0 || memcmp(o1, GEN1, sizeof o1) != 0;
    r1[0] &= 0x7F;                                                   // compression bit clear
    bad |= chk_decode_g1(r1, o1) != 1 || !all_zero(o1, 12);
    be48(r2, GEN2 + 6); be48(r2 + 48, GEN2); r2[0] |= 0x80;          // c1 | c0
    bad |= chk_decode_g2(r2, o2) != 0 || memcmp(o2, GEN2, sizeof o2) != 0;
    memset(r1, 0, sizeof r1); memset(r2, 0, sizeof r2);
    r2[0] = 0x80; r2[95] = 1;                                        // x = 1: 1 + 4 (1 + u) is no square
    bad |= chk_decode_g2(r2, o2) != 2 || !all_zero(o2, 24);
    r2[95] = 0;
    r1[0] = 0xC0; r2[0] = 0xC0;
    bad |= chk_decode_g1(r1, o1) != 0 || !all_zero(o1, 12) || chk_decode_g2(r2, o2) != 0 || !all_zero(o2, 24);
    r1[0] = 0xE0; r2[47] = 1;                                        // infinity with another bit set
    bad |= chk_decode_g1(r1, o1) != 1 || !all_zero(o1, 12) || chk_decode_g2(r2, o2) != 1 || !all_zero(o2, 24);
    r2[0] = 0x80; r2[47] = 0;                                        // x = 0: 4 (1 + u) is no square
    bad |= chk_decode_g2(r2, o2) != 2 || !all_zero(o2, 24);
    printf(bad ? "decode_check: FAILED\n" : "decode_check: ok\n");
    return bad;
}
#endif
