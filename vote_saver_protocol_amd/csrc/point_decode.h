// One ZCash-compressed BLS12-381 point -> Montgomery affine point and a status, shared by the gfx950 decoding kernel (decode.hip
// k_point_decode, both groups) and, through g++, by the CPU test build (tests/cpu_build/decode_check.cpp).
//
// A record is sizeof(F) big-endian bytes: x for G1 (48), x.c1 | x.c0 for G2 (96).  The top three bits of the first byte are flags:
// 0x80 compressed form (always set), 0x40 infinity (then every other bit is clear), 0x20 y is the larger of y and -y.  The y comes
// from the fixed chains of fp_sqrt.h / fp2_sqrt.h.
#pragma once
#include "curve.h"
#include "fp2_sqrt.h"

namespace vsp {

// ---- codec helpers on the 32-bit-limb field (wire.hip, msm_impl.inc and decode_record below)
// 48 big-endian bytes (12 words) -> 12 little-endian 32-bit limbs; the three flag bits of the first byte are cleared
VSP_HD Fp fp_from_be(const uint32_t *w, bool first) {
    Fp r;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < 12; j++) r.l[j] = __builtin_bswap32(w[11 - j]);
    if (first) r.l[11] &= 0x1FFFFFFFu;
    return r;
}
// a canonical value below p
VSP_HD bool canon_below_p(const Fp &a) {
    bool lt = false, gt = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = Fp::N - 1; i >= 0; i--) {
        lt = lt || (!gt && a.l[i] < FpP32::MOD[i]);
        gt = gt || (!lt && a.l[i] > FpP32::MOD[i]);
    }
    return lt;
}
VSP_HD bool canon_below_p(const Fp2 &a) { return canon_below_p(a.c0) && canon_below_p(a.c1); }

// what the two groups do differently: how the words of a record are read, and which root runs.  The G1 root is inlined; the G2 root
// is a real call on memory temporaries, one copy of its two chains beside the decoding code (the generic formulas inlined side by
// side next to the fixed-register product routine are what this toolchain's backend has tripped over: msm_impl.inc sgc_*)
VSP_HD void record_x(const uint32_t *w, Fp &x) { x = fp_from_be(w, true); }
VSP_HD void record_x(const uint32_t *w, Fp2 &x) { x.c1 = fp_from_be(w, true); x.c0 = fp_from_be(w + 12, false); }
template <class P> VSP_HD bool record_y(const Mont<P> &x, bool larger, Mont<P> &y) { return g1_y_from_x(x, larger, y); }
template <class F> VSP_HD_CALL bool record_y(const Fp2T<F> &x, bool larger, Fp2T<F> &y) { Fp2T<F> t; const bool ok = g2_y_from_x(x, larger, t); y = t; return ok; }

// the record of sizeof(F) bytes at w (F = Fp: G1, F = Fp2: G2) -> out, Montgomery form.  Returns 0 accepted (infinity 0xC0 00 .. 00
// included: it comes out all zero), 1 malformed (compression bit clear, infinity with any other bit set, a coordinate >= p), 2 no
// point has this x.  A rejected point comes out all zero
template <class F> VSP_HD uint32_t decode_record(const uint32_t *w, Affine<F> &out) {
    const uint32_t flags = w[0] & 0xFFu;                          // first byte of the record
    uint32_t rest = w[0] & ~0xE0u;                                // everything but the three flag bits
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 1; j < (int)(sizeof(F) / 4); j++) rest |= w[j];
    uint32_t st = 0;
    bool finite = false;
    if (!(flags & 0x80u)) st = 1u;                                // not the compressed form
    else if (flags & 0x40u) { if (rest != 0 || (flags & 0x20u)) st = 1u; }      // infinity: every other bit clear
    else finite = true;
    F x;
    record_x(w, x);
    if (finite && !canon_below_p(x)) { st = 1u; finite = false; }
    if (!finite) x = F::zero();
    // every lane walks the chain (rejected and infinity lanes on x = 0): the wave runs it anyway
    out.x = to_mont(x);
    const bool on_curve = record_y(out.x, (flags & 0x20u) != 0, out.y);
    if (finite && !on_curve) { st = 2u; finite = false; }
    if (!finite) { out.x = F::zero(); out.y = F::zero(); }
    return st;
}

}  // namespace vsp
