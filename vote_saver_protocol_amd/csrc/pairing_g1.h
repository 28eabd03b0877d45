// The G1 side of the pairing kernels that pairing.hip and decrypt.hip share: a checked load of canonical words and the curve.h group
// law as real calls on memory operands (one copy of each body in a kernel; see point_decode.h record_y).  Device code only.
#pragma once
#include "common.h"
#include "fp12.h"

namespace vsp {

static __device__ __noinline__ void pr_dbl(G1XYZZ *a) { *a = xyzz_dbl(*a); }
static __device__ __noinline__ void pr_madd(G1XYZZ *a, const G1Affine *p) { G1XYZZ t = *a; xyzz_madd(t, *p); *a = t; }
// canonical words -> Montgomery affine point; 0 accepted (infinity included), 1 a coordinate >= p, 2 off the curve.  A rejected point
// comes out as infinity
static __device__ __noinline__ uint32_t pr_load_g1(const uint64_t *src, G1Affine *out) {
    G1Affine c = *(const G1Affine *)src;
    uint32_t st = (canon_below_p(c.x) && canon_below_p(c.y)) ? 0u : 1u;
    G1Affine p; p.x = to_mont(c.x); p.y = to_mont(c.y);
    const Fp four = dbl(dbl(Fp::one()));
    if (!st && !is_inf(c) && !eq(sqr(p.y), add(mul(sqr(p.x), p.x), four))) st = 2u;
    if (st) { p.x = Fp::zero(); p.y = Fp::zero(); }
    *out = p;
    return st;
}
// the L canonical scalars at s (8 words each) all below r
static __device__ __forceinline__ bool pr_scalars_below_r(const uint32_t *s, size_t L) {
    bool ok = true;
    for (size_t i = 0; i < L; i++) {
        const uint4 lo = *(const uint4 *)(s + 8 * i), hi = *(const uint4 *)(s + 8 * i + 4);
        if (!scalar_below_r(lo, hi)) ok = false;
    }
    return ok;
}
// acc = sum s_i G_i over the key's table of multiples, rows[i * 16 + d] = d G_i: 4 bits of every scalar at a time from the top, 4
// doublings, then one table row per input
static __device__ __forceinline__ void pr_input_sum(G1XYZZ &acc, const uint32_t *s, size_t L, const G1Affine *__restrict__ rows) {
    acc = G1XYZZ::inf();
    if (!L) return;
#pragma unroll 1
    for (int w = 63; w >= 0; w--) {
        if (w != 63) { pr_dbl(&acc); pr_dbl(&acc); pr_dbl(&acc); pr_dbl(&acc); }
#pragma unroll 1
        for (size_t i = 0; i < L; i++) {
            const uint32_t d = (s[8 * i + (w >> 3)] >> ((w & 7) * 4)) & 15u;
            G1Affine t = rows[i * 16 + d];
            pr_madd(&acc, &t);
        }
    }
}
// the acc of a SAVER ballot before its ciphertext members are added (k_ballot_prepare of pairing.hip over canonical limbs,
// k_receive_prepare of receive.hip over decoded points; both add c_0 .. c_n with pr_madd, the generic addition):
// G_0 + sum x_i G_{n+1+i} over the L rest inputs at s; tab: the key's table of multiples
static __device__ __forceinline__ void pr_ballot_acc_start(G1XYZZ &acc, const uint32_t *s, size_t L, size_t n, const G1Affine *__restrict__ tab) {
    pr_input_sum(acc, s, L, tab + (n + 1) * 16);
    G1Affine g0 = tab[1];
    pr_madd(&acc, &g0);
}
// affine through one inversion: 1 / (ZZ ZZZ); infinity (ZZ = 0) comes out as x = y = 0
static __device__ __forceinline__ G1Affine pr_to_affine(const G1XYZZ &acc) {
    const Fp t = fp_inv_chain(mul(acc.ZZ, acc.ZZZ));
    G1Affine P;
    P.x = mul(acc.X, mul(t, acc.ZZZ));
    P.y = mul(acc.Y, mul(t, acc.ZZ));
    return P;
}

}  // namespace vsp
