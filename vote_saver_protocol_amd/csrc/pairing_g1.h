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
// affine through one inversion: 1 / (ZZ ZZZ); infinity (ZZ = 0) comes out as x = y = 0
static __device__ __forceinline__ G1Affine pr_to_affine(const G1XYZZ &acc) {
    const Fp t = fp_inv_chain(mul(acc.ZZ, acc.ZZZ));
    G1Affine P;
    P.x = mul(acc.X, mul(t, acc.ZZZ));
    P.y = mul(acc.Y, mul(t, acc.ZZ));
    return P;
}

}  // namespace vsp
