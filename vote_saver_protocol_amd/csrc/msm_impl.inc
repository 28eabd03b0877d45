// Pippenger (bucket-method) multi-scalar multiplication over BLS12-381 G1 / G2 for gfx950.
//
// Replaces algebra::multiexp<policies::multiexp_method_BDLO12>, multiexp_with_mixed_addition and the
// G2 half of kc_multiexp_with_mixed_addition (crypto3-algebra / crypto3-zk, absent submodules,
// /root/reference/.gitmodules:8-12; parameter table included at
// bin/cli/include/nil/vote_saver/common.hpp:38, reached from common.hpp:1132-1135).
// The reference algorithm is serial: for each c-bit window, add every base into bucket[digit], then a
// running sum over the buckets, then c doublings between windows.  The value sum_i k_i * P_i is unique
// as an affine point, so any bucket schedule gives bit-identical output after normalisation.
//
// MI355X pipeline (all on one stream, no host round trip until the last few hundred bytes):
//   0. k_glv_split (plain resident bases up to 2^20 G1 / 2^18 G2 points) k = k1 + k2 lambda: 2n points (P, phi(P)), signed 127-bit halves
//   1. k_digits    signed c-bit digits of every scalar (halves the buckets)
//   2. k_count_lds / k_chunk_prefix / scan / k_scatter_lds   counting sort of point indices (+ sign bit) into bucket order, the
//                  counters of one (chunk, window) in 128 KiB of LDS; k_plan splits buckets larger than T into parts,
//                  k_partsort orders the parts by size
//   3. k_accum28   ONE THREAD (G2: lane pair) PER BUCKET PART: gathers its affine points from the 14 x 28-bit-limb copy of the bases
//                  (128 B / 256 B rows) and folds them with mixed XYZZ additions -- this is where ~80 % of the time goes; it is VALU
//                  integer-multiply bound, not HBM bound.  (k_accum: the same on the 12 x 32-bit form, the fallback and the redo path)
//   4. k_merge_a / k_merge2   buckets that were split (skewed scalars: the 0/1-heavy witnesses of
//                  multiexp_with_mixed_addition) are folded by lane groups or by workgroups, LDS trees
//   5. k_dimsum    the weighted bucket sum  sum_b (b+1) B_b  is decomposed over the 2 (or 3) digits of the bucket
//                  index b = (v1, v0):  plain sums along each digit (lane group + LDS tree per sum),
//   6. k_dimweight then a <=256-term weighted sum per (window, digit) by suffix scan in LDS
//                  (steps 4-6 on the 28-bit form: XYZZ<Fp28> / XYZZ<Fp2x28>, fp28.h)
//   7. host        Horner over W*4 points (c*W doublings) in 64-bit limbs and the affine normalisation
//
// Zero scalars produce no digit and are skipped; scalars equal to one land in one bucket of window 0
// and are summed by steps 3-4 -- the two special cases of multiexp_with_mixed_addition need no
// separate pre-pass.
// (implementation include: compiled once per group by msm_g1.hip / msm_g2.hip so the two build in parallel)
#include "common.h"
#include "lane_view.h"
#include "fp28.h"
#if VSP_MSM_GROUP == 1
#include "accum28_asm_gfx950.h"
#endif


namespace vsp {
namespace {

static constexpr unsigned MSM_THREADS = 256;

// ------------------------------------------------------------------------------------------------
// digits (MsmGeom: common.h)

__device__ __forceinline__ uint32_t scalar_bits(const uint32_t *k, unsigned pos, unsigned c) {
    unsigned limb = pos >> 5, sh = pos & 31;
    if (limb >= 8) return 0;
    uint64_t v = k[limb];
    if (limb + 1 < 8) v |= (uint64_t)k[limb + 1] << 32;
    return (uint32_t)(v >> sh) & ((1u << c) - 1u);
}

// The scalar the windows are cut from, and whether every digit's sign flips.  Endomorphism split (g.sbits == 128): a magnitude below
// 2^127 with its sign in bit 255.  g.fold (255-bit scalars, windows whose width divides 255: c = 15, 17): k and r - k give opposite
// points, and the smaller of the two is below 2^254 -- 254 / c + 1 windows cover it AND the carry of the signed recoding, one fewer than
// 255 / c + 1 (c = 17: 15 windows instead of 16, whose last held nothing but that carry: one bucket with half of all points in it).
__device__ __forceinline__ uint32_t load_scalar(const Fr *scalars, size_t i, const MsmGeom &g, uint32_t (&k)[8]) {
    const uint32_t *p = scalars[i].l;
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = p[j];
    if (g.sbits == 128u) return k[7] >> 31;
    if (!g.fold) return 0u;
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {                                  // d = r - k
        const uint64_t t = (uint64_t)FrP32::MOD[j] - k[j] - borrow;
        d[j] = (uint32_t)t; borrow = (uint32_t)(t >> 63);
    }
    bool gt = false, decided = false;                              // k > d ?
#pragma unroll
    for (int j = 7; j >= 0; j--) if (!decided && k[j] != d[j]) { gt = k[j] > d[j]; decided = true; }
    if (!gt || borrow) return 0u;                                  // (k >= r is refused elsewhere; leave it alone here)
#pragma unroll
    for (int j = 0; j < 8; j++) k[j] = d[j];
    return 1u;
}

// calls f(window, bucket_index, negative) for every non-zero signed digit of scalar i
template <class Fn> __device__ __forceinline__ void for_each_digit(const Fr *scalars, size_t i, const MsmGeom &g, Fn f) {
    uint32_t k[8];
    const bool flip = load_scalar(scalars, i, g, k) != 0;
    uint32_t carry = 0;
    for (unsigned w = 0; w < g.W; w++) {
        uint32_t raw = scalar_bits(k, w * g.c, g.c) + carry;
        uint32_t mag; bool neg;
        if (raw > g.B) { mag = (1u << g.c) - raw; neg = true; carry = 1; }
        else { mag = raw; neg = false; carry = 0; }
        if (mag) f(w, mag - 1, neg != flip);
    }
}

// In "single set" mode (bases precomputed as 2^(c*w) * P for every window w) all windows share ONE set of B buckets and the
// sorted entry of digit w of scalar i is the index of that multiple: w * stride + first + i.
// (shared-set mode, g.single: ONE bucket set per scalar vector -- set w / Wk -- and slice w % Wk of the table of window multiples; one vector: Wk = W)
__device__ __forceinline__ size_t bucket_of(const MsmGeom &g, unsigned w, uint32_t b) { return (g.single ? (size_t)(w / g.Wk) * g.B : (size_t)w * g.B) + b; }
__device__ __forceinline__ uint32_t entry_of(const MsmGeom &g, unsigned w, size_t i) { return g.single ? (uint32_t)((size_t)(w % g.Wk) * g.idx_stride + g.idx_first + i) : (uint32_t)i; }

// ------------------------------------------------------------------------------------------------
// Endomorphism split (GLV) for PLAIN bases.  BLS12-381 has phi(x, y) = (beta x, y) with phi(P) = lambda P on the order-r subgroups
// (lambda = z^2 - 1, z the curve parameter; lambda^2 + lambda + 1 = 0 mod r; beta a cube root of unity in Fp, chosen per group so
// that the eigenvalue is this lambda).  lambda is 128 bits and r < lambda^2 + lambda + 1, so a division gives the split: k2 = round(k /
// lambda), k1 = k - k2 lambda in [-lambda/2, lambda/2]; and where k2 reaches 2^127 the relation lambda^2 + lambda + 1 = 0 mod r
// moves it back: (k1, k2) -> (k1 - 1, k2 - lambda - 1).  Both halves are then SIGNED values of magnitude below 2^127: 128 / c windows
// exactly, no carry out of the top window (an unsigned split needs one more, sparse window whose single bucket takes a quarter of
// the points).  The halves are stored as magnitude (bits 0..126) and sign (bit 255); a negative half negates its point.
// sum k_i P_i = sum k1_i P_i + sum k2_i phi(P_i): twice the points, half the scalar length -- the SAME number of bucket additions
// (n * 255 / c either way), but half as many windows, i.e. half as many bucket sets to reduce and half the host Horner chain.
// The table of the 28-bit accumulation kernel holds (P_i, phi(P_i)) interleaved (built once at upload), the split scalars are
// written interleaved too, and everything after this kernel is the ordinary pipeline over 2n points with 128-bit scalars.
#if VSP_MSM_GROUP == 1
static constexpr uint32_t GLV_BETA_MONT[12] = {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
#else
static constexpr uint32_t GLV_BETA_MONT[12] = {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au, 0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu};
#endif
__device__ __forceinline__ Fp glv_beta() { Fp b; for (int i = 0; i < 12; i++) b.l[i] = GLV_BETA_MONT[i]; return b; }
__device__ __forceinline__ void glv_apply(Fp &x) { x = mul(x, glv_beta()); }
__device__ __forceinline__ void glv_apply(Fp2 &x) { Fp b = glv_beta(); x.c0 = mul(x.c0, b); x.c1 = mul(x.c1, b); }
__device__ __forceinline__ void glv_apply(Fp2L &x) { x.v = mul(x.v, glv_beta()); }        // lane pair: each lane scales its own component

// out[2i] = k mod lambda, out[2i+1] = k div lambda (upper 128 bits zero).  Quotient by Barrett with mu = floor(2^383 / lambda)
// (256 bits): q' = floor(k mu / 2^383) is at most 2 below the quotient for k < 2^255; the remainder loop fixes it.
// k = k1 + k2 lambda: the magnitudes (below 2^127) and signs of the two halves
__device__ __forceinline__ void glv_split_scalar(const uint32_t (&k)[8], uint32_t (&m1)[4], bool &neg1, uint32_t (&m2)[4], bool &neg2) {
    const uint32_t LAM[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};
    const uint32_t MU[8] = {0xc4b6396eu, 0xed2f27c6u, 0x9345fbd1u, 0x1c4fa4d3u, 0x7b67f718u, 0xb1fb7291u, 0xf00fd56eu, 0xbe35f678u};
    // t = k * mu (16 limbs), schoolbook with 64-bit column accumulation
    uint32_t t[16];
    uint64_t carry = 0;
#pragma unroll
    for (int col = 0; col < 16; col++) {
        uint64_t lo = carry & 0xffffffffu, hi = carry >> 32;
#pragma unroll
        for (int a = 0; a < 8; a++) {
            int b = col - a;
            if (b < 0 || b > 7) continue;
            uint64_t pr = (uint64_t)k[a] * MU[b];
            lo += pr & 0xffffffffu; hi += pr >> 32;
        }
        t[col] = (uint32_t)lo;
        carry = hi + (lo >> 32);
    }
    // q = t >> 383 = (t >> 352) >> 31: limbs 11..15
    uint32_t q[5];
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = (t[11 + j] >> 31) | (t[12 + j] << 1);
    q[4] = t[15] >> 31;                                       // zero for k < r (q < 2^128); kept for the subtraction below
    // rem = k - q * lambda (fits 160 bits at this point: at most 3 lambda), 5 limbs
    uint32_t ql[6];
    carry = 0;
#pragma unroll
    for (int col = 0; col < 6; col++) {
        uint64_t lo = carry & 0xffffffffu, hi = carry >> 32;
#pragma unroll
        for (int a = 0; a < 4; a++) {
            int b = col - a;
            if (b < 0 || b > 3) continue;
            uint64_t pr = (uint64_t)q[a] * LAM[b];
            lo += pr & 0xffffffffu; hi += pr >> 32;
        }
        ql[col] = (uint32_t)lo;
        carry = hi + (lo >> 32);
    }
    uint32_t rem[5];
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        uint64_t d = (uint64_t)k[j] - ql[j] - borrow;
        rem[j] = (uint32_t)d; borrow = (uint32_t)(d >> 63);
    }
    auto ge_lam = [&](const uint32_t *x, const uint32_t *y) {       // x (5 limbs) >= y (4 limbs)
        if (x[4]) return true;
        for (int j = 3; j >= 0; j--) { if (x[j] > y[j]) return true; if (x[j] < y[j]) return false; }
        return true;
    };
    auto inc = [&](uint32_t *x, int nl) { uint32_t c = 1; for (int j = 0; j < nl; j++) { uint64_t sx = (uint64_t)x[j] + c; x[j] = (uint32_t)sx; c = (uint32_t)(sx >> 32); } };
    auto dec = [&](uint32_t *x, int nl) { uint32_t b = 1; for (int j = 0; j < nl; j++) { uint64_t d = (uint64_t)x[j] - b; x[j] = (uint32_t)d; b = (uint32_t)(d >> 63); } };
    for (int it = 0; it < 3 && ge_lam(rem, LAM); it++) {      // floor quotient: while rem >= lambda: rem -= lambda, q += 1
        borrow = 0;
        for (int j = 0; j < 5; j++) { uint64_t d = (uint64_t)rem[j] - (j < 4 ? LAM[j] : 0u) - borrow; rem[j] = (uint32_t)d; borrow = (uint32_t)(d >> 63); }
        inc(q, 5);
    }
    // nearest quotient: rem >= (lambda + 1) / 2  ->  q += 1, k1 = rem - lambda (negative, magnitude lambda - rem)
    const uint32_t HALF[4] = {0x80000000u, 0x00000000u, 0x8000d201u, 0x5622d200u};       // (lambda + 1) / 2
    neg1 = false;
    if (ge_lam(rem, HALF)) {
        inc(q, 5);
        borrow = 0;
        for (int j = 0; j < 4; j++) { uint64_t d = (uint64_t)LAM[j] - rem[j] - borrow; m1[j] = (uint32_t)d; borrow = (uint32_t)(d >> 63); }
        neg1 = true;
    } else { for (int j = 0; j < 4; j++) m1[j] = rem[j]; }
    // k2 = q unless q >= 2^127: then k2 = q - lambda - 1 (negative, magnitude lambda + 1 - q) and k1 -= 1
    neg2 = false;
    if (q[4] || (q[3] >> 31)) {
        uint32_t lp1[5] = {LAM[0], LAM[1], LAM[2], LAM[3], 0}; inc(lp1, 5);
        borrow = 0;
        for (int j = 0; j < 4; j++) { uint64_t d = (uint64_t)lp1[j] - q[j] - borrow; m2[j] = (uint32_t)d; borrow = (uint32_t)(d >> 63); }
        neg2 = true;
        const bool zero1 = (m1[0] | m1[1] | m1[2] | m1[3]) == 0;
        if (zero1) { m1[0] = 1; neg1 = true; }               // 0 - 1
        else if (neg1) inc(m1, 4);                           // -(m) - 1 = -(m + 1)
        else dec(m1, 4);                                     // m - 1
    } else { for (int j = 0; j < 4; j++) m2[j] = q[j]; }
}
__device__ __forceinline__ void load_scalar_words(const Fr *scalars, size_t i, uint32_t (&k)[8]) {
    const uint4 *p = (const uint4 *)scalars[i].l; const uint4 a = p[0], b = p[1];
    k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
}
__global__ __launch_bounds__(256) void k_glv_split(const Fr *scalars, size_t n, Fr *out) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8], m1[4], m2[4]; bool neg1, neg2;
    load_scalar_words(scalars, i, k);
    glv_split_scalar(k, m1, neg1, m2, neg2);
    uint4 *o0 = (uint4 *)out[2 * i].l, *o1 = (uint4 *)out[2 * i + 1].l;
    o0[0] = make_uint4(m1[0], m1[1], m1[2], m1[3]); o0[1] = make_uint4(0, 0, 0, neg1 ? 0x80000000u : 0u);
    o1[0] = make_uint4(m2[0], m2[1], m2[2], m2[3]); o1[1] = make_uint4(0, 0, 0, neg2 ? 0x80000000u : 0u);
}

__global__ void k_count(const Fr *scalars, MsmGeom g, uint32_t *cnt) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    for_each_digit(scalars, i, g, [&](unsigned w, uint32_t b, bool) { atomicAdd(&cnt[bucket_of(g, w, b)], 1u); });
}

__global__ void k_scatter(const Fr *scalars, MsmGeom g, uint32_t *cursor, uint32_t *sorted) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    for_each_digit(scalars, i, g, [&](unsigned w, uint32_t b, bool neg) {
        uint32_t pos = atomicAdd(&cursor[bucket_of(g, w, b)], 1u);
        sorted[pos] = entry_of(g, w, i) | (neg ? 0x80000000u : 0u);
    });
}

// ------------------------------------------------------------------------------------------------
// counters[1] = number of scalars that are neither 0 nor 1.  Real witnesses are mostly boolean wires
// (multiexp_with_mixed_addition's case): the window size is chosen from this count, not from n.
// counters[3] != 0: some scalar is not canonical (>= r) -- the digits of such a value would silently give another point
// (include/vsp.h promises VSP_ERR_ARG for it; the reference's field type cannot even hold such a value).
__device__ __forceinline__ bool scalar_below_r(const uint4 &lo, const uint4 &hi) {
    // r = 0x73eda753299d7d48 3339d80809a1d805 53bda402fffe5bfe ffffffff00000001, compared from the top 32-bit word down
    const uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t r[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    bool lt = false, gt = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt = lt || (!gt && k[i] < r[i]);
        gt = gt || (!lt && k[i] > r[i]);
    }
    return lt;
}
__global__ __launch_bounds__(256) void k_classify(const Fr *scalars, size_t n, uint32_t *counters, size_t kstride) {
    __shared__ uint32_t blk, bad;
    scalars += (size_t)blockIdx.y * kstride;                 // grid.y: the vectors of a batch, counted together
    if (threadIdx.x == 0) { blk = 0; bad = 0; }
    __syncthreads();
    uint32_t mine = 0, mybad = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 *k = (const uint4 *)scalars[i].l;
        uint4 lo = k[0], hi = k[1];
        uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
        mine += (rest != 0 || lo.x > 1) ? 1u : 0u;
        if (hi.w >= 0x73eda753u && !scalar_below_r(lo, hi)) mybad = 1;
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&blk, mine);
    if (mybad) bad = 1;
    __syncthreads();
    if (threadIdx.x == 0 && blk) atomicAdd(&counters[1], blk);          // one global atomic per workgroup
    if (threadIdx.x == 0 && bad) atomicOr(&counters[3], 1u);
}

// ------------------------------------------------------------------------------------------------
// LDS-privatised counting sort (c <= 16, large n): the 2 * n * W global atomics of k_count / k_scatter become LDS
// atomics.  A 1024-thread workgroup owns one (chunk of scalars, window) pair and keeps that window's 2^(c-1) counters
// in LDS (128 KiB at c = 16 -- the reason this needs CDNA's 160 KiB LDS).
#ifndef VSP_CS_ATTR
#define VSP_CS_ATTR
#endif
#ifndef VSP_CS_UNROLL
#define VSP_CS_UNROLL
#endif
#ifndef VSP_CS_THREADS
#define VSP_CS_THREADS 1024
#endif
static constexpr unsigned CS_THREADS = VSP_CS_THREADS;
static constexpr unsigned CS_MLP = 8;                         // digit loads in flight per thread in the LDS counting sort
static constexpr uint16_t DIGIT_NONE = 0xFFFFu;

// digits[w * n + i] = DIGIT_NONE for a zero digit, else (|d| - 1) | (d < 0) << 15     (|d| - 1 <= 32767, negative ones <= 32766)
// flips[i] (endomorphism split only) = 1 when scalar i is a negative half: its digits are stored unflipped -- a flipped digit of
// magnitude 2^15 would collide with DIGIT_NONE -- and k_scatter_lds applies the sign when it writes the sorted entry
// (grid.y = the vector of a batch, MsmGeom.K: its scalars start blockIdx.y * kstride elements on, its windows blockIdx.y * Wk windows on)
__global__ __launch_bounds__(256) void k_digits(const Fr *scalars, MsmGeom g, uint16_t *digits, uint8_t *flips) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    const unsigned kb = blockIdx.y;
    scalars += (size_t)kb * g.kstride;
    uint32_t k[8];
    const uint32_t flip = load_scalar(scalars, i, g, k);
    uint32_t carry = 0;
    if (g.sbits == 128u || g.fold) flips[(size_t)kb * g.n + i] = (uint8_t)flip;
    for (unsigned w = 0; w < g.Wk; w++) {
        uint32_t raw = scalar_bits(k, w * g.c, g.c) + carry;
        uint32_t mag; uint32_t neg;
        if (raw > g.B) { mag = (1u << g.c) - raw; neg = 1; carry = 1; }
        else { mag = raw; neg = 0; carry = 0; }
        digits[(size_t)(kb * g.Wk + w) * g.n + i] = mag ? (uint16_t)((mag - 1) | (neg << 15)) : DIGIT_NONE;
    }
}
// The split and the digits in one pass over the scalars (the LDS-sort path of split multi-exponentiations): thread i reads scalar i once and
// writes the digits of both halves, entries 2i and 2i + 1 of every window, as one 32-bit store -- no 2n x 32-byte array of split scalars
// written by one kernel and read back by the next (128 MB per 2^20-point multi-exponentiation; VERDICT round 2, weak 5).
__global__ __launch_bounds__(256) void k_glv_digits(const Fr *scalars, size_t n_orig, MsmGeom g, uint16_t *digits, uint8_t *flips) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_orig) return;
    const unsigned kb = blockIdx.y;                           // the vector of a batch (k_digits)
    scalars += (size_t)kb * g.kstride;
    flips += (size_t)kb * g.n;
    uint32_t k[8], m[2][8]; bool neg[2];
    load_scalar_words(scalars, i, k);
    {
        uint32_t m1[4], m2[4];
        glv_split_scalar(k, m1, neg[0], m2, neg[1]);
#pragma unroll
        for (int j = 0; j < 8; j++) { m[0][j] = j < 4 ? m1[j] : 0u; m[1][j] = j < 4 ? m2[j] : 0u; }
    }
    reinterpret_cast<uint16_t *>(flips)[i] = (uint16_t)((neg[0] ? 1u : 0u) | (neg[1] ? 0x100u : 0u));      // flips[2i], flips[2i + 1]
    uint32_t carry[2] = {0, 0};
    uint32_t *d32 = reinterpret_cast<uint32_t *>(digits);
    for (unsigned w = 0; w < g.Wk; w++) {
        uint32_t pair = 0;
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const uint32_t raw = scalar_bits(m[b], w * g.c, g.c) + carry[b];
            uint32_t mag, ng;
            if (raw > g.B) { mag = (1u << g.c) - raw; ng = 1; carry[b] = 1; }
            else { mag = raw; ng = 0; carry[b] = 0; }
            const uint32_t d = mag ? ((mag - 1) | (ng << 15)) : (uint32_t)DIGIT_NONE;
            pair |= d << (16 * b);
        }
        d32[((size_t)(kb * g.Wk + w) * g.n) / 2 + i] = pair;   // g.n = 2 n_orig: digits[w * g.n + 2i], [.. + 2i + 1]
    }
}

// Windows wider than 16 bits (c = 17 .. 23).  The bucket index |d| - 1 has c - 1 bits: the HIGH 15 go through the LDS counting sort above
// exactly as a 16-bit window's index does (hi[w * n + i], DIGIT_NONE for a zero digit), the low lb = c - 16 bits and the sign (digit sign
// xor the split half's sign: bit 7) travel beside them in a byte; a second pass (k_segment_sort) orders each of the 2^15 segments per
// window by those low bits.  Two passes cost ~1.1 x one; what they buy is fewer windows: at 2^26 points c = 22 is 12 windows instead of 16.
__global__ __launch_bounds__(256) void k_digits_wide(const Fr *scalars, MsmGeom g, uint16_t *hi, uint8_t *lo) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    uint32_t k[8];
    const uint32_t flip = load_scalar(scalars, i, g, k);
    uint32_t carry = 0;
    for (unsigned w = 0; w < g.W; w++) {
        uint32_t raw = scalar_bits(k, w * g.c, g.c) + carry;
        uint32_t mag, neg;
        if (raw > g.B) { mag = (1u << g.c) - raw; neg = 1; carry = 1; }
        else { mag = raw; neg = 0; carry = 0; }
        const uint32_t v = mag - 1u;
        hi[(size_t)w * g.n + i] = mag ? (uint16_t)(v >> g.lb) : DIGIT_NONE;
        lo[(size_t)w * g.n + i] = mag ? (uint8_t)((v & ((1u << g.lb) - 1u)) | ((neg ^ flip) << 7)) : (uint8_t)0;
    }
}

// blockhist[chunk][w][b] = number of digits of value b in (chunk, w)
__global__ __launch_bounds__(CS_THREADS) VSP_CS_ATTR void k_count_lds(const uint16_t *digits, MsmGeom g, unsigned nchunks, size_t chunk_len, uint32_t *blockhist) {
    extern __shared__ uint32_t lds_hist[];
    const unsigned w = blockIdx.x % g.W, chunk = blockIdx.x / g.W;
    VSP_CS_UNROLL
    for (unsigned b = threadIdx.x; b < g.B; b += CS_THREADS) lds_hist[b] = 0;
    __syncthreads();
    const size_t i0 = (size_t)chunk * chunk_len, i1 = i0 + chunk_len < g.n ? i0 + chunk_len : g.n;
    const uint16_t *dw = digits + (size_t)w * g.n;
    for (size_t base = i0; base < i1; base += (size_t)CS_MLP * CS_THREADS) {      // CS_MLP loads in flight per thread, as in k_scatter_lds
        uint16_t dd[CS_MLP];
#pragma unroll
        for (unsigned j = 0; j < CS_MLP; j++) { const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x; dd[j] = i < i1 ? dw[i] : DIGIT_NONE; }
#pragma unroll
        for (unsigned j = 0; j < CS_MLP; j++) {
            const uint16_t d = dd[j];
            const bool valid = d != DIGIT_NONE;
            const uint32_t key = d & 0x7FFFu;
            // one hot bucket (the scalars equal to one of a boolean witness: half of window 0) would serialise 64 LDS atomics per wave:
            // the lanes that share the first valid lane's bucket send ONE atomic of their count
            const unsigned long long act = __ballot(valid);
            if (act) {
                const int lead = __ffsll((long long)act) - 1;
                const uint32_t lkey = (uint32_t)__shfl((int)key, lead, 64);
                const bool same = valid && key == lkey;
                const unsigned long long grp = __ballot(same);
                if (same) { if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&lds_hist[lkey], (uint32_t)__popcll(grp)); }
                else if (valid) atomicAdd(&lds_hist[key], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *out = blockhist + ((size_t)chunk * g.W + w) * g.B;
    VSP_CS_UNROLL
    for (unsigned b = threadIdx.x; b < g.B; b += CS_THREADS) out[b] = lds_hist[b];
}

// per bucket: cnt = sum over the `nsets` partial histograms (stride G apart); blockhist becomes their exclusive prefix.
// Separate bucket sets per window: nsets = chunks, G = W*B.  Single set: nsets = chunks*W, G = B.
__device__ __forceinline__ void block_sum_to(uint32_t v, uint32_t *dst);
// A batch in the shared-set mode: K bucket sets of set_len = B buckets, each fed by its own nsets = Wk histograms, which lie one after the other
// (set_len = G everywhere else: one group of nsets histograms G apart).
__global__ __launch_bounds__(256) void k_chunk_prefix(uint32_t *blockhist, unsigned nsets, size_t G, uint32_t *cnt, uint32_t *tilesum, size_t set_len) {
    size_t gi = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t run = 0;
    if (gi < G) {
        const size_t base = (gi / set_len) * nsets * set_len + gi % set_len;
        for (unsigned c = 0; c < nsets; c++) {
            uint32_t t = blockhist[base + (size_t)c * set_len];
            blockhist[base + (size_t)c * set_len] = run;
            run += t;
        }
        cnt[gi] = run;
    }
    if (tilesum) block_sum_to(run, &tilesum[blockIdx.x]);         // the scan that follows (k_scan_tiles256) starts from these
}

__global__ __launch_bounds__(CS_THREADS) VSP_CS_ATTR void k_scatter_lds(const uint16_t *digits, const uint8_t *flips, MsmGeom g, unsigned nchunks, size_t chunk_len,
                                                            const uint32_t *blockhist, const uint32_t *off, uint32_t *sorted,
                                                            const uint8_t *lo_in, uint8_t *lo_out) {      // wide windows: the low-bits byte travels with the entry
    extern __shared__ uint32_t lds_cur[];
    const unsigned w = blockIdx.x % g.W, chunk = blockIdx.x / g.W;
    const size_t gbase = g.single ? (size_t)(w / g.Wk) * g.B : (size_t)w * g.B;
    const uint32_t *pre = blockhist + ((size_t)chunk * g.W + w) * g.B;
    VSP_CS_UNROLL
    for (unsigned b = threadIdx.x; b < g.B; b += CS_THREADS) lds_cur[b] = off[gbase + b] + pre[b];
    __syncthreads();
    const size_t i0 = (size_t)chunk * chunk_len, i1 = i0 + chunk_len < g.n ? i0 + chunk_len : g.n;
    const uint16_t *dw = digits + (size_t)w * g.n;
    const bool use_flips = !lo_in && (g.sbits == 128u || g.fold);
    // CS_MLP digits (and their sign bytes) are requested before the first of them is used.  (Measured: k_count_lds 40 -> 30 us; this
    // kernel stays at 0.21 ms for 16.7 M entries -- it is bound by its 16.7 M scattered 4-byte writes, not by the digit loads.)
    for (size_t base = i0; base < i1; base += (size_t)CS_MLP * CS_THREADS) {
        uint16_t dd[CS_MLP]; uint8_t ff[CS_MLP];
#pragma unroll
        for (unsigned j = 0; j < CS_MLP; j++) {
            const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x;
            dd[j] = i < i1 ? dw[i] : DIGIT_NONE;
            ff[j] = (use_flips && i < i1) ? flips[(size_t)(w / g.Wk) * g.n + i] : (uint8_t)0;      // (one sign byte per scalar of every vector of a batch)
        }
#pragma unroll
        for (unsigned j = 0; j < CS_MLP; j++) {
            const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x;
            const uint16_t d = dd[j];
            const bool valid = d != DIGIT_NONE;
            const uint32_t key = d & 0x7FFFu;
            const unsigned long long act = __ballot(valid);
            if (act) {
                // as k_count_lds: the lanes sharing the first valid lane's bucket take their positions from one atomic
                const int lead = __ffsll((long long)act) - 1;
                const uint32_t lkey = (uint32_t)__shfl((int)key, lead, 64);
                const bool same = valid && key == lkey;
                const unsigned long long grp = __ballot(same);
                const unsigned lane = threadIdx.x & 63u;
                uint32_t pos = 0;
                if (same && (int)lane == lead) pos = atomicAdd(&lds_cur[lkey], (uint32_t)__popcll(grp));
                pos = (uint32_t)__shfl((int)pos, lead, 64) + (uint32_t)__popcll(grp & ((1ull << lane) - 1ull));
                if (valid && !same) pos = atomicAdd(&lds_cur[key], 1u);
                if (valid) {
                    uint32_t sign;
                    if (lo_in) { const uint8_t l = lo_in[(size_t)w * g.n + i]; sign = l >> 7; lo_out[pos] = l & 0x7Fu; }
                    else sign = (uint32_t)(d >> 15) ^ (uint32_t)ff[j];
                    sorted[pos] = entry_of(g, w, i) | (sign << 31);
                }
            }
        }
    }
}

// Second pass of the wide-window sort: ONE WAVE per segment (the entries of one (window, high 15 bits) pair, contiguous in tmp after the
// first pass: n / 2^15 of them on average) orders it by the low lb <= 7 bits and writes, for its 2^lb buckets, their counts and offsets
// -- no global scan over the 2^(c-1) buckets per window is needed: a bucket starts at its segment's start plus a prefix inside the wave.
// The lanes of a wave that hold equal low bits find each other by lb ballots (a multisplit); the group's first lane takes the group's
// positions from a wave-private LDS counter.
__global__ __launch_bounds__(256) void k_segment_sort(const uint32_t *__restrict__ tmp_sorted, const uint8_t *__restrict__ tmp_lo, const uint32_t *__restrict__ off_hi,
                                                     size_t segments, unsigned lb, uint32_t *cnt, uint32_t *off, uint32_t *sorted) {
    __shared__ uint32_t sh[4][128];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t *c = sh[wave];
    const unsigned nb = 1u << lb;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (size_t s = (size_t)blockIdx.x * 4 + wave; s < segments; s += (size_t)gridDim.x * 4) {
        const uint32_t a = off_hi[s], b = off_hi[s + 1];
        c[lane] = 0; c[lane + 64] = 0;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j0 = a; j0 < b; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool valid = j < b;
            const uint32_t l = valid ? tmp_lo[j] : 0u;
            unsigned long long peers = __ballot(valid);
            for (unsigned k = 0; k < lb; k++) { const bool bit = (l >> k) & 1u; const unsigned long long m = __ballot(valid && bit); peers &= bit ? m : ~m; }
            if (valid && (int)lane == __ffsll((long long)peers) - 1) atomicAdd(&c[l], (uint32_t)__popcll(peers));
        }
        __builtin_amdgcn_wave_barrier();
        // exclusive prefix over the <= 128 bins: lane holds bins lane and lane + 64
        const uint32_t c0 = c[lane], c1 = c[lane + 64];
        uint32_t i0 = c0, i1 = c1;
        for (int d = 1; d < 64; d <<= 1) { uint32_t x0 = __shfl_up(i0, d, 64), x1 = __shfl_up(i1, d, 64); if ((int)lane >= d) { i0 += x0; i1 += x1; } }
        const uint32_t tot0 = __shfl(i0, 63, 64);
        const uint32_t e0 = a + i0 - c0, e1 = a + tot0 + i1 - c1;
        const size_t g0 = (s << lb) + lane;
        if (lane < nb) { cnt[g0] = c0; off[g0] = e0; }
        if (lane + 64 < nb) { cnt[g0 + 64] = c1; off[g0 + 64] = e1; }
        __builtin_amdgcn_wave_barrier();
        c[lane] = e0; c[lane + 64] = e1;                           // the bins' cursors
        __builtin_amdgcn_wave_barrier();
        for (uint32_t j0 = a; j0 < b; j0 += 64) {
            const uint32_t j = j0 + lane;
            const bool valid = j < b;
            const uint32_t l = valid ? tmp_lo[j] : 0u;
            unsigned long long peers = __ballot(valid);
            for (unsigned k = 0; k < lb; k++) { const bool bit = (l >> k) & 1u; const unsigned long long m = __ballot(valid && bit); peers &= bit ? m : ~m; }
            const int lead = valid ? __ffsll((long long)peers) - 1 : (int)lane;
            uint32_t base = 0;
            if (valid && (int)lane == lead) base = atomicAdd(&c[l], (uint32_t)__popcll(peers));
            base = (uint32_t)__shfl((int)base, lead, 64);
            if (valid) sorted[base + (uint32_t)__popcll(peers & below)] = tmp_sorted[j];
        }
        if (s == segments - 1 && lane == 0) off[segments << lb] = b;      // the end of the last bucket = the number of entries
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// Staged sort for LARGE wide-window problems (2^20 points and up, c >= 17).  The LDS counting sort above scatters every entry straight to
// its bucket: 2^15 open write cursors per workgroup, 4 bytes at a time, into an array of gigabytes -- at 2^26 points every write is its
// own DRAM sector (39 ms for the first pass, 34 ms for the second, against 107 ms of accumulation).  Here the bucket index (c - 1 =
// 16 + rb bits) is consumed EIGHT bits at a time: a pass splits its input 256 ways through a 4096-element LDS tile, so that what leaves
// for global memory are runs of ~16 entries per bin (128 bytes: whole lines).  Two such passes order the top 16 bits; what is left of a
// bucket index (rb = c - 17 <= 6 bits) is ordered inside LDS by one wave per segment (~n / 2^16 entries), which also writes the buckets'
// counts and offsets.  Elements are pairs {entry | sign << 31, bucket index} (no digit: index ~0, parked behind everything).
static constexpr unsigned MS_THREADS = 1024, MS_TILE = 8192, MS_CHUNK = 65536;
__global__ __launch_bounds__(256) void k_ms_pairs(const Fr *scalars, MsmGeom g, uint2 *pairs) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    uint32_t k[8];
    const uint32_t flip = load_scalar(scalars, i, g, k);
    uint32_t carry = 0;
    for (unsigned w = 0; w < g.W; w++) {
        uint32_t raw = scalar_bits(k, w * g.c, g.c) + carry;
        uint32_t mag, neg;
        if (raw > g.B) { mag = (1u << g.c) - raw; neg = 1; carry = 1; }
        else { mag = raw; neg = 0; carry = 0; }
        pairs[(size_t)w * g.n + i] = make_uint2(entry_of(g, w, i) | ((neg ^ flip) << 31), mag ? mag - 1u : 0xFFFFFFFFu);
    }
}
// One splitting pass.  Pass 1 (seg == nullptr): unit = (parent, chunk), parents of npp elements; histogram slot of bin b:
// H[(parent * 256 + b) * chunks + chunk], of the parked entries: H[parents * 256 * chunks + parent * chunks + chunk] (an exclusive scan
// of H in that order is where every (parent, bin, chunk) run goes).  Passes 2 and 3 (seg != nullptr): unit = a PIECE: MS_CHUNK elements
// of a segment of the pass before (segment s = seg[s * seg_stride] .. seg[(s + 1) * seg_stride]; its pieces are numbered
// pbase[s] .. pbase[s + 1] - 1); histogram slot of bin b: H[piece * slots + b].  Consecutive workgroups read consecutive memory in every
// pass: one workgroup per whole segment (2 MiB each at 2^26 points, all about equally long) left all running workgroups on the same
// memory channels at the same moment -- 32 ms for the histogram and 65 ms for the scatter of the second pass, against 1.3 and 3.9 ms for
// the first over the same data.
struct MsPass {
    size_t npp; unsigned parents, chunks;                   // pass 1
    const uint32_t *seg; unsigned seg_stride; const uint32_t *pbase; unsigned S;      // passes 2, 3: segments and their pieces
    unsigned shift, mask, bins, slots;                       // bin = (key >> shift) & mask; bins = mask + 1; histogram slots per piece
};
__device__ __forceinline__ unsigned ms_bin(uint32_t key, const MsPass &ps) { return key == 0xFFFFFFFFu ? 256u : ((key >> ps.shift) & ps.mask); }
struct MsUnit { size_t a, b; size_t cur_base, cur_stride, park, bin_base; bool live; };
__device__ __forceinline__ MsUnit ms_unit(const MsPass &ps) {
    MsUnit u;
    if (!ps.seg) {
        const unsigned parent = blockIdx.x / ps.chunks, chunk = blockIdx.x % ps.chunks;
        u.a = (size_t)parent * ps.npp + (size_t)chunk * MS_CHUNK;
        const size_t e = (size_t)parent * ps.npp + ps.npp;
        u.b = u.a + MS_CHUNK < e ? u.a + MS_CHUNK : e;
        u.cur_base = (size_t)parent * 256 * ps.chunks + chunk; u.cur_stride = ps.chunks;
        u.park = (size_t)ps.parents * 256 * ps.chunks + (size_t)parent * ps.chunks + chunk; u.bin_base = 0; u.live = true;
    } else {
        const uint32_t id = blockIdx.x;
        u.a = u.b = 0; u.cur_base = (size_t)id * ps.slots; u.cur_stride = 1; u.park = 0; u.bin_base = 0;
        u.live = id < ps.pbase[ps.S];                                 // the grid is sized for the worst case
        if (u.live) {
            unsigned lo = 0, hi = ps.S;                               // the segment with pbase[s] <= id < pbase[s + 1]
            while (hi - lo > 1) { const unsigned mid = (lo + hi) >> 1; if (ps.pbase[mid] <= id) lo = mid; else hi = mid; }
            const size_t s0 = ps.seg[(size_t)lo * ps.seg_stride], s1 = ps.seg[((size_t)lo + 1) * ps.seg_stride];
            u.a = s0 + (size_t)(id - ps.pbase[lo]) * MS_CHUNK;
            u.b = u.a + MS_CHUNK < s1 ? u.a + MS_CHUNK : s1;
            u.bin_base = (size_t)lo * ps.bins;
        }
    }
    return u;
}
// pieces per segment: every segment (pass 2: min_len = 0) or only those the last step does not order inside one wave (pass 3); an
// exclusive scan of pc[0 .. S] (pc[S] = 0) gives pbase
__global__ __launch_bounds__(MSM_THREADS) void k_ms_piece_counts(const uint32_t *seg, unsigned seg_stride, size_t S, uint32_t min_len, uint32_t *pc) {
    const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    uint32_t v = 0;
    if (s < S) { const uint32_t len = seg[(s + 1) * seg_stride] - seg[s * seg_stride]; if (len > min_len) v = (len + MS_CHUNK - 1) / MS_CHUNK; }
    pc[s] = v;
}
// second pass: one workgroup per segment, one thread per bin: the pieces' counts become running offsets inside the bin, and the bins'
// totals the starts of the (segment, bin) ranges: Hb[s * bins + b] (Hb[S1 * bins] = where the parked entries begin)
__global__ __launch_bounds__(256) void k_ms_cursors(uint32_t *H, const uint32_t *pbase, const uint32_t *seg, unsigned seg_stride, unsigned S1, unsigned bins, uint32_t *Hb) {
    __shared__ uint32_t sh[256];
    const unsigned s = blockIdx.x, t = threadIdx.x;
    uint32_t run = 0;
    if (t < bins) for (uint32_t p = pbase[s]; p < pbase[s + 1]; p++) { const uint32_t v = H[(size_t)p * 256 + t]; H[(size_t)p * 256 + t] = run; run += v; }
    sh[t] = run;
    __syncthreads();
    for (unsigned d = 1; d < 256; d <<= 1) { const uint32_t x = t >= d ? sh[t - d] : 0; __syncthreads(); sh[t] += x; __syncthreads(); }
    if (t < bins) Hb[(size_t)s * bins + t] = seg[(size_t)s * seg_stride] + sh[t] - run;
    if (s == S1 - 1 && t == 0) Hb[(size_t)S1 * bins] = seg[(size_t)S1 * seg_stride];
}
__global__ __launch_bounds__(MS_THREADS) void k_ms_hist(const uint2 *__restrict__ in, MsPass ps, uint32_t *H) {
    __shared__ uint32_t h[257];
    for (unsigned t = threadIdx.x; t < 257; t += MS_THREADS) h[t] = 0;
    __syncthreads();
    const MsUnit u = ms_unit(ps);
    if (!u.live) return;
    // eight independent loads in flight per thread: one load per iteration leaves the kernel waiting out a memory latency per 8 bytes
    // (380 GB/s measured at 2^26 points)
    for (size_t i = u.a + threadIdx.x; i < u.b; i += 8 * MS_THREADS) {
        uint32_t key[8]; bool live[8];
#pragma unroll
        for (unsigned j = 0; j < 8; j++) { const size_t idx = i + (size_t)j * MS_THREADS; live[j] = idx < u.b; key[j] = live[j] ? in[idx].y : 0u; }
#pragma unroll
        for (unsigned j = 0; j < 8; j++) if (live[j]) atomicAdd(&h[ms_bin(key[j], ps)], 1u);
    }
    __syncthreads();
    for (unsigned t = threadIdx.x; t < ps.slots; t += MS_THREADS) H[u.cur_base + (size_t)t * u.cur_stride] = h[t];
    if (!ps.seg && threadIdx.x == 0) H[u.park] = h[256];
}
// Hs: where this unit's run of every bin goes (pass 1: absolute; pass 2: inside the (segment, bin) range that starts at Hb[...]; pass 3:
// absolute, Hb == nullptr).  out_entries != nullptr (pass 3): the bucket index is used up -- only the entries leave, into the sorted array.
__global__ __launch_bounds__(MS_THREADS) void k_ms_scatter(const uint2 *__restrict__ in, uint2 *__restrict__ out, uint32_t *__restrict__ out_entries, MsPass ps,
                                                          const uint32_t *Hs, const uint32_t *Hb) {
    __shared__ uint32_t cur[257], tcnt[257], toff[258];
    __shared__ uint2 buf[MS_TILE];
    const MsUnit u = ms_unit(ps);
    if (!u.live || u.a >= u.b) return;
    const unsigned tid = threadIdx.x;
    for (unsigned t = tid; t < 257; t += MS_THREADS) {
        uint32_t v = 0;
        if (t < ps.bins) v = Hs[u.cur_base + (size_t)t * u.cur_stride] + (Hb ? Hb[u.bin_base + t] : 0u);
        else if (t == 256 && !ps.seg) v = Hs[u.park];
        cur[t] = v; tcnt[t] = 0;
    }
    __syncthreads();
    for (size_t base = u.a; base < u.b; base += MS_TILE) {
        uint2 e[MS_TILE / MS_THREADS]; unsigned bin[MS_TILE / MS_THREADS], rk[MS_TILE / MS_THREADS];
#pragma unroll
        for (unsigned k = 0; k < MS_TILE / MS_THREADS; k++) {        // all the tile's loads first (eight in flight per thread), then the LDS atomics
            const size_t i = base + (size_t)k * MS_THREADS + tid;
            bin[k] = 0xFFFFu; rk[k] = 0; e[k] = make_uint2(0u, 0u);
            if (i < u.b) { e[k] = in[i]; bin[k] = 0u; }
        }
#pragma unroll
        for (unsigned k = 0; k < MS_TILE / MS_THREADS; k++)
            if (bin[k] != 0xFFFFu) { bin[k] = ms_bin(e[k].y, ps); rk[k] = atomicAdd(&tcnt[bin[k]], 1u); }
        __syncthreads();
        if (tid < 64) {                                       // exclusive prefix of the 257 tile counts: lane L takes bins 4L .. 4L + 3
            const uint32_t v0 = tcnt[4 * tid], v1 = tcnt[4 * tid + 1], v2 = tcnt[4 * tid + 2], v3 = tcnt[4 * tid + 3];
            uint32_t incl = v0 + v1 + v2 + v3;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(incl, d, 64); if ((int)tid >= d) incl += x; }
            const uint32_t ex = incl - (v0 + v1 + v2 + v3);
            toff[4 * tid] = ex; toff[4 * tid + 1] = ex + v0; toff[4 * tid + 2] = ex + v0 + v1; toff[4 * tid + 3] = ex + v0 + v1 + v2;
            if (tid == 63) { toff[256] = incl; toff[257] = incl + tcnt[256]; }
        }
        __syncthreads();
#pragma unroll
        for (unsigned k = 0; k < MS_TILE / MS_THREADS; k++) if (bin[k] != 0xFFFFu) buf[toff[bin[k]] + rk[k]] = e[k];
        __syncthreads();
        const unsigned count = toff[257];
        for (unsigned i = tid; i < count; i += MS_THREADS) {
            const uint2 x = buf[i];
            const unsigned bn = ms_bin(x.y, ps);
            const size_t at = (size_t)cur[bn] + (i - toff[bn]);
            if (out_entries) out_entries[at] = x.x; else out[at] = x;
        }
        __syncthreads();
        if (tid < 257) { cur[tid] += tcnt[tid]; tcnt[tid] = 0; }
        __syncthreads();
    }
}
// The last step: ONE WAVE per segment of the second pass (all entries that share the top 16 bits of their bucket index in one parent:
// ~n / 2^16 of them) orders it by the remaining rb <= 6 bits and writes the counts and offsets of its 2^rb buckets.  Segments of up to
// MS_SEG_CAP entries are ordered in registers and LDS and leave as one coalesced run; up to MS_SEG_LONG a wave walks them twice in
// global memory; LONGER ones -- the top window's always are (its digits have few bits: 2^18 entries per segment at 2^26 points, which
// one wave walked for 14 ms), and so are those of skewed scalars -- went through a third splitting pass in pieces (k_ms_hist before this
// kernel, k_ms_scatter after it): here their pieces' histogram slots H3[piece * 64 + bucket] become the pieces' cursors.
static constexpr unsigned MS_SEG_CAP = 1536, MS_SEG_LONG = 8192;
__global__ __launch_bounds__(256) void k_ms_final(const uint2 *__restrict__ in, const uint32_t *__restrict__ seg, size_t segments, unsigned rb,
                                                 const uint32_t *__restrict__ pbase3, uint32_t *H3, uint32_t *cnt, uint32_t *off, uint32_t *sorted) {
    __shared__ uint32_t c_[4][64], ord_[4][MS_SEG_CAP];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t *c = c_[wave], *ord = ord_[wave];
    const unsigned nb = 1u << rb, mask = nb - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    constexpr unsigned PER = MS_SEG_CAP / 64;
    for (size_t s = (size_t)blockIdx.x * 4 + wave; s < segments; s += (size_t)gridDim.x * 4) {
        const uint32_t a = seg[s], b = seg[s + 1], len = b - a;
        c[lane] = 0;
        __builtin_amdgcn_wave_barrier();
        if (len <= MS_SEG_CAP) {
            // the whole segment in registers (all its loads in flight at once), ONE matching pass: an entry's place = the start of its
            // bucket (known after the count) + how many entries of that bucket came before it (known when it is counted)
            uint2 x[PER]; uint32_t pos[PER];
#pragma unroll
            for (unsigned q = 0; q < PER; q++) { const uint32_t j = 64 * q + lane; x[q] = j < len ? in[(size_t)a + j] : make_uint2(0u, 0u); }
#pragma unroll
            for (unsigned q = 0; q < PER; q++) {
                pos[q] = 0;
                if (64 * q < len) {
                    const bool valid = 64 * q + lane < len;
                    const uint32_t l = x[q].y & mask;
                    unsigned long long peers = __ballot(valid);
                    for (unsigned k = 0; k < rb; k++) { const bool bit = (l >> k) & 1u; const unsigned long long m = __ballot(valid && bit); peers &= bit ? m : ~m; }
                    const int lead = valid ? __ffsll((long long)peers) - 1 : (int)lane;
                    uint32_t base = 0;
                    if (valid && (int)lane == lead) base = atomicAdd(&c[l], (uint32_t)__popcll(peers));
                    base = (uint32_t)__shfl((int)base, lead, 64);
                    pos[q] = base + (uint32_t)__popcll(peers & below);
                }
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t c0 = c[lane];
            uint32_t i0 = c0;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t x0 = __shfl_up(i0, d, 64); if ((int)lane >= d) i0 += x0; }
            const uint32_t e0 = i0 - c0;                          // exclusive prefix inside the segment
            if (lane < nb) { cnt[(s << rb) + lane] = c0; off[(s << rb) + lane] = a + e0; }
            __builtin_amdgcn_wave_barrier();
            c[lane] = e0;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (unsigned q = 0; q < PER; q++) if (64 * q + lane < len) ord[c[x[q].y & mask] + pos[q]] = x[q].x;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j = lane; j < len; j += 64) sorted[(size_t)a + j] = ord[j];
        } else if (len > MS_SEG_LONG) {
            // the entries are placed by the third pass; lane = bucket: counts, offsets, and the pieces' cursors
            const uint32_t p0 = pbase3[s], p1 = pbase3[s + 1];
            uint32_t c0 = 0;
            for (uint32_t p = p0; p < p1; p++) c0 += H3[(size_t)p * 64 + lane];
            uint32_t i0 = c0;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t x0 = __shfl_up(i0, d, 64); if ((int)lane >= d) i0 += x0; }
            const uint32_t e0 = i0 - c0;
            if (lane < nb) { cnt[(s << rb) + lane] = c0; off[(s << rb) + lane] = a + e0; }
            uint32_t run = a + e0;
            for (uint32_t p = p0; p < p1; p++) { const uint32_t v = H3[(size_t)p * 64 + lane]; H3[(size_t)p * 64 + lane] = run; run += v; }
        } else {
            // count, then place, both from global memory
            for (uint32_t j0 = a; j0 < b; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool valid = j < b;
                const uint32_t l = valid ? (in[j].y & mask) : 0u;
                unsigned long long peers = __ballot(valid);
                for (unsigned k = 0; k < rb; k++) { const bool bit = (l >> k) & 1u; const unsigned long long m = __ballot(valid && bit); peers &= bit ? m : ~m; }
                if (valid && (int)lane == __ffsll((long long)peers) - 1) atomicAdd(&c[l], (uint32_t)__popcll(peers));
            }
            __builtin_amdgcn_wave_barrier();
            const uint32_t c0 = c[lane];
            uint32_t i0 = c0;
            for (int d = 1; d < 64; d <<= 1) { const uint32_t x0 = __shfl_up(i0, d, 64); if ((int)lane >= d) i0 += x0; }
            const uint32_t e0 = i0 - c0;
            if (lane < nb) { cnt[(s << rb) + lane] = c0; off[(s << rb) + lane] = a + e0; }
            __builtin_amdgcn_wave_barrier();
            c[lane] = e0;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j0 = a; j0 < b; j0 += 64) {
                const uint32_t j = j0 + lane;
                const bool valid = j < b;
                uint32_t entry = 0, l = 0;
                if (valid) { const uint2 x = in[j]; entry = x.x; l = x.y & mask; }
                unsigned long long peers = __ballot(valid);
                for (unsigned k = 0; k < rb; k++) { const bool bit = (l >> k) & 1u; const unsigned long long m = __ballot(valid && bit); peers &= bit ? m : ~m; }
                const int lead = valid ? __ffsll((long long)peers) - 1 : (int)lane;
                uint32_t base = 0;
                if (valid && (int)lane == lead) base = atomicAdd(&c[l], (uint32_t)__popcll(peers));
                base = (uint32_t)__shfl((int)base, lead, 64);
                if (valid) sorted[(size_t)a + base + (uint32_t)__popcll(peers & below)] = entry;
            }
        }
        if (s == segments - 1 && lane == 0) off[segments << rb] = b;
        __builtin_amdgcn_wave_barrier();
    }
}

// ------------------------------------------------------------------------------------------------
// exclusive scan of uint32 (three small kernels; arrays are <= a few million entries)
static constexpr unsigned SCAN_ITEMS = 8;                       // per thread
static constexpr unsigned SCAN_TILE = MSM_THREADS * SCAN_ITEMS;  // 2048 per block

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t sh[MSM_THREADS];
    unsigned t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (unsigned s = 1; s < MSM_THREADS; s <<= 1) {
        uint32_t x = t >= s ? sh[t - s] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    uint32_t incl = sh[t];
    if (total) *total = sh[MSM_THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(MSM_THREADS) void k_scan_reduce(const uint32_t *in, size_t n, uint32_t *blocksum) {
    size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t s = 0;
    for (unsigned i = 0; i < SCAN_ITEMS; i++) if (base + i < n) s += in[base + i];
    uint32_t tot;
    block_exclusive_scan(s, &tot);
    if (threadIdx.x == 0) blocksum[blockIdx.x] = tot;
}
// single block: exclusive scan of blocksum[0..nb) in place; writes the grand total to blocksum[nb]
__global__ __launch_bounds__(MSM_THREADS) void k_scan_top(uint32_t *blocksum, size_t nb) {
    uint32_t carry = 0;
    for (size_t base = 0; base < nb; base += MSM_THREADS) {
        size_t i = base + threadIdx.x;
        uint32_t v = i < nb ? blocksum[i] : 0, tot;
        uint32_t ex = block_exclusive_scan(v, &tot);
        if (i < nb) blocksum[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) blocksum[nb] = carry;
}
// out[i] = exclusive prefix; out2 (optional) gets a copy; out[n] = total
__global__ __launch_bounds__(MSM_THREADS) void k_scan_final(const uint32_t *in, size_t n, const uint32_t *blocksum, uint32_t *out, uint32_t *out2) {
    size_t base = (size_t)blockIdx.x * SCAN_TILE + (size_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS], s = 0;
    for (unsigned i = 0; i < SCAN_ITEMS; i++) { v[i] = base + i < n ? in[base + i] : 0; s += v[i]; }
    uint32_t ex = block_exclusive_scan(s, nullptr) + blocksum[blockIdx.x];
    for (unsigned i = 0; i < SCAN_ITEMS; i++) {
        if (base + i < n) { out[base + i] = ex; if (out2) out2[base + i] = ex; }
        ex += v[i];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == MSM_THREADS - 1) { out[n] = ex; if (out2) out2[n] = ex; }
}


// ------------------------------------------------------------------------------------------------
// A bucket of s points is cut into parts_of(s) parts of part_len points (the last one shorter), at most T points per part.
// (Measured: capping the number of parts of a giant bucket -- all the scalars equal to one -- at a few thousand makes its
// parts hundreds of points long, a latency-bound tail of the accumulation kernel that costs far more than merging tens of
// thousands of short partial sums in parallel.  The cap only guards the 32-bit part index.)
static constexpr uint32_t PART_CAP = 1u << 24;
__host__ __device__ __forceinline__ uint32_t parts_of(uint32_t s, unsigned T) {
    if (s <= T) return 1u;
    uint32_t p = (s + T - 1) / T;
    return p < PART_CAP ? p : PART_CAP;
}
// plan: number of parts per bucket (>= 1); buckets split in 2..MERGE_SMALL parts go to the "medium" list (merged by one
// thread each), larger ones to the "heavy" list (merged by workgroups).  counters[0] = #heavy, counters[2] = #medium, counters[4] = the
// most parts any heavy bucket has
static constexpr unsigned MERGE_SMALL = 16;
__global__ __launch_bounds__(MSM_THREADS) void k_plan(const uint32_t *cnt, size_t G, unsigned T, uint32_t *nsub, uint32_t *heavy, uint32_t *medium, uint32_t *counters, uint32_t *tilesum,
                                                      uint32_t *zero_words, unsigned zero_count, uint32_t *zero_one) {
    // (the size histogram of the part plan and the hand-back counter of the accumulation are cleared here instead of by two fill launches)
    if (blockIdx.x == 0) {
        for (unsigned z = threadIdx.x; z < zero_count; z += MSM_THREADS) zero_words[z] = 0u;
        if (zero_one && threadIdx.x == 0) *zero_one = 0u;
    }
    size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = g < G;
    uint32_t s = live ? cnt[g] : 0;
    uint32_t parts = parts_of(s, T);
    if (live) nsub[g] = parts;
    if (live && parts > MERGE_SMALL) { heavy[atomicAdd(&counters[0], 1u)] = (uint32_t)g; atomicMax(&counters[4], parts); }
    // in the shared-set mode EVERY bucket is medium: one atomic per wave (ballot + prefix count), not per lane
    const bool med = live && parts > 1 && parts <= MERGE_SMALL;
    const unsigned long long mask = __ballot(med);
    if (mask) {
        const unsigned lane = threadIdx.x & 63u;
        const unsigned leader = (unsigned)__ffsll((long long)mask) - 1u;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&counters[2], (uint32_t)__popcll(mask));
        base = __shfl(base, (int)leader, 64);
        if (med) medium[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)g;
    }
    if (tilesum) block_sum_to(live ? parts : 0u, &tilesum[blockIdx.x]);
}

// ------------------------------------------------------------------------------------------------
// Load balance: a wave runs as long as its longest part, and bucket sizes are Poisson (mean 32 -> the max of 64 is ~47),
// so parts are handed to threads in DESCENDING SIZE ORDER: a counting sort of the parts by size (<= 1024 bins).
static constexpr unsigned SZ_BINS = 1024;

__device__ __forceinline__ uint32_t part_len(uint32_t s, uint32_t parts) { return (s + parts - 1) / parts; }
__device__ __forceinline__ uint32_t part_size(uint32_t s, uint32_t parts, uint32_t j) {
    if (parts == 1) return s;
    uint32_t len = part_len(s, parts), st = j * len;
    if (st >= s) return 0;
    uint32_t rest = s - st;
    return rest < len ? rest : len;
}

// part_bucket[q] = bucket of part q (binary search in suboff); size_hist[bin] += 1.  One thread per part.
__global__ __launch_bounds__(256) void k_partinfo(const uint32_t *cnt, const uint32_t *suboff, size_t G, unsigned T, uint32_t *part_bucket, uint32_t *size_hist) {
    __shared__ uint32_t h[SZ_BINS];
    for (unsigned b = threadIdx.x; b < SZ_BINS; b += 256) h[b] = 0;
    __syncthreads();
    const uint32_t S = suboff[G];
    size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < S) {
        size_t lo = 0, hi = G - 1;                        // largest g with suboff[g] <= q (every bucket has >= 1 part)
        while (lo < hi) {
            size_t mid = (lo + hi + 1) >> 1;
            if (suboff[mid] <= q) lo = mid; else hi = mid - 1;
        }
        uint32_t g = (uint32_t)lo;
        part_bucket[q] = g;
        uint32_t q0 = suboff[g], parts = suboff[g + 1] - q0;
        uint32_t sz = part_size(cnt[g], parts, (uint32_t)q - q0);
        atomicAdd(&h[sz < SZ_BINS ? sz : SZ_BINS - 1], 1u);
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < SZ_BINS; b += 256) if (h[b]) atomicAdd(&size_hist[b], h[b]);
}
// single workgroup: bin_cursor[b] = number of parts in strictly larger bins (descending order start)
__global__ __launch_bounds__(SZ_BINS) void k_binscan(const uint32_t *size_hist, uint32_t *bin_cursor) {
    __shared__ uint32_t sh[SZ_BINS];
    unsigned t = threadIdx.x;
    unsigned rb = SZ_BINS - 1 - t;                 // thread t handles bin rb: reverse order
    uint32_t v = size_hist[rb];
    sh[t] = v;
    __syncthreads();
    for (unsigned s = 1; s < SZ_BINS; s <<= 1) {
        uint32_t x = t >= s ? sh[t - s] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    bin_cursor[rb] = sh[t] - v;
}
// perm[position in descending size order] = part
__global__ __launch_bounds__(256) void k_partsort(const uint32_t *cnt, const uint32_t *suboff, const uint32_t *part_bucket, size_t G, unsigned T,
                                                  uint32_t *bin_cursor, uint32_t *perm) {
    __shared__ uint32_t h[SZ_BINS];
    for (unsigned b = threadIdx.x; b < SZ_BINS; b += 256) h[b] = 0;
    __syncthreads();
    const uint32_t S = suboff[G];
    size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bin = 0, rank = 0;
    if (q < S) {
        uint32_t g = part_bucket[q];
        uint32_t q0 = suboff[g], parts = suboff[g + 1] - q0;
        uint32_t sz = part_size(cnt[g], parts, (uint32_t)q - q0);
        bin = sz < SZ_BINS ? sz : SZ_BINS - 1;
        rank = atomicAdd(&h[bin], 1u);
    }
    __syncthreads();
    for (unsigned b = threadIdx.x; b < SZ_BINS; b += 256) if (h[b]) h[b] = atomicAdd(&bin_cursor[b], h[b]);   // reserve a range per bin
    __syncthreads();
    if (q < S) perm[h[bin] + rank] = (uint32_t)q;
}

// ------------------------------------------------------------------------------------------------
// accumulate: one thread per bucket part, parts taken in descending size order
// waves per SIMD the kernel is compiled for (measured: 2 and 3 waves perform alike -- the kernel is issue bound)
template <class F> struct AccumWaves { static constexpr unsigned W = 2; };
template <class F>
__device__ __forceinline__ XYZZ<typename LaneView<F>::E> accumulate_part(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ off,
                                                const uint32_t *__restrict__ suboff, const uint32_t *__restrict__ part_bucket, uint32_t q,
                                                XYZZ<F> *buckets, XYZZ<F> *partials, bool glv = false) {
    using LV = LaneView<F>; using E = typename LV::E;
    // endomorphism split: entry 2i is P_i, entry 2i + 1 is phi(P_i) = (beta x, y) -- this generic kernel reads the n-row table and scales x
    auto load_entry = [&](uint32_t e) {
        const uint32_t idx = e & 0x7fffffffu;
        Affine<E> p = LV::load(&bases[glv ? (idx >> 1) : idx]);
        if (glv && (idx & 1u)) glv_apply(p.x);                 // infinity stays infinity: beta * 0 = 0
        return p;
    };
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ<E> acc = XYZZ<E>::inf();
    if (start < end) {
        // software pipeline: the next point (and the index after it) is in flight while the current addition runs -- a gather
        // misses L2 (and, with precomputed tables, the Infinity Cache too) and one addition is ~10 us of ALU work
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        Affine<E> p_cur = load_entry(e_cur);
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            Affine<E> p_nxt = p_cur;
            if (more) p_nxt = load_entry(e_nxt);
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            xyzz_madd(acc, p_cur, (e_cur >> 31) != 0);
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    LV::store(parts == 1 ? &buckets[g] : &partials[q], acc);
    return acc;
}
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_accum(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                       const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                       const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                       size_t G, unsigned T, XYZZ<F> *buckets, XYZZ<F> *partials) {
    size_t t = gid<F>();
    if (t >= suboff[G]) return;
    accumulate_part<F>(bases, sorted, off, suboff, part_bucket, perm[t], buckets, partials);
}
// the bucket parts another kernel handed back (k_accum28: equal-x pairs), a small grid striding over the list.  With the 28-bit bucket
// arrays (b28 / p28 not null) the redone part is converted and stored there as well -- one kernel, one wait for a wave slot on a full GPU
#if VSP_MSM_GROUP == 1
using Bucket28 = XYZZ<Fp28>;
__device__ __forceinline__ void store_part28(Bucket28 *dst, const XYZZ<Fp> &a) {
#if defined(__HIP_DEVICE_COMPILE__)
    *dst = xyzz28_from_fp(a);
#endif
}
#else
using Bucket28 = XYZZ<Fp2x28>;
__device__ __forceinline__ void store_part28(Bucket28 *dst, const XYZZ<Fp2L> &a) {      // each lane of the pair converts its own component
#if defined(__HIP_DEVICE_COMPILE__)
    Fp28 *row = reinterpret_cast<Fp28 *>(dst);
    const unsigned comp = threadIdx.x & 1;
    const bool inf = is_inf(a);
    row[comp] = inf ? Fp28::zero() : fp_to_fp28(a.X.v); row[2 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.Y.v);
    row[4 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.ZZ.v); row[6 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.ZZZ.v);
#endif
}
#endif
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_accum_redo(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                            const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                            const uint32_t *__restrict__ part_bucket, XYZZ<F> *buckets, XYZZ<F> *partials,
                                                            const uint32_t *redo_list, const uint32_t *redo_count, bool glv, Bucket28 *b28, Bucket28 *p28) {
    const uint32_t count = *redo_count;
    for (size_t t = gid<F>(); t < count; t += (size_t)gridDim.x * blockDim.x / LaneView<F>::LANES) {
        const uint32_t q = redo_list[t];
        auto acc = accumulate_part<F>(bases, sorted, off, suboff, part_bucket, q, buckets, partials, glv);
        if (b28) {
            const uint32_t g = part_bucket[q];
            store_part28(suboff[g + 1] - suboff[g] == 1 ? &b28[g] : &p28[q], acc);
        }
    }
}

#ifndef VSP_ACCUM28_WAVES
#define VSP_ACCUM28_WAVES 2
#endif
#if VSP_MSM_GROUP == 1
// G1: the same accumulation on 14 x 28-bit limbs with lazy reduction (fp28.h) -- a product is 1.38x faster there.  The table is read
// in that form and the bucket parts stay in it: the merges and the bucket reduction are instantiated over XYZZ<Fp28> (fp28.h gives
// it the full addition), and only the four results per window return to the 12 x 32-bit form (k_dimweight's store).
__global__ __launch_bounds__(MSM_THREADS, VSP_ACCUM28_WAVES) void k_accum28_cxx(const Affine28 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp28> *buckets, XYZZ<Fp28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t S = suboff[G];
    if (t >= S) return;
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ28 acc = xyzz28_inf();
    if (start < end) {
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        Affine28 p_cur = bases[e_cur & 0x7fffffffu];
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            Affine28 p_nxt = p_cur;
            if (more) p_nxt = bases[e_nxt & 0x7fffffffu];
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            if (!madd28(acc, p_cur, (e_cur >> 31) != 0)) {      // equal x (doubling / cancellation): the generic kernel redoes this part
                redo_list[atomicAdd(redo_count, 1u)] = q;
                return;
            }
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    XYZZ<Fp28> out; out.X = acc.X; out.Y = acc.Y; out.ZZ = acc.ZZ; out.ZZZ = acc.ZZZ;      // stays in the 28-bit form (infinity: all zero)
    if (parts == 1) buckets[g] = out; else partials[q] = out;
#endif
}
#ifdef VSP_DIAG_CLOCK
__device__ unsigned long long vsp_diag_clock_sums[4];          // shader cycles, 100 MHz ticks, waves (diagnostic build only)
#endif
// The same accumulation through the generated, hand-allocated routine (accum28_asm_gfx950.h, tools/gen_accum28_asm.py): the whole loop of a
// bucket part -- gather of the next point under the current addition, digit sign, points at infinity, the equal-x exit -- in 167 VGPRs, so
// THREE waves share a SIMD.  Measured in shader cycles (tools/ubench_madd28.hip, profiles/r3_ubench_madd28.txt): a wave sharing its SIMD
// with one other takes 1.8 x as long per product as a wave alone, and with two others still 1.8 x -- the third wave is free, which the
// compiler's allocation around the fixed-register product routines (227-238 VGPRs) could not use.  Option "msm_accum28_asm" = 0 runs
// k_accum28_cxx instead; results are identical (same formulas, same column schedule).
__global__ __launch_bounds__(MSM_THREADS, 3) void k_accum28(const Affine28 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp28> *buckets, XYZZ<Fp28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t S = suboff[G];
    if (t >= S) return;
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    const uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ<Fp28> out;
    uint32_t flag;
#ifdef VSP_DIAG_CLOCK
    // DIAGNOSTIC BUILD ONLY (libvsp_hip_diag.so, `make diag`): the clock the chip holds inside this loop = delta s_memtime / delta
    // s_memrealtime x 100 MHz (MI355X_MICROARCH.md, DVFS item 6), stamped once around the loop, summed over waves into a buffer of its own
    unsigned long long dc_t0, dc_r0, dc_t1, dc_r1;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t0), "=s"(dc_r0) :: "memory");
#endif
    accum28_asm(out.X.l, flag, bases, sorted, start, end);           // X | Y | ZZ | ZZZ: 56 consecutive words
#ifdef VSP_DIAG_CLOCK
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t1), "=s"(dc_r1) :: "memory");
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {      // first active lane of the wave
        atomicAdd(&vsp_diag_clock_sums[0], dc_t1 - dc_t0); atomicAdd(&vsp_diag_clock_sums[1], dc_r1 - dc_r0); atomicAdd(&vsp_diag_clock_sums[2], 1ull);
    }
#endif
    if (flag) { redo_list[atomicAdd(redo_count, 1u)] = q; return; }  // equal x (doubling / cancellation): the generic kernel redoes this part
    if (parts == 1) buckets[g] = out; else partials[q] = out;
#endif
}
__global__ __launch_bounds__(256) void k_table28(const Affine<Fp> *in, size_t n, Affine28 *out, bool glv) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp> p = in[i];
    Affine28 r;
    r.x = fp_to_fp28(p.x); r.y = fp_to_fp28(p.y);       // infinity (0, 0) stays (0, 0)
    out[glv ? 2 * i : i] = r;
    if (glv) { glv_apply(p.x); r.x = fp_to_fp28(p.x); out[2 * i + 1] = r; }      // phi(P) = (beta x, y); infinity stays infinity (beta * 0 = 0)
#endif
}
#endif

#if VSP_MSM_GROUP == 2
// G2: the accumulation over lane pairs on the 28-bit form (fp28.h: one dual product per Fp2 product and lane); rows of 224 bytes.
// The bucket parts stay in that form (XYZZ<Fp2x28>) through the merges and the bucket reduction, as on G1.
__global__ __launch_bounds__(MSM_THREADS, VSP_ACCUM28_WAVES) void k_accum28(const Affine28x2 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp2x28> *buckets, XYZZ<Fp2x28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t t = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
    const unsigned comp = threadIdx.x & 1;
    uint32_t S = suboff[G];
    if (t >= S) return;                                 // both lanes of a pair leave together
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    auto load = [&](uint32_t e) {
        const Fp28 *row = reinterpret_cast<const Fp28 *>(&bases[e & 0x7fffffffu]);      // x.c0, x.c1, y.c0, y.c1
        AffineHalf28 p; p.x = row[comp]; p.y = row[2 + comp]; return p;
    };
    XYZZHalf28 acc = xyzz_half28_inf();
    if (start < end) {
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        AffineHalf28 p_cur = load(e_cur);
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            AffineHalf28 p_nxt = p_cur;
            if (more) p_nxt = load(e_nxt);
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            if (!madd28_g2(acc, p_cur, (e_cur >> 31) != 0)) {        // equal x: the generic kernel redoes this part (one entry per pair)
                if (comp == 0) redo_list[atomicAdd(redo_count, 1u)] = q;
                return;
            }
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    Fp28 *dst = reinterpret_cast<Fp28 *>(parts == 1 ? &buckets[g] : &partials[q]);      // X.c0, X.c1, Y.c0, Y.c1, ZZ.c0, ...: stays in the 28-bit form
    dst[comp] = acc.X; dst[2 + comp] = acc.Y; dst[4 + comp] = acc.ZZ; dst[6 + comp] = acc.ZZZ;      // infinity: ZZ zero on both lanes
#endif
}
__global__ __launch_bounds__(256) void k_table28(const Affine<Fp2> *in, size_t n, Affine28x2 *out, bool glv) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp2> p = in[i];
    Affine28x2 r;
    r.xc0 = fp_to_fp28(p.x.c0); r.xc1 = fp_to_fp28(p.x.c1); r.yc0 = fp_to_fp28(p.y.c0); r.yc1 = fp_to_fp28(p.y.c1);
    out[glv ? 2 * i : i] = r;
    if (glv) { glv_apply(p.x); r.xc0 = fp_to_fp28(p.x.c0); r.xc1 = fp_to_fp28(p.x.c1); out[2 * i + 1] = r; }
#endif
}
#endif

// workgroup tree reduction of one XYZZ per logical thread; sh: NT entries.
// NT physical threads; with LANES lanes per value the result is valid in the first LANES threads (logical thread 0)
template <class F, unsigned NT>
__device__ __forceinline__ XYZZ<typename LaneView<F>::E> block_sum(XYZZ<typename LaneView<F>::E> acc, XYZZ<typename LaneView<F>::E> *sh) {
    unsigned t = threadIdx.x;
    sh[t] = acc;
    __syncthreads();
    for (unsigned s = NT / 2; s >= LaneView<F>::LANES; s >>= 1) {      // physical stride; lanes of a value keep their parity
        if (t < s) { xyzz_add(acc, sh[t + s]); sh[t] = acc; }
        __syncthreads();
    }
    return acc;
}

// NT physical threads per workgroup (48 KiB of LDS: 192 B per lane either way), NTL logical threads = values per tree
template <class F> struct MsmBlock { static constexpr unsigned NT = 256; static constexpr unsigned NTL = NT / LaneView<F>::LANES; };
// the merges' workgroups (k_merge_a, k_merge2): experiment knob -DVSP_MERGE_NT=64 -- one wave and 14 KiB of LDS per workgroup instead of four and 56 KiB
#ifndef VSP_MERGE_NT
#define VSP_MERGE_NT 256
#endif
template <class F> struct MergeBlock { static constexpr unsigned NT = VSP_MERGE_NT; static constexpr unsigned NTL = NT / LaneView<F>::LANES; };

// merge of split ("heavy") buckets in two stages so that a bucket with thousands of parts (the all-ones bucket of a
// boolean witness) is folded by many workgroups, not one:
//   stage 1: grid (chunks, heavy buckets): each workgroup tree-reduces NT consecutive partials into the chunk's first slot
//   stage 2: one workgroup per heavy bucket tree-reduces the chunk results (stride NT) into the bucket
// (stage 1 shares its launch with the fold of the buckets in few parts, k_merge_a below: disjoint buckets, one wait for wave slots)
// Stage 1's work items are (chunk, heavy bucket) pairs, chunk-major, dealt round-robin to MERGE1_BLOCKS workgroups: one bucket of 10^5
// parts (all the scalars equal to one) and 116 buckets of 550 parts each (the top window of a 19-bit split at 2^23 points: 8 bits of
// digit) both spread over the whole grid.  (A fixed grid of 256 chunks x 4 buckets walked the second case's buckets 29 deep with
// 3 of 256 workgroups busy: 3.8 ms.)
static constexpr unsigned MERGE1_BLOCKS = 1024;
template <class F>
__device__ __forceinline__ void merge1_block(unsigned b, const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                             XYZZ<F> *partials, XYZZ<typename LaneView<F>::E> *sh) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL;
    const uint32_t nh = counters[0], maxparts = counters[4];
    if (!nh || maxparts <= NTL) return;                       // small enough for stage 2 alone
    const uint64_t items = (uint64_t)nh * ((maxparts + NTL - 1) / NTL);
    for (uint64_t i = b; i < items; i += MERGE1_BLOCKS) {
        const uint32_t h = (uint32_t)(i % nh), k = (uint32_t)(i / nh);
        const uint32_t g = heavy[h];
        const uint32_t q0 = suboff[g], q1 = suboff[g + 1];
        if (q1 - q0 <= NTL) continue;
        const uint64_t c0 = (uint64_t)q0 + (uint64_t)k * NTL;
        if (c0 >= q1) continue;
        const uint32_t q = (uint32_t)c0 + lid<F>();
        XYZZ<E> acc = q < q1 ? LV::load(&partials[q]) : XYZZ<E>::inf();
        acc = block_sum<F, NT>(acc, sh);
        if (lid<F>() == 0) LV::store(&partials[c0], acc);
        __syncthreads();
    }
}
template <class F>
__global__ __launch_bounds__(MergeBlock<F>::NT, 2) void k_merge2(const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                                             const XYZZ<F> *partials, XYZZ<F> *buckets) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL;
    __shared__ XYZZ<E> sh[NT];
    uint32_t nh = counters[0];
    for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
        uint32_t g = heavy[h];
        uint32_t q0 = suboff[g], q1 = suboff[g + 1];
        const uint32_t stride = (q1 - q0 <= NTL) ? 1u : NTL;  // after stage 1 only every NTL-th slot is live
        XYZZ<E> acc = XYZZ<E>::inf();
        for (uint32_t q = q0 + lid<F>() * stride; q < q1; q += NTL * stride) xyzz_add(acc, LV::load(&partials[q]));
        acc = block_sum<F, NT>(acc, sh);
        if (lid<F>() == 0) LV::store(&buckets[g], acc);
        __syncthreads();
    }
}

// buckets split in a few parts (2..MERGE_SMALL): LPB logical lanes fold one bucket -- a serial prefix of parts / LPB additions, then a
// log2(LPB)-level tree through LDS.  (One lane per bucket, the earlier form, is a chain of up to 15 additions: a SINGLE such bucket
// in a plain multi-exponentiation held the stream for 0.55 ms on G2.)  launch_tail picks LPB from the expected parts per bucket:
// 16 where only outliers are split, 1 (no tree, no LDS) where every bucket is cut in two or three, 4 in between and in the shared-set mode.
// One launch: the first `small_blocks` workgroups fold the buckets in few parts, the last MERGE1_BLOCKS run stage 1 of the heavy ones.
template <class F, unsigned LPB>
__global__ __launch_bounds__(MergeBlock<F>::NT, 2) void k_merge_a(const uint32_t *medium, const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                                                XYZZ<F> *partials, XYZZ<F> *buckets, unsigned small_blocks) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL, PER_BLOCK = NTL / LPB;
    __shared__ XYZZ<E> sh[NT];
    if (blockIdx.x >= small_blocks) {                        // uniform over the workgroup
        const unsigned b = blockIdx.x - small_blocks;
        merge1_block<F>(b, heavy, counters, suboff, partials, sh);
        return;
    }
    const uint32_t nm = counters[2];
    const unsigned lt = lid<F>(), lane = lt % LPB, slot = lt / LPB;
    for (size_t base = (size_t)blockIdx.x * PER_BLOCK; base < nm; base += (size_t)small_blocks * PER_BLOCK) {      // uniform over the block
        const size_t t = base + slot;
        const bool live = t < nm;
        const uint32_t g = live ? medium[t] : 0u;
        const uint32_t q0 = live ? suboff[g] : 0u, q1 = live ? suboff[g + 1] : 0u;
        XYZZ<E> acc = XYZZ<E>::inf();
        for (uint32_t q = q0 + lane; q < q1; q += LPB) xyzz_add(acc, LV::load(&partials[q]));
        if constexpr (LPB > 1) {
            sh[threadIdx.x] = acc;
            __syncthreads();
            for (unsigned s = LPB / 2; s >= 1; s >>= 1) {       // lanes of a value keep their parity: physical stride s * LANES
                if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LV::LANES]); sh[threadIdx.x] = acc; }
                __syncthreads();
            }
        }
        if (live && lane == 0) LV::store(&buckets[g], acc);
    }
}

// ---- precomputation of the window multiples of resident bases: out = 2^c * in (XYZZ), then batch-normalised to affine
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_shift_window(const Affine<F> *in, size_t n, unsigned c, XYZZ<F> *out) {
    using LV = LaneView<F>; using E = typename LV::E;
    size_t i = gid<F>();
    if (i >= n) return;
    XYZZ<E> acc = xyzz_from_affine(LV::load(&in[i]));
    for (unsigned k = 0; k < c; k++) acc = xyzz_dbl(acc);
    LV::store(&out[i], acc);
}
static constexpr unsigned PRE_CHUNK = 32;
template <class F>
__global__ __launch_bounds__(64) void k_batch_affine_mont(const XYZZ<F> *in, size_t n, F *pre, Affine<F> *out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = t * PRE_CHUNK, e = b + PRE_CHUNK < n ? b + PRE_CHUNK : n;
    if (b >= n) return;
    F acc = F::one();
    for (size_t i = b; i < e; i++) {
        pre[i] = acc;
        F z = in[i].ZZZ;
        if (!is_zero(z)) acc = mul(acc, z);
    }
    F ai = inv(acc);
    for (size_t i = e; i-- > b;) {
        XYZZ<F> p = in[i];
        Affine<F> r;
        if (is_zero(p.ZZ)) { r.x = F::zero(); r.y = F::zero(); }
        else {
            F zi3 = mul(ai, pre[i]);
            ai = mul(ai, p.ZZZ);
            F zi = mul(zi3, p.ZZ);
            F zi2 = sqr(zi);
            r.x = mul(p.X, zi2);
            r.y = mul(p.Y, zi3);
        }
        out[i] = r;
    }
}

// ---- bucket reduction.  sum_b (b + 1) B_b over the 2^(c-1) buckets of a window is decomposed over the DIGITS of the bucket index
// b = (v2, v1, v0) (q2 + q1 + q0 = c - 1 bits; q2 = 0: two digits): with A_d[v] = the plain sum of the buckets whose digit d is v,
//     sum_b (b + 1) B_b = 2^(q1+q0) sum_v v A_2[v] + 2^q0 sum_v v A_1[v] + sum_v v A_0[v] + sum_b B_b.
// Every bucket goes into one plain sum per digit, so TWO digits cost two additions per bucket instead of three; the digits then
// have up to 2^8 values, which k_dimweight's 256-term trees still take (G1; the lane-pair G2 kernels have 128 slots and keep three
// digits at c = 16).  Why not the reference's running sum: that is one serial chain of 2^c additions per window.
__host__ __device__ __forceinline__ unsigned dims_n2(const MsmGeom &g) { return g.q2 ? (1u << g.q2) : 0u; }
__host__ __device__ __forceinline__ unsigned dims_per_w(const MsmGeom &g) { return (1u << g.q0) + (1u << g.q1) + dims_n2(g); }
// dimbits: the last step is k_dimbits (one wave per digit bit, any number of digit values), not k_dimweight (a tree of at most NTL values):
// two digits of up to 12 bits then serve windows of up to 25 bits with TWO additions per bucket
template <class F> static void split_digits(MsmGeom &g, bool dimbits) {
    const unsigned qb = g.c - 1;
    unsigned maxq = 0; while ((2u << maxq) <= MsmBlock<F>::NTL) maxq++;          // log2 of the slots of a k_dimweight tree
    if (qb <= 2 * maxq || (dimbits && qb <= 24)) { g.q0 = (qb + 1) / 2; g.q1 = qb - g.q0; g.q2 = 0; }
    else { g.q0 = qb / 3; g.q1 = (qb - g.q0) / 2; g.q2 = qb - g.q0 - g.q1; }
    g.bd = (g.q2 == 0 && g.q0 > 8) ? 12u : 8u;
}

// dimension sums A_d[v], dims[w][slot], slot = d-offset + v.  One sum = `items` = B >> q_d buckets.  A sum is folded by LPS lanes
// (logical lanes: a G2 value takes a lane pair): each lane adds items / LPS buckets serially, then a log2(LPS)-level tree through
// LDS.  Several sums share a wave (64 / LANES / LPS of them), one wave per workgroup.  Measured on the plain-bases 2^20 MSM
// (16 windows x 32768 buckets): the earlier form -- one 256-thread workgroup per sum, 4 serial additions and an 8-level tree in
// which half of the remaining lanes idle at every level -- spent 1.17 ms here, 43 % of the accumulation kernel's time, for 1 / 7 of
// its additions; serial prefixes of 8-16 additions per lane keep the lanes busy.
// LPS is chosen at launch (launch_tail): e.g. the whole wave for the single bucket set of the window-multiple mode (384 sums: 96 waves
// at 16 lanes per sum was a 20-addition serial chain on a tenth of the GPU, 280 us; 64 us with 64 lanes).
// (measured, dense 8-window case, 12 x 32-bit field: 32 lanes per sum = 1536 waves took 548 us against 404 us at 16 lanes = 768 waves --
// a second wave on a SIMD halves the speed of both; the 28-bit routines leave a lone wave at half the issue rate, so two per SIMD are free)
template <class F> struct DimSumWaves { static constexpr unsigned MAX = 1024; };
template <> struct DimSumWaves<Fp28> { static constexpr unsigned MAX = 2048; };
template <> struct DimSumWaves<Fp2x28> { static constexpr unsigned MAX = 2048; };
template <class F, unsigned LPS>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimsum(const XYZZ<F> *buckets, MsmGeom g, XYZZ<F> *dims) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LANES = LV::LANES, SPW = 64 / LANES / LPS;
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1;
    const unsigned per_w = dims_per_w(g);
    const unsigned lt = threadIdx.x / LANES;                  // logical lane of the wave
    const unsigned lane = lt % LPS;
    const unsigned sum_id = blockIdx.x * SPW + lt / LPS;
    const bool live = sum_id < g.Wr * per_w;
    const unsigned w = live ? sum_id / per_w : 0;
    const unsigned slot = live ? sum_id % per_w : 0;
    unsigned d, v;
    if (slot < n0) { d = 0; v = slot; } else if (slot < n0 + n1) { d = 1; v = slot - n0; } else { d = 2; v = slot - n0 - n1; }
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const unsigned items = live ? g.B >> qd : 0;
    const XYZZ<F> *bw = buckets + (size_t)w * g.B;
    XYZZ<E> acc = XYZZ<E>::inf();
    for (unsigned i = lane; i < items; i += LPS) {
        unsigned idx;
        if (d == 0) idx = (i << g.q0) | v;
        else if (d == 1) idx = ((i >> g.q0) << (g.q1 + g.q0)) | (v << g.q0) | (i & (n0 - 1));
        else idx = (v << (g.q1 + g.q0)) | i;
        xyzz_add(acc, LV::load(&bw[idx]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = LPS / 2; s >= 1; s >>= 1) {               // lanes of a value keep their parity: physical stride s * LANES
        if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (live && lane == 0) LV::store(&dims[(size_t)w * per_w + slot], acc);
}

// The same sums with a lane count PER DIGIT (round 3).  The sums of one digit run over 2^(other digits' bits) buckets each, so with two
// digits of 7 and 8 bits half of the sums are twice as long as the others; one lane count for all either leaves the short sums' lanes
// idle in the tree or puts 1.5 waves on every SIMD -- and a second wave on a SIMD nearly halves the speed of both (a lone wave takes
// 84 % of the multiplier's issue slots, DESIGN.md 3.1e).  Measured on the dense 8-window case: 32 lanes for every sum (1536 waves)
// 321 us, 16 lanes (768 waves) 284 us, 64 lanes 385 us, 8 lanes 478 us.  Here every digit gets items / 8 lanes (7 serial additions, then
// the tree): 32 lanes for the 256-bucket sums, 16 for the 128-bucket ones = 1024 waves, one per SIMD, 12-13 dependent additions.
// Block b serves digit d when wave0[d] <= b < wave0[d + 1]; one wave per block.
struct DimSumPlan { unsigned lps[3]; unsigned wave0[4]; };
template <class F, bool PREFETCH>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimsum_mixed(const XYZZ<F> *buckets, MsmGeom g, XYZZ<F> *dims, DimSumPlan pl) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LANES = LV::LANES, LL = 64 / LANES;
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1, n2 = dims_n2(g);
    const unsigned per_w = dims_per_w(g);
    const unsigned d = blockIdx.x < pl.wave0[1] ? 0u : (blockIdx.x < pl.wave0[2] ? 1u : 2u);      // uniform over the block
    const unsigned LPS = pl.lps[d], SPW = LL / LPS;
    const unsigned nd = d == 0 ? n0 : (d == 1 ? n1 : n2), base = d == 0 ? 0u : (d == 1 ? n0 : n0 + n1);
    const unsigned lt = threadIdx.x / LANES;                  // logical lane of the wave
    const unsigned lane = lt % LPS;
    const unsigned id = (blockIdx.x - pl.wave0[d]) * SPW + lt / LPS;      // sum of this digit: (window, value)
    const bool live = id < g.Wr * nd;
    const unsigned w = live ? id / nd : 0, v = live ? id % nd : 0;
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const unsigned items = live ? g.B >> qd : 0;
    const XYZZ<F> *bw = buckets + (size_t)w * g.B;
    auto index_of = [&](unsigned i) {
        if (d == 0) return (i << g.q0) | v;
        if (d == 1) return ((i >> g.q0) << (g.q1 + g.q0)) | (v << g.q0) | (i & (n0 - 1));
        return (v << (g.q1 + g.q0)) | i;
    };
    // PREFETCH (G1, option "msm_dimsum_prefetch" = 1; default 0): the next bucket is requested before the current addition starts -- two
    // records live across the field routines.  Round 3 measured this loop 297 -> 250 us and WRONG on doubling-heavy inputs; the cause was the
    // toolchain's machine scheduler (csrc/Makefile SOUND, DESIGN.md 3.7), not the loop: built without that scheduler it passes the probe, the
    // fuzzer and the suite -- and spills 42 registers, which makes it 5 % SLOWER than the plain loop (336 against 319 us, same box,
    // tools/gpu_r4k.sh).  Both are compiled; the plain loop runs.  Lane pairs (G2) have the plain loop only.
    XYZZ<E> acc = XYZZ<E>::inf();
    if constexpr (LANES == 1 && PREFETCH) {
        XYZZ<E> nxt = lane < items ? LV::load(&bw[index_of(lane)]) : XYZZ<E>::inf();
        for (unsigned i = lane; i < items; i += LPS) {
            const XYZZ<E> cur = nxt;
            if (i + LPS < items) nxt = LV::load(&bw[index_of(i + LPS)]);
            xyzz_add(acc, cur);
        }
    } else {
        for (unsigned i = lane; i < items; i += LPS) xyzz_add(acc, LV::load(&bw[index_of(i)]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = LPS / 2; s >= 1; s >>= 1) {               // lanes of a value keep their parity: physical stride s * LANES
        if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (live && lane == 0) LV::store(&dims[(size_t)w * per_w + base + v], acc);
}
template <class F> static DimSumPlan dimsum_plan(const MsmGeom &g, unsigned MAXW = 1024) {      // wave0[3] == 0: no plan; MAXW 1024 = one wave per SIMD of an MI355X
    constexpr unsigned LL = 64 / LaneView<F>::LANES;
    const unsigned nd[3] = {1u << g.q0, 1u << g.q1, dims_n2(g)};
    const unsigned qd[3] = {g.q0, g.q1, g.q2};
    DimSumPlan pl;
    auto lg2 = [](unsigned x) { unsigned l = 0; while ((1u << l) < x) l++; return l; };
    auto waves_of = [&](unsigned d, unsigned lps) { return nd[d] ? (unsigned)(((size_t)g.Wr * nd[d] * lps + LL - 1) / LL) : 0u; };
    auto steps_of = [&](unsigned d, unsigned lps) { const unsigned items = g.B >> qd[d]; return nd[d] ? (items + lps - 1) / lps + lg2(lps) : 0u; };
    for (unsigned d = 0; d < 3; d++) {
        unsigned l = (g.B >> qd[d]) / 8; if (l < 8) l = 8; if (l > LL) l = LL;
        unsigned p = 8; while (p * 2 <= l) p *= 2;
        pl.lps[d] = nd[d] ? p : 8;
    }
    auto total = [&]() { return waves_of(0, pl.lps[0]) + waves_of(1, pl.lps[1]) + waves_of(2, pl.lps[2]); };
    // more sums than one wave per SIMD serves at 8 items per lane (wide windows, many bucket sets): several rounds are unavoidable and
    // the one-count-for-all choice of launch_tail, which prices the rounds, stays in charge
    if (total() > MAXW) { pl.wave0[3] = 0; return pl; }
    for (int guard = 0; guard < 16; guard++) {                       // room left: more lanes where the chain is longest, while that shortens it
        int pick = -1;
        for (unsigned d = 0; d < 3; d++) {
            if (!nd[d] || pl.lps[d] >= LL || steps_of(d, pl.lps[d] * 2) >= steps_of(d, pl.lps[d])) continue;
            if (total() - waves_of(d, pl.lps[d]) + waves_of(d, pl.lps[d] * 2) > MAXW) continue;
            if (pick < 0 || steps_of(d, pl.lps[d]) > steps_of((unsigned)pick, pl.lps[pick])) pick = (int)d;
        }
        if (pick < 0) break;
        pl.lps[pick] *= 2;
    }
    pl.wave0[0] = 0;
    for (unsigned d = 0; d < 3; d++) pl.wave0[d + 1] = pl.wave0[d] + waves_of(d, pl.lps[d]);
    return pl;
}

// per (window, digit): D = sum_v v * A[v]  and  Tot = sum_v A[v]  by suffix scan + tree sum in LDS.
// winres[w][d] = D_d (d = 0,1,2; with two digits D_2 stays the all-zero record = infinity), winres[w][3] = Tot
// the window results leave in the 12 x 32-bit form the host folds (from the 28-bit form: one conversion per result)
template <class F> struct WinOut { using type = F; };
template <> struct WinOut<Fp28> { using type = Fp; };
template <> struct WinOut<Fp2x28> { using type = Fp2; };
template <class F> __device__ __forceinline__ void store_win(XYZZ<F> *p, const XYZZ<typename LaneView<F>::E> &v) { LaneView<F>::store(p, v); }
__device__ __forceinline__ void store_win(XYZZ<Fp> *p, const XYZZ<Fp28> &v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *p = xyzz28_to_fp(v);
#endif
}
__device__ __forceinline__ void store_win(XYZZ<Fp2> *p, const XYZZ<Fp28L> &v) {      // each lane of the pair converts and writes its component
#if defined(__HIP_DEVICE_COMPILE__)
    Fp *row = reinterpret_cast<Fp *>(p);
    const unsigned comp = threadIdx.x & 1;
    const bool inf = pair_all28(fp28_all_zero(v.ZZ.v));
    row[comp] = inf ? Fp::zero() : fp28_to_fp(v.X.v); row[2 + comp] = inf ? Fp::zero() : fp28_to_fp(v.Y.v);
    row[4 + comp] = inf ? Fp::zero() : fp28_to_fp(v.ZZ.v); row[6 + comp] = inf ? Fp::zero() : fp28_to_fp(v.ZZZ.v);
#endif
}
template <class F>
__global__ __launch_bounds__(MsmBlock<F>::NT, 2) void k_dimweight(const XYZZ<F> *dims, MsmGeom g, XYZZ<typename WinOut<F>::type> *winres) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MsmBlock<F>::NT, NTL = MsmBlock<F>::NTL;
    __shared__ XYZZ<E> sh[NT];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1, n2 = dims_n2(g);
    const unsigned per_w = dims_per_w(g);
    const unsigned w = blockIdx.x / 3u, d = blockIdx.x % 3u;
    if (d == 2 && !g.q2) {                                   // two digits: D_2 = infinity (uniform over the workgroup)
        if (lid<F>() == 0) store_win(&winres[(size_t)w * 4 + 2], XYZZ<E>::inf());
        return;
    }
    const unsigned cntv = d == 0 ? n0 : (d == 1 ? n1 : n2);
    const unsigned doff = d == 0 ? 0 : (d == 1 ? n0 : n0 + n1);
    const unsigned t = lid<F>();                          // logical thread = digit value
    XYZZ<E> x = t < cntv ? LV::load(&dims[(size_t)w * per_w + doff + t]) : XYZZ<E>::inf();
    sh[at<F>(t)] = x;
    __syncthreads();
    for (unsigned s = 1; s < cntv; s <<= 1) {            // inclusive suffix scan: x[t] = sum_{u >= t} A[u]
        XYZZ<E> y = (t + s < NTL) ? sh[at<F>(t + s)] : XYZZ<E>::inf();
        __syncthreads();
        xyzz_add(x, y);
        sh[at<F>(t)] = x;
        __syncthreads();
    }
    XYZZ<E> tot = sh[at<F>(0)];
    __syncthreads();
    XYZZ<E> acc = (t >= 1 && t < cntv) ? x : XYZZ<E>::inf();   // sum_{v>=1} suffix[v] = sum_v v*A[v]
    acc = block_sum<F, NT>(acc, sh);
    if (t == 0) {
        store_win(&winres[(size_t)w * 4 + d], acc);
        if (d == 0) store_win(&winres[(size_t)w * 4 + 3], tot);
    }
}

// The same weighted sums WITHOUT the weights: sum_v v A[v] = sum_j 2^j S_j with S_j = the plain sum of the A[v] whose digit value v has
// bit j set.  One wave per (window, digit, bit) folds its <= 128 values in ONE tree (7-9 dependent additions where k_dimweight's
// suffix scan + tree is 16), and the powers of two cost nothing: the host's Horner chain doubles once per bit position anyway and
// takes S_j at position (shift of the digit) + j.  The host pays c - 4 more additions per window, so launch_tail uses this form
// where that is cheap: G1 always (0.56 us per host addition), G2 when all windows share one bucket set.
// winres[w][DIMBITS_STRIDE]: [bd d + j] = S_{d,j} (bd = 8 slots per digit, or 12 with two wide digits: MsmGeom.bd), [24] = Tot (the plain sum of every bucket of the window).
static constexpr unsigned DIMBITS_STRIDE = 25;
// One WAVE per sum (a 256-thread workgroup per sum holds four 250-register wave slots and 57 KiB of LDS for a 7-level tree of 128
// values: with 25 sums per window that took a fifth of the throughput of concurrent proofs): a lane adds its 2 (Tot: 4) values, then
// a log2(lanes)-level tree through 14 KiB of LDS.
template <class F>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimbits(const XYZZ<F> *dims, MsmGeom g, XYZZ<typename WinOut<F>::type> *winres) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LL = 64 / LV::LANES;                      // logical lanes of the wave
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1;
    const unsigned per_w = dims_per_w(g);
    const unsigned w = blockIdx.x / DIMBITS_STRIDE, slot = blockIdx.x % DIMBITS_STRIDE;
    // Tot = the plain sum of the values of ANY one digit (each digit's values partition the buckets): the digit with the fewest values
    // (two digits: q1 <= q0; three: q0 <= q1 <= q2, split_digits) keeps this sum as deep as the bit sums -- 128 values at c = 16, not digit 0's 256
    const unsigned dtot = g.q2 ? 0u : 1u;
    const unsigned d = slot == 24 ? dtot : slot / g.bd, j = slot % g.bd;
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const bool live = slot == 24 || (d < 3 && j < qd);           // uniform over the workgroup
    const unsigned doff = d == 0 ? 0 : (d == 1 ? n0 : n0 + n1);
    const unsigned count = !live ? 0u : (slot == 24 ? (1u << qd) : (1u << (qd - 1)));      // values in this sum
    const unsigned t = threadIdx.x / LV::LANES;
    XYZZ<E> acc = XYZZ<E>::inf();
    for (unsigned u = t; u < count; u += LL) {
        // Tot: every value of digit 0.  Bit j: the u-th value with bit j set
        const unsigned v = slot == 24 ? u : (((u >> j) << (j + 1)) | (1u << j) | (u & ((1u << j) - 1u)));
        xyzz_add(acc, LV::load(&dims[(size_t)w * per_w + doff + v]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s2 = LL / 2; s2 >= 1; s2 >>= 1) {               // lanes of a value keep their parity: physical stride s2 * LANES
        if (t < s2) { xyzz_add(acc, sh[threadIdx.x + s2 * LV::LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (t == 0) store_win(&winres[(size_t)w * DIMBITS_STRIDE + slot], acc);      // dead slots: infinity
}

// canonical affine (host layout) -> Montgomery affine, with the boundary checks include/vsp.h promises:
//   flag bit 0: a coordinate is not canonical (>= p);  bit 1 (check_curve): a point is not on y^2 = x^3 + b
// (b = 4 for G1, 4 (1 + u) for G2; all-zero = infinity is accepted).  Subgroup membership is NOT checked here -- a scalar
// multiplication by r per point; vsp_g1_decompress / vsp_g2_decompress offer it for points that arrive as wire bytes.
__device__ __forceinline__ bool canon_below_p(const Fp &a) {
    bool lt = false, gt = false;
#pragma unroll
    for (int i = Fp::N - 1; i >= 0; i--) {
        lt = lt || (!gt && a.l[i] < FpP32::MOD[i]);
        gt = gt || (!lt && a.l[i] > FpP32::MOD[i]);
    }
    return lt;
}
__device__ __forceinline__ bool canon_below_p(const Fp2 &a) { return canon_below_p(a.c0) && canon_below_p(a.c1); }
__device__ __forceinline__ Fp curve_b_mont(const Fp &) { Fp four = Fp::one(); four = dbl(dbl(four)); return four; }
__device__ __forceinline__ Fp2 curve_b_mont(const Fp2 &) { Fp2 b; b.c0 = dbl(dbl(Fp::one())); b.c1 = b.c0; return b; }
template <class F> __global__ __launch_bounds__(256) void k_bases_to_mont(const Affine<F> *in, Affine<F> *out, size_t n, int check_curve, uint32_t *flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = in[i];
    uint32_t bad = (canon_below_p(p.x) && canon_below_p(p.y)) ? 0u : 1u;
    const bool inf = is_zero(p.x) && is_zero(p.y);
    p.x = to_mont(p.x); p.y = to_mont(p.y);
    if (check_curve && !inf && !bad) {
        F rhs = add(mul(sqr(p.x), p.x), curve_b_mont(p.x));
        if (!eq(sqr(p.y), rhs)) bad |= 2u;
    }
    if (bad) atomicOr(flag, bad);
    out[i] = p;
}

// ---- the precondition of the endomorphism split, checked: phi(P) = lambda P for every base.
// phi(x, y) = (beta x, y) acts as the scalar lambda = z^2 - 1 only on the order-r subgroup; the curve equation alone (checked at upload)
// also admits points with a cofactor component, for which sum k_i P_i computed through the split would be a DIFFERENT point than the
// plain pipeline's (and the reference's generic multiexp's).  The condition below is exactly what the split relies on: with it,
// (k1 + k2 lambda) P = k1 P + k2 phi(P), and the fold-back by lambda^2 + lambda + 1 = r is sound because (phi^2 + phi + 1) P = O holds on the
// whole curve, hence r P = O.  (It is also the known fast membership test of this curve family: phi(P) = -z^2 P for the other cube root.)
// lambda P = |z| (|z| P) - P with |z| = 0xd201000000010000 (Hamming weight 6): 126 doublings and 11 additions per point -- about 45 us of
// one lane's time, 20-30 ms for 2^20 G1 points, once per uploaded key.  flag bit 2 is raised for any point that fails.
static constexpr uint64_t BLS_ABS_Z = 0xd201000000010000ULL;
// the three group operations as REAL calls on memory temporaries: inlined side by side, the generic formulas crash this toolchain's
// machine scheduler next to the fixed-register product routine (as fp28.h notes for its cold branch); a one-off check can afford the calls
template <class E> __device__ __noinline__ void sgc_dbl(XYZZ<E> *a) { *a = xyzz_dbl(*a); }
template <class E> __device__ __noinline__ void sgc_madd(XYZZ<E> *a, const Affine<E> *p, bool negate) { XYZZ<E> t = *a; xyzz_madd(t, *p, negate); *a = t; }
template <class E> __device__ __noinline__ void sgc_add(XYZZ<E> *a, const XYZZ<E> *q) { XYZZ<E> t = *a; xyzz_add(t, *q); *a = t; }
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_subgroup_check(const Affine<F> *__restrict__ bases, size_t n, uint32_t *flag) {
    using LV = LaneView<F>; using E = typename LV::E;
    const size_t i = gid<F>();
    if (i >= n) return;                                     // both lanes of a pair leave together
    Affine<E> p = LV::load(&bases[i]);
    if (is_inf(p)) return;                                  // infinity is in every subgroup
    XYZZ<E> t1 = xyzz_from_affine(p);
#pragma unroll 1
    for (int b = 62; b >= 0; b--) { sgc_dbl(&t1); if ((BLS_ABS_Z >> b) & 1ull) sgc_madd(&t1, &p, false); }
    XYZZ<E> t2 = t1;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) { sgc_dbl(&t2); if ((BLS_ABS_Z >> b) & 1ull) sgc_add(&t2, &t1); }
    sgc_madd(&t2, &p, true);                                // z^2 P - P = lambda P
    Affine<E> q = p;
    glv_apply(q.x);                                         // phi(P) = (beta x, y)
    E lx, ly;
    mul_pair(q.x, t2.ZZ, q.y, t2.ZZZ, lx, ly);              // equal to t2 iff X = beta x ZZ and Y = y ZZZ (t2 finite)
    const bool inf2 = is_inf(t2);
    const bool ex = is_zero(sub(lx, t2.X));
    const bool ey = is_zero(sub(ly, t2.Y));
    if (inf2 || !ex || !ey) atomicOr(flag, 4u);
}

// the bit-decomposed last step (k_dimbits) or the weighted one (k_dimweight): `forced` (MsmTuning.dimbits) 1 / 0 forces either, -1 by group
template <class FT> static bool use_dimbits(long forced, const MsmGeom &g) {
    // room for 25 records per window in the slot's pinned buffer: the initial buffer for one vector (52 windows of 5 bits: no), the grown one
    // for a batch (msm_buffers grows it up to 64 MiB: K x Wk windows; k_dimweight's 16-addition chains took a fifth of a batch prover's kernel time)
    const size_t cap = g.K > 1 ? ((size_t)64 << 20) : MsmWork::PINNED_BYTES;
    const bool want = forced >= 0 ? forced != 0 : (LaneView<FT>::LANES == 1 || g.Wr <= 2 || g.c > 16);      // wide windows: digits of 2^10 values and more only k_dimbits takes
    return want && (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<typename WinOut<FT>::type>) <= cap;
}
// merges + bucket reduction over the bucket sums of field FT (F, or Fp28 on the G1 28-bit path); winres in the host's form; dimbits: the
// last step (use_dimbits)
template <class FT>
static int launch_tail(vsp_ctx *ctx, hipStream_t st, const MsmWork *pl, const MsmGeom &g, bool dimbits, XYZZ<FT> *buckets, XYZZ<FT> *partials, XYZZ<FT> *dims,
                       XYZZ<typename WinOut<FT>::type> *winres, XYZZ<typename WinOut<FT>::type> *winres_host) {
    using F = FT;
    constexpr unsigned NT = MsmBlock<F>::NT;
    const unsigned per_w = dims_per_w(g);
    // buckets split in 2..16 parts: up to every bucket (shared-set mode, or a small plain problem whose buckets alone would not fill the
    // GPU), a handful of outliers otherwise.  Expected parts per bucket = mean bucket size / part length.
    {
        const double est = (double)g.n * g.W / (double)g.G / (double)(g.T ? g.T : 1);
        const unsigned lpb = g.single ? 4u : (est < 0.6 ? 16u : (est <= 3.0 ? 1u : 4u));    // est ~ 1: half of the buckets are cut in two
        const unsigned per_block = MergeBlock<F>::NTL / lpb;
        const size_t want = (g.G + per_block - 1) / per_block;
        const dim3 grid((unsigned)(want < 4096 ? want : 4096));
        const uint32_t *medium = (const uint32_t *)pl->medium.p, *counters = (const uint32_t *)pl->counters.p, *suboff = (const uint32_t *)pl->suboff.p;
        const unsigned sb = lpb == 16 ? (grid.x < 1024 ? grid.x : 1024) : grid.x, all = sb + MERGE1_BLOCKS;
        const uint32_t *heavy = (const uint32_t *)pl->heavy.p;
        if (lpb == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 16>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
        else if (lpb == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 4>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 1>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge2<F>), dim3(256), dim3(MergeBlock<F>::NT), 0, st, (const uint32_t *)pl->heavy.p, (const uint32_t *)pl->counters.p,
                       (const uint32_t *)pl->suboff.p, (const XYZZ<F> *)partials, buckets);
    VSP_LAUNCH_CHECK();
    {
        constexpr unsigned LL = 64 / LaneView<F>::LANES;                    // logical lanes of a wave
        const unsigned sums = g.Wr * per_w;
        // lanes per sum: the serial prefix (items / lanes) plus the tree (log2 lanes) additions, times the rounds the grid needs on
        // the 1024 SIMDs -- a wave more than the SIMDs hold at full speed costs a whole extra round
        unsigned minq = g.q0 < g.q1 ? g.q0 : g.q1; if (g.q2 && g.q2 < minq) minq = g.q2;
        const unsigned items = g.B >> minq;
        unsigned lps = 16; size_t best = ~(size_t)0;
        for (unsigned cand = 8, lg = 3; cand <= LL; cand *= 2, lg++) {
            const size_t waves = ((size_t)sums * cand + LL - 1) / LL;
            const size_t rounds = (waves + DimSumWaves<F>::MAX - 1) / DimSumWaves<F>::MAX;
            const size_t cost = ((items + cand - 1) / cand + lg) * rounds;
            if (cost < best) { best = cost; lps = cand; }
        }
        long forced_lanes = 0;
        { const long t = opt(ctx, "msm_dimsum_lanes", 0); if (t == 8 || t == 16 || t == 32 || (t == 64 && LL == 64)) { lps = (unsigned)t; forced_lanes = t; } }
        const unsigned spw = LL / lps;
        const dim3 grid((sums + spw - 1) / spw);
        DimSumPlan pl; pl.wave0[3] = 0;
        const long mw = opt(ctx, "msm_dimsum_maxw", 1024); const unsigned maxw = mw >= 256 && mw <= 4096 ? (unsigned)mw : 1024u;
        if (!forced_lanes) pl = dimsum_plan<F>(g, maxw);      // a lane count per digit (k_dimsum_mixed); "msm_dimsum_lanes" keeps one count for all
        ctx->stats["msm_dimsum_waves"] = pl.wave0[3];
        const long pf = opt(ctx, "msm_dimsum_prefetch", 0);
        if (pl.wave0[3] && pf && LaneView<F>::LANES == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum_mixed<F, true>), dim3(pl.wave0[3]), dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims, pl);
        else if (pl.wave0[3]) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum_mixed<F, false>), dim3(pl.wave0[3]), dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims, pl);
        else
        if (lps == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 8>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else if (lps == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 16>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else if (lps == 32) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 32>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, (LL == 64 ? 64u : 32u)>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
    }
    VSP_LAUNCH_CHECK();
    if (dimbits) {
        // the results go straight into the slot's pinned host buffer (device-visible): no copy operation behind the kernel.  (A 29 KB
        // device-to-host copy per multi-exponentiation rides the DMA engines, behind the 32 MB witness upload of whichever proof another
        // context has just started: two contexts proved no faster than one.)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimbits<F>), dim3(g.Wr * DIMBITS_STRIDE), dim3(64), 0, st, (const XYZZ<F> *)dims, g, winres_host);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimweight<F>), dim3(g.Wr * 3u), dim3(NT), 0, st, (const XYZZ<F> *)dims, g, winres_host);
    }
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// ------------------------------------------------------------------------------------------------
// n: scalars that are neither 0 nor 1 (twice that with the endomorphism split: half-length scalars); windows: how many windows c bits need;
// forced: MsmTuning.window_bits
static unsigned pick_window_bits(vsp_ctx *ctx, long forced, size_t n, bool glv) {
    if (forced >= 2 && forced <= 23) return (unsigned)forced;
    unsigned L = ceil_log2(n ? n : 1);
    // mean bucket load n / 2^(c-1) of about 32 points balances the accumulation against the
    // bucket reduction, whose cost grows with 2^c
    int c = (int)L - 4;
    if (c < 4) c = 4;
    if (c > 16) c = 16;
    // From 2^23 points on the window may grow past 16 bits (staged sort, k_ms_*).  Cost in units of one sorted-and-accumulated point of
    // the 16-bit pipeline (0.18 ns at 2^25 points): n W for the accumulation -- x 0.87 behind the staged sort, which is cheaper per entry
    // than the LDS counting sort at these sizes -- plus 4.1 per bucket for the bucket reduction (0.74 ns; fitted to 2^24 .. 2^26 points at
    // c = 20 and 22, profiles/r3_window_sweep.txt).  Measured, ms per multi-exponentiation, c = 16 against the model's choice:
    // 2^23: 22.95 / 22.0 (c = 19; 17 .. 20 are within 3 %), 2^24: 45.7 / 38.95 (20), 2^25: 96.7 / 73.3 (20), 2^26: 218 / 139.6 (20);
    // G2 2^23: 66.4 / 61.9 (19), 2^24: 130.3 / 113.6 (20).  Below 2^23 points the 16-bit pipeline wins (2^22: 11.4 against 12.3 at c = 17).
    // Split scalars (magnitudes below 2^127): 16-bit windows cover them in exactly 8 windows; 15 bits need 9 and 14 bits 10, whose last
    // window holds 8 / 2 bits of digit -- a few hundred (or four) buckets with thousands of points each, cut into parts and merged by
    // workgroups.  Measured (three in flight / one in flight, ms), default against 16 bits: G1 2^17 points 0.83 / 1.29 -> 0.74 / 1.14,
    // 2^18 1.30 / 1.86 -> 1.13 / 1.50 (2^16: a tie); G2 2^18 3.05 / 4.21 -> 3.04 / 3.67 (2^17 and below: 16 bits lose when pipelined).
    // n is the doubled count here.
    if (glv && c < 16 && n >= ((size_t)1 << (VSP_MSM_GROUP == 1 ? 18 : 19))) c = 16;
    const long wide = opt(ctx, "msm_wide_windows", 1);
    // 255-bit scalars (no endomorphism split), 2^20 points and more: 17 bits.  255 = 15 x 17, and with the scalars folded to below 2^254
    // (load_scalar) 15 windows carry everything, against 16 windows of 16 bits: G1 2^21 5.84 against 6.01 ms, 2^22 10.57 against 10.91;
    // G2 2^20 9.15 against 9.44, 2^21 16.8 against 17.3, 2^22 31.4 against 32.8 (profiles/r3_window_sweep.txt)
    if (c == 16 && wide && !glv && n >= ((size_t)1 << 20)) c = 17;
    if (c >= 16 && wide && n >= ((size_t)1 << 23)) {
        double best = 0; int bc = 16;
        for (int k = 16; k <= 23; k++) {
            const double W = glv ? (double)((128 + k - 1) / k) : (double)((255 % k == 0 ? 254 : 255) / k + 1);      // (g.fold)
            const double cost = (double)n * W * (k > 16 ? 0.87 : 1.0) + W * (double)((size_t)1 << (k - 1)) * 4.1;
            if (k == 16 || cost < best) { best = cost; bc = k; }
        }
        c = bc;
    }
    return (unsigned)c;
}

// ------------------------------------------------------------------------------------------------
// Host side.  An MSM is split into launch (everything up to the asynchronous copy of W*4 window results into a pinned
// buffer, all on the work slot's own stream) and finish (wait + Horner on the host), so that several MSMs can be in
// flight at once: the prover runs its five on separate streams, and back-to-back MSMs pipeline.
static int ensure_w(vsp_ctx *ctx, hipStream_t st, DevBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes && b.p) return VSP_OK;
    if (b.p) { VSP_HIP(hipStreamSynchronize(st)); hipFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 8;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) { b.p = nullptr; return set_error(ctx, VSP_ERR_NOMEM, "msm: hipMalloc failed"); }
    b.cap = want;
    return VSP_OK;
}

// The two scans on every launch's path (bucket counts -> offsets, parts per bucket -> part offsets) take their tile sums from the kernel
// that PRODUCES their input (k_chunk_prefix, k_plan: 256 values per workgroup, block_sum_to) and finish in ONE kernel: every workgroup
// adds up the tile sums before its own (at most a few thousand values) and scans its 256 inputs -- two launches instead of six.
__device__ __forceinline__ void block_sum_to(uint32_t v, uint32_t *dst) {      // all MSM_THREADS threads of the block call it
    __shared__ uint32_t part[MSM_THREADS / 64];
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_down((int)v, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t t = 0; for (unsigned k = 0; k < MSM_THREADS / 64; k++) t += part[k]; *dst = t; }
}
__global__ __launch_bounds__(MSM_THREADS) void k_scan_tiles256(const uint32_t *in, size_t n, const uint32_t *tilesum, uint32_t *out, uint32_t *out2) {
    __shared__ uint32_t base_sh;
    uint32_t b = 0;
    for (unsigned j = threadIdx.x; j < blockIdx.x; j += MSM_THREADS) b += tilesum[j];
    uint32_t btot;
    block_exclusive_scan(b, &btot);
    if (threadIdx.x == 0) base_sh = btot;
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const uint32_t v = i < n ? in[i] : 0u;
    uint32_t tot;
    const uint32_t ex = block_exclusive_scan(v, &tot) + base_sh;
    if (i < n) { out[i] = ex; if (out2) out2[i] = ex; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) { out[n] = base_sh + tot; if (out2) out2[n] = base_sh + tot; }
}
static int exclusive_scan_w(vsp_ctx *ctx, MsmWork &wk, const uint32_t *in, size_t n, uint32_t *out, uint32_t *out2) {
    size_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    VSP_TRY(ensure_w(ctx, wk.stream, wk.blocksum, (nb + 1) * sizeof(uint32_t)));
    uint32_t *bs = (uint32_t *)wk.blocksum.p;
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(MSM_THREADS), 0, wk.stream, in, n, bs);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(MSM_THREADS), 0, wk.stream, bs, nb);
    hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(MSM_THREADS), 0, wk.stream, in, n, (const uint32_t *)bs, out, out2);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

static int work_init(vsp_ctx *ctx, MsmWork &wk, hipStream_t stream_or_null) {
    if (!wk.inited) {
        VSP_HIP(hipEventCreate(&wk.ev0)); VSP_HIP(hipEventCreate(&wk.ev1));
        VSP_HIP(hipEventCreateWithFlags(&wk.done, hipEventDisableTiming));
        VSP_HIP(hipEventCreateWithFlags(&wk.plan_ready, hipEventDisableTiming));
        VSP_HIP(hipHostMalloc(&wk.h_pinned, MsmWork::PINNED_BYTES, hipHostMallocDefault)); wk.pinned_cap = MsmWork::PINNED_BYTES;
        VSP_HIP(hipHostMalloc(&wk.h_census, 64, hipHostMallocDefault));
        VSP_HIP(hipHostMalloc(&wk.h_rec, MsmWork::REC_RING * 288, hipHostMallocDefault));
        for (unsigned k = 0; k < MsmWork::REC_RING; k++) VSP_HIP(hipEventCreateWithFlags(&wk.rec_ev[k], hipEventDisableTiming));
        VSP_HIP(hipEventCreateWithFlags(&wk.census_done, hipEventDisableTiming));
        wk.inited = true;
    }
    if (stream_or_null != nullptr) wk.stream = stream_or_null;       // slot 0 follows the context's current stream
    else if (wk.stream == nullptr) {                                 // no borrowed stream (msm_slot_use_stream): the slot's own, made on first need
        if (!wk.own) { VSP_TRY(msm_make_slot_stream(ctx, &wk.own)); wk.own_stream = true; }
        wk.stream = wk.own;
    }
    return VSP_OK;
}

// queue the 0/1 census of a scalar vector on the slot's stream (result read by the next msm_launch of the same vector)
static int msm_census(vsp_ctx *ctx, MsmWork &wk, const Fr *d_scalars, size_t n, hipStream_t on_stream = nullptr, unsigned batch = 1, size_t batch_stride = 0) {
    hipStream_t st = on_stream ? on_stream : wk.stream;
    VSP_TRY(ensure_w(ctx, st, wk.counters, 64));
    VSP_HIP(hipMemsetAsync(wk.counters.p, 0, 64, st));
    { unsigned cb = (unsigned)((n + 255) / 256); if (cb > 1024) cb = 1024;
      hipLaunchKernelGGL(k_classify, dim3(cb, batch), dim3(256), 0, st, d_scalars, n, (uint32_t *)wk.counters.p, batch_stride); }
    VSP_HIP(hipMemcpyAsync(wk.h_census, (uint32_t *)wk.counters.p + 1, 12, hipMemcpyDeviceToHost, st));      // [0] count, [2] non-canonical flag
    VSP_HIP(hipEventRecord(wk.census_done, st));
    wk.census_pending = true; wk.census_n = n; wk.census_scalars = (const void *)d_scalars;
    return VSP_OK;
}

#if VSP_MSM_GROUP == 1
using F28 = Fp28; using Row28 = Affine28;                   // this group's field and base rows on 28-bit limbs
#else
using F28 = Fp2x28; using Row28 = Affine28x2;
#endif
// what the stages of one msm_launch share: the request as the kernels see it and the sizes its geometry gives
struct MsmLaunch {
    MsmRequest rq;                      // the caller's, with batch >= 1 and glv only where the interleaved table is there
    hipStream_t st;
    const MsmWork *plan_from;           // the work whose digit sort / bucket plan this launch reuses, or null
    const void *table28;                // the bases (or table) on 28-bit limbs, or null
    const Fr *scalars; size_t n;        // what the sort reads: with the endomorphism split 2 rq.n half-length scalars (k_glv_split)
    long sort_mode;                     // option "msm_sort": 1 never staged, 2 staged whenever c >= 17
    MsmTuning tune;                     // the request's, or the options'
    bool fused_split, fused_scans, dimbits;      // dimbits: the bucket reduction's last step is k_dimbits (which decides how wide a digit may be)
    size_t M, Smax;                     // upper bounds on sorted entries and on bucket parts
    unsigned per_w, nblk, gblk, ablk;
};

// geometry: the window size and the part length from the effective problem size (or from the shared plan), then the digit split
template <class F> static int msm_geometry(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, MsmGeom &g, size_t &n_eff) {
    const MsmPre *pre = L.rq.pre; const bool glv = L.rq.glv; const size_t n = L.rq.n; const unsigned batch = L.rq.batch;
    const uint32_t imul = glv ? 2u : 1u;                    // rows per point in the interleaved table
    n_eff = n;
    if (L.plan_from) {
        g = L.plan_from->g; n_eff = L.plan_from->n_eff;
        if (L.plan_from->n != n) return set_error(ctx, VSP_ERR_ARG, "msm: shared plan of a different size");
        if ((g.single != 0) != (pre != nullptr) || (pre && (g.idx_stride != pre->stride * imul || g.idx_first != pre->first * imul || g.c != pre->c)))
            return set_error(ctx, VSP_ERR_ARG, "msm: shared plan needs bases precomputed alike");
    } else {
        VSP_TRY(ensure_w(ctx, L.st, wk.counters, 64));
        // effective problem size: scalars other than 0 and 1 (one small kernel + a read-back); the census may have been queued
        // earlier by msm_census (the prover queues all of them before any heavy kernel).  The same kernel flags scalars >= r.
        // The count only steers the window size / part length, never the result, so a slot that has seen a vector of this
        // length before plans from that earlier count and reads the fresh one at finish: no host wait on the launch path.
        wk.check_pending = false;
        if (!L.rq.dense) {
            if (!(wk.census_pending && wk.census_n == n && wk.census_scalars == (const void *)L.rq.scalars)) VSP_TRY(msm_census(ctx, wk, L.rq.scalars, n, nullptr, batch, L.rq.stride));
            wk.check_pending = true;
            if (n >= 4096) {
                if (wk.neff_cache_n == n && !opt(ctx, "msm_census_sync", 0)) n_eff = wk.neff_cache;
                else {
                    VSP_HIP(hipEventSynchronize(wk.census_done));
                    uint32_t h_cnt = *(volatile uint32_t *)wk.h_census / batch;      // (a batch is counted together: the mean per vector)
                    n_eff = h_cnt < 256 ? 256 : h_cnt;
                }
            }
        }
        wk.census_pending = false;
        if (glv) n_eff *= 2;                                  // two half-length scalars per counted scalar
        g.c = pre ? pre->c : pick_window_bits(ctx, L.tune.window_bits, n_eff, glv);
        g.sbits = glv ? 128u : 255u;
        // 255-bit scalars: 255 / c + 1 windows cover the bits plus the carry of the signed recoding; split halves are magnitudes below
        // 2^127: ceil(128 / c) windows, and the top window's spare bit absorbs the carry
        g.fold = (!glv && opt(ctx, "msm_fold", 1) && 255u % g.c == 0u) ? 1u : 0u;
        if (batch > 1 && g.c > 16) g.c = 16;
        if (batch > 1 && g.c < 7) g.c = 7;                      // (a batch of tiny vectors: not hundreds of 4-bit windows per vector)
        g.Wk = glv ? (128u + g.c - 1) / g.c : (g.fold ? 254u / g.c + 1 : g.sbits / g.c + 1);
        g.K = batch; g.kstride = batch > 1 ? L.rq.stride : 0;
        g.W = g.Wk * g.K;                                      // what the sort, the accumulation and the reduction see: one bucket set per (vector, window)
        g.B = 1u << (g.c - 1);
        g.lb = g.c > 16 ? g.c - 16 : 0u;
        g.n = glv ? 2 * n : n;
        g.single = pre ? 1u : 0u; g.idx_stride = pre ? (uint32_t)(pre->stride * imul) : 0u; g.idx_first = pre ? (uint32_t)(pre->first * imul) : 0u;
        g.Wr = pre ? g.K : g.W;                                // bucket sets: one per vector over a table of window multiples, else one per window
        g.G = (size_t)g.Wr * g.B;
        const long t = L.tune.split;
        if (pre) {
            // one bucket set: ~n_eff*W/B points per bucket; parts of T points, about 2^18 of them to fill the GPU evenly
            size_t est = n_eff * g.W / ((size_t)1 << 18);
            unsigned T = 16; while (T < est && T < (1u << 20)) T <<= 1;      // ~n_eff*W/B points per bucket -> <= ~8 parts per bucket
            // ... but not a length that fills the GPU a whole number of times: 2^18 equal parts of 64 points are exactly two rounds of the
            // 2048 resident waves, every wave slot has to run exactly two parts, and nothing evens out the stagger of the second round
            // (accumulation 2.87 ms, one multi-exponentiation 4.0 ms); 7/8 of the length makes it 2.5 rounds (2.54 ms, 3.7 ms)
            if (T >= 64) T = T / 8 * 7;
            g.T = t > 0 ? (unsigned)t : T;
            if ((size_t)g.Wk * pre->stride * imul >= ((size_t)1 << 31)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: precomputed table too large to index");
        } else {
            // parts of at most T points; buckets alone may not give the ~2^18 lanes that fill the GPU (few windows, narrow windows,
            // or two lanes per part): then T shrinks until bucket parts do
            size_t mean = n_eff / g.B + 1;
            size_t T = mean * 4 < 128 ? 128 : mean * 4;
            const size_t target = ((size_t)1 << 18) / LaneView<F>::LANES;
            if (g.G < target) {
                size_t t2 = n_eff * g.W / (target - g.G) + 1, p2 = 16;
                while (p2 < t2) p2 <<= 1;
                if (p2 < T) T = p2;
            }
            g.T = t > 0 ? (unsigned)t : (unsigned)T;
        }
    }
    g.bd = 8;
    // per group: a shared plan carries the window size, not the digit split.  Which last step the bucket reduction takes decides how wide a digit may be
    L.dimbits = L.table28 ? use_dimbits<F28>(L.tune.dimbits, g) : use_dimbits<F>(L.tune.dimbits, g);
    split_digits<F>(g, L.dimbits);
    return VSP_OK;
}

// the endomorphism split k = k1 + k2 lambda: a kernel of its own, or inside the digit kernel where the LDS counting sort follows (k_glv_digits)
static int msm_split_scalars(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
    const size_t n = L.rq.n;
    L.fused_split = L.rq.glv && !L.plan_from && g.c <= 16 && ((opt(ctx, "msm_fused_split", 1) && 2 * n >= ((size_t)1 << 15) && L.sort_mode != 2) || g.K > 1);
    if (!L.rq.glv) return VSP_OK;
    if (!L.plan_from && !L.fused_split) {
        VSP_TRY(ensure_w(ctx, L.st, wk.glv_scalars, 2 * n * sizeof(Fr)));
        hipLaunchKernelGGL(k_glv_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.st, L.rq.scalars, n, (Fr *)wk.glv_scalars.p);
        VSP_LAUNCH_CHECK();
        L.scalars = (const Fr *)wk.glv_scalars.p;
    }
    L.n = 2 * n;                                            // from here on: 2n points (P_i, phi(P_i)), 2n scalars (k1_i, k2_i)
    return VSP_OK;
}

// buffer sizing: the pinned landing buffer of the window results, the bucket arrays, and the plan's arrays when this launch makes a plan
template <class F> static int msm_buffers(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st;
    if (!L.dimbits && ((1u << g.q0) > MsmBlock<F>::NTL || (1u << g.q2) > MsmBlock<F>::NTL)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: window too wide");
    if (g.c > 23) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: windows wider than 23 bits are not built");
    L.M = L.n * g.W;
    if (L.M >= ((size_t)1 << 32)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: n * windows >= 2^32 (sorted positions are 32-bit); use wider windows or shard the points");
    L.Smax = g.G + L.M / g.T + 1;
    L.per_w = dims_per_w(g);
    { const size_t need = (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<F>);      // room for either layout of the window results
      if (need > wk.pinned_cap) {                                                // (a batch: K times the windows; the slot is idle here, nothing writes the old buffer)
          if (need > ((size_t)64 << 20)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: too many windows (a batch: fewer vectors per call)");
          VSP_HIP(hipStreamSynchronize(st));
          void *nb = nullptr;
          if (hipHostMalloc(&nb, need, hipHostMallocDefault) != hipSuccess) return set_error(ctx, VSP_ERR_NOMEM, "msm: pinned buffer for the window results");
          hipHostFree(wk.h_pinned); wk.h_pinned = nb; wk.pinned_cap = need;
      } }
    VSP_TRY(ensure_w(ctx, st, wk.buckets, g.G * sizeof(XYZZ<F>)));
    VSP_TRY(ensure_w(ctx, st, wk.partials, L.Smax * sizeof(XYZZ<F>)));
    VSP_TRY(ensure_w(ctx, st, wk.dims, (size_t)g.Wr * L.per_w * sizeof(XYZZ<F>)));
    VSP_TRY(ensure_w(ctx, st, wk.winres, (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<F>)));      // room for either layout (4 or 25 records per window)
    L.nblk = (unsigned)((L.n + MSM_THREADS - 1) / MSM_THREADS);
    L.gblk = (unsigned)((g.G + MSM_THREADS - 1) / MSM_THREADS);
    L.ablk = (unsigned)((L.Smax + MSM_THREADS - 1) / MSM_THREADS);
    if (L.plan_from) return VSP_OK;
    for (DevBuf *b : {&wk.cnt, &wk.off, &wk.cursor, &wk.nsub, &wk.suboff, &wk.heavy, &wk.medium}) VSP_TRY(ensure_w(ctx, st, *b, (g.G + 1) * 4));
    VSP_TRY(ensure_w(ctx, st, wk.sorted, L.M * 4));
    VSP_TRY(ensure_w(ctx, st, wk.partbucket, L.Smax * 4));
    VSP_TRY(ensure_w(ctx, st, wk.perm, L.Smax * 4));
    VSP_TRY(ensure_w(ctx, st, wk.sizehist, 2 * SZ_BINS * 4));
    return VSP_OK;
}

// the LDS counting sort's two kernels take up to 128 KiB of LDS: allowed once per context (= per device) and per code object
static int lds_sort_attrs(vsp_ctx *ctx) {
    bool &attr_set = ctx->lds_attr_set[VSP_MSM_GROUP - 1];
    if (attr_set) return VSP_OK;
    VSP_HIP(hipFuncSetAttribute((const void *)k_count_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    VSP_HIP(hipFuncSetAttribute((const void *)k_scatter_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    attr_set = true;
    return VSP_OK;
}
// chunks per window of the LDS counting sort: about 256 workgroups over all windows, none with fewer than 8192 scalars
static unsigned lds_chunks(const MsmGeom &g, size_t n) {
    unsigned nchunks = 256 / g.W; if (nchunks < 1) nchunks = 1;
    while (nchunks > 1 && n / nchunks < 8192) nchunks >>= 1;
    return nchunks;
}

// staged sort: 8 + 8 bits through LDS tiles, the rest inside LDS (k_ms_*): every global write is a run of whole lines
static int msm_sort_staged(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st; const size_t M = L.M;
    uint32_t *cnt = (uint32_t *)wk.cnt.p, *off = (uint32_t *)wk.off.p, *sorted = (uint32_t *)wk.sorted.p;
    // the bits of the bucket index (c - 1): 8 for the first pass, rb <= 6 for the last step, the rest (1 .. 8) for the second pass;
    // rb as large as keeps the last step's segments at ~1024 entries (2^23 points, c = 19: 2^13 segments per window, not 2^16
    // of 128 entries each -- the last step paid per segment: 1.4 ms)
    const unsigned parents = g.single ? 1u : g.W;
    const size_t npp = g.single ? (size_t)g.W * L.n : L.n;
    unsigned rb = g.c > 17 ? g.c - 17 : 0;          // (the staged sort forced below 17 bits, "msm_sort" = 2: no minimum)
    { const unsigned hi = g.c - 10 < 6 ? g.c - 10 : 6; const unsigned lg = ceil_log2(npp / 1024 + 1);
      const unsigned want = g.c - 1 > lg ? g.c - 1 - lg : 0; if (want > rb) rb = want; if (rb > hi) rb = hi; }
    const unsigned bits2 = g.c - 9 - rb, nb2 = 1u << bits2;
    if (bits2 < 1 || bits2 > 8) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: staged sort: window size outside its range");
    const unsigned chunks = (unsigned)((npp + MS_CHUNK - 1) / MS_CHUNK);
    const size_t H1 = (size_t)parents * 257 * chunks, S1 = (size_t)parents * 256, H2 = S1 * nb2;
    const size_t P2 = (M + MS_CHUNK - 1) / MS_CHUNK + S1;      // pieces of the second pass: at most one partial piece per segment
    VSP_TRY(ensure_w(ctx, st, wk.pairs_a, M * sizeof(uint2)));
    VSP_TRY(ensure_w(ctx, st, wk.pairs_b, M * sizeof(uint2)));
    VSP_TRY(ensure_w(ctx, st, wk.ms_h1, (H1 + 1) * 4)); VSP_TRY(ensure_w(ctx, st, wk.ms_h1s, (H1 + 1) * 4));
    const size_t P3 = (M + MS_CHUNK - 1) / MS_CHUNK + M / MS_SEG_LONG + 1;      // pieces of the third: only segments longer than MS_SEG_LONG have any
    // ms_h2: the second pass's piece histograms | the third's | piece counts | pbase2 | pbase3
    VSP_TRY(ensure_w(ctx, st, wk.ms_h2, (P2 * 256 + P3 * 64 + (H2 + 1) + (S1 + 1) + (H2 + 1)) * 4)); VSP_TRY(ensure_w(ctx, st, wk.ms_h2s, (H2 + 1) * 4));
    uint2 *pa = (uint2 *)wk.pairs_a.p, *pb = (uint2 *)wk.pairs_b.p;
    uint32_t *h1 = (uint32_t *)wk.ms_h1.p, *h1s = (uint32_t *)wk.ms_h1s.p, *h2 = (uint32_t *)wk.ms_h2.p, *h2s = (uint32_t *)wk.ms_h2s.p;
    uint32_t *h3 = h2 + P2 * 256, *pcount = h3 + P3 * 64, *pbase2 = pcount + (H2 + 1), *pbase3 = pbase2 + (S1 + 1);
    hipLaunchKernelGGL(k_ms_pairs, dim3(L.nblk), dim3(MSM_THREADS), 0, st, L.scalars, g, pa);
    MsPass p1; p1.npp = npp; p1.parents = parents; p1.chunks = chunks; p1.seg = nullptr; p1.seg_stride = 0; p1.pbase = nullptr; p1.S = 0;
    p1.shift = g.c - 9; p1.mask = 0xFFu; p1.bins = 256; p1.slots = 256;
    MsPass p2 = p1; p2.seg = h1s; p2.seg_stride = chunks; p2.pbase = pbase2; p2.S = (unsigned)S1; p2.shift = rb; p2.mask = nb2 - 1u; p2.bins = nb2;
    MsPass p3 = p1; p3.seg = h2s; p3.seg_stride = 1; p3.pbase = pbase3; p3.S = (unsigned)H2; p3.shift = 0; p3.mask = (1u << rb) - 1u; p3.bins = 1u << rb; p3.slots = 64;
    hipLaunchKernelGGL(k_ms_hist, dim3(parents * chunks), dim3(MS_THREADS), 0, st, (const uint2 *)pa, p1, h1);
    VSP_LAUNCH_CHECK();
    VSP_TRY(exclusive_scan_w(ctx, wk, h1, H1, h1s, nullptr));
    hipLaunchKernelGGL(k_ms_scatter, dim3(parents * chunks), dim3(MS_THREADS), 0, st, (const uint2 *)pa, pb, (uint32_t *)nullptr, p1, (const uint32_t *)h1s, (const uint32_t *)nullptr);
    // second pass over the segments of the first ((parent, top 8 bits): h1s[segment * chunks] is where one starts; the parked entries
    // follow the last one at h1s[S1 * chunks]), in pieces of MS_CHUNK elements
    hipLaunchKernelGGL(k_ms_piece_counts, dim3((unsigned)((S1 + MSM_THREADS) / MSM_THREADS)), dim3(MSM_THREADS), 0, st, (const uint32_t *)h1s, chunks, S1, 0u, pcount);
    VSP_TRY(exclusive_scan_w(ctx, wk, pcount, S1 + 1, pbase2, nullptr));
    hipLaunchKernelGGL(k_ms_hist, dim3((unsigned)P2), dim3(MS_THREADS), 0, st, (const uint2 *)pb, p2, h2);
    hipLaunchKernelGGL(k_ms_cursors, dim3((unsigned)S1), dim3(256), 0, st, h2, (const uint32_t *)pbase2, (const uint32_t *)h1s, chunks, (unsigned)S1, nb2, h2s);
    hipLaunchKernelGGL(k_ms_scatter, dim3((unsigned)P2), dim3(MS_THREADS), 0, st, (const uint2 *)pb, pa, (uint32_t *)nullptr, p2, (const uint32_t *)h2, (const uint32_t *)h2s);
    // what is left of the bucket index: inside one wave per segment (k_ms_final), or -- segments longer than MS_SEG_LONG -- a third pass in pieces
    hipLaunchKernelGGL(k_ms_piece_counts, dim3((unsigned)((H2 + MSM_THREADS) / MSM_THREADS)), dim3(MSM_THREADS), 0, st, (const uint32_t *)h2s, 1u, H2, MS_SEG_LONG, pcount);
    VSP_TRY(exclusive_scan_w(ctx, wk, pcount, H2 + 1, pbase3, nullptr));
    hipLaunchKernelGGL(k_ms_hist, dim3((unsigned)P3), dim3(MS_THREADS), 0, st, (const uint2 *)pa, p3, h3);
    { size_t wg = (H2 + 3) / 4; if (wg > 65536) wg = 65536;
      hipLaunchKernelGGL(k_ms_final, dim3((unsigned)wg), dim3(256), 0, st, (const uint2 *)pa, (const uint32_t *)h2s, H2, rb, (const uint32_t *)pbase3, h3, cnt, off, sorted); }
    hipLaunchKernelGGL(k_ms_scatter, dim3((unsigned)P3), dim3(MS_THREADS), 0, st, (const uint2 *)pa, (uint2 *)nullptr, sorted, p3, (const uint32_t *)h3, (const uint32_t *)nullptr);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// windows wider than 16 bits: the LDS counting sort over the HIGH 15 bits of the bucket index (as a 16-bit window), then k_segment_sort over the low ones
static int msm_sort_wide(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st; const size_t n = L.n;
    MsmGeom gh = g; gh.c = 16; gh.B = 1u << 15; gh.lb = 0; gh.G = (size_t)g.Wr << 15;
    const unsigned nchunks = lds_chunks(g, n);
    const size_t chunk_len = (n + nchunks - 1) / nchunks;
    VSP_TRY(ensure_w(ctx, st, wk.digits, (size_t)g.W * n * 3));
    VSP_TRY(ensure_w(ctx, st, wk.blockhist, (size_t)nchunks * g.W * gh.B * sizeof(uint32_t)));
    VSP_TRY(ensure_w(ctx, st, wk.cnt_hi, (gh.G + 1) * 4));
    VSP_TRY(ensure_w(ctx, st, wk.off_hi, (gh.G + 1) * 4));
    VSP_TRY(ensure_w(ctx, st, wk.tmp_sorted, L.M * 4));
    VSP_TRY(ensure_w(ctx, st, wk.tmp_lo, L.M));
    uint16_t *hi = (uint16_t *)wk.digits.p; uint8_t *lo = (uint8_t *)(hi + (size_t)g.W * n);
    uint32_t *blockhist = (uint32_t *)wk.blockhist.p, *cnt_hi = (uint32_t *)wk.cnt_hi.p, *off_hi = (uint32_t *)wk.off_hi.p;
    const size_t lds_bytes = (size_t)gh.B * sizeof(uint32_t);
    VSP_TRY(lds_sort_attrs(ctx));
    hipLaunchKernelGGL(k_digits_wide, dim3(L.nblk), dim3(MSM_THREADS), 0, st, L.scalars, g, hi, lo);
    hipLaunchKernelGGL(k_count_lds, dim3(nchunks * g.W), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)hi, gh, nchunks, chunk_len, blockhist);
    hipLaunchKernelGGL(k_chunk_prefix, dim3((unsigned)((gh.G + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st, blockhist, g.single ? nchunks * g.W : nchunks, gh.G, cnt_hi, (uint32_t *)nullptr, gh.G);
    VSP_LAUNCH_CHECK();
    VSP_TRY(exclusive_scan_w(ctx, wk, cnt_hi, gh.G, off_hi, nullptr));
    hipLaunchKernelGGL(k_scatter_lds, dim3(nchunks * g.W), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)hi, (const uint8_t *)nullptr, gh, nchunks, chunk_len,
                       (const uint32_t *)blockhist, (const uint32_t *)off_hi, (uint32_t *)wk.tmp_sorted.p, (const uint8_t *)lo, (uint8_t *)wk.tmp_lo.p);
    { size_t wg = (gh.G + 3) / 4; if (wg > 65536) wg = 65536;
      hipLaunchKernelGGL(k_segment_sort, dim3((unsigned)wg), dim3(256), 0, st, (const uint32_t *)wk.tmp_sorted.p, (const uint8_t *)wk.tmp_lo.p, (const uint32_t *)off_hi,
                         gh.G, g.lb, (uint32_t *)wk.cnt.p, (uint32_t *)wk.off.p, (uint32_t *)wk.sorted.p); }
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the LDS counting sort (windows of at most 16 bits: large problems and every batch)
static int msm_sort_lds(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st; const size_t n = L.n;
    uint32_t *cnt = (uint32_t *)wk.cnt.p, *off = (uint32_t *)wk.off.p;
    const bool batch_single = g.single && g.K > 1;          // K bucket sets, each fed by its vector's Wk windows: their histograms must lie together
    const unsigned nchunks = batch_single ? 1u : lds_chunks(g, n);
    const size_t chunk_len = (n + nchunks - 1) / nchunks;
    VSP_TRY(ensure_w(ctx, st, wk.digits, (size_t)g.W * n * sizeof(uint16_t) + (size_t)g.K * n));      // + one sign byte per scalar (endomorphism split), per vector of a batch
    VSP_TRY(ensure_w(ctx, st, wk.blockhist, (size_t)nchunks * g.W * g.B * sizeof(uint32_t)));
    uint16_t *digits = (uint16_t *)wk.digits.p; uint32_t *blockhist = (uint32_t *)wk.blockhist.p;
    uint8_t *flips = (uint8_t *)(digits + (size_t)g.W * n);
    const size_t lds_bytes = (size_t)g.B * sizeof(uint32_t);
    VSP_TRY(lds_sort_attrs(ctx));
    if (L.fused_split) hipLaunchKernelGGL(k_glv_digits, dim3((unsigned)((L.rq.n + MSM_THREADS - 1) / MSM_THREADS), g.K), dim3(MSM_THREADS), 0, st, L.rq.scalars, L.rq.n, g, digits, flips);
    else hipLaunchKernelGGL(k_digits, dim3(L.nblk, g.K), dim3(MSM_THREADS), 0, st, L.scalars, g, digits, flips);
    hipLaunchKernelGGL(k_count_lds, dim3(nchunks * g.W), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)digits, g, nchunks, chunk_len, blockhist);
    VSP_TRY(ensure_w(ctx, st, wk.blocksum, ((size_t)L.gblk + 2) * sizeof(uint32_t)));      // (the three-kernel scan shares this buffer and may have regrown it)
    uint32_t *tilesum = (uint32_t *)wk.blocksum.p;
    hipLaunchKernelGGL(k_chunk_prefix, dim3(L.gblk), dim3(MSM_THREADS), 0, st, blockhist, batch_single ? g.Wk : (g.single ? nchunks * g.W : nchunks), g.G, cnt,
                       L.fused_scans ? tilesum : (uint32_t *)nullptr, batch_single ? (size_t)g.B : g.G);
    VSP_LAUNCH_CHECK();
    if (L.fused_scans) hipLaunchKernelGGL(k_scan_tiles256, dim3(L.gblk), dim3(MSM_THREADS), 0, st, (const uint32_t *)cnt, g.G, (const uint32_t *)tilesum, off, (uint32_t *)nullptr);
    else VSP_TRY(exclusive_scan_w(ctx, wk, cnt, g.G, off, nullptr));
    hipLaunchKernelGGL(k_scatter_lds, dim3(nchunks * g.W), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)digits, (const uint8_t *)flips, g, nchunks, chunk_len,
                       (const uint32_t *)blockhist, (const uint32_t *)off, (uint32_t *)wk.sorted.p, (const uint8_t *)nullptr, (uint8_t *)nullptr);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the digit sort: the entries of every bucket together (cnt, off, sorted), by one of four sorts
static int msm_digit_sort(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
    VSP_HIP(hipMemsetAsync(wk.counters.p, 0, 64, L.st));
    // the two scans over the buckets in one kernel each (k_scan_tiles256) while a workgroup can add up the tile sums before its own
    // cheaply: up to 4096 tiles of 256 buckets (2^20 buckets); beyond that the three-kernel scan.  Option "msm_fused_scans" = 0: never.
    L.fused_scans = opt(ctx, "msm_fused_scans", 1) && L.gblk <= 4096;
    const size_t n = L.n;
    const bool staged = g.K == 1 && g.c >= 12 && g.c <= 23 && n >= 4096 && L.sort_mode != 1 && (L.sort_mode == 2 || (g.c >= 17 && n >= ((size_t)1 << 20)));
    if (staged) return msm_sort_staged(ctx, wk, L, g);
    if (g.c > 16 && n >= ((size_t)1 << 15)) return msm_sort_wide(ctx, wk, L, g);
    if (g.c <= 16 && (n >= ((size_t)1 << 15) || g.K > 1)) return msm_sort_lds(ctx, wk, L, g);
    // small problems: a global counting sort
    uint32_t *cnt = (uint32_t *)wk.cnt.p, *cursor = (uint32_t *)wk.cursor.p;
    VSP_HIP(hipMemsetAsync(cnt, 0, (g.G + 1) * 4, L.st));
    hipLaunchKernelGGL(k_count, dim3(L.nblk), dim3(MSM_THREADS), 0, L.st, L.scalars, g, cnt);
    VSP_LAUNCH_CHECK();
    VSP_TRY(exclusive_scan_w(ctx, wk, cnt, g.G, (uint32_t *)wk.off.p, cursor));
    hipLaunchKernelGGL(k_scatter, dim3(L.nblk), dim3(MSM_THREADS), 0, L.st, L.scalars, g, cursor, (uint32_t *)wk.sorted.p);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the bucket plan over the sorted entries: parts of at most T points per bucket, ordered by size (k_plan .. k_partsort)
static int msm_bucket_plan(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st;
    const uint32_t *cnt = (const uint32_t *)wk.cnt.p;
    uint32_t *nsub = (uint32_t *)wk.nsub.p, *suboff = (uint32_t *)wk.suboff.p;
    VSP_TRY(ensure_w(ctx, st, wk.blocksum, ((size_t)L.gblk + 2) * sizeof(uint32_t)));
    uint32_t *tilesum = (uint32_t *)wk.blocksum.p;
    uint32_t *size_hist = (uint32_t *)wk.sizehist.p, *bin_cursor = size_hist + SZ_BINS;
    uint32_t *redo0 = nullptr;                              // the accumulation's hand-back counter, cleared by k_plan when this launch goes on to accumulate over its own plan
    if (!L.rq.plan_only && L.table28) { VSP_TRY(ensure_w(ctx, st, wk.redo, (L.Smax + 1) * sizeof(uint32_t))); redo0 = (uint32_t *)wk.redo.p; }
    hipLaunchKernelGGL(k_plan, dim3(L.gblk), dim3(MSM_THREADS), 0, st, cnt, g.G, g.T, nsub, (uint32_t *)wk.heavy.p, (uint32_t *)wk.medium.p, (uint32_t *)wk.counters.p,
                       L.fused_scans ? tilesum : (uint32_t *)nullptr, size_hist, 2u * SZ_BINS, redo0);
    VSP_LAUNCH_CHECK();
    if (L.fused_scans) hipLaunchKernelGGL(k_scan_tiles256, dim3(L.gblk), dim3(MSM_THREADS), 0, st, (const uint32_t *)nsub, g.G, (const uint32_t *)tilesum, suboff, (uint32_t *)nullptr);
    else VSP_TRY(exclusive_scan_w(ctx, wk, nsub, g.G, suboff, nullptr));
    uint32_t *part_bucket = (uint32_t *)wk.partbucket.p, *perm = (uint32_t *)wk.perm.p;
    hipLaunchKernelGGL(k_partinfo, dim3(L.ablk), dim3(256), 0, st, cnt, (const uint32_t *)suboff, g.G, g.T, part_bucket, size_hist);
    hipLaunchKernelGGL(k_binscan, dim3(1), dim3(SZ_BINS), 0, st, (const uint32_t *)size_hist, bin_cursor);
    hipLaunchKernelGGL(k_partsort, dim3(L.ablk), dim3(256), 0, st, cnt, (const uint32_t *)suboff, (const uint32_t *)part_bucket, g.G, g.T, bin_cursor, perm);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipEventRecord(wk.plan_ready, st));
    return VSP_OK;
}

// accumulation over the plan (this slot's own or the shared one), then the bucket reduction (launch_tail)
template <class F> static int msm_accumulate(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const Affine<F> *bases = (const Affine<F> *)L.rq.bases;
    const hipStream_t st = L.st;
    const MsmWork *pl = L.plan_from ? L.plan_from : &wk;
    XYZZ<F> *buckets = (XYZZ<F> *)wk.buckets.p, *partials = (XYZZ<F> *)wk.partials.p, *winres = (XYZZ<F> *)wk.winres.p;
    wk.dimbits = L.dimbits;
    // (the diagnostic build without hand-laid-out routines runs the multi-exponentiation on the generic 12 x 32-bit kernels only: the
    // 28-bit reduction kernels over portable products crash this toolchain's backend -- Machine Copy Propagation / post-RA pseudo
    // expansion segfault in k_dimsum<Fp28> / k_dimsum<Fp2x28>; the 28-bit and 29-bit FIELD forms stay covered by vsp_selftest_field,
    // vsp_selftest_xyzz_add and the transforms)
#if defined(VSP_PORTABLE_MUL)
    constexpr bool have28 = sizeof(F) == 0;
#else
    constexpr bool have28 = sizeof(F) != 0;
#endif
    if constexpr (have28) if (L.table28) {
        // 14 x 28-bit accumulation; bucket parts that meet an equal-x pair are listed and redone by the generic kernel
        VSP_TRY(ensure_w(ctx, st, wk.redo, (L.Smax + 1) * sizeof(uint32_t)));
        uint32_t *redo = (uint32_t *)wk.redo.p;               // [0] = count, list from [1]
        if (L.plan_from) VSP_HIP(hipMemsetAsync(redo, 0, sizeof(uint32_t), st));      // (k_plan cleared it when it ran in this launch)
        // the bucket sums stay in the 28-bit form from here to the results per window; the parts the generic kernel redoes (equal-x
        // pairs) are written to the 12 x 32-bit arrays of the same indexing and, converted, to the 28-bit ones
        VSP_TRY(ensure_w(ctx, st, wk.buckets28, g.G * sizeof(XYZZ<F28>)));
        VSP_TRY(ensure_w(ctx, st, wk.partials28, L.Smax * sizeof(XYZZ<F28>)));
        VSP_TRY(ensure_w(ctx, st, wk.dims, (size_t)g.Wr * L.per_w * sizeof(XYZZ<F28>)));
        XYZZ<F28> *buckets28 = (XYZZ<F28> *)wk.buckets28.p, *partials28 = (XYZZ<F28> *)wk.partials28.p;
        VSP_HIP(hipEventRecord(wk.ev0, st));                  // ev0 .. ev1 bracket the accumulation kernel alone
#if VSP_MSM_GROUP == 1
        long use_asm = opt(ctx, "msm_accum28_asm", 1);
#if defined(VSP_PORTABLE_MUL)
        use_asm = 0;                                        // the diagnostic build without hand-laid-out routines: the C++ twin of the generated loop
#endif
        if (!use_asm)
            hipLaunchKernelGGL(k_accum28_cxx, dim3(L.ablk), dim3(MSM_THREADS), 0, st, (const Row28 *)L.table28, (const uint32_t *)pl->sorted.p,
                               (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                               g.G, g.T, buckets28, partials28, redo + 1, redo);
        else
#endif
        hipLaunchKernelGGL(k_accum28, dim3(L.ablk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, (const Row28 *)L.table28, (const uint32_t *)pl->sorted.p,
                           (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                           g.G, g.T, buckets28, partials28, redo + 1, redo);
        VSP_HIP(hipEventRecord(wk.ev1, st));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_accum_redo<F>), dim3(L.ablk < 64 ? L.ablk : 64), dim3(MSM_THREADS), 0, st, bases, (const uint32_t *)pl->sorted.p,
                           (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->partbucket.p, buckets, partials,
                           (const uint32_t *)(redo + 1), (const uint32_t *)redo, L.rq.glv, buckets28, partials28);
        VSP_LAUNCH_CHECK();
        return launch_tail<F28>(ctx, st, pl, g, L.dimbits, buckets28, partials28, (XYZZ<F28> *)wk.dims.p, winres, (XYZZ<F> *)wk.h_pinned);
    }
    VSP_HIP(hipEventRecord(wk.ev0, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_accum<F>), dim3(L.ablk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, bases, (const uint32_t *)pl->sorted.p,
                       (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                       g.G, g.T, buckets, partials);
    VSP_HIP(hipEventRecord(wk.ev1, st));
    VSP_LAUNCH_CHECK();
    return launch_tail<F>(ctx, st, pl, g, L.dimbits, buckets, partials, (XYZZ<F> *)wk.dims.p, winres, (XYZZ<F> *)wk.h_pinned);
}

// one multi-exponentiation (common.h MsmRequest); plan_from: the work slot rq.plan_from names, or null
template <class F>
static int msm_launch(vsp_ctx *ctx, MsmWork &wk, const MsmRequest &rq, const MsmWork *plan_from) {
    const size_t n = rq.n;
    wk.active = false; wk.n = n;
    if (n == 0) { wk.active = true; wk.empty = true; wk.g.K = rq.batch ? rq.batch : 1; return VSP_OK; }
    wk.empty = false;
    const unsigned batch = rq.batch ? rq.batch : 1;
    // a batch (MsmGeom.K): plain bases, its own digit sort through the LDS counting sort, 16-bit windows at most
    // (a shared plan must be a batch of the same vectors: the prover's A, B1 and B2 multiply by the same K witness vectors)
    if (batch > 1 && rq.plan_only) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: a batch plans and accumulates in one launch");
    if (batch > 1 && plan_from && (plan_from->g.K != batch || plan_from->g.kstride != rq.stride || !plan_from->active || plan_from->empty))
        return set_error(ctx, VSP_ERR_ARG, "msm: shared plan of another batch");
    MsmLaunch L{};
    L.rq = rq; L.rq.batch = batch; L.st = wk.stream; L.scalars = rq.scalars; L.n = n;
    L.table28 = rq.pre ? rq.pre->table28 : rq.table28;
    L.rq.glv = rq.glv && (rq.pre ? rq.pre->glv && rq.pre->table28 : rq.table28 != nullptr);      // the split needs the interleaved table
    if (n >= ((size_t)1 << (L.rq.glv ? 30 : 31))) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: n >= 2^31");
    L.plan_from = plan_from && plan_from->glv == L.rq.glv ? plan_from : nullptr;      // a plan over split scalars serves only launches that split alike
    wk.glv = L.rq.glv;
    L.sort_mode = opt(ctx, "msm_sort", 0);
    L.tune = rq.tuning ? *rq.tuning : MsmTuning{opt(ctx, "msm_window_bits", 0), opt(ctx, "msm_split", 0), opt(ctx, "msm_dimbits", -1)};
    MsmGeom g; size_t n_eff = n;
    VSP_TRY(msm_geometry<F>(ctx, wk, L, g, n_eff));
    wk.g = g; wk.n_eff = n_eff;
    VSP_TRY(msm_split_scalars(ctx, wk, L, g));
    VSP_TRY(msm_buffers<F>(ctx, wk, L, g));
    if (L.plan_from) VSP_HIP(hipStreamWaitEvent(L.st, L.plan_from->plan_ready, 0));
    else { VSP_TRY(msm_digit_sort(ctx, wk, L, g)); VSP_TRY(msm_bucket_plan(ctx, wk, L, g)); }
    if (rq.plan_only) return VSP_OK;                        // the accumulation follows in a later launch over this slot's own plan
    VSP_TRY(msm_accumulate<F>(ctx, wk, L, g));
    VSP_HIP(hipEventRecord(wk.done, L.st));
    wk.active = true;
    return VSP_OK;
}

// A finish in two halves: msm_finish_wait (the wait for the slot's kernels, the census verdict, the statistics -- touches the context, so on
// the caller's thread) and msm_fold (the Horner chains over the window results in the slot's pinned buffer -- pure host arithmetic that reads
// only the slot, so the prover runs the folds of its five multi-exponentiations on host threads while it waits for the next slot).
// out: one result per vector of the batch the launch ran over (MsmGeom.K; one for an ordinary launch)
template <class F, class HF> static void msm_fold(const MsmWork &wk, XYZZ<HF> *out);
template <class F, class HF>
static int msm_finish_wait(vsp_ctx *ctx, MsmWork &wk, unsigned out_count, bool *empty);
template <class F, class HF>
static int msm_finish(vsp_ctx *ctx, MsmWork &wk, XYZZ<HF> *out, unsigned out_count = 1) {
    for (unsigned k = 0; k < out_count; k++) out[k] = XYZZ<HF>::inf();
    bool empty = false;
    VSP_TRY((msm_finish_wait<F, HF>(ctx, wk, out_count, &empty)));
    if (!empty) msm_fold<F, HF>(wk, out);
    return VSP_OK;
}
template <class F, class HF>
static int msm_finish_wait(vsp_ctx *ctx, MsmWork &wk, unsigned out_count, bool *empty) {
    static_assert(sizeof(F) == sizeof(HF), "host/device field layouts must match");
    *empty = true;
    if (!wk.active) return set_error(ctx, VSP_ERR_ARG, "msm: finish without launch");
    wk.active = false;
    if (wk.empty) return VSP_OK;
    *empty = false;
    if (wk.g.K != out_count) return set_error(ctx, VSP_ERR_ARG, "msm: finish asks for another number of results than the launch's batch");
    VSP_HIP(hipEventSynchronize(wk.done));
    const MsmGeom &g = wk.g;
#ifdef VSP_DEBUG_DUMP
    // experiment builds only (tools/dimsum_prefetch_probe.py): the bucket sums and the digit sums of the multi-exponentiation just finished,
    // generic 12 x 32-bit form ("msm_fp28" = 0), for an off-line comparison against big-integer sums
    if (const char *dir = getenv("VSP_DEBUG_DUMP_DIR")) {
        if (FILE *f = fopen((std::string(dir) + "/winres.bin").c_str(), "wb")) { fwrite(wk.h_pinned, 1, (size_t)g.Wr * (wk.dimbits ? DIMBITS_STRIDE : 4) * sizeof(XYZZ<HF>), f); fclose(f); }
        const unsigned per_w = dims_per_w(g);
        std::vector<char> hb(g.G * sizeof(XYZZ<F>)), hd((size_t)g.Wr * per_w * sizeof(XYZZ<F>));
        if (wk.buckets.p && wk.dims.p && hipMemcpy(hb.data(), wk.buckets.p, hb.size(), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(hd.data(), wk.dims.p, hd.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            std::string d(dir);
            if (FILE *f = fopen((d + "/buckets.bin").c_str(), "wb")) { fwrite(hb.data(), 1, hb.size(), f); fclose(f); }
            if (FILE *f = fopen((d + "/dims.bin").c_str(), "wb")) { fwrite(hd.data(), 1, hd.size(), f); fclose(f); }
            if (FILE *f = fopen((d + "/geom.txt").c_str(), "w")) { fprintf(f, "%u %u %u %u %u %u %u %zu\n", g.c, g.W, g.Wr, g.B, g.q0, g.q1, g.q2, sizeof(XYZZ<F>)); fclose(f); }
        }
    }
#endif
    if (wk.check_pending) {
        // the census of this launch (queued before the kernels `done` follows): remember the count for the next plan of this
        // length, refuse the result when a scalar was not canonical
        wk.check_pending = false;
        VSP_HIP(hipEventSynchronize(wk.census_done));
        const volatile uint32_t *hc = (const volatile uint32_t *)wk.h_census;
        if (wk.n >= 4096) { const uint32_t c0 = hc[0] / (wk.g.K ? wk.g.K : 1u); wk.neff_cache_n = wk.n; wk.neff_cache = c0 < 256 ? 256 : c0; }
        if (hc[2]) return set_error(ctx, VSP_ERR_ARG, "msm: a scalar is not canonical (>= r)");
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, wk.ev0, wk.ev1) == hipSuccess) {
        ctx->stats["msm_accum_ms"] += ms;
        ctx->stats["msm_accum_launches"] += 1;
    }
    ctx->stats["msm_calls"] += 1;
    ctx->stats["msm_n_eff"] = (double)wk.n_eff;
    ctx->stats["msm_window_bits"] = g.c;
    ctx->stats["msm_windows"] = g.W;
    ctx->stats["msm_bucket_sets"] = g.Wr;
    ctx->stats["msm_split"] = g.T;
    ctx->stats["msm_endomorphism_split"] = wk.glv ? 1 : 0;
    if (opt(ctx, "msm_debug_counts", 0) && wk.counters.p && wk.suboff.p) {      // diagnostic: the plan's counts (a blocking read-back), only when asked for
        uint32_t c4[4] = {0, 0, 0, 0}, parts = 0;
        if (hipMemcpy(c4, wk.counters.p, sizeof c4, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(&parts, (const uint32_t *)wk.suboff.p + g.G, 4, hipMemcpyDeviceToHost) == hipSuccess) {
            ctx->stats["msm_heavy_buckets"] = c4[0]; ctx->stats["msm_medium_buckets"] = c4[2]; ctx->stats["msm_parts"] = parts;
            ctx->stats["msm_buckets"] = (double)g.G;
        }
    }
    return VSP_OK;
}
template <class F, class HF> static void msm_fold(const MsmWork &wk, XYZZ<HF> *out) {
    const MsmGeom &g = wk.g;
    const XYZZ<HF> *wr = (const XYZZ<HF> *)wk.h_pinned;
    // Horner over bit positions: window w contributes D2 at c*w + q1 + q0, D1 at c*w + q0, D0 + Tot at c*w.  A batch: one chain per vector over
    // its own windows [k Wk, (k + 1) Wk) (one bucket set per window), or over its one bucket set in the shared-set mode
    const unsigned per = g.single ? 1u : (g.K > 1 ? g.Wk : g.Wr);      // window results per vector (shared-set mode: its one bucket set)
    const bool dimbits_layout = wk.dimbits;
    host_parallel_for(g.K, [&, per, dimbits_layout](size_t kb) {
        XYZZ<HF> acc = XYZZ<HF>::inf();
        const int w_lo = (int)(kb * per), w_hi = (int)(kb * per + per);
        if (dimbits_layout) {
            // k_dimbits layout: S_{d,j} enters at bit position (shift of digit d) + j of the window, Tot at position 0 -- one doubling per
            // position, c per window, exactly as below
            const unsigned q[3] = {g.q0, g.q1, g.q2};
            for (int w = w_hi - 1; w >= w_lo; w--) {
                const XYZZ<HF> *rec = wr + (size_t)w * DIMBITS_STRIDE;
                acc = xyzz_dbl(acc);                                    // position c - 1: bucket indices have c - 1 bits
                for (int d = 2; d >= 0; d--)
                    for (int j = (int)q[d] - 1; j >= 0; j--) { acc = xyzz_dbl(acc); xyzz_add(acc, rec[g.bd * d + j]); }
                xyzz_add(acc, rec[24]);
            }
        } else {
            for (int w = w_hi - 1; w >= w_lo; w--) {
                for (unsigned i = 0; i < g.q2 + 1; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 2]);
                for (unsigned i = 0; i < g.q1; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 1]);
                for (unsigned i = 0; i < g.q0; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 0]);
                xyzz_add(acc, wr[(size_t)w * 4 + 3]);
            }
        }
        out[kb] = acc;
    });
}

static MsmWork &slot(vsp_ctx *ctx, unsigned i) { return ctx->msm_work[i]; }

// A batch reuses the plan of ANOTHER slot only.  A single launch may name its own slot: that is how the accumulation follows a plan-only launch.
template <class F> static int launch_slot(vsp_ctx *ctx, unsigned slot_id, const MsmRequest &rq) {
    if (slot_id >= VSP_MSM_SLOTS || rq.plan_from >= (int)VSP_MSM_SLOTS || (rq.batch && rq.plan_from == (int)slot_id)) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    VSP_TRY(work_init(ctx, slot(ctx, slot_id), slot_id == 0 ? ctx->stream : nullptr));
    return msm_launch<F>(ctx, slot(ctx, slot_id), rq, rq.plan_from >= 0 ? &slot(ctx, (unsigned)rq.plan_from) : nullptr);
}

}  // anonymous namespace

// the entry points of common.h, defined once for both groups; msm_g1.hip / msm_g2.hip instantiate them for their group (VSP_MSM_GROUP)
// table[w][i] = 2^(c*w) * table[0][i] for w = 1..W-1 (slice 0 already holds the bases); affine, Montgomery
template <class G> int msm_precompute(vsp_ctx *ctx, typename G::Point *table, size_t n, unsigned c) {
    using F = typename G::F;
    const unsigned W = 255 / c + 1;
    hipStream_t st = ctx->stream;
    DevBuf tmp, pre;
    VSP_TRY(ensure_w(ctx, st, tmp, n * sizeof(XYZZ<F>)));
    int rc = ensure_w(ctx, st, pre, n * sizeof(F));
    if (rc == VSP_OK) {
        const unsigned blk = (unsigned)((n + MSM_THREADS - 1) / MSM_THREADS);
        const size_t chunks = (n + PRE_CHUNK - 1) / PRE_CHUNK;
        for (unsigned w = 1; w < W; w++) {
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_shift_window<F>), dim3(blk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, (const Affine<F> *)(table + (size_t)(w - 1) * n), n, c, (XYZZ<F> *)tmp.p);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_affine_mont<F>), dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, st, (const XYZZ<F> *)tmp.p, n, (F *)pre.p,
                               table + (size_t)w * n);
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "precompute: kernel failed");
    }
    if (tmp.p) hipFree(tmp.p);
    if (pre.p) hipFree(pre.p);
    return rc;
}

template <class G> int msm_table28(vsp_ctx *ctx, const typename G::Point *table, size_t count, void *d_out, bool glv) {
    if (!count) return VSP_OK;
#if defined(VSP_PORTABLE_MUL)
    return VSP_ERR_UNSUPPORTED;                              // the diagnostic build without hand-laid-out routines: generic kernels (no 28-bit table, no split)
#endif
    hipLaunchKernelGGL(k_table28, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, table, count, (Row28 *)d_out, glv);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
template <class G> int msm_slot_launch(vsp_ctx *ctx, unsigned slot_id, const MsmRequest &rq) { return launch_slot<typename G::F>(ctx, slot_id, rq); }
template <class G> int msm_slot_finish(vsp_ctx *ctx, unsigned slot_id, XYZZ<typename G::HF> *out, unsigned count) {
    return msm_finish<typename G::F, typename G::HF>(ctx, slot(ctx, slot_id), out, count);
}
template <class G> int msm_slot_finish_wait(vsp_ctx *ctx, unsigned slot_id, unsigned count, bool *empty) {
    return msm_finish_wait<typename G::F, typename G::HF>(ctx, slot(ctx, slot_id), count, empty);
}
template <class G> void msm_slot_fold(vsp_ctx *ctx, unsigned slot_id, XYZZ<typename G::HF> *out) { msm_fold<typename G::F, typename G::HF>(slot(ctx, slot_id), out); }
template <class G> int subgroup_check(vsp_ctx *ctx, const typename G::Point *d_mont, size_t n, uint32_t *d_flag) {
    using F = typename G::F;
    if (!n) return VSP_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_check<F>), dim3((unsigned)((LaneView<F>::LANES * n + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, ctx->stream,
                       d_mont, n, d_flag);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
template <class G> int bases_to_mont(vsp_ctx *ctx, const void *d_canon, typename G::Point *d_out, size_t n, int check_curve, uint32_t *d_flag) {
    using F = typename G::F;
    if (!n) return VSP_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bases_to_mont<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const Affine<F> *)d_canon, d_out, n, check_curve, d_flag);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the group-independent entry points: compiled once, with G1
#if VSP_MSM_GROUP == 1
// the census kernel runs on the CONTEXT's stream (so it cannot be held up behind low-priority work); the slot picks it up
// A stream for a work slot: the LOWEST priority -- work on the context's stream (the NTTs of witness_map, whose result gates the H
// multi-exponentiation) gets compute units first.  (Option "msm_slot_normal_priority" = 1: the context's own priority instead -- the
// open lead of DESIGN.md 3.3.)
int msm_make_slot_stream(vsp_ctx *ctx, hipStream_t *out) {
    int least = 0, greatest = 0;
    VSP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const long normal = opt(ctx, "msm_slot_normal_priority", 0);
    VSP_HIP(hipStreamCreateWithPriority(out, hipStreamNonBlocking, normal ? 0 : least));
    return VSP_OK;
}
int msm_slot_census(vsp_ctx *ctx, unsigned slot_id, const Fr *d_scalars, size_t n) {
    if (slot_id >= VSP_MSM_SLOTS) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    VSP_TRY(work_init(ctx, slot(ctx, slot_id), slot_id == 0 ? ctx->stream : nullptr));
    if (n == 0) return VSP_OK;
    return msm_census(ctx, slot(ctx, slot_id), d_scalars, n, ctx->stream);
}
int msm_slot_stream(vsp_ctx *ctx, unsigned slot_id, hipStream_t *out) {
    if (slot_id >= VSP_MSM_SLOTS) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    VSP_TRY(work_init(ctx, slot(ctx, slot_id), slot_id == 0 ? ctx->stream : nullptr));
    *out = slot(ctx, slot_id).stream;
    return VSP_OK;
}
// wait for every slot's stream and mark the slots idle (error paths: nothing may stay in flight over buffers about to be reused)
// queue the slot's next launches on `stream` (not owned by the slot), or on the slot's own stream again (nullptr).  Slots 1..: slot 0
// follows the context's stream.  Only between a finish and the next launch of that slot.
int msm_slot_use_stream(vsp_ctx *ctx, unsigned slot_id, hipStream_t stream_or_null) {
    if (slot_id == 0 || slot_id >= VSP_MSM_SLOTS) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    MsmWork &wk = slot(ctx, slot_id);
    wk.stream = stream_or_null;                             // nullptr: the next work_init puts the own stream back (creating it if need be)
    return stream_or_null ? work_init(ctx, wk, nullptr) : VSP_OK;
}
void msm_drain_slots(vsp_ctx *ctx) {
    for (unsigned i = 0; i < VSP_MSM_SLOTS; i++) {
        MsmWork &w = ctx->msm_work[i];
        if (!w.inited) continue;
        if (w.stream) hipStreamSynchronize(w.stream);
        w.active = false; w.check_pending = false; w.census_pending = false;
    }
    hipStreamSynchronize(ctx->stream);
    hipGetLastError();
}
void msm_free_slots(vsp_ctx *ctx) {
    for (unsigned i = 0; i < VSP_MSM_SLOTS; i++) {
        MsmWork &w = ctx->msm_work[i];
        DevBuf *bufs[] = {&w.cnt, &w.off, &w.cursor, &w.nsub, &w.suboff, &w.blocksum, &w.sorted, &w.heavy, &w.counters, &w.digits, &w.blockhist,
                          &w.partbucket, &w.perm, &w.sizehist, &w.buckets, &w.partials, &w.dims, &w.winres, &w.medium, &w.redo, &w.glv_scalars, &w.buckets28, &w.partials28, &w.tmp_sorted, &w.tmp_lo, &w.off_hi, &w.cnt_hi, &w.pairs_a, &w.pairs_b, &w.ms_h1, &w.ms_h1s, &w.ms_h2, &w.ms_h2s};
        for (DevBuf *b : bufs) { if (b->p) hipFree(b->p); b->p = nullptr; b->cap = 0; }
        if (w.inited) {
            hipEventDestroy(w.ev0); hipEventDestroy(w.ev1); hipEventDestroy(w.done); hipEventDestroy(w.plan_ready);
            hipHostFree(w.h_pinned); hipHostFree(w.h_census); hipEventDestroy(w.census_done);
            hipHostFree(w.h_rec); for (unsigned k = 0; k < MsmWork::REC_RING; k++) hipEventDestroy(w.rec_ev[k]);
            if (w.own_stream && w.own) hipStreamDestroy(w.own);
            w.own = nullptr; w.stream = nullptr; w.own_stream = false;
            w.inited = false;
        }
    }
}
// diagnostic build: clock held inside the G1 accumulation loop since the last reset (0: no data / production build)
int msm_diag_clock(vsp_ctx *ctx, int reset, double *ghz, double *waves) {
#ifdef VSP_DIAG_CLOCK
    unsigned long long h[4] = {0, 0, 0, 0};
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    VSP_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(vsp_diag_clock_sums), sizeof h));
    if (ghz) *ghz = h[1] ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
    if (waves) *waves = (double)h[2];
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; VSP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(vsp_diag_clock_sums), z, sizeof z)); }
    return VSP_OK;
#else
    (void)reset; if (ghz) *ghz = 0.0; if (waves) *waves = 0.0;
    return set_error(ctx, VSP_ERR_UNSUPPORTED, "diag_clock: this is not the diagnostic build (make diag -> libvsp_hip_diag.so)");
#endif
}
#endif

}  // namespace vsp
