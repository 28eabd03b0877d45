// The group-independent half of the multi-exponentiation pipeline (msm_impl.inc lists the whole of it, steps 0-7): the endomorphism
// split of the scalars, their signed digits, the four digit sorts, the scans and the bucket plan (steps 0-2).  These kernels see scalars,
// digits, 32-bit entries and counters, never a field element, so they are compiled here once and serve G1 and G2 alike: a slot that
// reuses another slot's digit sort (MsmRequest.plan_from: the prover's A, B1 and B2 queries) reads what these same kernels wrote.
// The library is built without relocatable device code -- a kernel is launched from the translation unit that defines it -- so the
// host stages that launch them live here too (prototypes: common.h; msm_launch<F> in msm_impl.inc calls them in order), and so do the
// work slots' stream and census functions, which exist once per library.
#include "common.h"

namespace vsp {
namespace {

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
// written by one kernel and read back by the next (128 MB per 2^20-point multi-exponentiation).
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

// blockhist[chunk][w][b] = number of digits of value b in (chunk, w); the block's (w, chunk) and the grid: lds_sort_map.h
__global__ __launch_bounds__(CS_THREADS) VSP_CS_ATTR void k_count_lds(const uint16_t *digits, MsmGeom g, unsigned nchunks, size_t chunk_len, uint32_t *blockhist, bool labelled) {
    extern __shared__ uint32_t lds_hist[];
    const LdsSortBlock blk = lds_sort_block(blockIdx.x, g.W, nchunks, labelled);
    if (!blk.valid) return;                                   // (the whole block: the labelled grid, rounded up for a W that is no multiple of 8)
    const unsigned w = blk.w, chunk = blk.chunk;
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

__device__ __forceinline__ void block_sum_to(uint32_t v, uint32_t *dst) {      // all MSM_THREADS threads of the block call it
    __shared__ uint32_t part[MSM_THREADS / 64];
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_down((int)v, d, 64);
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t t = 0; for (unsigned k = 0; k < MSM_THREADS / 64; k++) t += part[k]; *dst = t; }
}
// per bucket: cnt = sum over the `nsets` partial histograms (stride G apart); blockhist becomes their exclusive prefix.
// Separate bucket sets per window: nsets = chunks, G = W*B.  Single set: nsets = chunks*W, G = B.
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

// Places every entry of the block's (window, chunk) at its bucket's cursor, in `rounds` passes over the chunk: pass r handles exactly the
// entries whose bucket index lies in range r of `rounds` equal ranges (index >> range_shift == r, range_shift = log2(B / rounds)) and
// skips the rest.  The cursors are set up once; every entry is placed once, through the same cursor, so cnt, off and the set of
// entries of every bucket are those of a single pass -- only the order inside a bucket may differ, as it does from run to run anyway.
// Why: the kernel is bound by its scattered 4-byte stores.  In one pass the workgroups of a window spray their window's slice of
// `sorted` (8 MB at 2^21 entries) for the whole life of the kernel, twice the 4 MiB of the L2 they share (lds_sort_map.h), and a dirty
// line is evicted holding one or two valid dwords: WRITE_SIZE 627 MB per launch for 67 MB of entries.  A range whose slice stays
// resident is completed in L2 and leaves once: with the rounds put around the single-pass loop below, 16 of them brought WRITE_SIZE
// to 67 MB; the round loop as it stands, which keeps the workgroups less in step, to 303 MB (486 MB at 4 rounds).  But a round is a
// whole pass of ballots and shuffles over the chunk, about 25 us per 16.7 M digits -- it is bound by instruction issue, not by the
// non-temporal re-read of the digits and sign bytes -- so the host asks for few rounds or none (lds_sort_rounds): 4 at 2^20 points,
// where the kernel takes 196 us instead of 215 and the step with four in flight 2.74 ms instead of 2.84.  One round is the single
// pass as it always was, loop and loads.  No barrier between rounds: workgroups that start together stay roughly in step, which is
// all the locality needs.  Figures: profiles/scatter_rounds_*.txt, DESIGN.md 3.1.
__global__ __launch_bounds__(CS_THREADS) VSP_CS_ATTR void k_scatter_lds(const uint16_t *digits, const uint8_t *flips, MsmGeom g, unsigned nchunks, size_t chunk_len,
                                                            const uint32_t *blockhist, const uint32_t *off, uint32_t *sorted,
                                                            const uint8_t *lo_in, uint8_t *lo_out,      // wide windows: the low-bits byte travels with the entry
                                                            unsigned rounds, unsigned range_shift, bool labelled) {
    extern __shared__ uint32_t lds_cur[];
    const LdsSortBlock blk = lds_sort_block(blockIdx.x, g.W, nchunks, labelled);      // the histogram this block reads is the one the same block of k_count_lds wrote
    if (!blk.valid) return;
    const unsigned w = blk.w, chunk = blk.chunk;
    const size_t gbase = g.single ? (size_t)(w / g.Wk) * g.B : (size_t)w * g.B;
    const uint32_t *pre = blockhist + ((size_t)chunk * g.W + w) * g.B;
    VSP_CS_UNROLL
    for (unsigned b = threadIdx.x; b < g.B; b += CS_THREADS) lds_cur[b] = off[gbase + b] + pre[b];
    __syncthreads();
    const size_t i0 = (size_t)chunk * chunk_len, i1 = i0 + chunk_len < g.n ? i0 + chunk_len : g.n;
    const uint16_t *dw = digits + (size_t)w * g.n;
    const uint8_t *fw = flips ? flips + (size_t)(w / g.Wk) * g.n : nullptr;     // (one sign byte per scalar of every vector of a batch)
    const bool use_flips = !lo_in && (g.sbits == 128u || g.fold);
    const unsigned lane = threadIdx.x & 63u;
    const size_t step = (size_t)CS_MLP * CS_THREADS;
    if (rounds == 1) {
        // the single pass: CS_MLP digits (and their sign bytes) are requested before the first of them is used.  (Measured: k_count_lds
        // 40 -> 30 us; this kernel stays at 0.21 ms for 16.7 M entries -- it is bound by its 16.7 M scattered 4-byte writes.)
        for (size_t base = i0; base < i1; base += step) {
            uint16_t dd[CS_MLP]; uint8_t ff[CS_MLP];
#pragma unroll
            for (unsigned j = 0; j < CS_MLP; j++) {
                const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x;
                dd[j] = i < i1 ? dw[i] : DIGIT_NONE;
                ff[j] = (use_flips && i < i1) ? fw[i] : (uint8_t)0;
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
        return;
    }
    // rounds: the streams are read again and again, non-temporally, so that they do not push the dirty lines of `sorted` out of L2
    // CS_MLP digits (and their sign bytes) per thread and batch
    auto load_batch = [&](size_t base, uint16_t (&dd)[CS_MLP], uint8_t (&ff)[CS_MLP]) {
#pragma unroll
        for (unsigned j = 0; j < CS_MLP; j++) {
            const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x;
            dd[j] = i < i1 ? __builtin_nontemporal_load(&dw[i]) : DIGIT_NONE;
            ff[j] = (use_flips && i < i1) ? __builtin_nontemporal_load(&fw[i]) : (uint8_t)0;
        }
    };
#pragma unroll 1
    for (unsigned round = 0; round < rounds; round++) {
        // The next batch is requested before this one is worked on, and the LDS atomics of the whole batch are issued before the first
        // of their results is used (the build runs without the machine scheduler: the order below is the order of issue).  Measured
        // against rounds around the single-pass loop, 8 MiB of `sorted` per label: 4 rounds 188 -> 173 us; a pass by itself got no
        // cheaper (26 us), so it is issue that bounds it, not these latencies (profiles/scatter_rounds_sweep.txt, A against B)
        uint16_t dn[CS_MLP]; uint8_t fn[CS_MLP];
        load_batch(i0, dn, fn);
        for (size_t base = i0; base < i1; base += step) {
            uint16_t dd[CS_MLP]; uint8_t ff[CS_MLP];
#pragma unroll
            for (unsigned j = 0; j < CS_MLP; j++) { dd[j] = dn[j]; ff[j] = fn[j]; }
            if (base + step < i1) load_batch(base + step, dn, fn);
            // first half: the atomics.  grp: the lanes that share the first valid lane's bucket lkey (as in k_count_lds, they take their
            // positions from ONE atomic, their leader's); got: what the lane's own atomic returned (the leader's, or a lane's outside grp)
            unsigned long long grp[CS_MLP]; uint32_t lkey[CS_MLP], got[CS_MLP];
#pragma unroll
            for (unsigned j = 0; j < CS_MLP; j++) {
                const uint16_t d = dd[j];
                const uint32_t key = d & 0x7FFFu;             // (the sign bit is no part of the bucket index; DIGIT_NONE is tested on the whole digit)
                const bool valid = d != DIGIT_NONE && (key >> range_shift) == round;
                const unsigned long long act = __ballot(valid);
                grp[j] = 0; lkey[j] = 0; got[j] = 0;
                if (act) {
                    const int lead = __ffsll((long long)act) - 1;
                    lkey[j] = (uint32_t)__shfl((int)key, lead, 64);
                    const bool same = valid && key == lkey[j];
                    grp[j] = __ballot(same);
                    if (same && (int)lane == lead) got[j] = atomicAdd(&lds_cur[key], (uint32_t)__popcll(grp[j]));
                    if (valid && !same) got[j] = atomicAdd(&lds_cur[key], 1u);
                }
            }
            // second half: the positions and the stores
#pragma unroll
            for (unsigned j = 0; j < CS_MLP; j++) {
                if (grp[j]) {                                 // (a wave with a valid lane has a leader's group, and the leader is its first lane)
                    const size_t i = base + (size_t)j * CS_THREADS + threadIdx.x;
                    const uint16_t d = dd[j];
                    const uint32_t key = d & 0x7FFFu;
                    const bool valid = d != DIGIT_NONE && (key >> range_shift) == round;
                    const bool same = valid && key == lkey[j];
                    const uint32_t from_lead = (uint32_t)__shfl((int)got[j], __ffsll((long long)grp[j]) - 1, 64);      // (every lane takes part)
                    const uint32_t pos = same ? from_lead + (uint32_t)__popcll(grp[j] & ((1ull << lane) - 1ull)) : got[j];
                    if (valid) {
                        uint32_t sign;
                        if (lo_in) { const uint8_t l = __builtin_nontemporal_load(&lo_in[(size_t)w * g.n + i]); sign = l >> 7; lo_out[pos] = l & 0x7Fu; }
                        else sign = (uint32_t)(d >> 15) ^ (uint32_t)ff[j];
                        sorted[pos] = entry_of(g, w, i) | (sign << 31);
                    }
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
// The two scans on every launch's path (bucket counts -> offsets, parts per bucket -> part offsets) take their tile sums from the kernel
// that PRODUCES their input (k_chunk_prefix, k_plan: 256 values per workgroup, block_sum_to) and finish in ONE kernel: every workgroup
// adds up the tile sums before its own (at most a few thousand values) and scans its 256 inputs -- two launches instead of six.
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

}  // anonymous namespace

// ------------------------------------------------------------------------------------------------
// Host side: the stages of msm_launch (msm_impl.inc) that launch the kernels above, declared in common.h, and the work slots.
static int exclusive_scan_w(vsp_ctx *ctx, MsmWork &wk, const uint32_t *in, size_t n, uint32_t *out, uint32_t *out2) {
    size_t nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    VSP_TRY(ensure(ctx, wk.blocksum, (nb + 1) * sizeof(uint32_t), wk.stream));
    uint32_t *bs = (uint32_t *)wk.blocksum.p;
    hipLaunchKernelGGL(k_scan_reduce, dim3((unsigned)nb), dim3(MSM_THREADS), 0, wk.stream, in, n, bs);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(MSM_THREADS), 0, wk.stream, bs, nb);
    hipLaunchKernelGGL(k_scan_final, dim3((unsigned)nb), dim3(MSM_THREADS), 0, wk.stream, in, n, (const uint32_t *)bs, out, out2);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

int work_init(vsp_ctx *ctx, MsmWork &wk, hipStream_t stream_or_null) {
    if (!wk.inited) {
        VSP_HIP(hipEventCreate(&wk.ev0)); VSP_HIP(hipEventCreate(&wk.ev1));
        VSP_HIP(hipEventCreateWithFlags(&wk.done, hipEventDisableTiming));
        VSP_HIP(hipEventCreateWithFlags(&wk.plan_ready, hipEventDisableTiming));
        VSP_HIP(wk.h_pinned.alloc(MsmWork::PINNED_BYTES)); VSP_HIP(wk.h_census.alloc(64)); VSP_HIP(wk.h_rec.alloc(MsmWork::REC_RING * 288));
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
int msm_census(vsp_ctx *ctx, MsmWork &wk, const Fr *d_scalars, size_t n, hipStream_t on_stream, unsigned batch, size_t batch_stride) {
    hipStream_t st = on_stream ? on_stream : wk.stream;
    VSP_TRY(ensure(ctx, wk.counters, 64, st));
    VSP_HIP(hipMemsetAsync(wk.counters.p, 0, 64, st));
    { unsigned cb = (unsigned)((n + 255) / 256); if (cb > 1024) cb = 1024;
      hipLaunchKernelGGL(k_classify, dim3(cb, batch), dim3(256), 0, st, d_scalars, n, (uint32_t *)wk.counters.p, batch_stride); }
    VSP_HIP(hipMemcpyAsync(wk.h_census.p, (uint32_t *)wk.counters.p + 1, 12, hipMemcpyDeviceToHost, st));      // [0] count, [2] non-canonical flag
    VSP_HIP(hipEventRecord(wk.census_done, st));
    wk.census_pending = true; wk.census_n = n; wk.census_scalars = (const void *)d_scalars;
    return VSP_OK;
}

// the endomorphism split k = k1 + k2 lambda: a kernel of its own, or inside the digit kernel where the LDS counting sort follows (k_glv_digits)
int msm_split_scalars(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
    const size_t n = L.rq.n;
    L.fused_split = L.rq.glv && !L.plan_from && g.c <= 16 && ((opt(ctx, "msm_fused_split", 1) && 2 * n >= ((size_t)1 << 15) && L.sort_mode != 2) || g.K > 1);
    if (!L.rq.glv) return VSP_OK;
    if (!L.plan_from && !L.fused_split) {
        VSP_TRY(ensure(ctx, wk.glv_scalars, 2 * n * sizeof(Fr), L.st));
        hipLaunchKernelGGL(k_glv_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, L.st, L.rq.scalars, n, (Fr *)wk.glv_scalars.p);
        VSP_LAUNCH_CHECK();
        ctx->stats["msm_glv_split_launches"] += 1;
        L.scalars = (const Fr *)wk.glv_scalars.p;
    }
    L.n = 2 * n;                                            // from here on: 2n points (P_i, phi(P_i)), 2n scalars (k1_i, k2_i)
    return VSP_OK;
}

// the LDS counting sort's two kernels take up to 128 KiB of LDS: allowed once per context (= per device)
static int lds_sort_attrs(vsp_ctx *ctx) {
    if (ctx->lds_attr_set) return VSP_OK;
    VSP_HIP(hipFuncSetAttribute((const void *)k_count_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    VSP_HIP(hipFuncSetAttribute((const void *)k_scatter_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    ctx->lds_attr_set = true;
    return VSP_OK;
}
// chunks per window of the LDS counting sort: about 256 workgroups over all windows, none with fewer than 8192 scalars
static unsigned lds_chunks(const MsmGeom &g, size_t n) {
    unsigned nchunks = 256 / g.W; if (nchunks < 1) nchunks = 1;
    while (nchunks > 1 && n / nchunks < 8192) nchunks >>= 1;
    return nchunks;
}
// rounds of k_scatter_lds over bucket ranges (lds_sort_map.h; option "msm_scatter_rounds": 0 = by the size of the slices, n = n rounds,
// 1 = a single pass) and the shift that takes a bucket index to its range; g: the geometry the kernel is launched with
// `automatic`: whether the rule may take rounds by itself (the sort of windows up to 16 bits, which the sweep covered; the two-pass sort of
// wider windows runs in rounds only where the option asks for them).  labelled: which block mapping both kernels use (lds_sort_map.h):
// the labelled one only where rounds run -- for the rule's own choices, multiples of 8, it is the even mapping anyway
static void lds_scatter_rounds(vsp_ctx *ctx, const MsmGeom &g, size_t n, bool automatic, unsigned &rounds, unsigned &range_shift, bool &labelled) {
    const long forced = opt(ctx, "msm_scatter_rounds", 0);
    rounds = forced > 0 || automatic ? lds_sort_rounds(g.W, g.Wk, g.K, g.single != 0, g.B, n, forced) : 1u;
    labelled = rounds > 1;
    range_shift = (unsigned)(__builtin_ctz(g.B) - __builtin_ctz(rounds));
    ctx->stats["msm_scatter_rounds"] = rounds;
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
    VSP_TRY(ensure(ctx, wk.pairs_a, M * sizeof(uint2), st));
    VSP_TRY(ensure(ctx, wk.pairs_b, M * sizeof(uint2), st));
    VSP_TRY(ensure(ctx, wk.ms_h1, (H1 + 1) * 4, st)); VSP_TRY(ensure(ctx, wk.ms_h1s, (H1 + 1) * 4, st));
    const size_t P3 = (M + MS_CHUNK - 1) / MS_CHUNK + M / MS_SEG_LONG + 1;      // pieces of the third: only segments longer than MS_SEG_LONG have any
    // ms_h2: the second pass's piece histograms | the third's | piece counts | pbase2 | pbase3
    VSP_TRY(ensure(ctx, wk.ms_h2, (P2 * 256 + P3 * 64 + (H2 + 1) + (S1 + 1) + (H2 + 1)) * 4, st)); VSP_TRY(ensure(ctx, wk.ms_h2s, (H2 + 1) * 4, st));
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
    VSP_TRY(ensure(ctx, wk.digits, (size_t)g.W * n * 3, st));
    VSP_TRY(ensure(ctx, wk.blockhist, (size_t)nchunks * g.W * gh.B * sizeof(uint32_t), st));
    VSP_TRY(ensure(ctx, wk.cnt_hi, (gh.G + 1) * 4, st));
    VSP_TRY(ensure(ctx, wk.off_hi, (gh.G + 1) * 4, st));
    VSP_TRY(ensure(ctx, wk.tmp_sorted, L.M * 4, st));
    VSP_TRY(ensure(ctx, wk.tmp_lo, L.M, st));
    uint16_t *hi = (uint16_t *)wk.digits.p; uint8_t *lo = (uint8_t *)(hi + (size_t)g.W * n);
    uint32_t *blockhist = (uint32_t *)wk.blockhist.p, *cnt_hi = (uint32_t *)wk.cnt_hi.p, *off_hi = (uint32_t *)wk.off_hi.p;
    const size_t lds_bytes = (size_t)gh.B * sizeof(uint32_t);
    VSP_TRY(lds_sort_attrs(ctx));
    hipLaunchKernelGGL(k_digits_wide, dim3(L.nblk), dim3(MSM_THREADS), 0, st, L.scalars, g, hi, lo);
    unsigned rounds, range_shift; bool labelled;
    lds_scatter_rounds(ctx, gh, n, false, rounds, range_shift, labelled);
    const unsigned grid = lds_sort_grid(g.W, nchunks, labelled);
    hipLaunchKernelGGL(k_count_lds, dim3(grid), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)hi, gh, nchunks, chunk_len, blockhist, labelled);
    hipLaunchKernelGGL(k_chunk_prefix, dim3((unsigned)((gh.G + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st, blockhist, g.single ? nchunks * g.W : nchunks, gh.G, cnt_hi, (uint32_t *)nullptr, gh.G);
    VSP_LAUNCH_CHECK();
    VSP_TRY(exclusive_scan_w(ctx, wk, cnt_hi, gh.G, off_hi, nullptr));
    hipLaunchKernelGGL(k_scatter_lds, dim3(grid), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)hi, (const uint8_t *)nullptr, gh, nchunks, chunk_len,
                       (const uint32_t *)blockhist, (const uint32_t *)off_hi, (uint32_t *)wk.tmp_sorted.p, (const uint8_t *)lo, (uint8_t *)wk.tmp_lo.p, rounds, range_shift, labelled);
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
    VSP_TRY(ensure(ctx, wk.digits, (size_t)g.W * n * sizeof(uint16_t) + (size_t)g.K * n, st));      // + one sign byte per scalar (endomorphism split), per vector of a batch
    VSP_TRY(ensure(ctx, wk.blockhist, (size_t)nchunks * g.W * g.B * sizeof(uint32_t), st));
    uint16_t *digits = (uint16_t *)wk.digits.p; uint32_t *blockhist = (uint32_t *)wk.blockhist.p;
    uint8_t *flips = (uint8_t *)(digits + (size_t)g.W * n);
    const size_t lds_bytes = (size_t)g.B * sizeof(uint32_t);
    VSP_TRY(lds_sort_attrs(ctx));
    if (L.fused_split) hipLaunchKernelGGL(k_glv_digits, dim3((unsigned)((L.rq.n + MSM_THREADS - 1) / MSM_THREADS), g.K), dim3(MSM_THREADS), 0, st, L.rq.scalars, L.rq.n, g, digits, flips);
    else hipLaunchKernelGGL(k_digits, dim3(L.nblk, g.K), dim3(MSM_THREADS), 0, st, L.scalars, g, digits, flips);
    unsigned rounds, range_shift; bool labelled;
    lds_scatter_rounds(ctx, g, n, true, rounds, range_shift, labelled);
    const unsigned grid = lds_sort_grid(g.W, nchunks, labelled);
    hipLaunchKernelGGL(k_count_lds, dim3(grid), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)digits, g, nchunks, chunk_len, blockhist, labelled);
    VSP_TRY(ensure(ctx, wk.blocksum, ((size_t)L.gblk + 2) * sizeof(uint32_t), st));      // (the three-kernel scan shares this buffer and may have regrown it)
    uint32_t *tilesum = (uint32_t *)wk.blocksum.p;
    hipLaunchKernelGGL(k_chunk_prefix, dim3(L.gblk), dim3(MSM_THREADS), 0, st, blockhist, batch_single ? g.Wk : (g.single ? nchunks * g.W : nchunks), g.G, cnt,
                       L.fused_scans ? tilesum : (uint32_t *)nullptr, batch_single ? (size_t)g.B : g.G);
    VSP_LAUNCH_CHECK();
    if (L.fused_scans) hipLaunchKernelGGL(k_scan_tiles256, dim3(L.gblk), dim3(MSM_THREADS), 0, st, (const uint32_t *)cnt, g.G, (const uint32_t *)tilesum, off, (uint32_t *)nullptr);
    else { VSP_TRY(exclusive_scan_w(ctx, wk, cnt, g.G, off, nullptr)); ctx->stats["msm_scan3_launches"] += 1; }
    hipLaunchKernelGGL(k_scatter_lds, dim3(grid), dim3(CS_THREADS), lds_bytes, st, (const uint16_t *)digits, (const uint8_t *)flips, g, nchunks, chunk_len,
                       (const uint32_t *)blockhist, (const uint32_t *)off, (uint32_t *)wk.sorted.p, (const uint8_t *)nullptr, (uint8_t *)nullptr, rounds, range_shift, labelled);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the digit sort: the entries of every bucket together (cnt, off, sorted), by one of four sorts
int msm_digit_sort(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
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
int msm_bucket_plan(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st;
    const uint32_t *cnt = (const uint32_t *)wk.cnt.p;
    uint32_t *nsub = (uint32_t *)wk.nsub.p, *suboff = (uint32_t *)wk.suboff.p;
    VSP_TRY(ensure(ctx, wk.blocksum, ((size_t)L.gblk + 2) * sizeof(uint32_t), st));
    uint32_t *tilesum = (uint32_t *)wk.blocksum.p;
    uint32_t *size_hist = (uint32_t *)wk.sizehist.p, *bin_cursor = size_hist + SZ_BINS;
    uint32_t *redo0 = nullptr;                              // the accumulation's hand-back counter, cleared by k_plan when this launch goes on to accumulate over its own plan
    if (!L.rq.plan_only && L.table28) { VSP_TRY(ensure(ctx, wk.redo, (L.Smax + 1) * sizeof(uint32_t), st)); redo0 = (uint32_t *)wk.redo.p; }
    hipLaunchKernelGGL(k_plan, dim3(L.gblk), dim3(MSM_THREADS), 0, st, cnt, g.G, g.T, nsub, (uint32_t *)wk.heavy.p, (uint32_t *)wk.medium.p, (uint32_t *)wk.counters.p,
                       L.fused_scans ? tilesum : (uint32_t *)nullptr, size_hist, 2u * SZ_BINS, redo0);
    VSP_LAUNCH_CHECK();
    if (L.fused_scans) hipLaunchKernelGGL(k_scan_tiles256, dim3(L.gblk), dim3(MSM_THREADS), 0, st, (const uint32_t *)nsub, g.G, (const uint32_t *)tilesum, suboff, (uint32_t *)nullptr);
    else { VSP_TRY(exclusive_scan_w(ctx, wk, nsub, g.G, suboff, nullptr)); ctx->stats["msm_scan3_launches"] += 1; }
    uint32_t *part_bucket = (uint32_t *)wk.partbucket.p, *perm = (uint32_t *)wk.perm.p;
    hipLaunchKernelGGL(k_partinfo, dim3(L.ablk), dim3(256), 0, st, cnt, (const uint32_t *)suboff, g.G, g.T, part_bucket, size_hist);
    hipLaunchKernelGGL(k_binscan, dim3(1), dim3(SZ_BINS), 0, st, (const uint32_t *)size_hist, bin_cursor);
    hipLaunchKernelGGL(k_partsort, dim3(L.ablk), dim3(256), 0, st, cnt, (const uint32_t *)suboff, (const uint32_t *)part_bucket, g.G, g.T, bin_cursor, perm);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipEventRecord(wk.plan_ready, st));
    return VSP_OK;
}

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
// queue the slot's next launches on `stream` (not owned by the slot), or on the slot's own stream again (nullptr).  Slots 1..: slot 0
// follows the context's stream.  Only between a finish and the next launch of that slot.
int msm_slot_use_stream(vsp_ctx *ctx, unsigned slot_id, hipStream_t stream_or_null) {
    if (slot_id == 0 || slot_id >= VSP_MSM_SLOTS) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    MsmWork &wk = slot(ctx, slot_id);
    wk.stream = stream_or_null;                             // nullptr: the next work_init puts the own stream back (creating it if need be)
    return stream_or_null ? work_init(ctx, wk, nullptr) : VSP_OK;
}
// wait for every slot's stream and mark the slots idle (error paths: nothing may stay in flight over buffers about to be reused)
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
// the events and the own stream of every slot (its memory goes with the context)
void msm_free_slots(vsp_ctx *ctx) {
    for (unsigned i = 0; i < VSP_MSM_SLOTS; i++) {
        MsmWork &w = ctx->msm_work[i];
        if (!w.inited) continue;
        hipEventDestroy(w.ev0); hipEventDestroy(w.ev1); hipEventDestroy(w.done); hipEventDestroy(w.plan_ready); hipEventDestroy(w.census_done);
        for (unsigned k = 0; k < MsmWork::REC_RING; k++) hipEventDestroy(w.rec_ev[k]);
        if (w.own_stream && w.own) hipStreamDestroy(w.own);
        w.own = nullptr; w.stream = nullptr; w.own_stream = false;
        w.inited = false;
    }
}

}  // namespace vsp
