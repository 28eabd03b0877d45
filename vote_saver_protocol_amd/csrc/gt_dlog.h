// Discrete logarithms of small exponents in GT, shared by the gfx950 decryption kernels (decrypt.hip, 32-bit limbs) and, through g++,
// by the CPU test build (tests/cpu_build/dlog_check.cpp, both limb types).
//
//     given  value, base  in GT (the cyclotomic subgroup of Fp12, order r)  find  m in [0, max_value]  with  base^m = value
//
// Baby-step / giant-step with B = 2^b baby steps: m = k B + j, j < B, k < K = ceil((max_value + 1) / B), and
//     base^m = value   <=>   value g^k = base^j,    g = conj(base^B) = base^(-B)     (conjugation inverts in the cyclotomic subgroup)
// TABLE.  The baby steps are kept as (fingerprint(base^j), j), sorted by fingerprint: two arrays, 8 + 4 bytes per entry, not the 576-byte
// elements.  The FINGERPRINT of x is the low fp_bits bits of the low 64 bits of its first coefficient (c0.c0.c0: limb 0 of the 64-bit
// type, limbs 0 and 1 of the 32-bit type) in MONTGOMERY form -- the form every value of the search is in, the table's and the walk's
// alike; both limb types hold the same Montgomery value (radix 2^384), so they give the same fingerprint.
// SEARCH.  A run of giant steps walks x = value g^k, looks the fingerprint of every x up by binary search and tries EVERY table entry
// with that fingerprint: the candidate m = k B + j is dropped when it exceeds max_value (the last giant step reaches up to K B - 1),
// and is CONFIRMED by computing base^m in full and comparing all twelve coefficients with value.  So there is no false positive
// whatever fp_bits is, and no false negative: the true (k, j) meets its own fingerprint.  base has prime order r > max_value, so at
// most one m exists.
// Field products: a giant step is one Fp12 product (54) and a binary search; a baby step the same without the search; a run starts
// with a power by square-and-multiply (cyclotomic squares, 18 each).
#pragma once
#include <algorithm>
#include <vector>
#include "pairing.h"

namespace vsp {

static constexpr unsigned DLOG_RUN_STEPS = 64;          // giant steps (and baby steps) of one run: what one lane of the kernels walks
static constexpr unsigned DLOG_BLOCK_LANES = 64;        // lanes of a block of the kernels: one wave
static constexpr uint64_t DLOG_LAUNCH_LANES = (uint64_t)1 << 16;  // lanes of one launch of the giant search, about: whole blocks per item, at least one
static constexpr unsigned DLOG_MAX_BABY_BITS = 20;
static constexpr uint64_t DLOG_MAX_GIANT_STEPS = (uint64_t)1 << 24;
static constexpr uint64_t DLOG_NONE = ~(uint64_t)0;     // no m in [0, max_value]

template <class F> VSP_HD uint64_t gt_fingerprint(const Fp12T<F> &x, unsigned fp_bits) {
    using L = typename F::L;
    uint64_t w = (uint64_t)x.c0.c0.c0.l[0];
    if constexpr (sizeof(L) == 4) w |= (uint64_t)x.c0.c0.c0.l[1] << 32;
    return fp_bits >= 64 ? w : (w & (((uint64_t)1 << fp_bits) - 1));
}

// a^e for a in the cyclotomic subgroup and e given as nwords little-endian 64-bit words; e = 0 gives one
template <class F> VSP_HD Fp12T<F> gt_pow(const Fp12T<F> &a, const uint64_t *e, int nwords) {
    int top = -1;
    for (int i = nwords * 64 - 1; i >= 0; i--) if ((e[i >> 6] >> (i & 63)) & 1) { top = i; break; }
    if (top < 0) return Fp12T<F>::one();
    Fp12T<F> r = a;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (int i = top - 1; i >= 0; i--) {
        r = cyclotomic_sqr(r);
        if ((e[i >> 6] >> (i & 63)) & 1) r = mul(r, a);
    }
    return r;
}
template <class F> VSP_HD Fp12T<F> gt_pow_u64(const Fp12T<F> &a, uint64_t e) { return gt_pow(a, &e, 1); }
// the giant stride g = base^(-B), B = 2^b
template <class F> VSP_HD Fp12T<F> dlog_giant_stride(const Fp12T<F> &base, unsigned b) { return conj(gt_pow_u64(base, (uint64_t)1 << b)); }

// b for max_value when the caller does not choose: ceil(log2(max_value + 1) / 2), kept within 1 .. DLOG_MAX_BABY_BITS
VSP_HD unsigned dlog_auto_baby_bits(uint64_t max_value) {
    unsigned bits = 0;                                    // ceil(log2(max_value + 1)): the bit length of max_value
    while (bits < 64 && (max_value >> bits)) bits++;
    const unsigned b = (bits + 1) / 2;
    return b < 1 ? 1 : (b > DLOG_MAX_BABY_BITS ? DLOG_MAX_BABY_BITS : b);
}
// K = ceil((max_value + 1) / 2^b) without the overflow of max_value + 1
VSP_HD uint64_t dlog_giant_steps(uint64_t max_value, unsigned b) { return (max_value >> b) + 1; }

// the first index in the sorted keys[0 .. B) whose key is not below `key` (B when there is none)
VSP_HD size_t dlog_lower_bound(const uint64_t *keys, size_t B, uint64_t key) {
    size_t lo = 0, hi = B;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// baby steps j0 .. j0 + steps - 1: keys_out[s] = fingerprint(base^(j0 + s)).  The start by square-and-multiply, then one product a step
template <class F> VSP_HD void dlog_baby_run(const Fp12T<F> &base, uint64_t j0, unsigned steps, unsigned fp_bits, uint64_t *keys_out) {
    Fp12T<F> x = gt_pow_u64(base, j0);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (unsigned s = 0; s < steps; s++) {
        keys_out[s] = gt_fingerprint(x, fp_bits);
        if (s + 1 < steps) x = mul(x, base);
    }
}

// giant steps k0 .. k0 + steps - 1 over the sorted table (keys, js) of 2^b entries: the m in [0, max_value] with base^m = value that
// this run reaches, or DLOG_NONE.  k0 + steps <= 2^24 and b <= 20: k 2^b + j stays below 2^45
template <class F> VSP_HD uint64_t dlog_giant_run(const Fp12T<F> &value, const Fp12T<F> &base, const Fp12T<F> &g, uint64_t k0, unsigned steps, const uint64_t *keys,
                                                  const uint32_t *js, unsigned b, unsigned fp_bits, uint64_t max_value) {
    const size_t B = (size_t)1 << b;
    Fp12T<F> x = mul(value, gt_pow_u64(g, k0));
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (unsigned s = 0; s < steps; s++) {
        const uint64_t key = gt_fingerprint(x, fp_bits);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (size_t at = dlog_lower_bound(keys, B, key); at < B && keys[at] == key; at++) {
            const uint64_t m = ((k0 + s) << b) + js[at];
            if (m > max_value) continue;
            if (eq(gt_pow_u64(base, m), value)) return m;
        }
        if (s + 1 < steps) x = mul(x, g);
    }
    return DLOG_NONE;
}

// lanes that every item gets in one launch of the giant search over `items` items whose whole range takes `runs` lanes each
VSP_HD uint64_t dlog_launch_lanes(uint64_t items, uint64_t runs) {
    uint64_t lanes = DLOG_LAUNCH_LANES / items / DLOG_BLOCK_LANES * DLOG_BLOCK_LANES;
    if (lanes < DLOG_BLOCK_LANES) lanes = DLOG_BLOCK_LANES;
    return lanes > runs ? runs : lanes;
}

// host: the table of one base in the order the search reads it.  keys[j] = fingerprint(base^j) on entry; sorted by key (ties by j) on
// return, js the exponents beside them
inline void dlog_sort_table(uint64_t *keys, uint32_t *js, size_t B) {
    std::vector<std::pair<uint64_t, uint32_t>> e(B);
    for (size_t j = 0; j < B; j++) e[j] = {keys[j], (uint32_t)j};
    std::sort(e.begin(), e.end());
    for (size_t j = 0; j < B; j++) { keys[j] = e[j].first; js[j] = e[j].second; }
}

}  // namespace vsp
