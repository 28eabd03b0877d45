// Jubjub and its Pedersen hash (pedersen.hip; include/vsp.h "the voter registry"): everything about the registry that is
// not a launch -- the curve constants, the group law in extended coordinates, the table entry and the mixed addition, the chunk
// encoding, the (segment, window) schedule of a message, the share of a hash's chunks that a lane adds up and the order in which a group
// of lanes folds its partial sums, the on-curve and prime-order tests, the blob bit order and the rt split.  Shared by the gfx950 kernels
// (Mont<FrP32>), by the host side of the same calls (Mont<FrP64>: the generators are validated on the host) and, through g++, by the
// CPU test build (tests/cpu_build/jubjub_check.cpp).
//
// THE CURVE.  -u^2 + v^2 = 1 + d u^2 v^2 over Fr (the scalar field of BLS12-381), d = -10240 / 10241; order 8 s, s prime.  -1 is a
// square in Fr and d is not, so the unified addition below has no exceptional inputs: equal operands double, opposite ones give the
// identity (0, 1), points of small order are added like any other.
//
// THE HASH.  A message of n >= 1 bits is padded with zero bits to whole chunks of 3; chunk c = (s0, s1, s2) encodes
// (1 - 2 s2)(1 + s0 + 2 s1), a value in +-1 .. +-4, and belongs to segment c / 63, window c % 63:
//     P = sum_c enc(c) 2^(4 (c % 63)) G_(c / 63)          digest = u(P), 255 bits
// The table holds, for every generator and window, the four multiples k 2^(4 j) G_i, k = 1 .. 4, as (v + u, v - u, 2 d u v): a chunk is
// ONE mixed addition, and the negative of an entry is the two sums swapped and the product's sign flipped.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "field.h"

namespace vsp {

static constexpr unsigned JJ_WINDOWS = 63, JJ_ENTRIES = 4, JJ_SEGMENT_BITS = 3 * JJ_WINDOWS, JJ_DIGEST_BITS = 255;
static constexpr unsigned JJ_GEN_ENTRIES = JJ_WINDOWS * JJ_ENTRIES;             // table entries of one generator: 252 x 96 bytes
static constexpr unsigned JJ_NODE_BITS = 2 * JJ_DIGEST_BITS, JJ_NODE_GENERATORS = 3;      // an inner node hashes 510 bits: 170 chunks, 3 segments
static constexpr unsigned JJ_MAX_DEPTH = 24;

// a field value from the four 64-bit words of its stored form (Montgomery, radix 2^256 for both limb widths: the same bytes)
template <class F> VSP_HD F jj_words(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    const uint64_t w[4] = {w0, w1, w2, w3};
    F r;
    if constexpr (sizeof(typename F::L) == 8) { for (int i = 0; i < 4; i++) r.l[i] = (typename F::L)w[i]; }
    else { for (int i = 0; i < 4; i++) { r.l[2 * i] = (typename F::L)w[i]; r.l[2 * i + 1] = (typename F::L)(w[i] >> 32); } }
    return r;
}
// d and 2 d in Montgomery form (d = 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1)
template <class F> VSP_HD F jj_d() { return jj_words<F>(0x2a522455b974f6b0ULL, 0xfc6cc9ef0d9acab3ULL, 0x7a08fb94c27628d1ULL, 0x57f8f6a8fe0e262eULL); }
template <class F> VSP_HD F jj_2d() { return jj_words<F>(0x54a448ac72e9ed5fULL, 0xa51befdb1b373967ULL, 0xc0d81f217b4a799eULL, 0x3c0445fed27ecf14ULL); }
// the prime s (252 bits), little-endian words
VSP_HD uint64_t jj_order_word(int i) {
    return i == 0 ? 0xd0970e5ed6f72cb7ULL : i == 1 ? 0xa6682093ccc81082ULL : i == 2 ? 0x06673b0101343b00ULL : 0x0e7db4ea6533afa9ULL;
}
static constexpr int JJ_ORDER_BITS = 252;

// ---- points: extended coordinates (X : Y : Z : T), u = X / Z, v = Y / Z, T = X Y / Z
template <class F> struct JjPoint {
    F X, Y, Z, T;
    VSP_HD static JjPoint identity() { JjPoint p; p.X = F::zero(); p.Y = F::one(); p.Z = F::one(); p.T = F::zero(); return p; }
};
template <class F> struct JjAffine { F u, v; };                     // Montgomery form
template <class F> struct JjEntry { F yp, ym, t2d; };              // v + u, v - u, 2 d u v

template <class F> VSP_HD JjPoint<F> jj_from_affine(const JjAffine<F> &a) { JjPoint<F> p; p.X = a.u; p.Y = a.v; p.Z = F::one(); p.T = mul(a.u, a.v); return p; }
template <class F> VSP_HD bool jj_is_identity(const JjPoint<F> &p) { return is_zero(p.X) && eq(p.Y, p.Z); }
template <class F> VSP_HD JjEntry<F> jj_entry(const JjAffine<F> &a) {
    JjEntry<F> e; e.yp = add(a.v, a.u); e.ym = sub(a.v, a.u); e.t2d = mul(jj_2d<F>(), mul(a.u, a.v)); return e;
}
// the unified addition (a = -1): 9 products
template <class F> VSP_HD JjPoint<F> jj_add(const JjPoint<F> &p, const JjPoint<F> &q) {
    const F A = mul(sub(p.Y, p.X), sub(q.Y, q.X)), B = mul(add(p.Y, p.X), add(q.Y, q.X));
    const F C = mul(mul(p.T, jj_2d<F>()), q.T), D = dbl(mul(p.Z, q.Z));
    const F E = sub(B, A), Fv = sub(D, C), G = add(D, C), H = add(B, A);
    JjPoint<F> r; r.X = mul(E, Fv); r.Y = mul(G, H); r.T = mul(E, H); r.Z = mul(Fv, G); return r;
}
// the doubling: 8 products
template <class F> VSP_HD JjPoint<F> jj_dbl(const JjPoint<F> &p) {
    const F A = sqr(p.X), B = sqr(p.Y), C = dbl(sqr(p.Z));
    const F E = sub(sub(sqr(add(p.X, p.Y)), A), B), G = sub(B, A), Fv = sub(G, C), H = neg(add(A, B));
    JjPoint<F> r; r.X = mul(E, Fv); r.Y = mul(G, H); r.T = mul(E, H); r.Z = mul(Fv, G); return r;
}
// the mixed addition with a table entry, or with its negative: 7 products; unified as the full one
template <class F> VSP_HD JjPoint<F> jj_madd(const JjPoint<F> &p, const JjEntry<F> &e, bool negative) {
    const F yp = negative ? e.ym : e.yp, ym = negative ? e.yp : e.ym, t = negative ? neg(e.t2d) : e.t2d;
    const F A = mul(sub(p.Y, p.X), ym), B = mul(add(p.Y, p.X), yp), C = mul(p.T, t), D = dbl(p.Z);
    const F E = sub(B, A), Fv = sub(D, C), G = add(D, C), H = add(B, A);
    JjPoint<F> r; r.X = mul(E, Fv); r.Y = mul(G, H); r.T = mul(E, H); r.Z = mul(Fv, G); return r;
}
// 1 / a = a^(r - 2); 0 -> 0.  255 steps
template <class F> VSP_HD F jj_inv(const F &a) {
    F acc = F::one(), base = a;
    for (int w = 0; w < 4; w++) {
        const uint64_t e = w == 0 ? 0xfffffffeffffffffULL : w == 1 ? 0x53bda402fffe5bfeULL : w == 2 ? 0x3339d80809a1d805ULL : 0x73eda753299d7d48ULL;
        const int bits = w == 3 ? 63 : 64;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
        for (int i = 0; i < bits; i++) {
            if ((e >> i) & 1) acc = mul(acc, base);
            base = sqr(base);
        }
    }
    return acc;
}
template <class F> VSP_HD JjAffine<F> jj_to_affine(const JjPoint<F> &p) { const F zi = jj_inv(p.Z); JjAffine<F> a; a.u = mul(p.X, zi); a.v = mul(p.Y, zi); return a; }
// the four entries k B, k = 1 .. 4, of a window whose base is B: one inversion for the four
template <class F> VSP_HD void jj_window_entries(const JjPoint<F> &B, JjEntry<F> out[JJ_ENTRIES]) {
    JjPoint<F> m[JJ_ENTRIES];
    m[0] = B; m[1] = jj_dbl(B); m[2] = jj_add(m[1], B); m[3] = jj_dbl(m[1]);
    const F z01 = mul(m[0].Z, m[1].Z), z23 = mul(m[2].Z, m[3].Z), all = jj_inv(mul(z01, z23));
    const F i01 = mul(all, z23), i23 = mul(all, z01);
    const F zi[JJ_ENTRIES] = {mul(i01, m[1].Z), mul(i01, m[0].Z), mul(i23, m[3].Z), mul(i23, m[2].Z)};
    for (unsigned k = 0; k < JJ_ENTRIES; k++) { JjAffine<F> a; a.u = mul(m[k].X, zi[k]); a.v = mul(m[k].Y, zi[k]); out[k] = jj_entry(a); }
}
// the base of window j of a generator: 2^(4 j) G, 4 j doublings
template <class F> VSP_HD JjPoint<F> jj_window_base(const JjAffine<F> &G, unsigned j) {
    JjPoint<F> B = jj_from_affine(G);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (unsigned i = 0; i < 4 * j; i++) B = jj_dbl(B);
    return B;
}

// ---- what a generator must be: canonical coordinates (the caller checks the words), on the curve, of order exactly s
template <class F> VSP_HD bool jj_on_curve(const JjAffine<F> &a) {
    const F uu = sqr(a.u), vv = sqr(a.v);
    return eq(sub(vv, uu), add(F::one(), mul(jj_d<F>(), mul(uu, vv))));
}
template <class F> VSP_HD JjPoint<F> jj_mul_order(const JjPoint<F> &p) {       // s P: 251 doublings, double-and-add from the top bit
    JjPoint<F> acc = JjPoint<F>::identity();
    for (int i = JJ_ORDER_BITS - 1; i >= 0; i--) {
        acc = jj_dbl(acc);
        if ((jj_order_word(i >> 6) >> (i & 63)) & 1) acc = jj_add(acc, p);
    }
    return acc;
}
template <class F> VSP_HD bool jj_prime_order(const JjAffine<F> &a) {
    const JjPoint<F> p = jj_from_affine(a);
    return !jj_is_identity(p) && jj_is_identity(jj_mul_order(p));
}

VSP_HD bool jj_below_r(const uint64_t w[4]) {
    for (int i = 3; i >= 0; i--) {
        const uint64_t m = i == 3 ? 0x73eda753299d7d48ULL : i == 2 ? 0x3339d80809a1d805ULL : i == 1 ? 0x53bda402fffe5bfeULL : 0xffffffff00000001ULL;
        if (w[i] < m) return true;
        if (w[i] > m) return false;
    }
    return false;
}
// the verdict on a generator given as canonical words u | v
enum { JJ_GEN_OK = 0, JJ_GEN_NOT_CANONICAL = 1, JJ_GEN_OFF_CURVE = 2, JJ_GEN_IDENTITY = 3, JJ_GEN_NOT_PRIME_ORDER = 4 };
template <class F> VSP_HD F jj_load_canonical(const uint64_t in[4]);
template <class F> VSP_HD int jj_generator_fault(const uint64_t pt[8], JjAffine<F> *out) {
    if (!jj_below_r(pt) || !jj_below_r(pt + 4)) return JJ_GEN_NOT_CANONICAL;
    JjAffine<F> a; a.u = jj_load_canonical<F>(pt); a.v = jj_load_canonical<F>(pt + 4);
    if (!jj_on_curve(a)) return JJ_GEN_OFF_CURVE;
    if (jj_is_identity(jj_from_affine(a))) return JJ_GEN_IDENTITY;
    if (!jj_prime_order(a)) return JJ_GEN_NOT_PRIME_ORDER;
    if (out) *out = a;
    return JJ_GEN_OK;
}

// ---- the message: nbits bits in 64-bit words, bit k at word k / 64, position k % 64; bits at or above nbits read as zero whatever the
// words hold.  gap = 1: two digests of 255 bits, each in four words (a node's children): message bit k >= 255 is stored one place on
struct JjMessage { const uint64_t *w; uint32_t nbits, gap; };
VSP_HD unsigned jj_message_bit(const JjMessage &m, uint32_t k) {
    if (k >= m.nbits) return 0;
    const uint32_t at = k + ((m.gap && k >= JJ_DIGEST_BITS) ? 1u : 0u);
    return (unsigned)(m.w[at >> 6] >> (at & 63)) & 1u;
}
VSP_HD uint32_t jj_chunks(uint32_t nbits) { return (nbits + 2) / 3; }
VSP_HD uint32_t jj_chunk_segment(uint32_t c) { return c / JJ_WINDOWS; }
VSP_HD uint32_t jj_chunk_window(uint32_t c) { return c % JJ_WINDOWS; }
VSP_HD size_t jj_max_bits(size_t generators) { return (size_t)JJ_SEGMENT_BITS * generators; }
// chunk (s0, s1, s2): magnitude 1 + s0 + 2 s1 in 1 .. 4, negative when s2
VSP_HD unsigned jj_chunk_magnitude(unsigned s0, unsigned s1) { return 1 + s0 + 2 * s1; }
VSP_HD size_t jj_table_index(uint32_t segment, uint32_t window, unsigned magnitude) { return ((size_t)segment * JJ_WINDOWS + window) * JJ_ENTRIES + magnitude - 1; }
// chunk c of a message: its table entry and sign
VSP_HD size_t jj_chunk_entry(const JjMessage &m, uint32_t c, bool *negative) {
    const unsigned s0 = jj_message_bit(m, 3 * c), s1 = jj_message_bit(m, 3 * c + 1), s2 = jj_message_bit(m, 3 * c + 2);
    *negative = s2 != 0;
    return jj_table_index(jj_chunk_segment(c), jj_chunk_window(c), jj_chunk_magnitude(s0, s1));
}

// ---- a hash is summed by a GROUP of `lanes` lanes (1, 4, 16 or 64): lane l adds the chunks l, l + lanes, l + 2 lanes ...
template <class F> VSP_HD JjPoint<F> jj_lane_sum(const JjEntry<F> *tab, const JjMessage &m, unsigned lane, unsigned lanes) {
    JjPoint<F> acc = JjPoint<F>::identity();
    const uint32_t chunks = jj_chunks(m.nbits);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t c = lane; c < chunks; c += lanes) {
        bool negative;
        const size_t at = jj_chunk_entry(m, c, &negative);
        acc = jj_madd(acc, tab[at], negative);
    }
    return acc;
}
// THE FOLD of a group's partial sums, in levels s = lanes / 2, lanes / 4 .. 1: at level s lane l in [s, 2 s) gives its sum away and lane
// l - s takes it (a unified addition: coinciding and opposite partial sums are added like any other); after level 1 lane 0 holds the hash
VSP_HD bool jj_fold_gives(unsigned lane, unsigned lanes, unsigned s) { return s < lanes && lane >= s && lane < 2 * s; }
VSP_HD bool jj_fold_takes(unsigned lane, unsigned lanes, unsigned s) { return s < lanes && lane < s; }
// which group size a launch of `count` hashes takes: a lane per hash once the hashes alone give every SIMD of the chip a wave (2^16
// lanes), wider groups for fewer -- but only as wide as keeps the launch near one wave a SIMD, because lane 0's inversion costs its
// whole wave 255 steps however many hashes the wave holds
VSP_HD unsigned jj_group_lanes(size_t count) { return count >= ((size_t)1 << 16) ? 1u : count >= ((size_t)1 << 13) ? 4u : count >= ((size_t)1 << 11) ? 16u : 64u; }
VSP_HD bool jj_lanes_valid(long lanes) { return lanes == 1 || lanes == 4 || lanes == 16 || lanes == 64; }

// the digest: canonical u, four words (bit 255 is zero: u < r < 2^255)
template <class F> VSP_HD void jj_store_canonical(uint64_t out[4], const F &mont) {
    const F c = from_mont(mont);
    if constexpr (sizeof(typename F::L) == 8) { for (int i = 0; i < 4; i++) out[i] = (uint64_t)c.l[i]; }
    else { for (int i = 0; i < 4; i++) out[i] = (uint64_t)c.l[2 * i] | ((uint64_t)c.l[2 * i + 1] << 32); }
}
template <class F> VSP_HD F jj_load_canonical(const uint64_t in[4]) {
    return to_mont(jj_words<F>(in[0], in[1], in[2], in[3]));
}

// ---- the tree: 2^(depth + 1) - 1 nodes of four words, leaves first, root last.  Level l (0 = the leaves) has 2^(depth - l) nodes
VSP_HD uint64_t jj_tree_nodes(unsigned depth) { return ((uint64_t)2 << depth) - 1; }
VSP_HD uint64_t jj_level_nodes(unsigned depth, unsigned level) { return (uint64_t)1 << (depth - level); }
VSP_HD uint64_t jj_level_first(unsigned depth, unsigned level) { return ((uint64_t)2 << depth) - ((uint64_t)2 << (depth - level)); }
// the sibling on level l of the path of leaf x
VSP_HD uint64_t jj_sibling(uint64_t x, unsigned level) { return (x >> level) ^ 1; }
// THE BLOB: 32 octets a node, digest bit b at octet b / 8, bit position 7 - b % 8.  On the words of a digest and on the octets of a blob
// read as little-endian words that is one map, its own inverse: the bits of every byte reversed
VSP_HD uint64_t jj_blob_word(uint64_t x) {
    x = ((x & 0x0f0f0f0f0f0f0f0fULL) << 4) | ((x >> 4) & 0x0f0f0f0f0f0f0f0fULL);
    x = ((x & 0x3333333333333333ULL) << 2) | ((x >> 2) & 0x3333333333333333ULL);
    x = ((x & 0x5555555555555555ULL) << 1) | ((x >> 1) & 0x5555555555555555ULL);
    return x;
}
// rt as the circuit's public inputs take it: the low 254 bits and the bit above them (two scalars of four words)
VSP_HD void jj_rt_split(const uint64_t digest[4], uint64_t out[8]) {
    out[0] = digest[0]; out[1] = digest[1]; out[2] = digest[2]; out[3] = digest[3] & 0x3fffffffffffffffULL;
    out[4] = (digest[3] >> 62) & 1; out[5] = 0; out[6] = 0; out[7] = 0;
}

}  // namespace vsp
