// The voting circuit (vote_circuit.hip; include/vsp.h "the voting circuit"): the statement of the election's proofs as
// data.  One description -- the variable index of every gadget, the row range of every gadget, the rows themselves and the value of every
// wire -- shared by the host builder of the three CSR matrices, by the gfx950 kernels that fill witnesses (Mont<FrP32>) and, through g++,
// by the CPU test build (tests/cpu_build/vote_circuit_check.cpp, Mont<FrP64>).  Everything is a pure function of the parameters
// (msg_size n, eid_bits, depth, hash_leaves) and of the hash's table; nothing is tabulated at run time.
//
// THE STATEMENT.  Public: m_1 .. m_n | eid_packed | sn_packed (2) | rt_packed (2).  Private: sk (255 bits), the eid bits, `depth` address
// bits, `depth` copath digests of 255 bits.
//   1. every m_i is 0 or 1 and they sum to 1
//   2. every private bit is 0 or 1; eid_packed, sn_packed and rt_packed pack the eid bits, the sn digest and the last digest of the path in
//      chunks of 254 bits (bit i of a block: scalar i / 254, weight 2^(i % 254))
//   3. pk = H(sk); leaf = H(pk) with hash_leaves, else pk
//   4. cur_0 = leaf; cur_(l + 1) = H(L | R), (L, R) = (cur_l, sib_l) when address bit l is 0, (sib_l, cur_l) otherwise; rt = cur_depth
//   5. sn = H(eid | sk)
// H is the hash of jubjub.h; its digest in the circuit is the 255 bits of the canonical u, held below r by a strict comparison.
//
// WIRES (index into a witness; the R1CS variable is the index + 1, variable 0 is the constant 1), in this order:
//   M n | EID_PACKED E = ceil(eid_bits / 254) | SN_PACKED 2 | RT_PACKED 2                                  -- the public inputs
//   EID_BITS | SK_BITS 255 | ADDRESS_BITS depth | COPATH_BITS 255 depth (level by level)                  -- the private bits
//   the digest bits, 255 a hash | the comparison's run wires, VC_RUNS a hash | the selected children, 510 a level (L then R)
//   the chunk wires of every hash: chunk 0 has (s01, x), every later chunk (s01, x, U, A, B, C, u3, v3)
// The hashes in order: PK, LEAF (with hash_leaves), NODE 0 .. depth - 1, SN.  SN_BITS and RT_BITS are the digest bits of SN and of the last
// hash of the path.  ROWS, in this order: the n + 1 rows of m | the E + 4 packings | a row per private bit | 510 rows a digest (255
// booleans, the packing against the hash's last u3, 254 rows of the comparison) | 510 rows a level (L, R) | the chunk rows, one per chunk
// wire in the same order.
//
// A CHUNK (s0, s1, s2) of segment i, window j, with the table's points P_k = k 2^(4 j) G_i = (u_k, v_k), k = 1 .. 4:
//   s01 = s0 s1                  the selected point is (ulc, vlc) = P_1 + s0 (P_2 - P_1) + s1 (P_3 - P_1) + s01 (P_4 - P_3 - P_2 + P_1),
//   (1 - 2 s2) ulc = x           linear in the wires coordinate by coordinate: a lookup into constants; the sign flips only u
// and the affine accumulator (x1, y1) takes (x2, y2) = (x, vlc) by the complete twisted Edwards addition (a = -1):
//   U = (x1 + y1)(x2 + y2), A = y2 x1, B = x2 y1, C = d A B, (1 + C) u3 = A + B, (1 - C) v3 = U - A - B
// The accumulator of chunk 1 is chunk 0's own point (x, vlc); no denominator vanishes for points of the curve.  8 rows a chunk, 2 for the first.
//
// THE COMPARISON of digest bits b_254 .. b_0 with r - 1: with q_0 = 254 > q_1 > ... the positions of the one bits of r - 1, run wire j is
// b_(q_0) b_(q_1) .. b_(q_(j + 1)).  The row of position p < 254: R(p) b_p = (the next run wire) where r - 1 has a one at p, and
// R(p) b_p = 0 where it has a zero, R(p) being the run over the ones above p.  A pattern above r - 1 has a first position where it is 1
// and r - 1 is 0 with every one of r - 1 above it present: that row fails.  Without it a digest u < 2^255 - r has the second pattern u + r.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "jubjub.h"

namespace vsp {

struct VcParams { uint32_t n, eid_bits, depth, hash_leaves; };

static constexpr uint32_t VC_PACK_BITS = 254, VC_NONE = 0xffffffffu;
static constexpr uint32_t VC_DIGEST_ROWS = 2 * JJ_DIGEST_BITS, VC_LEVEL_WIRES = 2 * JJ_DIGEST_BITS;
static constexpr uint32_t VC_KEY_CHUNKS = (JJ_DIGEST_BITS + 2) / 3, VC_NODE_CHUNKS = (JJ_NODE_BITS + 2) / 3;      // 85, 170
static constexpr uint32_t VC_CHUNK_WIRES = 8, VC_FIRST_CHUNK_WIRES = 2;
// the named blocks of vsp_vote_circuit_wires
enum { VC_M = 0, VC_EID_PACKED = 1, VC_SN_PACKED = 2, VC_RT_PACKED = 3, VC_EID_BITS = 4, VC_SK_BITS = 5, VC_ADDRESS_BITS = 6, VC_COPATH_BITS = 7,
       VC_SN_BITS = 8, VC_RT_BITS = 9, VC_BLOCKS = 10 };
// the chunk wires
enum { VC_W_S01 = 0, VC_W_X = 1, VC_W_U = 2, VC_W_A = 3, VC_W_B = 4, VC_W_C = 5, VC_W_U3 = 6, VC_W_V3 = 7 };

// ---- r - 1 and its one bits
VSP_HD uint64_t vc_rm1_word(int i) {
    return i == 0 ? 0xffffffff00000000ULL : i == 1 ? 0x53bda402fffe5bfeULL : i == 2 ? 0x3339d80809a1d805ULL : 0x73eda753299d7d48ULL;
}
constexpr unsigned vc_ones64(uint64_t x) { unsigned n = 0; for (int i = 0; i < 64; i++) n += (unsigned)((x >> i) & 1); return n; }
// run wires of one comparison: the one bits of r - 1 below bit 254
static constexpr uint32_t VC_RUNS = vc_ones64(0xffffffff00000000ULL) + vc_ones64(0x53bda402fffe5bfeULL) + vc_ones64(0x3339d80809a1d805ULL) + vc_ones64(0x73eda753299d7d48ULL) - 1;
VSP_HD unsigned vc_rm1_bit(unsigned p) { return (unsigned)(vc_rm1_word((int)(p >> 6)) >> (p & 63)) & 1u; }
// the words of r - 1 with the bits below position p cleared
VSP_HD uint64_t vc_rm1_from(unsigned p, int i) {
    const unsigned lo = 64u * (unsigned)i;
    if (p >= lo + 64) return 0;
    const uint64_t w = vc_rm1_word(i);
    return p <= lo ? w : w & (~(uint64_t)0 << (p - lo));
}
// how many one bits r - 1 has above position p (p <= 254): 0 for p = 254
VSP_HD unsigned vc_rm1_rank(unsigned p) {
    unsigned n = 0;
    for (int i = 0; i < 4; i++) n += (unsigned)__builtin_popcountll(vc_rm1_from(p + 1, i));
    return n;
}
// the position q_k of the k-th one bit of r - 1 from the top (q_0 = 254); k <= VC_RUNS.  At most 255 steps
VSP_HD unsigned vc_rm1_one(unsigned k) {
    unsigned seen = 0;
    for (unsigned p = JJ_DIGEST_BITS; p-- > 0;) {
        if (!vc_rm1_bit(p)) continue;
        if (seen == k) return p;
        seen++;
    }
    return 0;
}

// ---- the hashes
VSP_HD uint32_t vc_hashes(const VcParams &P) { return 2 + (P.hash_leaves ? 1u : 0u) + P.depth; }
VSP_HD uint32_t vc_hash_pk(const VcParams &) { return 0; }
VSP_HD uint32_t vc_hash_leaf(const VcParams &P) { return P.hash_leaves ? 1u : 0u; }                 // the hash whose digest is the leaf
VSP_HD uint32_t vc_hash_node(const VcParams &P, uint32_t l) { return 1 + (P.hash_leaves ? 1u : 0u) + l; }
VSP_HD uint32_t vc_hash_sn(const VcParams &P) { return vc_hash_node(P, P.depth); }
VSP_HD uint32_t vc_hash_cur(const VcParams &P, uint32_t l) { return l ? vc_hash_node(P, l - 1) : vc_hash_leaf(P); }      // the hash whose digest is cur_l
VSP_HD uint32_t vc_hash_top(const VcParams &P) { return vc_hash_cur(P, P.depth); }
VSP_HD uint32_t vc_sn_bits(const VcParams &P) { return P.eid_bits + JJ_DIGEST_BITS; }
VSP_HD uint32_t vc_hash_bits(const VcParams &P, uint32_t h) {
    return h == vc_hash_sn(P) ? vc_sn_bits(P) : h < vc_hash_node(P, 0) ? JJ_DIGEST_BITS : JJ_NODE_BITS;
}
VSP_HD uint32_t vc_hash_chunks(const VcParams &P, uint32_t h) { return jj_chunks(vc_hash_bits(P, h)); }
// the chunks of the hashes before h (h = vc_hashes: all of them)
VSP_HD uint32_t vc_chunks_before(const VcParams &P, uint32_t h) {
    const uint32_t keys = vc_hash_node(P, 0);
    uint32_t c = h <= keys ? VC_KEY_CHUNKS * h : VC_KEY_CHUNKS * keys + VC_NODE_CHUNKS * ((h < vc_hash_sn(P) ? h : vc_hash_sn(P)) - keys);
    if (h > vc_hash_sn(P)) c += jj_chunks(vc_sn_bits(P));
    return c;
}
VSP_HD uint32_t vc_total_chunks(const VcParams &P) { return vc_chunks_before(P, vc_hashes(P)); }

// ---- the wires
VSP_HD uint32_t vc_eid_scalars(const VcParams &P) { return (P.eid_bits + VC_PACK_BITS - 1) / VC_PACK_BITS; }
VSP_HD uint32_t vc_w_m(const VcParams &) { return 0; }
VSP_HD uint32_t vc_w_eid_packed(const VcParams &P) { return P.n; }
VSP_HD uint32_t vc_w_sn_packed(const VcParams &P) { return P.n + vc_eid_scalars(P); }
VSP_HD uint32_t vc_w_rt_packed(const VcParams &P) { return vc_w_sn_packed(P) + 2; }
VSP_HD uint32_t vc_num_inputs(const VcParams &P) { return vc_w_rt_packed(P) + 2; }
VSP_HD uint32_t vc_w_eid(const VcParams &P) { return vc_num_inputs(P); }
VSP_HD uint32_t vc_w_sk(const VcParams &P) { return vc_w_eid(P) + P.eid_bits; }
VSP_HD uint32_t vc_w_addr(const VcParams &P) { return vc_w_sk(P) + JJ_DIGEST_BITS; }
VSP_HD uint32_t vc_w_copath(const VcParams &P) { return vc_w_addr(P) + P.depth; }
VSP_HD uint32_t vc_w_digest(const VcParams &P) { return vc_w_copath(P) + JJ_DIGEST_BITS * P.depth; }
VSP_HD uint32_t vc_w_run(const VcParams &P) { return vc_w_digest(P) + JJ_DIGEST_BITS * vc_hashes(P); }
VSP_HD uint32_t vc_w_sel(const VcParams &P) { return vc_w_run(P) + VC_RUNS * vc_hashes(P); }
VSP_HD uint32_t vc_w_chunk(const VcParams &P) { return vc_w_sel(P) + VC_LEVEL_WIRES * P.depth; }
VSP_HD uint32_t vc_chunk_span(const VcParams &P) { return VC_CHUNK_WIRES * vc_total_chunks(P) - (VC_CHUNK_WIRES - VC_FIRST_CHUNK_WIRES) * vc_hashes(P); }
VSP_HD uint32_t vc_num_vars(const VcParams &P) { return vc_w_chunk(P) + vc_chunk_span(P); }
// chunk c of hash h: offset of its first wire (and of its first row) inside the chunk region
VSP_HD uint32_t vc_chunk_offset(const VcParams &P, uint32_t h, uint32_t c) {
    return VC_CHUNK_WIRES * vc_chunks_before(P, h) - (VC_CHUNK_WIRES - VC_FIRST_CHUNK_WIRES) * h + (c ? VC_CHUNK_WIRES * c - (VC_CHUNK_WIRES - VC_FIRST_CHUNK_WIRES) : 0);
}
VSP_HD uint32_t vc_w_chunk_wire(const VcParams &P, uint32_t h, uint32_t c, uint32_t which) { return vc_w_chunk(P) + vc_chunk_offset(P, h, c) + which; }
VSP_HD uint32_t vc_w_digest_bit(const VcParams &P, uint32_t h, uint32_t i) { return vc_w_digest(P) + JJ_DIGEST_BITS * h + i; }
VSP_HD uint32_t vc_w_run_wire(const VcParams &P, uint32_t h, uint32_t j) { return vc_w_run(P) + VC_RUNS * h + j; }
VSP_HD uint32_t vc_w_sel_bit(const VcParams &P, uint32_t l, uint32_t right, uint32_t i) { return vc_w_sel(P) + VC_LEVEL_WIRES * l + JJ_DIGEST_BITS * right + i; }
VSP_HD uint32_t vc_w_copath_bit(const VcParams &P, uint32_t l, uint32_t i) { return vc_w_copath(P) + JJ_DIGEST_BITS * l + i; }
// the wire that holds u of hash h (every hash has at least 85 chunks)
VSP_HD uint32_t vc_w_hash_u(const VcParams &P, uint32_t h) { return vc_w_chunk_wire(P, h, vc_hash_chunks(P, h) - 1, VC_W_U3); }
// the wire of bit k of hash h's message, VC_NONE for the padding
VSP_HD uint32_t vc_msg_wire(const VcParams &P, uint32_t h, uint32_t k) {
    if (k >= vc_hash_bits(P, h)) return VC_NONE;
    if (h == vc_hash_sn(P)) return k < P.eid_bits ? vc_w_eid(P) + k : vc_w_sk(P) + (k - P.eid_bits);
    if (h == 0) return vc_w_sk(P) + k;
    if (h < vc_hash_node(P, 0)) return vc_w_digest_bit(P, 0, k);
    const uint32_t l = h - vc_hash_node(P, 0);
    return k < JJ_DIGEST_BITS ? vc_w_sel_bit(P, l, 0, k) : vc_w_sel_bit(P, l, 1, k - JJ_DIGEST_BITS);
}
VSP_HD bool vc_block(const VcParams &P, int block, uint32_t *first, uint32_t *count) {
    switch (block) {
    case VC_M: *first = vc_w_m(P); *count = P.n; return true;
    case VC_EID_PACKED: *first = vc_w_eid_packed(P); *count = vc_eid_scalars(P); return true;
    case VC_SN_PACKED: *first = vc_w_sn_packed(P); *count = 2; return true;
    case VC_RT_PACKED: *first = vc_w_rt_packed(P); *count = 2; return true;
    case VC_EID_BITS: *first = vc_w_eid(P); *count = P.eid_bits; return true;
    case VC_SK_BITS: *first = vc_w_sk(P); *count = JJ_DIGEST_BITS; return true;
    case VC_ADDRESS_BITS: *first = vc_w_addr(P); *count = P.depth; return true;
    case VC_COPATH_BITS: *first = vc_w_copath(P); *count = JJ_DIGEST_BITS * P.depth; return true;
    case VC_SN_BITS: *first = vc_w_digest_bit(P, vc_hash_sn(P), 0); *count = JJ_DIGEST_BITS; return true;
    case VC_RT_BITS: *first = vc_w_digest_bit(P, vc_hash_top(P), 0); *count = JJ_DIGEST_BITS; return true;
    }
    return false;
}

// ---- the rows
VSP_HD uint32_t vc_r_m(const VcParams &) { return 0; }
VSP_HD uint32_t vc_r_pack(const VcParams &P) { return P.n + 1; }
VSP_HD uint32_t vc_r_bool(const VcParams &P) { return vc_r_pack(P) + vc_eid_scalars(P) + 4; }
VSP_HD uint32_t vc_r_digest(const VcParams &P) { return vc_r_bool(P) + (vc_w_digest(P) - vc_w_eid(P)); }
VSP_HD uint32_t vc_r_sel(const VcParams &P) { return vc_r_digest(P) + VC_DIGEST_ROWS * vc_hashes(P); }
VSP_HD uint32_t vc_r_chunk(const VcParams &P) { return vc_r_sel(P) + VC_LEVEL_WIRES * P.depth; }
VSP_HD uint32_t vc_num_constraints(const VcParams &P) { return vc_r_chunk(P) + vc_chunk_span(P); }
// what the parameters must satisfy (g: the hash's generators)
VSP_HD bool vc_params_valid(const VcParams &P, size_t g) {
    return P.n >= 1 && P.eid_bits >= 1 && g >= JJ_NODE_GENERATORS && P.depth <= JJ_MAX_DEPTH && (size_t)P.eid_bits + JJ_DIGEST_BITS <= jj_max_bits(g) &&
           P.n <= (1u << 20);
}

// ---- the values of a witness
// One stored step of a hash's chain.  While the chain runs: a, b, c = X, Y, Z of the prefix sum after this chunk and d = the product of
// every Z so far; after the shared inversion: a, b = the affine u, v of the prefix sum (Montgomery form)
template <class F> struct VcSlot { F a, b, c, d; };

// the chain of one hash: a mixed addition per chunk, every prefix sum kept; ONE inversion (Montgomery's trick over the stored products)
// makes them all affine.  Loops: chunks(m.nbits) forward, the 255 steps of the inversion, chunks backward.  digest: the canonical u
template <class F> VSP_HD void vc_chain(const JjEntry<F> *tab, const JjMessage &m, VcSlot<F> *slot, uint64_t digest[4]) {
    const uint32_t chunks = jj_chunks(m.nbits);
    JjPoint<F> acc = JjPoint<F>::identity();
    F run = F::one();
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t c = 0; c < chunks; c++) {
        bool negative;
        const size_t at = jj_chunk_entry(m, c, &negative);
        acc = jj_madd(acc, tab[at], negative);
        run = mul(run, acc.Z);
        slot[c].a = acc.X; slot[c].b = acc.Y; slot[c].c = acc.Z; slot[c].d = run;
    }
    F inv = jj_inv(run);
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t c = chunks; c-- > 0;) {
        const F zi = c ? mul(inv, slot[c - 1].d) : inv;
        inv = mul(inv, slot[c].c);
        slot[c].a = mul(slot[c].a, zi); slot[c].b = mul(slot[c].b, zi);
    }
    jj_store_canonical(digest, slot[chunks - 1].a);
}

// What the values of one ballot's wires are read from.  nodes: with `tree` the registry's tree (the path's digests are node(l, index >> l)
// and its siblings), else the copath alone, depth x 4 words.  digests: 4 words a hash, in the order of the hashes; slots: the chains' affine prefix
// sums, hash h chunk c at vc_chunks_before(h) + c.  (One base pointer and a flag on purpose: with a tree pointer and a copath pointer
// side by side, the pinned toolchain's SimplifyCFG pass crashed on the select between them while compiling k_vote_fill_wires.)
template <class F> struct VcBallot {
    const uint64_t *sk, *eid;
    uint64_t index;
    uint32_t vote;
    const uint64_t *nodes;
    bool tree;
    const uint64_t *digests;
    const VcSlot<F> *slots;
};
VSP_HD unsigned vc_word_bit(const uint64_t *w, uint32_t k) { return (unsigned)(w[k >> 6] >> (k & 63)) & 1u; }
template <class F> VSP_HD const uint64_t *vc_sibling(const VcParams &P, const VcBallot<F> &b, uint32_t l) {
    const uint64_t at = b.tree ? jj_level_first(P.depth, l) + jj_sibling(b.index, l) : l;
    return b.nodes + 4 * at;
}
template <class F> VSP_HD unsigned vc_cur_bit(const VcParams &P, const VcBallot<F> &b, uint32_t l, uint32_t i) { return vc_word_bit(b.digests + 4 * vc_hash_cur(P, l), i); }
template <class F> VSP_HD unsigned vc_sel_value(const VcParams &P, const VcBallot<F> &b, uint32_t l, uint32_t right, uint32_t i) {
    const unsigned a = (unsigned)(b.index >> l) & 1u;
    return a != right ? vc_word_bit(vc_sibling(P, b, l), i) : vc_cur_bit(P, b, l, i);
}
// bit k of hash h's message
template <class F> VSP_HD unsigned vc_msg_value(const VcParams &P, const VcBallot<F> &b, uint32_t h, uint32_t k) {
    if (k >= vc_hash_bits(P, h)) return 0;
    if (h == vc_hash_sn(P)) return k < P.eid_bits ? vc_word_bit(b.eid, k) : vc_word_bit(b.sk, k - P.eid_bits);
    if (h == 0) return vc_word_bit(b.sk, k);
    if (h < vc_hash_node(P, 0)) return vc_word_bit(b.digests, k);
    const uint32_t l = h - vc_hash_node(P, 0);
    return k < JJ_DIGEST_BITS ? vc_sel_value(P, b, l, 0, k) : vc_sel_value(P, b, l, 1, k - JJ_DIGEST_BITS);
}
// bits [start, start + len) of `nbits` bits of words, len <= 254, as a scalar
VSP_HD void vc_pack_value(const uint64_t *w, uint32_t nbits, uint32_t start, uint32_t len, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    for (uint32_t i = 0; i < len && start + i < nbits; i++) out[i >> 6] |= (uint64_t)vc_word_bit(w, start + i) << (i & 63);
}
VSP_HD void vc_store_small(uint64_t *o, uint64_t v) { o[0] = v; o[1] = 0; o[2] = 0; o[3] = 0; }
// the items of a fill: one per wire below the chunk region, then one per chunk
VSP_HD uint32_t vc_fill_items(const VcParams &P) { return vc_w_chunk(P) + vc_total_chunks(P); }
// the value of wire t below the chunk region: one if-chain, one result (a bit, or a packed scalar) that the caller stores.  Loops: at
// most 254 steps (a packing, a run wire's position)
template <class F> VSP_HD void vc_wire_value(const VcParams &P, const VcBallot<F> &b, uint32_t t, uint64_t val[4]) {
    val[0] = val[1] = val[2] = val[3] = 0;
    if (t < vc_w_eid_packed(P)) val[0] = t == b.vote ? 1 : 0;
    else if (t < vc_w_sn_packed(P)) vc_pack_value(b.eid, P.eid_bits, VC_PACK_BITS * (t - vc_w_eid_packed(P)), VC_PACK_BITS, val);
    else if (t < vc_num_inputs(P)) {
        const uint32_t j = t - vc_w_sn_packed(P);
        const uint64_t *d = b.digests + 4 * (j < 2 ? vc_hash_sn(P) : vc_hash_top(P));
        if (j & 1) val[0] = (d[3] >> 62) & 1;
        else { val[0] = d[0]; val[1] = d[1]; val[2] = d[2]; val[3] = d[3] & 0x3fffffffffffffffULL; }      // jj_rt_split's two scalars
    }
    else if (t < vc_w_sk(P)) val[0] = vc_word_bit(b.eid, t - vc_w_eid(P));
    else if (t < vc_w_addr(P)) val[0] = vc_word_bit(b.sk, t - vc_w_sk(P));
    else if (t < vc_w_copath(P)) val[0] = (b.index >> (t - vc_w_addr(P))) & 1;
    else if (t < vc_w_digest(P)) { const uint32_t k = t - vc_w_copath(P); val[0] = vc_word_bit(vc_sibling(P, b, k / JJ_DIGEST_BITS), k % JJ_DIGEST_BITS); }
    else if (t < vc_w_run(P)) { const uint32_t k = t - vc_w_digest(P); val[0] = vc_word_bit(b.digests, k + k / JJ_DIGEST_BITS); }      // 255 bits in four words
    else if (t < vc_w_sel(P)) {
        const uint32_t k = t - vc_w_run(P), h = k / VC_RUNS, q = vc_rm1_one(k % VC_RUNS + 1);
        const uint64_t *d = b.digests + 4 * h;
        uint64_t missing = 0;
        for (int i = 0; i < 4; i++) { const uint64_t need = vc_rm1_from(q, i); missing |= (d[i] & need) ^ need; }
        val[0] = missing ? 0 : 1;
    }
    else { const uint32_t k = t - vc_w_sel(P), l = k / VC_LEVEL_WIRES, i = k % VC_LEVEL_WIRES; val[0] = vc_sel_value(P, b, l, i / JJ_DIGEST_BITS, i % JJ_DIGEST_BITS); }
}
// chunk g of a ballot (counted over all its hashes): its 2 or 8 wires, written to `out` (the ballot's witness, four canonical words a
// wire).  aff: the affine table, (u, v) of k 2^(4 j) G_i at jj_table_index(i, j, k).  Which hash: at most depth + 3 steps
template <class F> VSP_HD void vc_fill_chunk(const VcParams &P, const JjAffine<F> *aff, const VcBallot<F> &b, uint32_t g, uint64_t *out) {
    uint32_t h = 0;
    while (h + 1 < vc_hashes(P) && vc_chunks_before(P, h + 1) <= g) h++;
    const uint32_t c = g - vc_chunks_before(P, h);
    const unsigned s0 = vc_msg_value(P, b, h, 3 * c), s1 = vc_msg_value(P, b, h, 3 * c + 1), s2 = vc_msg_value(P, b, h, 3 * c + 2);
    uint64_t *o = out + 4 * (size_t)vc_w_chunk_wire(P, h, c, 0);
    const VcSlot<F> *slot = b.slots + vc_chunks_before(P, h);
    const JjAffine<F> pt = aff[jj_table_index(jj_chunk_segment(c), jj_chunk_window(c), jj_chunk_magnitude(s0, s1))];
    const F minus_u = neg(pt.u), x2 = s2 ? minus_u : pt.u, y2 = pt.v;
    vc_store_small(o + 4 * VC_W_S01, s0 & s1);
    jj_store_canonical(o + 4 * VC_W_X, x2);
    if (c) {
        const F x1 = slot[c - 1].a, y1 = slot[c - 1].b;
        const F U = mul(add(x1, y1), add(x2, y2)), A = mul(y2, x1), B = mul(x2, y1), Cc = mul(mul(jj_d<F>(), A), B);
        jj_store_canonical(o + 4 * VC_W_U, U);
        jj_store_canonical(o + 4 * VC_W_A, A);
        jj_store_canonical(o + 4 * VC_W_B, B);
        jj_store_canonical(o + 4 * VC_W_C, Cc);
        jj_store_canonical(o + 4 * VC_W_U3, slot[c].a);
        jj_store_canonical(o + 4 * VC_W_V3, slot[c].b);
    }
}
// item t of a ballot's fill: the wires it owns (the host path's loop; the device runs the two halves as kernels of their own)
template <class F> VSP_HD void vc_fill_item(const VcParams &P, const JjAffine<F> *aff, const VcBallot<F> &b, uint32_t t, uint64_t *out) {
    if (t < vc_w_chunk(P)) {
        uint64_t val[4];
        vc_wire_value(P, b, t, val);
        uint64_t *o = out + 4 * (size_t)t;
        o[0] = val[0]; o[1] = val[1]; o[2] = val[2]; o[3] = val[3];
        return;
    }
    vc_fill_chunk(P, aff, b, t - vc_w_chunk(P), out);
}

}  // namespace vsp

// ---- the host side: the rows as linear combinations, the affine table, a ballot's witness on one core
#include <string.h>
#include <vector>
namespace vsp {

// a linear combination over the variables (column 0: the constant 1), columns ascending and distinct
template <class F> struct VcLc {
    std::vector<uint32_t> col;
    std::vector<F> coef;
    void clear() { col.clear(); coef.clear(); }
    void add_term(uint32_t column, const F &k) {
        if (is_zero(k)) return;
        size_t at = 0;
        while (at < col.size() && col[at] < column) at++;
        if (at < col.size() && col[at] == column) {
            coef[at] = add(coef[at], k);
            if (is_zero(coef[at])) { col.erase(col.begin() + at); coef.erase(coef.begin() + at); }
            return;
        }
        col.insert(col.begin() + at, column); coef.insert(coef.begin() + at, k);
    }
    void add_wire(uint32_t wire, const F &k) { if (wire != VC_NONE) add_term(wire + 1, k); }
    void add_const(const F &k) { add_term(0, k); }
    void add_lc(const VcLc &o) { for (size_t i = 0; i < o.col.size(); i++) add_term(o.col[i], o.coef[i]); }
};

// the affine points of a table of entries (v + u, v - u, 2 d u v): u = (yp - ym) / 2, v = (yp + ym) / 2
template <class F> inline void vc_affine_table(const JjEntry<F> *tab, size_t entries, JjAffine<F> *out) {
    const F half = jj_inv(add(F::one(), F::one()));
    for (size_t i = 0; i < entries; i++) { out[i].u = mul(sub(tab[i].yp, tab[i].ym), half); out[i].v = mul(add(tab[i].yp, tab[i].ym), half); }
}

template <class F> struct VcRows {
    VcParams P;
    const JjAffine<F> *aff;
    F one, minus_one;
    VcRows(const VcParams &p, const JjAffine<F> *a) : P(p), aff(a), one(F::one()), minus_one(neg(F::one())) {}

    void boolean(uint32_t wire, VcLc<F> &A, VcLc<F> &B) const { A.add_wire(wire, one); B.add_const(one); B.add_wire(wire, minus_one); }
    // sum of 2^i wire(first + i), i < count
    void packing(uint32_t first, uint32_t count, VcLc<F> &A) const {
        F w = one;
        for (uint32_t i = 0; i < count; i++) { A.add_wire(first + i, w); w = dbl(w); }
    }
    // the selected point of chunk c of hash h before the sign: coordinate 0 = u, 1 = v
    void lookup(uint32_t h, uint32_t c, int coordinate, VcLc<F> &out) const {
        const JjAffine<F> *p = aff + jj_table_index(jj_chunk_segment(c), jj_chunk_window(c), 1);
        const F k1 = coordinate ? p[0].v : p[0].u, k2 = coordinate ? p[1].v : p[1].u, k3 = coordinate ? p[2].v : p[2].u, k4 = coordinate ? p[3].v : p[3].u;
        out.add_const(k1);
        out.add_wire(vc_msg_wire(P, h, 3 * c), sub(k2, k1));
        out.add_wire(vc_msg_wire(P, h, 3 * c + 1), sub(k3, k1));
        out.add_wire(vc_w_chunk_wire(P, h, c, VC_W_S01), add(sub(sub(k4, k3), k2), k1));
    }
    // row `row`: A, B, C (cleared first)
    void row(uint32_t r, VcLc<F> &A, VcLc<F> &B, VcLc<F> &C) const {
        A.clear(); B.clear(); C.clear();
        if (r < P.n) { boolean(vc_w_m(P) + r, A, B); return; }
        if (r == P.n) { for (uint32_t i = 0; i < P.n; i++) A.add_wire(vc_w_m(P) + i, one); B.add_const(one); C.add_const(one); return; }
        if (r < vc_r_bool(P)) {
            const uint32_t j = r - vc_r_pack(P), E = vc_eid_scalars(P);
            B.add_const(one);
            if (j < E) {
                const uint32_t start = VC_PACK_BITS * j, len = P.eid_bits - start < VC_PACK_BITS ? P.eid_bits - start : VC_PACK_BITS;
                packing(vc_w_eid(P) + start, len, A);
                C.add_wire(vc_w_eid_packed(P) + j, one);
                return;
            }
            const uint32_t k = j - E, bits = vc_w_digest_bit(P, k < 2 ? vc_hash_sn(P) : vc_hash_top(P), 0);
            if (k & 1) A.add_wire(bits + VC_PACK_BITS, one); else packing(bits, VC_PACK_BITS, A);
            C.add_wire(vc_w_sn_packed(P) + k, one);
            return;
        }
        if (r < vc_r_digest(P)) { boolean(vc_w_eid(P) + (r - vc_r_bool(P)), A, B); return; }
        if (r < vc_r_sel(P)) {
            const uint32_t k = r - vc_r_digest(P), h = k / VC_DIGEST_ROWS, i = k % VC_DIGEST_ROWS;
            if (i < JJ_DIGEST_BITS) { boolean(vc_w_digest_bit(P, h, i), A, B); return; }
            if (i == JJ_DIGEST_BITS) { packing(vc_w_digest_bit(P, h, 0), JJ_DIGEST_BITS, A); B.add_const(one); C.add_wire(vc_w_hash_u(P, h), one); return; }
            const uint32_t p = JJ_DIGEST_BITS - 2 - (i - JJ_DIGEST_BITS - 1), rank = vc_rm1_rank(p);      // p = 253 .. 0; rank >= 1
            A.add_wire(rank == 1 ? vc_w_digest_bit(P, h, JJ_DIGEST_BITS - 1) : vc_w_run_wire(P, h, rank - 2), one);
            B.add_wire(vc_w_digest_bit(P, h, p), one);
            if (vc_rm1_bit(p)) C.add_wire(vc_w_run_wire(P, h, rank - 1), one);
            return;
        }
        if (r < vc_r_chunk(P)) {
            const uint32_t k = r - vc_r_sel(P), l = k / VC_LEVEL_WIRES, right = (k % VC_LEVEL_WIRES) / JJ_DIGEST_BITS, i = k % JJ_DIGEST_BITS;
            const uint32_t cur = vc_w_digest_bit(P, vc_hash_cur(P, l), i), sib = vc_w_copath_bit(P, l, i);
            // L = cur + a (sib - cur), R = sib + a (cur - sib)
            A.add_wire(vc_w_addr(P) + l, one);
            B.add_wire(right ? cur : sib, one); B.add_wire(right ? sib : cur, minus_one);
            C.add_wire(vc_w_sel_bit(P, l, right, i), one); C.add_wire(right ? sib : cur, minus_one);
            return;
        }
        // a chunk row: the hash (at most depth + 3 steps), the chunk, the wire
        const uint32_t g = r - vc_r_chunk(P);
        uint32_t h = 0;
        while (h + 1 < vc_hashes(P) && vc_chunk_offset(P, h + 1, 0) <= g) h++;
        const uint32_t in_hash = g - vc_chunk_offset(P, h, 0);
        const uint32_t c = in_hash < VC_FIRST_CHUNK_WIRES ? 0 : (in_hash - VC_FIRST_CHUNK_WIRES) / VC_CHUNK_WIRES + 1;
        const uint32_t which = r - vc_r_chunk(P) - vc_chunk_offset(P, h, c);
        auto wire = [&](uint32_t cc, uint32_t w) { return vc_w_chunk_wire(P, h, cc, w); };
        if (which == VC_W_S01) { A.add_wire(vc_msg_wire(P, h, 3 * c), one); B.add_wire(vc_msg_wire(P, h, 3 * c + 1), one); C.add_wire(wire(c, VC_W_S01), one); return; }
        if (which == VC_W_X) {
            A.add_const(one); A.add_wire(vc_msg_wire(P, h, 3 * c + 2), neg(dbl(one)));
            lookup(h, c, 0, B);
            C.add_wire(wire(c, VC_W_X), one);
            return;
        }
        VcLc<F> x1, y1, x2, y2;
        if (c == 1) { x1.add_wire(wire(0, VC_W_X), one); lookup(h, 0, 1, y1); }
        else { x1.add_wire(wire(c - 1, VC_W_U3), one); y1.add_wire(wire(c - 1, VC_W_V3), one); }
        x2.add_wire(wire(c, VC_W_X), one); lookup(h, c, 1, y2);
        switch (which) {
        case VC_W_U: A.add_lc(x1); A.add_lc(y1); B.add_lc(x2); B.add_lc(y2); C.add_wire(wire(c, VC_W_U), one); break;
        case VC_W_A: A.add_lc(y2); B.add_lc(x1); C.add_wire(wire(c, VC_W_A), one); break;
        case VC_W_B: A.add_lc(x2); B.add_lc(y1); C.add_wire(wire(c, VC_W_B), one); break;
        case VC_W_C: A.add_wire(wire(c, VC_W_A), jj_d<F>()); B.add_wire(wire(c, VC_W_B), one); C.add_wire(wire(c, VC_W_C), one); break;
        case VC_W_U3: A.add_const(one); A.add_wire(wire(c, VC_W_C), one); B.add_wire(wire(c, VC_W_U3), one); C.add_wire(wire(c, VC_W_A), one); C.add_wire(wire(c, VC_W_B), one); break;
        default: A.add_const(one); A.add_wire(wire(c, VC_W_C), minus_one); B.add_wire(wire(c, VC_W_V3), one);
                 C.add_wire(wire(c, VC_W_U), one); C.add_wire(wire(c, VC_W_A), minus_one); C.add_wire(wire(c, VC_W_B), minus_one); break;
        }
    }
};

// the three matrices in CSR form, coefficients canonical
struct VcCsr { std::vector<uint32_t> row_ptr[3], col[3]; std::vector<uint64_t> coef[3]; };
template <class F> inline void vc_build_csr(const VcParams &P, const JjAffine<F> *aff, VcCsr &out) {
    const VcRows<F> rows(P, aff);
    const uint32_t m = vc_num_constraints(P);
    VcLc<F> lc[3];
    for (int k = 0; k < 3; k++) { out.row_ptr[k].assign(1, 0); out.col[k].clear(); out.coef[k].clear(); }
    for (uint32_t r = 0; r < m; r++) {
        rows.row(r, lc[0], lc[1], lc[2]);
        for (int k = 0; k < 3; k++) {
            for (size_t i = 0; i < lc[k].col.size(); i++) {
                uint64_t w[4];
                jj_store_canonical(w, lc[k].coef[i]);
                out.col[k].push_back(lc[k].col[i]);
                out.coef[k].insert(out.coef[k].end(), w, w + 4);
            }
            out.row_ptr[k].push_back((uint32_t)out.col[k].size());
        }
    }
}

// One ballot's witness on the host, one core: the chains of its depth + 3 hashes one after the other from sk and the copath (depth x 4
// words), then every item of the fill.  out: vc_num_vars x 4 canonical words.  leaf_out (may be null): the leaf computed from sk.
// The caller has checked vote < n, index < 2^depth, sk < 2^255
template <class F> inline void vc_witness_host(const VcParams &P, const JjEntry<F> *tab, const JjAffine<F> *aff, const uint64_t *eid, const uint64_t *sk, uint64_t index,
                                               uint32_t vote, const uint64_t *copath, uint64_t *out, uint64_t *leaf_out) {
    const uint32_t H = vc_hashes(P);
    std::vector<uint64_t> digests(4 * (size_t)H);
    std::vector<VcSlot<F>> slots(vc_total_chunks(P));
    auto chain = [&](uint32_t h, const uint64_t *words, uint32_t gap) {
        const JjMessage m{words, vc_hash_bits(P, h), gap};
        vc_chain(tab, m, slots.data() + vc_chunks_before(P, h), digests.data() + 4 * (size_t)h);
    };
    chain(0, sk, 0);
    if (P.hash_leaves) chain(1, digests.data(), 0);
    if (leaf_out) memcpy(leaf_out, digests.data() + 4 * (size_t)vc_hash_leaf(P), 4 * sizeof(uint64_t));
    for (uint32_t l = 0; l < P.depth; l++) {
        uint64_t pair[8];
        const unsigned a = (unsigned)(index >> l) & 1u;
        memcpy(pair + 4 * a, digests.data() + 4 * (size_t)vc_hash_cur(P, l), 4 * sizeof(uint64_t));
        memcpy(pair + 4 * (1 - a), copath + 4 * l, 4 * sizeof(uint64_t));
        chain(vc_hash_node(P, l), pair, 1);
    }
    std::vector<uint64_t> sn((vc_sn_bits(P) + 63) / 64 + 1, 0);
    for (uint32_t k = 0; k < vc_sn_bits(P); k++) sn[k >> 6] |= (uint64_t)(k < P.eid_bits ? vc_word_bit(eid, k) : vc_word_bit(sk, k - P.eid_bits)) << (k & 63);
    chain(vc_hash_sn(P), sn.data(), 0);
    VcBallot<F> b;
    b.sk = sk; b.eid = eid; b.index = index; b.vote = vote; b.nodes = copath; b.tree = false; b.digests = digests.data(); b.slots = slots.data();
    for (uint32_t t = 0; t < vc_fill_items(P); t++) vc_fill_item(P, aff, b, t, out);
}

}  // namespace vsp
