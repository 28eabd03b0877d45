// CPU test build of the registry's rules (vote_saver_protocol_amd/csrc/jubjub.h: the group law, the table entry and the mixed addition,
// the chunk encoding, the schedule, the lane shares and the fold order, the generator tests, the blob bit order and the rt split),
// compiled by g++ over 64-bit limbs.  A hash is computed the way a group of L lanes computes it on the device -- every lane its share,
// then the fold level by level -- and the additions are counted.  Test infrastructure only.  With -DJUBJUB_CHECK_MAIN the file is a
// program of its own (the sanitizer run of tests/test_jubjub_cpu.py; with an argument, the one-core timing of tools/registry_time.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/jubjub.h"
using namespace vsp;

namespace {

using F = HFr;
using Point = JjPoint<F>;

JjAffine<F> load_affine(const uint64_t *w) { JjAffine<F> a; a.u = jj_load_canonical<F>(w); a.v = jj_load_canonical<F>(w + 4); return a; }
void store_point(uint64_t *out, const Point &p) { const JjAffine<F> a = jj_to_affine(p); jj_store_canonical(out, a.u); jj_store_canonical(out + 4, a.v); }

struct Table {
    size_t g;
    std::vector<JjEntry<F>> rows;
};

// the hash of a message as a group of `lanes` lanes computes it.  added[c]: additions of chunk c; gave[l]: times lane l gave its sum away
Point hash_as_lanes(const Table &t, const JjMessage &m, unsigned lanes, uint32_t *added, uint32_t *gave) {
    std::vector<Point> acc(lanes);
    for (unsigned l = 0; l < lanes; l++) {
        acc[l] = jj_lane_sum(t.rows.data(), m, l, lanes);
        if (added) for (uint32_t c = l; c < jj_chunks(m.nbits); c += lanes) added[c]++;
    }
    for (unsigned s = 32; s >= 1; s >>= 1) {
        std::vector<Point> part(lanes);
        for (unsigned l = 0; l < lanes; l++) if (jj_fold_gives(l, lanes, s)) { part[l] = acc[l]; if (gave) gave[l]++; }
        for (unsigned l = 0; l < lanes; l++) if (jj_fold_takes(l, lanes, s)) acc[l] = jj_add(acc[l], part[l + s]);
    }
    return acc[0];
}

void digest_of(const Point &p, uint64_t out[4]) { const JjAffine<F> a = jj_to_affine(p); jj_store_canonical(out, a.u); }

}  // namespace

extern "C" {

void chk_jj_add(const uint64_t *a, const uint64_t *b, uint64_t *out) { store_point(out, jj_add(jj_from_affine(load_affine(a)), jj_from_affine(load_affine(b)))); }
void chk_jj_dbl(const uint64_t *a, uint64_t *out) { store_point(out, jj_dbl(jj_from_affine(load_affine(a)))); }
// p + q or p - q through q's table entry; p arrives with Z = 3 so that the mixed form meets a projective operand
void chk_jj_madd(const uint64_t *p, const uint64_t *q, int negative, uint64_t *out) {
    Point P = jj_from_affine(load_affine(p));
    const F three = add(F::one(), dbl(F::one()));
    P.X = mul(P.X, three); P.Y = mul(P.Y, three); P.Z = three; P.T = mul(P.T, three);
    store_point(out, jj_madd(P, jj_entry(load_affine(q)), negative != 0));
}
int chk_jj_encode(unsigned s0, unsigned s1, unsigned s2) { const int m = (int)jj_chunk_magnitude(s0, s1); return s2 ? -m : m; }
size_t chk_jj_schedule(uint32_t nbits, uint32_t *segment, uint32_t *window) {
    const uint32_t n = jj_chunks(nbits);
    for (uint32_t c = 0; c < n; c++) { segment[c] = jj_chunk_segment(c); window[c] = jj_chunk_window(c); }
    return n;
}
size_t chk_jj_max_bits(size_t g) { return jj_max_bits(g); }
unsigned chk_jj_message_bit(const uint64_t *w, uint32_t nbits, uint32_t gap, uint32_t k) { const JjMessage m{w, nbits, gap}; return jj_message_bit(m, k); }
int chk_jj_generator_fault(const uint64_t *pt) { return jj_generator_fault<F>(pt, nullptr); }
int chk_jj_on_curve(const uint64_t *pt) { return jj_below_r(pt) && jj_below_r(pt + 4) && jj_on_curve(load_affine(pt)) ? 1 : 0; }
int chk_jj_prime_order(const uint64_t *pt) { return jj_prime_order(load_affine(pt)) ? 1 : 0; }
unsigned chk_jj_group_lanes(size_t count) { return jj_group_lanes(count); }
int chk_jj_fold(unsigned lane, unsigned lanes, unsigned s) { return (jj_fold_gives(lane, lanes, s) ? 1 : 0) | (jj_fold_takes(lane, lanes, s) ? 2 : 0); }

void *chk_jj_table_new(const uint64_t *gens, size_t g) {
    Table *t = new Table();
    t->g = g;
    t->rows.resize(g * JJ_GEN_ENTRIES);
    for (size_t i = 0; i < g; i++) {
        Point base = jj_from_affine(load_affine(gens + 8 * i));
        for (unsigned j = 0; j < JJ_WINDOWS; j++) {
            jj_window_entries(base, &t->rows[(i * JJ_WINDOWS + j) * JJ_ENTRIES]);
            for (int k = 0; k < 4; k++) base = jj_dbl(base);
        }
    }
    return t;
}
void chk_jj_table_free(void *t) { delete (Table *)t; }
// window j of generator i computed the way a lane of k_pedersen_table does (4 j doublings from the generator) against the running one
int chk_jj_table_window(const void *tp, const uint64_t *gens, size_t i, unsigned j) {
    const Table *t = (const Table *)tp;
    JjEntry<F> e[JJ_ENTRIES];
    jj_window_entries(jj_window_base(load_affine(gens + 8 * i), j), e);
    return memcmp(e, &t->rows[(i * JJ_WINDOWS + j) * JJ_ENTRIES], sizeof e) == 0 ? 1 : 0;
}
// added: a counter per chunk, gave: a counter per lane (both zeroed by the caller; either may be null)
int chk_jj_hash(const void *tp, const uint64_t *words, uint32_t nbits, uint32_t gap, unsigned lanes, uint64_t *digest, uint64_t *point, uint32_t *added, uint32_t *gave) {
    const Table *t = (const Table *)tp;
    if (nbits == 0 || nbits > jj_max_bits(t->g) || !jj_lanes_valid((long)lanes)) return -1;
    const JjMessage m{words, nbits, gap};
    const Point p = hash_as_lanes(*t, m, lanes, added, gave);
    digest_of(p, digest);
    if (point) store_point(point, p);
    return 0;
}
// the tree of `count` keys (four words each; absent keys zero): nodes_out has 2^(depth + 1) - 1 nodes, leaves first
int chk_jj_tree(const void *tp, const uint64_t *pks, size_t count, unsigned depth, int hash_leaves, uint64_t *nodes) {
    const Table *t = (const Table *)tp;
    if (t->g < JJ_NODE_GENERATORS || depth > JJ_MAX_DEPTH || count > ((size_t)1 << depth)) return -1;
    const uint64_t leaves = jj_level_nodes(depth, 0);
    for (uint64_t i = 0; i < leaves; i++) {
        uint64_t key[4] = {0, 0, 0, 0};
        if (i < count) memcpy(key, pks + 4 * i, sizeof key);
        if (hash_leaves) { const JjMessage m{key, JJ_DIGEST_BITS, 0}; digest_of(hash_as_lanes(*t, m, 1, nullptr, nullptr), nodes + 4 * i); }
        else memcpy(nodes + 4 * i, key, sizeof key);
    }
    for (unsigned l = 1; l <= depth; l++) {
        const uint64_t *below = nodes + 4 * jj_level_first(depth, l - 1);
        uint64_t *here = nodes + 4 * jj_level_first(depth, l);
        for (uint64_t i = 0; i < jj_level_nodes(depth, l); i++) {
            const JjMessage m{below + 8 * i, JJ_NODE_BITS, 1};
            digest_of(hash_as_lanes(*t, m, 1, nullptr, nullptr), here + 4 * i);
        }
    }
    return 0;
}
uint64_t chk_jj_level_first(unsigned depth, unsigned level) { return jj_level_first(depth, level); }
uint64_t chk_jj_sibling(uint64_t x, unsigned level) { return jj_sibling(x, level); }
void chk_jj_blob(const uint64_t *digest, uint8_t *out) { for (int i = 0; i < 4; i++) { const uint64_t w = jj_blob_word(digest[i]); memcpy(out + 8 * i, &w, 8); } }
void chk_jj_unblob(const uint8_t *in, uint64_t *digest) { for (int i = 0; i < 4; i++) { uint64_t w; memcpy(&w, in + 8 * i, 8); digest[i] = jj_blob_word(w); } }
void chk_jj_rt_split(const uint64_t *digest, uint64_t *out) { jj_rt_split(digest, out); }

}  // extern "C"

#ifdef JUBJUB_CHECK_MAIN
// The program's generators are G, 2 G and 3 G for the point G = (u, v) of order s below: tests/jubjub_model.py generator(b"vsp-test-pedersen", 0)
static const uint64_t G0[8] = {0x3286496a1493875fULL, 0x2a31ede0cebb3f57ULL, 0x7bb6f12b6d21103bULL, 0x0cad345f7ab8683cULL,
                               0x6584ea1c5a8d6706ULL, 0xf0d482f70bdb53a8ULL, 0xaec84a962b9f9975ULL, 0x3ecb3b2010af4d0cULL};
int main(int argc, char **argv) {
    if (chk_jj_generator_fault(G0) != JJ_GEN_OK) { printf("jubjub_check: the built-in generator is refused\n"); return 1; }
    uint64_t gens[24];
    memcpy(gens, G0, sizeof G0);
    chk_jj_dbl(G0, gens + 8);
    chk_jj_add(gens + 8, G0, gens + 16);
    void *t = chk_jj_table_new(gens, 3);
    if (argc > 1) {                                                 // timing: the tree of depth argv[1] over random-looking keys, one core
        const unsigned depth = (unsigned)atoi(argv[1]);
        if (depth > 16) return 2;
        std::vector<uint64_t> pks(4 << depth), nodes(4 * jj_tree_nodes(depth));
        uint64_t x = 0x9E3779B97F4A7C15ULL;
        for (size_t i = 0; i < pks.size(); i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; pks[i] = (i & 3) == 3 ? x >> 1 : x; }
        const auto t0 = std::chrono::steady_clock::now();
        if (chk_jj_tree(t, pks.data(), (size_t)1 << depth, depth, 1, nodes.data())) return 3;
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        printf("jubjub_check: depth %u hashes %llu ms %.3f root %016llx\n", depth, (unsigned long long)jj_tree_nodes(depth), ms, (unsigned long long)nodes[4 * (jj_tree_nodes(depth) - 1)]);
        chk_jj_table_free(t);
        return 0;
    }
    int bad = 0;
    // every lane count gives the digest of one lane; every chunk is added once and every lane gives at most once
    const uint32_t sizes[] = {1, 2, 3, 4, 188, 189, 190, 255, 378, 510, 567};
    for (uint32_t n : sizes) {
        uint64_t words[9];
        for (int i = 0; i < 9; i++) words[i] = 0xA5A5F00F12345678ULL * (i + 1) + n;
        uint64_t want[4], pt[8];
        std::vector<uint32_t> added(jj_chunks(n), 0);
        if (chk_jj_hash(t, words, n, 0, 1, want, pt, added.data(), nullptr)) bad++;
        if (!chk_jj_on_curve(pt)) bad++;
        for (unsigned L : {4u, 16u, 64u}) {
            uint64_t got[4];
            std::vector<uint32_t> a(jj_chunks(n), 0), g(L, 0);
            if (chk_jj_hash(t, words, n, 0, L, got, nullptr, a.data(), g.data())) bad++;
            if (memcmp(got, want, sizeof got)) bad++;
            for (uint32_t c : a) if (c != 1) bad++;
            for (uint32_t c : g) if (c > 1) bad++;
        }
    }
    // a small tree, its blob and back
    std::vector<uint64_t> pks(4 * 3, 7), nodes(4 * jj_tree_nodes(2));
    if (chk_jj_tree(t, pks.data(), 3, 2, 1, nodes.data())) bad++;
    uint8_t blob[32]; uint64_t back[4], rt[8];
    chk_jj_blob(&nodes[4 * 6], blob); chk_jj_unblob(blob, back);
    if (memcmp(back, &nodes[4 * 6], sizeof back)) bad++;
    chk_jj_rt_split(back, rt);
    if (rt[3] >> 62) bad++;
    const uint64_t minus_one[8] = {0, 0, 0, 0, 0xffffffff00000000ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};      // (0, -1)
    const uint64_t identity[8] = {0, 0, 0, 0, 1, 0, 0, 0};
    if (chk_jj_generator_fault(minus_one) != JJ_GEN_NOT_PRIME_ORDER || chk_jj_generator_fault(identity) != JJ_GEN_IDENTITY) bad++;
    chk_jj_table_free(t);
    if (bad) { printf("jubjub_check: %d failures\n", bad); return 1; }
    printf("jubjub_check: ok\n");
    return 0;
}
#endif
