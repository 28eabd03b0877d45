// CPU test build of the voting circuit's rules (vote_saver_protocol_amd/csrc/vote_circuit.h: the layout functions, the rows, the chains
// and the fill), compiled by g++ over 64-bit limbs: the header's host path builds a witness, and every row of the matrices the header's
// builder made is evaluated on it in 64-bit limbs.  Test infrastructure only.  With -DVOTE_CIRCUIT_CHECK_MAIN the file is a program of
// its own (the sanitizer run of tests/test_vote_circuit_cpu.py; with arguments, the one-core timing of tools/vote_witness_time.py).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/vote_circuit.h"
using namespace vsp;

namespace {

using F = HFr;

struct Circuit {
    VcParams P;
    size_t g;
    std::vector<JjEntry<F>> tab;
    std::vector<JjAffine<F>> aff;
    VcCsr csr;
};

}  // namespace

extern "C" {

void *chk_vc_new(const uint64_t *gens, size_t g, uint32_t n, uint32_t eid_bits, uint32_t depth, int hash_leaves, int with_csr) {
    VcParams P{n, eid_bits, depth, hash_leaves ? 1u : 0u};
    if (!vc_params_valid(P, g)) return nullptr;
    Circuit *c = new Circuit();
    c->P = P; c->g = g;
    c->tab.resize(g * JJ_GEN_ENTRIES); c->aff.resize(g * JJ_GEN_ENTRIES);
    for (size_t i = 0; i < g; i++) {
        JjAffine<F> a; a.u = jj_load_canonical<F>(gens + 8 * i); a.v = jj_load_canonical<F>(gens + 8 * i + 4);
        JjPoint<F> base = jj_from_affine(a);
        for (unsigned j = 0; j < JJ_WINDOWS; j++) {
            jj_window_entries(base, &c->tab[(i * JJ_WINDOWS + j) * JJ_ENTRIES]);
            for (int k = 0; k < 4; k++) base = jj_dbl(base);
        }
    }
    vc_affine_table(c->tab.data(), c->tab.size(), c->aff.data());
    if (with_csr) vc_build_csr(c->P, c->aff.data(), c->csr);
    return c;
}
void chk_vc_free(void *h) { delete (Circuit *)h; }
// out: the layout functions' totals (rows, inputs, variables, hashes, chunks, fill items) and the built matrices' rows and entries
void chk_vc_sizes(const void *h, uint64_t out[10]) {
    const Circuit *c = (const Circuit *)h;
    out[0] = vc_num_constraints(c->P); out[1] = vc_num_inputs(c->P); out[2] = vc_num_vars(c->P);
    out[3] = vc_hashes(c->P); out[4] = vc_total_chunks(c->P); out[5] = vc_fill_items(c->P);
    out[6] = c->csr.row_ptr[0].size() - 1;
    for (int k = 0; k < 3; k++) out[7 + k] = c->csr.col[k].size();
}
void chk_vc_csr(const void *h, int matrix, uint32_t *row_ptr, uint32_t *col, uint64_t *coef) {
    const Circuit *c = (const Circuit *)h;
    memcpy(row_ptr, c->csr.row_ptr[matrix].data(), c->csr.row_ptr[matrix].size() * sizeof(uint32_t));
    memcpy(col, c->csr.col[matrix].data(), c->csr.col[matrix].size() * sizeof(uint32_t));
    memcpy(coef, c->csr.coef[matrix].data(), c->csr.coef[matrix].size() * sizeof(uint64_t));
}
int chk_vc_wires(const void *h, int block, uint32_t *first, uint32_t *count) { return vc_block(((const Circuit *)h)->P, block, first, count) ? 0 : -1; }
// columns ascending inside every row and below num_vars + 1, row pointers monotone
int chk_vc_columns_ok(const void *h) {
    const Circuit *c = (const Circuit *)h;
    const uint32_t cols = vc_num_vars(c->P) + 1;
    for (int k = 0; k < 3; k++) {
        const auto &rp = c->csr.row_ptr[k]; const auto &ci = c->csr.col[k];
        if (rp.size() != (size_t)vc_num_constraints(c->P) + 1 || rp[0] != 0 || rp.back() != ci.size()) return 0;
        for (size_t r = 0; r + 1 < rp.size(); r++) {
            if (rp[r] > rp[r + 1]) return 0;
            for (uint32_t i = rp[r]; i < rp[r + 1]; i++) if (ci[i] >= cols || (i > rp[r] && ci[i - 1] >= ci[i])) return 0;
        }
    }
    return 1;
}
int chk_vc_witness(const void *h, const uint64_t *eid, const uint64_t *sk, uint64_t index, uint32_t vote, const uint64_t *copath, uint64_t *out, uint64_t *leaf_out) {
    const Circuit *c = (const Circuit *)h;
    if (vote >= c->P.n || (index >> c->P.depth) || (sk[3] >> 63)) return -1;
    vc_witness_host<F>(c->P, c->tab.data(), c->aff.data(), eid, sk, index, vote, copath, out, leaf_out);
    return 0;
}
// the first row that z = (1, witness) fails, in 64-bit limbs; num_constraints when none does; *bad_rows the number of failing rows
uint64_t chk_vc_first_bad_row(const void *h, const uint64_t *witness, uint64_t *bad_rows) {
    const Circuit *c = (const Circuit *)h;
    const uint32_t nv = vc_num_vars(c->P), m = vc_num_constraints(c->P);
    std::vector<F> z(nv + 1);
    z[0] = F::one();
    for (uint32_t i = 0; i < nv; i++) z[i + 1] = jj_load_canonical<F>(witness + 4 * (size_t)i);
    uint64_t first = m, bad = 0;
    for (uint32_t r = 0; r < m; r++) {
        F dot[3];
        for (int k = 0; k < 3; k++) {
            dot[k] = F::zero();
            for (uint32_t i = c->csr.row_ptr[k][r]; i < c->csr.row_ptr[k][r + 1]; i++)
                dot[k] = add(dot[k], mul(jj_load_canonical<F>(&c->csr.coef[k][4 * (size_t)i]), z[c->csr.col[k][i]]));
        }
        if (!eq(mul(dot[0], dot[1]), dot[2])) { if (first == m) first = r; bad++; }
    }
    if (bad_rows) *bad_rows = bad;
    return first;
}

}  // extern "C"

#ifdef VOTE_CIRCUIT_CHECK_MAIN
// generators G, 2 G, 3 G of tests/jubjub_model.py generator(b"vsp-test-pedersen", 0); a voter alone in a tree of absent keys
static const uint64_t G0[8] = {0x3286496a1493875fULL, 0x2a31ede0cebb3f57ULL, 0x7bb6f12b6d21103bULL, 0x0cad345f7ab8683cULL,
                               0x6584ea1c5a8d6706ULL, 0xf0d482f70bdb53a8ULL, 0xaec84a962b9f9975ULL, 0x3ecb3b2010af4d0cULL};
int main(int argc, char **argv) {
    uint64_t gens[24];
    memcpy(gens, G0, sizeof G0);
    {
        const JjAffine<F> a{jj_load_canonical<F>(G0), jj_load_canonical<F>(G0 + 4)};
        const JjPoint<F> p = jj_from_affine(a), p2 = jj_dbl(p), p3 = jj_add(p2, p);
        const JjAffine<F> a2 = jj_to_affine(p2), a3 = jj_to_affine(p3);
        jj_store_canonical(gens + 8, a2.u); jj_store_canonical(gens + 12, a2.v); jj_store_canonical(gens + 16, a3.u); jj_store_canonical(gens + 20, a3.v);
    }
    const bool timing = argc > 4;                                   // depth eid_bits n repeats: witnesses only, timed
    const uint32_t depth = timing ? (uint32_t)atoi(argv[1]) : 2, eid_bits = timing ? (uint32_t)atoi(argv[2]) : 5, n = timing ? (uint32_t)atoi(argv[3]) : 3;
    const int repeats = timing ? atoi(argv[4]) : 1;
    void *h = chk_vc_new(gens, 3, n, eid_bits, depth, 1, timing ? 0 : 1);
    if (!h) { printf("vote_circuit_check: parameters refused\n"); return 2; }
    uint64_t sizes[10];
    chk_vc_sizes(h, sizes);
    std::vector<uint64_t> copath(4 * (size_t)depth + 4), wit(4 * sizes[2]);
    uint64_t x = 0x9E3779B97F4A7C15ULL;
    for (auto &w : copath) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; w = x >> 2; }
    const uint64_t sk[4] = {0x1234567, 0x89abcdef, 0x5555, 0x0123456789abcdefULL}, eid[2] = {0x1d, 0};
    if (timing) {
        for (int i = 0; i < repeats; i++) {
            const auto t0 = std::chrono::steady_clock::now();
            if (chk_vc_witness(h, eid, sk, 1, 0, copath.data(), wit.data(), nullptr)) return 3;
            printf("vote_circuit_check: witness_ms %.3f\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        printf("vote_circuit_check: num_constraints %llu num_vars %llu\n", (unsigned long long)sizes[0], (unsigned long long)sizes[2]);
        chk_vc_free(h);
        return 0;
    }
    int bad = 0;
    if (sizes[6] != sizes[0] || !chk_vc_columns_ok(h)) bad++;
    for (uint64_t index = 0; index < 4; index++) {
        if (chk_vc_witness(h, eid, sk, index, (uint32_t)(index % n), copath.data(), wit.data(), nullptr)) bad++;
        uint64_t rows = 0;
        if (chk_vc_first_bad_row(h, wit.data(), &rows) != sizes[0] || rows) bad++;
    }
    uint32_t first, count;
    chk_vc_wires(h, VC_SK_BITS, &first, &count);
    wit[4 * (size_t)first] ^= 1;                                   // a flipped sk bit must fail
    if (chk_vc_first_bad_row(h, wit.data(), nullptr) == sizes[0]) bad++;
    chk_vc_free(h);
    if (bad) { printf("vote_circuit_check: %d failures\n", bad); return 1; }
    printf("vote_circuit_check: ok\n");
    return 0;
}
#endif
