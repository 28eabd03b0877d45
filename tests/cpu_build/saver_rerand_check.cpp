// CPU test build of the batch rerandomization's shared rules (vote_saver_protocol_amd/csrc/saver_rerand.h: the column plans, the place
// where a ballot's own point joins a column, the scalar records with their shared inversion and the table of a fixed point, compiled by
// g++ with the 32-bit-limb types the kernels use and with the host's 64-bit-limb types).  Test infrastructure only.  All arguments
// canonical little-endian u64 limbs: a G1 point x | y (12 words, all zero = infinity), a G2 point 24 words, a scalar 4 words.  With
// -DSAVER_RERAND_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_saver_rerand_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/saver_rerand.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }
template <class F> static Affine<F> load_point(const uint64_t *p) { Affine<F> a; a.x = to_mont(load<F>(p)); a.y = to_mont(load<F>(p + sizeof(F) / 8)); return a; }
template <class F> static void store_point(uint64_t *p, const XYZZ<F> &s) { const Affine<F> a = xyzz_to_affine(s); store(p, from_mont(a.x)); store(p + sizeof(F) / 8, from_mont(a.y)); }

// the tables of `nb` fixed points of one group (saver_fixed_table) and the plan over them
template <class F> struct Tables {
    std::vector<Affine<F>> tab; std::vector<uint8_t> inf;
    Tables(const uint64_t *bases, size_t nb) {
        Affine<F> zero; zero.x = F::zero(); zero.y = F::zero();
        tab.assign(nb * SAVER_TABLE_POINTS, zero); inf.assign(nb, 0);
        for (size_t b = 0; b < nb; b++) inf[b] = !saver_fixed_table(load_point<F>(bases + b * (sizeof(Affine<F>) / 8)), tab.data() + b * SAVER_TABLE_POINTS);
    }
};
// a key: the n + 3 bases X_0 .. X_{n+1} | P2 of the G1 columns
template <class F> struct Key {
    size_t n; Tables<F> t; SaverPlan plan;
    Key(size_t n_, const uint64_t *bases) : n(n_), t(bases, saver_rerand_columns(n_)) { plan = saver_rerand_plan(n, t.inf.data()); }
};
// the columns of a plan as the lane groups of k_rr_columns compute them, one host lane per lane of a group: every lane sums its share,
// the group folds level by level (gives before takes, as the barrier orders them), lane 0 adds the given point of the column
template <class F> static void columns(const SaverPlan &pl, const Affine<F> *tab, const uint64_t *rec, const uint64_t *given, uint64_t *out) {
    auto madd_ = [](XYZZ<F> *a, const Affine<F> *q) { xyzz_madd(*a, *q); };
    constexpr size_t PW = sizeof(Affine<F>) / 8;
    for (size_t c = 0; c < pl.cols.size(); c++) {
        const SaverColumn &col = pl.cols[c];
        std::vector<XYZZ<F>> acc(col.lanes), part(col.lanes);
        for (unsigned l = 0; l < col.lanes; l++) saver_lane_sum(acc[l], tab, rec, col, pl.pairs.data(), l, col.lanes, madd_);
        for (unsigned s = 32; s >= 1; s >>= 1) {
            for (unsigned l = 0; l < col.lanes; l++) if (saver_fold_gives(l, col.lanes, s)) part[l] = acc[l];
            for (unsigned l = 0; l < col.lanes; l++) if (saver_fold_takes(l, col.lanes, s)) xyzz_add(acc[l], part[l + s]);
        }
        Affine<F> g;
        if (given) g = load_point<F>(given + PW * c);
        saver_rerand_join(acc[0], given ? &g : nullptr, madd_);
        store_point(out + PW * c, acc[0]);
    }
}
// one ballot: rnd = r' | z1 | z2, given = ct_0 .. ct_{n+1} | C; out = the n + 3 columns
template <class F, class FR> static void ballot(const Key<F> &key, const uint64_t *rnd, const uint64_t *given, uint64_t *out) {
    uint64_t rec[4 * RR_SCALARS]; FR pre;
    saver_rerand_scalars<FR>(rnd, 1, rec, &pre);
    columns<F>(key.plan, key.t.tab.data(), rec, given, out);
}
// z2 delta_g2 through the G2 column
template <class F2, class FR> static void delta(const uint64_t *delta_g2, const uint64_t *rnd, uint64_t *out) {
    Tables<F2> t(delta_g2, 1);
    uint64_t rec[4 * RR_SCALARS]; FR pre;
    saver_rerand_scalars<FR>(rnd, 1, rec, &pre);
    columns<F2>(saver_rerand_delta_plan(t.inf[0] != 0), t.tab.data(), rec, nullptr, out);
}
// the plan's shape: 0 when there are n + 3 columns of one pair, column c over base c under scalar r' and starting at given point c, every
// lane names its column, no two groups overlap, and with the spans of 64 ballots laid end to end no group straddles a wave;
// *longest = the longest dependent chain of additions (a lane's terms + the fold's levels + the given point)
static int plan_shape(size_t n, unsigned *longest, unsigned *span) {
    const SaverPlan pl = saver_rerand_plan(n, nullptr), p2 = saver_rerand_delta_plan(false);
    int bad = pl.cols.size() != n + 3 || pl.pairs.size() != n + 3 || saver_rerand_given(n) != n + 4 || saver_rerand_given_C(n) != n + 2 || saver_rerand_given_A(n) != n + 3;
    bad |= p2.cols.size() != 1 || p2.pairs.size() != 1 || p2.pairs[0].scalar != RR_Z2 || p2.pairs[0].base != 0 || p2.lane_col.size() != p2.cols[0].lanes || 64 % p2.cols[0].lanes;
    std::vector<unsigned> seen(pl.cols.size(), 0);
    for (size_t l = 0; l < pl.lane_col.size(); l++) {
        const uint32_t c = pl.lane_col[l];
        if (c == SAVER_NO_COLUMN) continue;
        bad |= c >= pl.cols.size() || l < pl.cols[c].lane0 || l >= pl.cols[c].lane0 + pl.cols[c].lanes;
        if (c < pl.cols.size()) seen[c]++;
    }
    *longest = 0; *span = (unsigned)pl.lane_col.size();
    for (size_t c = 0; c < pl.cols.size(); c++) {
        const SaverColumn &col = pl.cols[c];
        const SaverPair &p = pl.pairs[col.first_pair];
        bad |= col.pairs != 1 || col.first_pair != c || p.scalar != RR_R || p.base != c || p.skip;
        bad |= seen[c] != col.lanes || (col.lanes & (col.lanes - 1)) || col.lanes < 8 || col.lanes > 64;
        for (size_t k = 0; k < 64; k++) { const size_t first = k * *span + col.lane0; bad |= first / 64 != (first + col.lanes - 1) / 64; }
        unsigned levels = 0;
        while ((1u << levels) < col.lanes) levels++;
        const unsigned chain = (col.pairs * SAVER_WINDOWS + col.lanes - 1) / col.lanes + levels + 1;
        if (chain > *longest) *longest = chain;
    }
    const uint8_t flags[4] = {0, 1, 0, 1};
    const SaverPlan pf = saver_rerand_plan(1, flags);
    bad |= pf.pairs[0].skip || !pf.pairs[1].skip || pf.pairs[2].skip || !pf.pairs[3].skip || !saver_rerand_delta_plan(true).pairs[0].skip;
    return bad;
}

extern "C" {
void *chk_key(size_t n, const uint64_t *bases) { return new Key<Fp>(n, bases); }
void *chk_hkey(size_t n, const uint64_t *bases) { return new Key<HFp>(n, bases); }
void chk_key_free(void *k) { delete (Key<Fp> *)k; }
void chk_hkey_free(void *k) { delete (Key<HFp> *)k; }
void chk_ballot(const void *key, const uint64_t *rnd, const uint64_t *given, uint64_t *out) { ballot<Fp, Fr>(*(const Key<Fp> *)key, rnd, given, out); }
void chk_hballot(const void *key, const uint64_t *rnd, const uint64_t *given, uint64_t *out) { ballot<HFp, HFr>(*(const Key<HFp> *)key, rnd, given, out); }
void chk_delta(const uint64_t *delta_g2, const uint64_t *rnd, uint64_t *out) { delta<Fp2, Fr>(delta_g2, rnd, out); }
void chk_hdelta(const uint64_t *delta_g2, const uint64_t *rnd, uint64_t *out) { delta<HFp2, HFr>(delta_g2, rnd, out); }
int chk_plan_shape(size_t n, unsigned *longest, unsigned *span) { return plan_shape(n, longest, span); }
// rec: count x 20 words r' | z1 | z1 z2 | 1 / z1 | z2
void chk_scalars(const uint64_t *rnd, size_t count, uint64_t *rec) { std::vector<Fr> pre(count); saver_rerand_scalars<Fr>(rnd, count, rec, pre.data()); }
void chk_hscalars(const uint64_t *rnd, size_t count, uint64_t *rec) { std::vector<HFr> pre(count); saver_rerand_scalars<HFr>(rnd, count, rec, pre.data()); }
}

#ifdef SAVER_RERAND_CHECK_MAIN
#include <stdio.h>
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
static const uint64_t GEN2[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                  0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                  0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                  0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
// msg_size 1 with every base the generator G but X_1, which is at infinity; r' = 5, z1 = 3, z2 = 7.  Given ct_0 = 5 G (the addition
// doubles), ct_1 = 2 G (its base is skipped), ct_2 = infinity and C = G: the columns are 10 G, 2 G, 5 G, 6 G; z2 delta = 7 H; and
// z1 z2 = 21, z1 (1 / z1) = 1 -- for both limb types, which must agree on the bytes
template <class F, class F2, class FR> static int run(uint64_t *out, uint64_t *out2) {
    const size_t n = 1;
    std::vector<uint64_t> bases(12 * 4);
    for (size_t b = 0; b < 4; b++) memcpy(bases.data() + 12 * b, GEN1, sizeof GEN1);
    memset(bases.data() + 12, 0, 96);
    XYZZ<F> g = xyzz_from_affine(load_point<F>(GEN1)), k = XYZZ<F>::inf();
    uint64_t mult[11][12];
    memset(mult[0], 0, 96);
    for (int i = 1; i <= 10; i++) { xyzz_add(k, g); store_point(mult[i], k); }
    const uint64_t rnd[12] = {5, 0, 0, 0, 3, 0, 0, 0, 7, 0, 0, 0};
    uint64_t given[48];
    const int have[4] = {5, 2, 0, 1}, want[4] = {10, 2, 5, 6};
    for (int c = 0; c < 4; c++) memcpy(given + 12 * c, mult[have[c]], 96);
    ballot<F, FR>(Key<F>(n, bases.data()), rnd, given, out);
    int bad = 0;
    for (int c = 0; c < 4; c++) bad |= memcmp(out + 12 * c, mult[want[c]], 96) != 0;
    delta<F2, FR>(GEN2, rnd, out2);
    XYZZ<F2> h = xyzz_from_affine(load_point<F2>(GEN2)), k2 = XYZZ<F2>::inf();
    for (int i = 0; i < 7; i++) xyzz_add(k2, h);
    uint64_t seven[24]; store_point(seven, k2);
    bad |= memcmp(out2, seven, 192) != 0;
    uint64_t rec[20]; FR pre;
    saver_rerand_scalars<FR>(rnd, 1, rec, &pre);
    bad |= rec[8] != 21 || rec[9] || rec[10] || rec[11];
    const FR one = mul(to_mont(load<FR>(rec + 4)), to_mont(load<FR>(rec + 12)));
    bad |= !eq(one, FR::one());
    unsigned longest = 0, span = 0;
    bad |= plan_shape(25, &longest, &span) || longest != 12 || span != 224;
    return bad;
}
int main() {
    uint64_t a32[48], a64[48], b32[24], b64[24];
    int bad = run<Fp, Fp2, Fr>(a32, b32) | run<HFp, HFp2, HFr>(a64, b64);
    bad |= memcmp(a32, a64, sizeof a32) != 0 || memcmp(b32, b64, sizeof b32) != 0;
    printf(bad ? "saver_rerand_check: FAILED\n" : "saver_rerand_check: ok\n");
    return bad;
}
#endif
