// CPU test build of the batch ciphertext's arithmetic (vote_saver_protocol_amd/csrc/saver_ct.h: the column descriptions, the lanes'
// shares of a column's terms and the fold order, compiled by g++ with the 32-bit-limb type the kernel uses and with the host's 64-bit-limb
// type).  Test infrastructure only.  All arguments canonical little-endian u64 limbs: a G1 point x | y (12 words, all zero = infinity),
// a scalar 4 words.  With -DSAVER_CT_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_saver_ct_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/saver_ct.h"
using namespace vsp;

template <class T> static T load(const uint64_t *p) { T t; memcpy(&t, p, sizeof(T)); return t; }
template <class T> static void store(uint64_t *p, const T &t) { memcpy(p, &t, sizeof(T)); }
template <class F> static Affine<F> load_point(const uint64_t *p) { Affine<F> a; a.x = to_mont(load<F>(p)); a.y = to_mont(load<F>(p + 6)); return a; }
template <class F> static void store_point(uint64_t *p, const XYZZ<F> &s) { const Affine<F> a = xyzz_to_affine(s); store(p, from_mont(a.x)); store(p + 6, from_mont(a.y)); }

// the table of every base in the layout of saver_ct.h: d 16^w P by repeated addition, a base's 960 entries made affine through one
// inversion (nothing of the library's own table build)
template <class F> static std::vector<Affine<F>> tables(const uint64_t *bases, size_t nb, std::vector<uint8_t> &inf) {
    Affine<F> zero; zero.x = F::zero(); zero.y = F::zero();
    std::vector<Affine<F>> tab(nb * SAVER_TABLE_POINTS, zero);
    inf.assign(nb, 0);
    for (size_t b = 0; b < nb; b++) {
        const Affine<F> P = load_point<F>(bases + 12 * b);
        inf[b] = is_inf(P);
        if (inf[b]) continue;
        std::vector<XYZZ<F>> pts(SAVER_TABLE_POINTS);
        std::vector<F> pre(SAVER_TABLE_POINTS);
        XYZZ<F> step = xyzz_from_affine(P);
        F run = F::one();
        for (unsigned w = 0; w < SAVER_WINDOWS; w++) {
            XYZZ<F> acc = step;
            for (unsigned d = 1; d <= SAVER_ENTRIES; d++) {
                const size_t i = saver_table_index(0, w, d);
                pts[i] = acc; pre[i] = run; run = mul(run, acc.ZZZ);
                xyzz_add(acc, step);
            }
            step = acc;
        }
        F ri = inv(run);
        for (size_t i = SAVER_TABLE_POINTS; i-- > 0;) {
            const F zi3 = mul(ri, pre[i]), zi = mul(zi3, pts[i].ZZ);          // 1 / ZZZ_i, 1 / Z_i
            ri = mul(ri, pts[i].ZZZ);
            tab[b * SAVER_TABLE_POINTS + i].x = mul(pts[i].X, sqr(zi)); tab[b * SAVER_TABLE_POINTS + i].y = mul(pts[i].Y, zi3);
        }
    }
    return tab;
}
// a key: the tables of its 3 n + 3 fixed points (bases, in the order of saver_ct.h) and the plan over them
template <class F> struct Key {
    size_t n; std::vector<Affine<F>> tab; SaverPlan plan;
    Key(size_t n_, const uint64_t *bases) : n(n_) { std::vector<uint8_t> inf; tab = tables<F>(bases, saver_bases(n), inf); plan = saver_plan(n, inf.data()); }
};
// one ballot as the lane groups of k_saver_ct compute it: scalars = r_enc | m_1 .. m_n; out = the n + 3 columns.  Every lane sums its
// share; the group folds level by level, gives before takes as the barrier orders them
template <class F> static void ballot(const Key<F> &key, const uint64_t *scalars, uint64_t *out) {
    const SaverPlan &pl = key.plan;
    auto madd_ = [](XYZZ<F> *a, const Affine<F> *q) { xyzz_madd(*a, *q); };
    for (size_t c = 0; c < pl.cols.size(); c++) {
        const SaverColumn &col = pl.cols[c];
        std::vector<XYZZ<F>> acc(col.lanes), part(col.lanes);
        for (unsigned l = 0; l < col.lanes; l++) saver_lane_sum(acc[l], key.tab.data(), scalars, col, pl.pairs.data(), l, col.lanes, madd_);
        for (unsigned s = 32; s >= 1; s >>= 1) {
            for (unsigned l = 0; l < col.lanes; l++) if (saver_fold_gives(l, col.lanes, s)) part[l] = acc[l];
            for (unsigned l = 0; l < col.lanes; l++) if (saver_fold_takes(l, col.lanes, s)) xyzz_add(acc[l], part[l + s]);
        }
        store_point(out + 12 * c, acc[0]);
    }
}
// the plan's shape: 0 when every column's group lies inside one wave of the ballot's span, no two groups overlap, the span is a whole
// number of waves and every lane names its column; *longest = the longest dependent chain of additions (a lane's terms + the fold's levels)
static int plan_shape(size_t n, unsigned *longest, unsigned *span) {
    const SaverPlan pl = saver_plan(n, nullptr);
    int bad = pl.cols.size() != saver_columns(n) || pl.pairs.size() != saver_bases(n) || pl.lane_col.size() % 64 != 0;
    std::vector<unsigned> seen(pl.cols.size(), 0);
    for (size_t l = 0; l < pl.lane_col.size(); l++) {
        const uint32_t c = pl.lane_col[l];
        if (c == SAVER_NO_COLUMN) continue;
        bad |= c >= pl.cols.size() || l < pl.cols[c].lane0 || l >= pl.cols[c].lane0 + pl.cols[c].lanes;
        if (c < pl.cols.size()) seen[c]++;
    }
    *longest = 0;
    for (size_t c = 0; c < pl.cols.size(); c++) {
        const SaverColumn &col = pl.cols[c];
        bad |= seen[c] != col.lanes || (col.lanes & (col.lanes - 1)) || col.lanes < 8 || col.lanes > 64 || col.lane0 / 64 != (col.lane0 + col.lanes - 1) / 64;
        unsigned levels = 0;
        while ((1u << levels) < col.lanes) levels++;
        const unsigned chain = (col.pairs * SAVER_WINDOWS + col.lanes - 1) / col.lanes + levels;
        if (chain > *longest) *longest = chain;
    }
    *span = (unsigned)pl.lane_col.size();
    return bad;
}

extern "C" {
void *chk_key(size_t n, const uint64_t *bases) { return new Key<Fp>(n, bases); }
void *chk_hkey(size_t n, const uint64_t *bases) { return new Key<HFp>(n, bases); }
void chk_key_free(void *k) { delete (Key<Fp> *)k; }
void chk_hkey_free(void *k) { delete (Key<HFp> *)k; }
void chk_ballot(const void *key, const uint64_t *scalars, uint64_t *out) { ballot(*(const Key<Fp> *)key, scalars, out); }
void chk_hballot(const void *key, const uint64_t *scalars, uint64_t *out) { ballot(*(const Key<HFp> *)key, scalars, out); }
int chk_plan_shape(size_t n, unsigned *longest, unsigned *span) { return plan_shape(n, longest, span); }
unsigned chk_digit(const uint64_t *k, unsigned w) { return saver_digit(k, w); }
}

#ifdef SAVER_CT_CHECK_MAIN
#include <stdio.h>
static const uint64_t GEN1[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                  0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
// msg_size 2 with every base the generator but X_1, which is at infinity: r_enc = 5 and m = (3, 0) give c_0 = 5 G, c_1 = 3 G (X_1
// skipped), c_2 = 5 G, psi = 5 G + 3 G = 8 G and the addend 5 G -- for both limb types, which must agree on the bytes
template <class F> static int run(uint64_t *out) {
    const size_t n = 2;
    std::vector<uint64_t> bases(12 * saver_bases(n));
    for (size_t b = 0; b < saver_bases(n); b++) memcpy(bases.data() + 12 * b, GEN1, sizeof GEN1);
    memset(bases.data() + 12 * saver_base_X(1), 0, 96);
    const uint64_t scalars[12] = {5, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0};
    ballot(Key<F>(n, bases.data()), scalars, out);
    XYZZ<F> g = xyzz_from_affine(load_point<F>(GEN1)), k = XYZZ<F>::inf();
    uint64_t mult[9][12];
    for (int i = 1; i <= 8; i++) { xyzz_add(k, g); store_point(mult[i], k); }
    int bad = 0;
    const int want[5] = {5, 3, 5, 8, 5};
    for (int c = 0; c < 5; c++) bad |= memcmp(out + 12 * c, mult[want[c]], 96) != 0;
    unsigned longest = 0, span = 0;
    bad |= plan_shape(25, &longest, &span) || longest > 32 || span != 512;
    return bad;
}
int main() {
    uint64_t m32[60], m64[60];
    int bad = run<Fp>(m32) | run<HFp>(m64);
    bad |= memcmp(m32, m64, sizeof m32) != 0;
    printf(bad ? "saver_ct_check: FAILED\n" : "saver_ct_check: ok\n");
    return bad;
}
#endif
