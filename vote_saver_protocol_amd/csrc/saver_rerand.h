// Rerandomization of SAVER ballots in batches (saver_rerand.hip; include/vsp.h "SAVER ballots in batches"): everything
// about the call that is not a launch -- which scalars meet which tables in which column, where the member's own point joins a column,
// a ballot's record of scalars with its shared inversion, and the table of a fixed point of either group.  Built on saver_ct.h: the
// columns are SaverPlans, summed by saver_lane_sum and folded in its order.  Shared by the gfx950 kernels (32-bit limbs), by the host
// side of the same call (the scalars, the delta_g2 table) and, through g++, by the CPU test build (tests/cpu_build/saver_rerand_check.cpp).
#pragma once
#include <string.h>
#include "saver_ct.h"

namespace vsp {

// THE SCALARS of a ballot, five canonical values of four words: rnd = (r', z1, z2) as given and the two derived ones
//     0: r'     1: z1     2: z1 z2     3: 1 / z1     4: z2
static constexpr unsigned RR_SCALARS = 5, RR_R = 0, RR_Z1 = 1, RR_ZZ = 2, RR_ZINV = 3, RR_Z2 = 4;
// records of `count` ballots from their rnd (count x 12 words, every z1 non-zero and everything below r: the caller checks).  ONE
// inversion for all of them: run_k = z1_0 .. z1_{k-1}, 1 / z1_k = run_k / run_{k+1}, walked back from 1 / run_count.  FR: Mont<FrP64> or
// Mont<FrP32>.  pre: count values of scratch
template <class FR> inline void saver_rerand_scalars(const uint64_t *rnd, size_t count, uint64_t *rec, FR *pre) {
    auto load = [](const uint64_t *p) { FR t; memcpy(&t, p, 32); return to_mont(t); };
    auto store = [](uint64_t *p, const FR &m) { const FR t = from_mont(m); memcpy(p, &t, 32); };
    FR run = FR::one();
    for (size_t k = 0; k < count; k++) { pre[k] = run; run = mul(run, load(rnd + 12 * k + 4)); }
    FR ri = inv(run);
    for (size_t k = count; k-- > 0;) {
        const uint64_t *r = rnd + 12 * k;
        uint64_t *o = rec + 4 * RR_SCALARS * k;
        const FR z1 = load(r + 4);
        memcpy(o + 4 * RR_R, r, 32); memcpy(o + 4 * RR_Z1, r + 4, 32); memcpy(o + 4 * RR_Z2, r + 8, 32);
        store(o + 4 * RR_ZZ, mul(z1, load(r + 8)));
        store(o + 4 * RR_ZINV, mul(ri, pre[k]));
        ri = mul(ri, z1);
    }
}

// THE COLUMNS in G1, n + 3 of one pair each over the key's tables (saver_ct.h: base c is X_c for c <= n + 1 and P2 for c = n + 2):
//     c = 0 .. n + 1: ct_c + r' X_c          c = n + 2: C + r' P2, the fixed part of C'
// and in G2 one column over the one table of the rerandomizer: z2 delta_g2.  A pair is 64 terms, so a group is 8 lanes and a chain
// 8 + 3 additions and the given point's.  Every group has 8 lanes and lies at a multiple of 8 in a ballot's span, which is a multiple
// of 8 too: laid end to end the spans keep every group inside one wave, so a span needs no filling up to whole waves.
VSP_HD size_t saver_rerand_columns(size_t n) { return n + 3; }
inline SaverPlan saver_rerand_plan(size_t n, const uint8_t *base_inf) {
    SaverPlan pl;
    for (size_t c = 0; c < saver_rerand_columns(n); c++) {
        pl.pairs.push_back(SaverPair{(uint16_t)RR_R, (uint16_t)c, base_inf && base_inf[c] ? 1u : 0u});
        pl.cols.push_back(SaverColumn{(uint32_t)c, 1u, saver_group_lanes(1), (uint32_t)pl.lane_col.size()});
        pl.lane_col.insert(pl.lane_col.end(), pl.cols[c].lanes, (uint32_t)c);
    }
    return pl;
}
inline SaverPlan saver_rerand_delta_plan(bool delta_inf) {
    SaverPlan pl;
    pl.pairs.push_back(SaverPair{(uint16_t)RR_Z2, 0, delta_inf ? 1u : 0u});
    pl.cols.push_back(SaverColumn{0u, 1u, saver_group_lanes(1), 0u});
    pl.lane_col.assign(pl.cols[0].lanes, 0u);
    return pl;
}
// THE GIVEN POINT.  A ballot's given points lie in the order of its G1 outputs: ct_0 .. ct_{n+1} | C | A, so column c starts from given
// point c.  After the fold lane 0 of the group holds the table's share of the column and adds the given point to it by the complete
// mixed addition (ct_i = r' X_i doubles, ct_i = -r' X_i gives infinity, either side may be infinity)
VSP_HD size_t saver_rerand_given(size_t n) { return n + 4; }
VSP_HD size_t saver_rerand_given_C(size_t n) { return n + 2; }
VSP_HD size_t saver_rerand_given_A(size_t n) { return n + 3; }
template <class F, class Madd> VSP_HD void saver_rerand_join(XYZZ<F> &acc, const Affine<F> *given, Madd madd_) { if (given) madd_(&acc, given); }

// the table of one fixed point in the layout of saver_ct.h, tab[saver_table_index(0, w, d)] = d 16^w P for d = 1 .. 15, w = 0 .. 63 as
// affine Montgomery points through one inversion; false (and nothing written) for P at infinity.  As for the key's tables P is in the
// order-r subgroup: a multiple at infinity does not survive the shared inversion
template <class F> inline bool saver_fixed_table(const Affine<F> &P, Affine<F> *tab) {
    if (is_inf(P)) return false;
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
        step = acc;                                                 // 16 * step
    }
    F ri = inv(run);
    for (size_t i = SAVER_TABLE_POINTS; i-- > 0;) {
        const F zi3 = mul(ri, pre[i]), zi = mul(zi3, pts[i].ZZ);    // 1 / ZZZ_i, 1 / Z_i
        ri = mul(ri, pts[i].ZZZ);
        tab[i].x = mul(pts[i].X, sqr(zi)); tab[i].y = mul(pts[i].Y, zi3);
    }
    return true;
}

}  // namespace vsp
