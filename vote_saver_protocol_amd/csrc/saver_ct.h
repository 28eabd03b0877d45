// The SAVER ciphertext as sums of fixed-base window terms (saver_batch.hip; include/vsp.h "SAVER ballots in batches"):
// everything about k_saver_ct that is not a launch -- the table layout, the digit of a scalar, which scalars meet which bases in which
// output column, the share of a column's terms that a lane adds up and the order in which a group of lanes folds its partial sums.
// Shared by the gfx950 kernel (32-bit limbs), by the host leg of the same call (option "saver_encrypt_gpu" = 0: one lane per column) and,
// through g++, by the CPU test build (tests/cpu_build/saver_ct_check.cpp, both limb types).
#pragma once
#include <stdint.h>
#include <vector>
#include "curve.h"

namespace vsp {

// THE TABLES.  Base b of a key with n = msg_size message blocks, 3 n + 3 in all:
//     X_0 .. X_{n+1} (delta_g1 | delta_s_g1[i] | delta_sum_s_g1)   b = 0 .. n + 1
//     P2 = gamma_inverse_sum_s_g1                                   b = n + 2
//     G_1 .. G_n (the message bases)                                b = n + 2 + i
//     Y_1 .. Y_n (t_g1[i])                                          b = 2 n + 2 + i
// each with 64 windows of 4 bits x 15 affine entries d 16^w P in Montgomery form (960 points, 92 160 bytes)
static constexpr unsigned SAVER_WINDOWS = 64, SAVER_ENTRIES = 15, SAVER_TABLE_POINTS = SAVER_WINDOWS * SAVER_ENTRIES;
VSP_HD size_t saver_bases(size_t n) { return 3 * n + 3; }
VSP_HD size_t saver_base_X(size_t i) { return i; }
VSP_HD size_t saver_base_P2(size_t n) { return n + 2; }
VSP_HD size_t saver_base_G(size_t n, size_t i) { return n + 2 + i; }
VSP_HD size_t saver_base_Y(size_t n, size_t i) { return 2 * n + 2 + i; }
VSP_HD size_t saver_table_index(size_t base, unsigned w, unsigned d) { return base * SAVER_TABLE_POINTS + w * SAVER_ENTRIES + d - 1; }      // d = 1 .. 15
// digit w (0 .. 63) of a canonical scalar of four 64-bit words
VSP_HD unsigned saver_digit(const uint64_t *k, unsigned w) { return (unsigned)(k[w >> 4] >> ((w & 15) * 4)) & 15u; }

// THE COLUMNS.  A ballot's scalars are r_enc (scalar 0) and m_1 .. m_n (scalars 1 .. n); its outputs are the n + 3 columns
//     0: c_0 = r X_0      i: c_i = r X_i + m_i G_i      n + 1: psi = r X_{n+1} + sum m_i Y_i      n + 2: the proof's addend r P2
// A column is a list of (scalar, base) pairs, and each pair stands for the 64 window terms (base, w, digit w of the scalar): term t of a
// column is window t % 64 of its pair t / 64.  `skip` marks a base at infinity.
struct SaverPair { uint16_t scalar, base; uint32_t skip; };
// A column is summed by a GROUP of `lanes` lanes (a power of two, 8 .. 64) that sit at lanes [lane0, lane0 + lanes) of the ballot's span
struct SaverColumn { uint32_t first_pair, pairs, lanes, lane0; };
VSP_HD size_t saver_columns(size_t n) { return n + 3; }
// The cost of a column is its longest DEPENDENT chain of additions -- a lone wave takes 11-16 us for one -- not its operation count: a
// group of L lanes makes it ceil(64 pairs / L) + log2(L).  L = terms / 8, within 8 .. 64: 8 + 3 for c_0 and the addend, 8 + 4 for c_i, and for
// psi 64 lanes x (n + 1) + 6, which is 32 at msg_size 25.
VSP_HD unsigned saver_group_lanes(unsigned pairs) {
    unsigned L = 8;
    while (L < 64 && L * 8 < pairs * SAVER_WINDOWS) L *= 2;
    return L;
}
// lane `lane` of a group of `lanes` adds up the terms lane, lane + lanes, lane + 2 lanes ...; madd_(XYZZ *, const Affine *) is the mixed
// addition, complete (curve.h xyzz_madd: equal operands double, opposite ones give infinity, infinity on either side); a zero digit has no term
template <class F, class Madd>
VSP_HD void saver_lane_sum(XYZZ<F> &acc, const Affine<F> *tab, const uint64_t *scalars, const SaverColumn &col, const SaverPair *pairs, unsigned lane, unsigned lanes, Madd madd_) {
    acc = XYZZ<F>::inf();
    const unsigned terms = col.pairs * SAVER_WINDOWS;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (unsigned t = lane; t < terms; t += lanes) {
        const SaverPair p = pairs[col.first_pair + t / SAVER_WINDOWS];
        const unsigned w = t % SAVER_WINDOWS, d = saver_digit(scalars + 4 * p.scalar, w);
        if (d && !p.skip) madd_(&acc, &tab[saver_table_index(p.base, w, d)]);
    }
}
// THE FOLD of a group's partial sums, in levels s = lanes / 2, lanes / 4 .. 1: at level s lane l in [s, 2 s) gives its sum away and lane
// l - s takes it (a full addition, complete as well); after level 1 lane 0 holds the column
VSP_HD bool saver_fold_gives(unsigned lane, unsigned lanes, unsigned s) { return s < lanes && lane >= s && lane < 2 * s; }
VSP_HD bool saver_fold_takes(unsigned lane, unsigned lanes, unsigned s) { return s < lanes && lane < s; }
#if defined(__HIPCC__)
// the fold in a kernel, through the block's LDS: part has a slot per thread (a group lies inside one wave, the barriers are the block's:
// EVERY thread of the block calls this, an idle one with lanes = 0).  A lane gives once: no slot is written twice, one barrier a level
template <class F> __device__ __forceinline__ void saver_fold_lds(XYZZ<F> &acc, XYZZ<F> *part, unsigned lane, unsigned lanes) {
#pragma unroll 1
    for (unsigned s = 32; s >= 1; s >>= 1) {
        if (saver_fold_gives(lane, lanes, s)) part[threadIdx.x] = acc;
        __syncthreads();
        if (saver_fold_takes(lane, lanes, s)) xyzz_add(acc, part[threadIdx.x + s]);
    }
}
#endif

// the columns of a key of n message blocks, the pairs behind them, and the column of every lane of a ballot's span (SAVER_NO_COLUMN: an
// idle lane).  Groups lie in the span by descending size, so none straddles a wave; the span is a whole number of waves.
static constexpr uint32_t SAVER_NO_COLUMN = 0xffffffffu;
struct SaverPlan {
    std::vector<SaverColumn> cols;
    std::vector<SaverPair> pairs;
    std::vector<uint32_t> lane_col;                 // lane_col.size() = the lanes of a ballot
};
// base_inf[b] != 0: base b is at infinity (may be null: none is)
inline SaverPlan saver_plan(size_t n, const uint8_t *base_inf) {
    SaverPlan pl;
    auto pair = [&](size_t scalar, size_t base) { pl.pairs.push_back(SaverPair{(uint16_t)scalar, (uint16_t)base, base_inf && base_inf[base] ? 1u : 0u}); };
    auto column = [&](size_t pairs) { pl.cols.push_back(SaverColumn{(uint32_t)(pl.pairs.size() - pairs), (uint32_t)pairs, saver_group_lanes((unsigned)pairs), 0}); };
    pair(0, saver_base_X(0)); column(1);
    for (size_t i = 1; i <= n; i++) { pair(0, saver_base_X(i)); pair(i, saver_base_G(n, i)); column(2); }
    pair(0, saver_base_X(n + 1));
    for (size_t i = 1; i <= n; i++) pair(i, saver_base_Y(n, i));
    column(n + 1);
    pair(0, saver_base_P2(n)); column(1);
    for (unsigned L = 64; L >= 8; L /= 2)
        for (size_t c = 0; c < pl.cols.size(); c++)
            if (pl.cols[c].lanes == L) { pl.cols[c].lane0 = (uint32_t)pl.lane_col.size(); pl.lane_col.insert(pl.lane_col.end(), L, (uint32_t)c); }
    pl.lane_col.resize((pl.lane_col.size() + 63) / 64 * 64, SAVER_NO_COLUMN);
    return pl;
}

}  // namespace vsp
