// Rerandomization of SAVER ballots in batches (include/vsp.h "SAVER ballots in batches"): what the ballot box does to every
// ballot it receives, for a whole piece of them at a time.
//
//     ct_i' = ct_i + r' X_i      A' = z1 A      B' = z1^-1 B + z2 delta_g2      C' = C + (z1 z2) A + r' P2
//
// saver_rerand.h has the columns, the scalars' shared inversion and the table of delta_g2; this file has the kernels and the call.  Stages
// per piece, all on the context's stream:
//   0. k_rr_check<G1>, <G2>   one lane per input point: coordinates below p, Montgomery form, on the curve or all zero; a status word per ballot
//   1. k_rr_columns<Fp>       the n + 3 fixed-base columns over the key's tables, 8 lanes each; lane 0 adds the ballot's own ct_i or C
//      k_rr_columns<Fp2>      z2 delta_g2 over the rerandomizer's table
//   2. k_rr_affine            ct' as canonical affine words: one lane and one inversion per ballot
//   3. k_rr_mul<Fp>           two lanes per ballot: z1 A -> A', and (z1 z2) A + column n + 2 -> C'
//      k_rr_mul<Fp2>          one lane per ballot: z1^-1 B + the delta column -> B'
// G1 lanes and G2 lanes never share a wave.  The scalars z1 z2 and 1 / z1 come from the host, one inversion per piece.
#include "common.h"
#include "fp12.h"

struct vsp_saver_rerandomizer {
    vsp_saver_pk *spk = nullptr;
    int device = 0;
    size_t n = 0;
    vsp::SaverPlan plan, plan2;             // the G1 columns over the key's tables, the G2 column over d_tab2
    vsp::DevBuf d_desc, d_desc2, d_tab2;    // a plan on the device: columns | pairs | lane_col
    size_t device_bytes = 0;
};

namespace vsp {
namespace {

static constexpr unsigned RR_THREADS = 64;
static constexpr size_t RR_CHUNK_MAX = (size_t)1 << 16, RR_CHUNK_DEFAULT = RR_CHUNK_MAX;      // profiles/saver_rerandomize_time.txt: 2^16 over 2^14, 616 against 375 thousand ballots/s

// the group law as real calls on memory operands, one copy of each body in a kernel (as pairing_g1.h's pr_dbl and pr_madd, for either group)
template <class F> __device__ __noinline__ void rr_dbl(XYZZ<F> *a) { *a = xyzz_dbl(*a); }
template <class F> __device__ __noinline__ void rr_add(XYZZ<F> *a, const XYZZ<F> *b) { XYZZ<F> t = *a; xyzz_add(t, *b); *a = t; }
template <class F> __device__ __noinline__ void rr_madd(XYZZ<F> *a, const Affine<F> *p) { XYZZ<F> t = *a; xyzz_madd(t, *p); *a = t; }
__device__ __forceinline__ Fp rr_inv(const Fp &a) { return fp_inv_chain(a); }
__device__ __forceinline__ Fp2 rr_inv(const Fp2 &a) { return f2inv(a); }
__device__ __forceinline__ Fp rr_curve_b(const Fp *) { return dbl(dbl(Fp::one())); }
__device__ __forceinline__ Fp2 rr_curve_b(const Fp2 *) { Fp2 b; b.c0 = dbl(dbl(Fp::one())); b.c1 = b.c0; return b; }
// canonical affine words of a sum through one inversion, 1 / (ZZ ZZZ); infinity (ZZ = 0) comes out all zero
template <class F> __device__ __noinline__ void rr_store_affine(const XYZZ<F> *acc, Affine<F> *out) {
    const F t = rr_inv(mul(acc->ZZ, acc->ZZZ));
    Affine<F> P;
    P.x = from_mont(mul(acc->X, mul(t, acc->ZZZ)));
    P.y = from_mont(mul(acc->Y, mul(t, acc->ZZ)));
    *out = P;
}
// canonical words -> Montgomery affine point; 0 accepted (infinity included), 1 a coordinate >= p, 2 off the curve.  A rejected point
// comes out as infinity
template <class F> __device__ __noinline__ uint32_t rr_load(const uint64_t *src, Affine<F> *out) {
    const Affine<F> c = *(const Affine<F> *)src;
    uint32_t st = (canon_below_p(c.x) && canon_below_p(c.y)) ? 0u : 1u;
    Affine<F> p; p.x = to_mont(c.x); p.y = to_mont(c.y);
    if (!st && !is_inf(c) && !eq(sqr(p.y), add(mul(sqr(p.x), p.x), rr_curve_b((const F *)nullptr)))) st = 2u;
    if (st) { p.x = F::zero(); p.y = F::zero(); }
    *out = p;
    return st;
}

// stage 0.  words: `per` canonical points of a ballot in a row; point j of ballot k -> out[k * per + j]; a rejected one raises its ballot's status
template <class F> __global__ __launch_bounds__(RR_THREADS) void k_rr_check(const uint64_t *__restrict__ words, size_t per, size_t count, Affine<F> *__restrict__ out,
                                                                           uint32_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (i >= per * count) return;
    Affine<F> P;
    const uint32_t st = rr_load<F>(words + i * (sizeof(Affine<F>) / 8), &P);
    out[i] = P;
    if (st) atomicOr(&status[i / per], 1u);
}

// stage 1.  k_saver_ct's lane groups over another plan (saver_ct.h saver_lane_sum, saver_fold_lds); then lane 0 of a group adds the ballot's
// own point of that column (given: `given_per` points a ballot, column c starts from point c; null: no given point).  A ballot's scalars
// are its record of RR_SCALARS values.  sums[ballot][column] = the column in XYZZ
template <class F, unsigned BLOCK>
__global__ __launch_bounds__(BLOCK) void k_rr_columns(const Affine<F> *__restrict__ tab, const SaverColumn *__restrict__ cols, const SaverPair *__restrict__ pairs,
                                                      const uint32_t *__restrict__ lane_col, unsigned ballot_lanes, unsigned n_cols, const uint64_t *__restrict__ scalars,
                                                      const Affine<F> *__restrict__ given, unsigned given_per, size_t count, XYZZ<F> *__restrict__ sums) {
    __shared__ XYZZ<F> part[BLOCK];
    const size_t g = (size_t)blockIdx.x * BLOCK + threadIdx.x, ballot = g / ballot_lanes;
    const uint32_t c = ballot < count ? lane_col[g % ballot_lanes] : SAVER_NO_COLUMN;
    unsigned lane = 0, lanes = 0;
    XYZZ<F> acc = XYZZ<F>::inf();
    if (c != SAVER_NO_COLUMN) {
        const SaverColumn col = cols[c];
        lanes = col.lanes; lane = (unsigned)(g % ballot_lanes) - col.lane0;
        saver_lane_sum(acc, tab, scalars + ballot * RR_SCALARS * 4, col, pairs, lane, lanes, [](XYZZ<F> *a, const Affine<F> *q) { rr_madd(a, q); });
    }
    saver_fold_lds(acc, part, lane, lanes);
    if (lanes && lane == 0) {
        saver_rerand_join(acc, given ? given + ballot * given_per + c : nullptr, [](XYZZ<F> *a, const Affine<F> *q) { rr_madd(a, q); });
        sums[ballot * n_cols + c] = acc;
    }
}

// stage 2.  the first `per` of a ballot's n_cols column sums -> the first `per` of its out_per output points, canonical.  One lane per
// ballot and ONE inversion for its points, as in the single call: with t_c = ZZ_c ZZZ_c (a sum at infinity counts as one) the lane leaves
// t_0 .. t_{c-1} in point c's x slot on the way up, inverts the whole product and on the way down takes 1 / t_c = that slot times
// 1 / (t_0 .. t_c); x = X ZZZ / t, y = Y ZZ / t
__global__ __launch_bounds__(RR_THREADS) void k_rr_affine(const G1XYZZ *__restrict__ sums, unsigned n_cols, unsigned per, unsigned out_per, size_t count, G1Affine *__restrict__ out) {
    const size_t ballot = (size_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (ballot >= count) return;
    const G1XYZZ *s = sums + ballot * n_cols;
    G1Affine *o = out + ballot * out_per;
    Fp run = Fp::one();
#pragma unroll 1
    for (unsigned c = 0; c < per; c++) {
        o[c].x = run;
        const Fp zz = s[c].ZZ;
        if (!is_zero(zz)) run = mul(run, mul(zz, s[c].ZZZ));
    }
    Fp ri = fp_inv_chain(run);
#pragma unroll 1
    for (unsigned c = per; c-- > 0;) {
        const G1XYZZ p = s[c];
        G1Affine a; a.x = Fp::zero(); a.y = Fp::zero();
        if (!is_zero(p.ZZ)) {
            const Fp ti = mul(ri, o[c].x);
            ri = mul(ri, mul(p.ZZ, p.ZZZ));
            a.x = from_mont(mul(p.X, mul(ti, p.ZZZ)));
            a.y = from_mont(mul(p.Y, mul(ti, p.ZZ)));
        }
        o[c] = a;
    }
}

// k * P for a canonical scalar of eight 32-bit words: 4-bit windows from the top (a table of 14 additions, then 4 doublings and at most
// one addition a window: 252 + 14 + 64) or bit by bit (255 doublings, an addition per set bit) -- curve.h xyzz_mul_scalar_w4 and
// xyzz_mul_scalar as calls.  Every step is complete, so P may be any curve point
template <class F> __device__ __forceinline__ void rr_mul_w4(XYZZ<F> &acc, const Affine<F> &P, const uint32_t *k) {
    XYZZ<F> tab[16];
    tab[0] = XYZZ<F>::inf(); tab[1] = xyzz_from_affine(P);
#pragma unroll 1
    for (int d = 2; d < 16; d++) {
        if (d & 1) { tab[d] = tab[d - 1]; rr_add(&tab[d], &tab[1]); }
        else { tab[d] = tab[d >> 1]; rr_dbl(&tab[d]); }
    }
    acc = XYZZ<F>::inf();
#pragma unroll 1
    for (int w = 63; w >= 0; w--) {
        if (w != 63) { rr_dbl(&acc); rr_dbl(&acc); rr_dbl(&acc); rr_dbl(&acc); }
        const uint32_t d = (k[w >> 3] >> ((w & 7) * 4)) & 15u;
        if (d) rr_add(&acc, &tab[d]);
    }
}
template <class F> __device__ __forceinline__ void rr_mul_bits(XYZZ<F> &acc, const Affine<F> &P, const uint32_t *k) {
    acc = XYZZ<F>::inf();
#pragma unroll 1
    for (int i = 254; i >= 0; i--) {
        rr_dbl(&acc);
        if ((k[i >> 5] >> (i & 31)) & 1u) rr_madd(&acc, &P);
    }
}
// stage 3.  Task t of a piece: ballot t / per, scalar s0 + t % per of its record times its base point (base[ballot * base_per + base_at]);
// the LAST task of a ballot adds addend[ballot * addend_per + addend_at]; the product leaves as canonical affine words at
// out[ballot * out_per + out_at - t % per].  G1 (per 2, s0 = RR_Z1): z1 A -> A' and (z1 z2) A + column n + 2 -> C', the slot before A'.
// G2 (per 1, s0 = RR_ZINV): z1^-1 B + the delta column -> B'
template <class F> __global__ __launch_bounds__(RR_THREADS) void k_rr_mul(const Affine<F> *__restrict__ base, unsigned base_per, unsigned base_at, const uint64_t *__restrict__ scalars,
                                                                         unsigned s0, unsigned per, const XYZZ<F> *__restrict__ addend, unsigned addend_per, unsigned addend_at,
                                                                         size_t count, int w4, Affine<F> *__restrict__ out, unsigned out_per, unsigned out_at) {
    const size_t t = (size_t)blockIdx.x * RR_THREADS + threadIdx.x;
    if (t >= (size_t)per * count) return;
    const size_t ballot = t / per;
    const unsigned j = (unsigned)(t % per);
    const Affine<F> P = base[ballot * base_per + base_at];
    uint32_t k[8];
    const uint4 *ks = (const uint4 *)(scalars + (ballot * RR_SCALARS + s0 + j) * 4);
    const uint4 lo = ks[0], hi = ks[1];
    k[0] = lo.x; k[1] = lo.y; k[2] = lo.z; k[3] = lo.w; k[4] = hi.x; k[5] = hi.y; k[6] = hi.z; k[7] = hi.w;
    XYZZ<F> acc;
    if (w4) rr_mul_w4(acc, P, k); else rr_mul_bits(acc, P, k);
    if (j == per - 1) { const XYZZ<F> a = addend[ballot * addend_per + addend_at]; rr_add(&acc, &a); }
    rr_store_affine(&acc, &out[ballot * out_per + out_at - j]);
}

template <class F> static void launch_columns(hipStream_t st, const void *d_tab, const void *d_desc, const SaverPlan &pl, const uint64_t *d_scalars, const void *d_given, unsigned given_per,
                                              size_t c, void *d_sums) {
    constexpr unsigned BLOCK = sizeof(XYZZ<F>) > 192 ? 128 : 256;           // 48 KB of LDS either way
    const SaverColumn *d_cols = (const SaverColumn *)d_desc;
    const SaverPair *d_pairs = (const SaverPair *)(d_cols + pl.cols.size());
    const uint32_t *d_lane_col = (const uint32_t *)(d_pairs + pl.pairs.size());
    const unsigned ballot_lanes = (unsigned)pl.lane_col.size();
    hipLaunchKernelGGL((k_rr_columns<F, BLOCK>), dim3((unsigned)((c * ballot_lanes + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, (const Affine<F> *)d_tab, d_cols, d_pairs, d_lane_col,
                       ballot_lanes, (unsigned)pl.cols.size(), d_scalars, (const Affine<F> *)d_given, given_per, c, (XYZZ<F> *)d_sums);
}

// THE PIECE.  At most "saver_rerandomize_chunk" ballots (option, default and maximum 2^16) go through the kernels at a time.  Per ballot
// on the device: 96 (n + 4) + 192 bytes of canonical words (the inputs, then the outputs), 160 of scalars, 96 (n + 4) + 192 of Montgomery
// points, 192 (n + 3) + 384 of column sums and a status word; in pinned memory the words and scalars going in and the words and status
// coming back
static size_t piece_ballots(const vsp_ctx *ctx) { const long c = opt(ctx, "saver_rerandomize_chunk", (long)RR_CHUNK_DEFAULT); return c < 1 ? 1 : ((size_t)c > RR_CHUNK_MAX ? RR_CHUNK_MAX : (size_t)c); }

// c ballots from ballot `at` on: staged, through the kernels, back in pinned memory (h_out: c x (n + 4) G1 points | c G2 points | c status words)
static int rr_piece(vsp_ctx *ctx, const vsp_saver_rerandomizer *rr, const uint64_t *rnd, const uint64_t *ct, const uint64_t *A, const uint64_t *B, const uint64_t *C, size_t at, size_t c,
                    std::vector<HFr> &pre) {
    auto &w = ctx->saver_rr;
    const vsp_saver_pk *spk = rr->spk;
    const size_t n = rr->n, ng = saver_rerand_given(n), nc = saver_rerand_columns(n), ctw = (n + 2) * 12;
    const size_t g1_bytes = c * ng * sizeof(G1Affine), g2_bytes = c * sizeof(G2Affine), sc_bytes = c * RR_SCALARS * 32;
    hipStream_t st = ctx->stream;
    VSP_TRY(ensure(ctx, w.words, g1_bytes + g2_bytes));
    VSP_TRY(ensure(ctx, w.scalars, sc_bytes));
    VSP_TRY(ensure(ctx, w.given, g1_bytes));
    VSP_TRY(ensure(ctx, w.b_in, g2_bytes));
    VSP_TRY(ensure(ctx, w.sums, c * nc * sizeof(G1XYZZ)));
    VSP_TRY(ensure(ctx, w.sums2, c * sizeof(G2XYZZ)));
    VSP_TRY(ensure(ctx, w.status, c * sizeof(uint32_t)));
    VSP_TRY(ensure_pinned(ctx, w.h_in, g1_bytes + g2_bytes + sc_bytes));
    VSP_TRY(ensure_pinned(ctx, w.h_out, g1_bytes + g2_bytes + c * sizeof(uint32_t)));
    // the given points of a ballot in the order of its G1 outputs: ct | C | A; then every B; then the scalar records
    uint64_t *h1 = w.h_in.as<uint64_t>(), *h2 = h1 + c * ng * 12, *hs = h2 + c * 24;
    host_parallel_for(c, [&](size_t k) {
        uint64_t *row = h1 + k * ng * 12;
        memcpy(row, ct + (at + k) * ctw, ctw * 8);
        memcpy(row + 12 * saver_rerand_given_C(n), C + (at + k) * 12, 96);
        memcpy(row + 12 * saver_rerand_given_A(n), A + (at + k) * 12, 96);
    });
    memcpy(h2, B + at * 24, g2_bytes);
    pre.resize(c);
    saver_rerand_scalars<HFr>(rnd + at * 12, c, hs, pre.data());
    uint64_t *d_words = (uint64_t *)w.words.p, *d_words2 = d_words + c * ng * 12;
    VSP_HIP(hipMemcpyAsync(d_words, h1, g1_bytes + g2_bytes, hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemcpyAsync(w.scalars.p, hs, sc_bytes, hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemsetAsync(w.status.p, 0, c * sizeof(uint32_t), st));
    const int w4 = opt(ctx, "saver_rerandomize_w4", 1) != 0;
    const uint64_t *d_scal = (const uint64_t *)w.scalars.p;
    G1Affine *given = (G1Affine *)w.given.p, *out1 = (G1Affine *)d_words;
    G2Affine *b_in = (G2Affine *)w.b_in.p, *out2 = (G2Affine *)d_words2;
    auto blocks = [](size_t lanes) { return dim3((unsigned)((lanes + RR_THREADS - 1) / RR_THREADS)); };
    VSP_TRY(w.timer[0].mark(ctx, 0, st));
    hipLaunchKernelGGL(k_rr_check<Fp>, blocks(c * ng), dim3(RR_THREADS), 0, st, (const uint64_t *)d_words, ng, c, given, (uint32_t *)w.status.p);
    VSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_rr_check<Fp2>, blocks(c), dim3(RR_THREADS), 0, st, (const uint64_t *)d_words2, (size_t)1, c, b_in, (uint32_t *)w.status.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer[0].mark(ctx, 1, st));
    launch_columns<Fp>(st, spk->d_tab.p, rr->d_desc.p, rr->plan, d_scal, given, (unsigned)ng, c, w.sums.p);
    VSP_LAUNCH_CHECK();
    launch_columns<Fp2>(st, rr->d_tab2.p, rr->d_desc2.p, rr->plan2, d_scal, nullptr, 0, c, w.sums2.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer[0].mark(ctx, 2, st));
    // from here on the canonical inputs are dead: the outputs take their place
    hipLaunchKernelGGL(k_rr_affine, blocks(c), dim3(RR_THREADS), 0, st, (const G1XYZZ *)w.sums.p, (unsigned)nc, (unsigned)(n + 2), (unsigned)ng, c, out1);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer[0].mark(ctx, 3, st));
    VSP_TRY(w.timer[1].mark(ctx, 0, st));
    hipLaunchKernelGGL(k_rr_mul<Fp>, blocks(2 * c), dim3(RR_THREADS), 0, st, (const G1Affine *)given, (unsigned)ng, (unsigned)saver_rerand_given_A(n), d_scal, RR_Z1, 2u,
                       (const G1XYZZ *)w.sums.p, (unsigned)nc, (unsigned)(n + 2), c, w4, out1, (unsigned)ng, (unsigned)saver_rerand_given_A(n));
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer[1].mark(ctx, 1, st));
    hipLaunchKernelGGL(k_rr_mul<Fp2>, blocks(c), dim3(RR_THREADS), 0, st, (const G2Affine *)b_in, 1u, 0u, d_scal, RR_ZINV, 1u, (const G2XYZZ *)w.sums2.p, 1u, 0u, c, w4, out2, 1u, 0u);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer[1].mark(ctx, 2, st));
    VSP_HIP(hipMemcpyAsync(w.h_out.p, d_words, g1_bytes + g2_bytes, hipMemcpyDeviceToHost, st));
    VSP_HIP(hipMemcpyAsync(w.h_out.as<char>() + g1_bytes + g2_bytes, w.status.p, c * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    w.timer[0].add(ctx, 0, "saver_rerandomize_check_ms"); w.timer[0].add(ctx, 1, "saver_rerandomize_columns_ms"); w.timer[0].add(ctx, 2, "saver_rerandomize_affine_ms");
    w.timer[1].add(ctx, 0, "saver_rerandomize_g1_ms"); w.timer[1].add(ctx, 1, "saver_rerandomize_g2_ms");
    float ms = 0;
    if (hipEventElapsedTime(&ms, w.timer[0].ev[0], w.timer[1].ev[2]) == hipSuccess) ctx->stats["saver_rerandomize_ms"] += ms;
    return VSP_OK;
}

}  // anonymous namespace

}  // namespace vsp

using namespace vsp;
extern "C" {

vsp_saver_rerandomizer *vsp_saver_rerandomizer_new(vsp_ctx *ctx, vsp_saver_pk *spk, const uint64_t delta_g2[24]) {
    if (!ctx) return nullptr;
    if (!spk || !delta_g2) { set_error(ctx, VSP_ERR_ARG, "saver_rerandomizer_new: null argument"); return nullptr; }
    if (!affine_valid<G2>(delta_g2)) { set_error(ctx, VSP_ERR_ARG, "saver_rerandomizer_new: delta_g2 is not a curve point"); return nullptr; }
    if (vsp_saver_pk_upload(ctx, spk) != VSP_OK) return nullptr;
    std::unique_ptr<vsp_saver_rerandomizer> rr(new vsp_saver_rerandomizer());      // nothing has used its memory when a failure below lets it go
    rr->spk = spk; rr->device = ctx->device; rr->n = spk->n;
    const size_t n = spk->n;
    std::vector<uint8_t> base_inf(saver_rerand_columns(n), 0);
    for (size_t i = 0; i < n + 2; i++) base_inf[saver_base_X(i)] = spk->X[i].inf;
    base_inf[saver_base_P2(n)] = spk->P2.inf;
    rr->plan = saver_rerand_plan(n, base_inf.data());
    Affine<HFp2> zero; zero.x = HFp2::zero(); zero.y = HFp2::zero();
    std::vector<Affine<HFp2>> tab(SAVER_TABLE_POINTS, zero);
    rr->plan2 = saver_rerand_delta_plan(!saver_fixed_table(host_load_affine<HFp2>(delta_g2), tab.data()));
    // host Montgomery points and device ones are the same bytes
    static_assert(sizeof(Affine<HFp2>) == sizeof(G2Affine), "one table for the host and the device");
    const size_t tab_bytes = tab.size() * sizeof(G2Affine);
    if (hipSetDevice(ctx->device) != hipSuccess) { set_error(ctx, VSP_ERR_HIP, "saver_rerandomizer_new: hipSetDevice failed"); return nullptr; }
    if (rr->d_tab2.alloc(tab_bytes) != hipSuccess) { set_error(ctx, VSP_ERR_NOMEM, "saver_rerandomizer_new: hipMalloc of the delta_g2 table failed"); return nullptr; }
    if (const hipError_t e = hipMemcpy(rr->d_tab2.p, tab.data(), tab_bytes, hipMemcpyHostToDevice); e != hipSuccess) { set_hip_error(ctx, e, "hipMemcpy of the delta_g2 table", __FILE__, __LINE__); return nullptr; }
    if (upload_plan(ctx, rr->plan, rr->d_desc) != VSP_OK || upload_plan(ctx, rr->plan2, rr->d_desc2) != VSP_OK) return nullptr;
    rr->device_bytes = rr->d_tab2.cap + rr->d_desc.cap + rr->d_desc2.cap;
    return rr.release();
}
void vsp_saver_rerandomizer_free(vsp_ctx *, vsp_saver_rerandomizer *rr) {
    if (!rr) return;
    hipSetDevice(rr->device);
    hipDeviceSynchronize();                  // a context may still be reading the table
    delete rr;
}
size_t vsp_saver_rerandomizer_msg_size(const vsp_saver_rerandomizer *rr) { return rr ? rr->n : 0; }
size_t vsp_saver_rerandomizer_device_bytes(const vsp_saver_rerandomizer *rr) { return rr ? rr->device_bytes : 0; }

int vsp_saver_rerandomize_batch(vsp_ctx *ctx, const vsp_saver_rerandomizer *rr, const uint64_t *rnd, const uint64_t *ct, const uint64_t *A, const uint64_t *B, const uint64_t *C,
                                size_t count, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!rr || (count && (!rnd || !ct || !A || !B || !C))) return set_error(ctx, VSP_ERR_ARG, "saver_rerandomize_batch: null argument");
    if (ctx->prove.active && ctx->prove.batch) return set_error(ctx, VSP_ERR_ARG, "saver_rerandomize_batch: a batch of ballots or proofs is in flight on this context (finish it first)");
    if (rr->device != ctx->device) return set_error(ctx, VSP_ERR_UNSUPPORTED, "saver_rerandomize_batch: the rerandomizer's tables are resident on another device");
    char m[160];
    for (size_t k = 0; k < count; k++) {
        static const char *const name[3] = {"r'", "z1", "z2"};
        for (int j = 0; j < 3; j++)
            if (!below_mod<FrP64>(rnd + 12 * k + 4 * j)) { snprintf(m, sizeof m, "saver_rerandomize_batch: %s of member %zu is not canonical (>= r)", name[j], k); return set_error(ctx, VSP_ERR_ARG, m); }
        if (limbs_zero(rnd + 12 * k + 4, 4)) { snprintf(m, sizeof m, "saver_rerandomize_batch: z1 of member %zu must be invertible", k); return set_error(ctx, VSP_ERR_ARG, m); }
    }
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t n = rr->n, ng = saver_rerand_given(n), ctw = (n + 2) * 12, blob = vsp_g1_vector_blob_size(n + 2), piece = piece_ballots(ctx);
    std::vector<HFr> pre;
    size_t first_bad = count;
    for (size_t at = 0; at < count; at += piece) {
        const size_t c = count - at < piece ? count - at : piece;
        VSP_TRY(rr_piece(ctx, rr, rnd, ct, A, B, C, at, c, pre));
        const uint64_t *h1 = ctx->saver_rr.h_out.as<const uint64_t>(), *h2 = h1 + c * ng * 12;
        const uint32_t *hst = (const uint32_t *)(h2 + c * 24);
        host_parallel_for(c, [&](size_t j) {
            const size_t k = at + j;
            const uint64_t *row = h1 + j * ng * 12, *a = row + 12 * saver_rerand_given_A(n), *cc = row + 12 * saver_rerand_given_C(n), *b = h2 + j * 24;
            const bool bad = hst[j] != 0;
            if (status_out) status_out[k] = bad ? 1 : 0;
            if (bad) {
                // a ballot with a rejected point leaves nothing
                if (ct_out) memset(ct_out + k * ctw, 0, ctw * 8);
                if (A_out) memset(A_out + 12 * k, 0, 96);
                if (B_out) memset(B_out + 24 * k, 0, 192);
                if (C_out) memset(C_out + 12 * k, 0, 96);
                if (proofs_out) memset(proofs_out + 192 * k, 0, 192);
                if (ct_blobs_out) memset(ct_blobs_out + k * blob, 0, blob);
                return;
            }
            if (ct_out) memcpy(ct_out + k * ctw, row, ctw * 8);
            if (A_out) memcpy(A_out + 12 * k, a, 96);
            if (B_out) memcpy(B_out + 24 * k, b, 192);
            if (C_out) memcpy(C_out + 12 * k, cc, 96);
            if (proofs_out) { uint8_t *p = proofs_out + 192 * k; vsp_g1_compress(a, p); vsp_g2_compress(b, p + 48); vsp_g1_compress(cc, p + 144); }
            if (ct_blobs_out) vsp_g1_vector_to_blob(row, n + 2, ct_blobs_out + k * blob);
        });
        for (size_t j = 0; j < c && first_bad == count; j++) if (hst[j]) first_bad = at + j;
        ctx->stats["saver_rerandomize_ballots"] += (double)c;
    }
    if (!status_out && first_bad != count) {
        snprintf(m, sizeof m, "saver_rerandomize_batch: a point of member %zu is not a curve point (its outputs are zero; pass status_out to learn every such member)", first_bad);
        return set_error(ctx, VSP_ERR_ARG, m);
    }
    return VSP_OK;
}

}  // extern "C"
