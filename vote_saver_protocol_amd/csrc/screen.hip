// SAVER ballots screened in bulk (include/vsp.h "SAVER ballots screened in bulk"): with caller-supplied 128-bit
// coefficients z_i the well-formed ballots of a range R are accepted together when two pairing-product equations hold,
//     equation 1:  fexp( prod_{j=0..n} ml(S_j, t_g2[j]) * ml(S_psi, -H) ) = 1
//     equation 2:  fexp( prod_{i in R} ml(z_i A_i, B_i) * ml(ACC, -gamma_g2) * ml(Csum, -delta_g2) * ml(-Z alpha_g1, beta_g2) ) = 1
// S_j = sum z_i c_{i,j}, S_psi = sum z_i psi_i, ACC = sum z_i acc_i, Csum = sum z_i C_i, Z = sum z_i mod r.  A range that fails is cut
// once into "saver_screen_split" sub-ranges, and the sub-ranges that fail go to the exact path (pairing.hip saver_verify_source), which
// alone gives a verdict of 0 and its reason.  Stages per piece of a call:
//   0. k_ballot_prepare    (pairing.hip, unchanged; k_receive_prepare of receive.hip for a decoded piece) the arguments column by column, A, B,
//                          a status byte per ballot
//   1. k_screen_scale      one lane per ballot: A_i <- z_i A_i, z_i widened to a canonical scalar; a malformed ballot: infinity and 0;
//                          then the digit sort and bucket plan over the z of the piece (step 4), so that its column sums run beside step 2
//   2. k_miller            (pairing.hip) one lane per ballot: ml(z_i A_i, B_i), kept for the second level
//   then per level (the whole piece; its sub-ranges in one pass):
//   3. k_screen_product    the Miller values of every range multiplied by a tree (screen.h), one lane per SCREEN_FAN values and level
//   4. the n + 4 column sums of every range by the multi-exponentiation engine: one digit sort and bucket plan over the z of a range
//      (MsmRequest.plan_only on slot 0), every column an accumulation over that plan on slots 1 .. 5 (plan_from); plain bases and
//      generic additions, so equal, opposite and infinity points and any curve point sum exactly
//   5. host: the sums to affine, Z and -Z alpha_g1: n + 5 arguments per range
//   6. k_screen_miller     one lane per (range, argument): miller_multi with g = 1 over the prepared lines of the argument's key member
//      k_screen_combine    one lane per (range, equation): the product of its Miller values
//   7. k_final_exp         (pairing.hip) both equations of every range in one launch, each judged "is one"
#include "common.h"
#include "pairing.h"
#include "pairing_g1.h"
#include "screen.h"

namespace vsp {

static constexpr size_t SCREEN_CHUNK = (size_t)1 << 16;            // ballots of one piece (option "saver_screen_chunk"); both defaults: the sweeps of DESIGN.md 3.6f
static constexpr size_t SCREEN_CHUNK_MAX = (size_t)1 << 16;
static constexpr long SCREEN_SPLIT = 4;                            // sub-ranges of a failed piece (option "saver_screen_split"; 0 or 1: none)
static constexpr size_t SCREEN_SPLIT_MAX = 1024;
static constexpr unsigned SCREEN_THREADS = 64;                     // one wave per block, as the pairing kernels

__device__ __noinline__ void sc_mul(Fp12 *f, const Fp12 *g) { const Fp12 t = mul(*f, *g); *f = t; }
__device__ __noinline__ void sc_miller_one(Fp12 *f, const G1Affine *P, const LineCoeffs<Fp> *lines) { *f = miller_multi<Fp>(P, 0, lines, 1, nullptr, nullptr); }

// ballot k of a piece: a_pts[k] <- z_k a_pts[k], z_out[k] = z_k as a canonical scalar; a malformed ballot (status not zero) leaves every
// sum and product: scalar 0, point at infinity (Miller value one)
__global__ __launch_bounds__(SCREEN_THREADS) void k_screen_scale(G1Affine *__restrict__ a_pts, const uint8_t *__restrict__ status, const uint64_t *__restrict__ coeff, size_t c,
                                                                 Fr *__restrict__ z_out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const bool bad = status[k] != 0;
    const uint64_t lo = bad ? 0 : coeff[2 * k], hi = bad ? 0 : coeff[2 * k + 1];
    const G1Affine P = a_pts[k];
    G1XYZZ acc;
    screen_mul128(acc, P, lo, hi, [](G1XYZZ *a) { pr_dbl(a); }, [](G1XYZZ *a, const G1Affine *q) { pr_madd(a, q); });
    a_pts[k] = pr_to_affine(acc);
    Fr z = Fr::zero();
    z.l[0] = (uint32_t)lo; z.l[1] = (uint32_t)(lo >> 32); z.l[2] = (uint32_t)hi; z.l[3] = (uint32_t)(hi >> 32);
    z_out[k] = z;
}

// one level of the product tree: blockIdx.y = range, lane = value of the next level
__global__ __launch_bounds__(SCREEN_THREADS) void k_screen_product(const Fp12 *__restrict__ in, ScreenLevel lv, size_t out_stride, Fp12 *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    const size_t count = lv.count(r);
    if (t >= screen_level_count(count)) return;
    out[r * out_stride + t] = screen_segment_product(in + r * lv.stride, count, t, [](Fp12 *f, const Fp12 *g) { sc_mul(f, g); });
}

// argument j < na of range r at args[r na + j], its lines at lines[j MILLER_LINES]: the Miller value to out[r na + j]
__global__ __launch_bounds__(SCREEN_THREADS) void k_screen_miller(const G1Affine *__restrict__ args, const LineCoeffs<Fp> *__restrict__ lines, size_t na, size_t total,
                                                                  Fp12 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    Fp12 f;
    sc_miller_one(&f, args + i, lines + (i % na) * MILLER_LINES);
    out[i] = f;
}

// lane 2 r + e: equation e of range r.  Equation 1: the first na - 3 values of the range (c_0 .. c_n, psi); equation 2: the product of
// the range's ballots, tree[r], times the last three (acc, C, alpha)
__global__ __launch_bounds__(SCREEN_THREADS) void k_screen_combine(const Fp12 *__restrict__ ml, const Fp12 *__restrict__ tree, size_t na, size_t ranges,
                                                                   Fp12 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * ranges) return;
    const size_t r = i >> 1;
    const Fp12 *v = ml + r * na;
    Fp12 f;
    size_t first, last;
    if (i & 1) { f = tree[r]; first = na - 3; last = na; }
    else { f = v[0]; first = 1; last = na - 3; }
#pragma unroll 1
    for (size_t j = first; j < last; j++) { Fp12 g = v[j]; sc_mul(&f, &g); }
    out[i] = f;
}

namespace {

// the workspace of one piece of c ballots evaluated in up to R ranges with na arguments each (ctx->screen_ws)
struct ScreenWork {
    uint64_t *coeff; Fr *z; G1Affine *args; Fp12 *ml, *tree[2], *eq; uint8_t *flags;
    static size_t tree_values(size_t c, size_t R) { return screen_level_count(c) + R; }
    static size_t bytes(size_t c, size_t R, size_t na) {
        return c * 16 + c * sizeof(Fr) + R * na * (sizeof(G1Affine) + sizeof(Fp12)) + (2 * tree_values(c, R) + 2 * R) * sizeof(Fp12) + 2 * R;
    }
    ScreenWork(void *p, size_t c, size_t R, size_t na) {
        char *q = (char *)p;
        ml = (Fp12 *)q; q += R * na * sizeof(Fp12);
        tree[0] = (Fp12 *)q; q += tree_values(c, R) * sizeof(Fp12);
        tree[1] = (Fp12 *)q; q += tree_values(c, R) * sizeof(Fp12);
        eq = (Fp12 *)q; q += 2 * R * sizeof(Fp12);
        args = (G1Affine *)q; q += R * na * sizeof(G1Affine);
        z = (Fr *)q; q += c * sizeof(Fr);
        coeff = (uint64_t *)q; q += c * 16;
        flags = (uint8_t *)q;
    }
};

// one piece in flight: what the levels share
struct ScreenPiece {
    vsp_ctx *ctx; const vsp_saver_verifier *ver;
    size_t c, n, na;                        // ballots, msg_size, arguments of a range (n + 5)
    const uint64_t *coeff;                  // the piece's coefficients (host)
    const uint8_t *status;                  // the piece's status bytes (host)
    bool from_device;                       // prepared by k_receive_prepare: its time counts as "saver_receive_prepare_ms" too
    ScreenWork w;
};

// the digit sort and bucket plan over the coefficients of a range, on slot 0 (the context's stream): every column sum reuses it
int screen_plan(vsp_ctx *ctx, const Fr *z, size_t cnt) {
    MsmRequest plan(z, cnt);
    plan.dense = true; plan.plan_only = true;
    return msm_slot_launch<G1>(ctx, 0, plan);
}

// steps 3 to 7 over the ranges of `len` ballots of the piece: holds[r] = both equations of range r hold.  first: the level over the
// whole piece, whose timers already hold the prepare, scale and Miller stages and whose plan is queued
int screen_level(ScreenPiece &p, size_t len, bool first, std::vector<uint8_t> &holds) {
    vsp_ctx *ctx = p.ctx;
    hipStream_t st = ctx->stream;
    StageTimer &t0 = ctx->screen_timer[0], &t1 = ctx->screen_timer[1];
    const size_t c = p.c, n = p.n, na = p.na;
    ScreenLevel lv = screen_first_level(c, len);
    const size_t R = lv.ranges;
    if (!first) for (int i = 0; i < 3; i++) VSP_TRY(t0.mark(ctx, i, st));
    // 3. the tree: levels until a range is one value (at stride 1 value r is the product of range r)
    const Fp12 *prod = (const Fp12 *)ctx->pair_ml.p;
    for (int side = 0; lv.stride > 1; side ^= 1) {
        const ScreenLevel nx = lv.next();
        hipLaunchKernelGGL(k_screen_product, dim3((unsigned)((nx.count_full + SCREEN_THREADS - 1) / SCREEN_THREADS), (unsigned)R), dim3(SCREEN_THREADS), 0, st, prod, lv,
                           nx.stride, p.w.tree[side]);
        VSP_LAUNCH_CHECK();
        prod = p.w.tree[side]; lv = nx;
    }
    VSP_TRY(t0.mark(ctx, 3, st));
    VSP_TRY(t1.mark(ctx, 0, st));
    // 4. and 5. the column sums of every range; Z and -Z alpha
    std::vector<Affine<HFp>> args(R * na);
    const G1Affine *pts = (const G1Affine *)ctx->pair_g1.p;
    constexpr unsigned LANES = VSP_MSM_SLOTS - 1;
    for (size_t r = 0; r < R; r++) {
        const size_t lo = r * len, cnt = lv.ranges == r + 1 ? c - lo : len;
        if (!first) VSP_TRY(screen_plan(ctx, p.w.z + lo, cnt));
        auto finish = [&](size_t j) -> int {
            XYZZ<HFp> sum;
            VSP_TRY(msm_slot_finish<G1>(ctx, 1 + (unsigned)(j % LANES), &sum));
            args[r * na + j] = xyzz_to_affine(sum);
            return VSP_OK;
        };
        for (size_t j = 0; j < n + 4; j++) {
            if (j >= LANES) VSP_TRY(finish(j - LANES));
            MsmRequest col(p.w.z + lo, cnt);
            col.dense = true; col.plan_from = 0; col.bases = pts + j * c + lo;
            ctx->slot_group[1 + j % LANES] = 1;
            VSP_TRY(msm_slot_launch<G1>(ctx, 1 + (unsigned)(j % LANES), col));
        }
        for (size_t j = n + 4 < LANES ? 0 : n + 4 - LANES; j < n + 4; j++) VSP_TRY(finish(j));
        // Z = sum z_i over the well-formed ballots: below 2^145, so canonical as it stands
        uint64_t Z[4] = {0, 0, 0, 0};
        for (size_t k = lo; k < lo + cnt; k++) {
            if (p.status[k]) continue;
            unsigned __int128 s = (unsigned __int128)Z[0] + p.coeff[2 * k];
            Z[0] = (uint64_t)s; s = (s >> 64) + Z[1] + p.coeff[2 * k + 1];
            Z[1] = (uint64_t)s; s = (s >> 64) + Z[2];
            Z[2] = (uint64_t)s;
        }
        args[r * na + n + 4] = xyzz_to_affine(xyzz_neg(xyzz_mul_scalar(xyzz_from_affine(p.ver->alpha_g1), Z, 192)));
    }
    VSP_HIP(hipMemcpyAsync(p.w.args, args.data(), R * na * sizeof(G1Affine), hipMemcpyHostToDevice, st));      // (args outlives the copy: the stream is waited for below)
    VSP_TRY(t1.mark(ctx, 1, st));
    // 6. the fixed-argument Miller loops and the two values of every range
    hipLaunchKernelGGL(k_screen_miller, dim3((unsigned)((R * na + SCREEN_THREADS - 1) / SCREEN_THREADS)), dim3(SCREEN_THREADS), 0, st, (const G1Affine *)p.w.args,
                       p.ver->d_lines.as<const LineCoeffs<Fp>>(), na, R * na, p.w.ml);
    VSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_screen_combine, dim3((unsigned)((2 * R + SCREEN_THREADS - 1) / SCREEN_THREADS)), dim3(SCREEN_THREADS), 0, st, (const Fp12 *)p.w.ml, prod, na, R,
                       p.w.eq);
    VSP_LAUNCH_CHECK();
    VSP_TRY(t1.mark(ctx, 2, st));
    // 7.
    VSP_TRY(pairing_final_exp(ctx, p.w.eq, 2 * R, nullptr, p.w.flags));
    VSP_TRY(t1.mark(ctx, 3, st));
    std::vector<uint8_t> flags(2 * R);
    VSP_HIP(hipMemcpyAsync(flags.data(), p.w.flags, 2 * R, hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    holds.resize(R);
    size_t failed = 0;
    for (size_t r = 0; r < R; r++) { holds[r] = flags[2 * r] && flags[2 * r + 1]; failed += !holds[r]; }
    ctx->stats["saver_screen_checks"] += (double)R;
    ctx->stats["saver_screen_failed"] += (double)failed;
    if (first && p.from_device) t0.add(ctx, 0, "saver_receive_prepare_ms");
    t0.add(ctx, 0, "saver_screen_prepare_ms"); t0.add(ctx, 1, "saver_screen_scale_ms"); t0.add(ctx, 2, "saver_screen_miller_ms");
    t1.add(ctx, 0, "saver_screen_msm_ms"); t1.add(ctx, 1, "saver_screen_miller_ms"); t1.add(ctx, 2, "saver_screen_finalexp_ms");
    return VSP_OK;
}

}  // anonymous namespace

size_t screen_piece_ballots(const vsp_ctx *ctx) {
    const long cv = opt(ctx, "saver_screen_chunk", (long)SCREEN_CHUNK);
    return cv < 1 ? 1 : ((size_t)cv > SCREEN_CHUNK_MAX ? SCREEN_CHUNK_MAX : (size_t)cv);
}

int screen_piece(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t at, size_t c, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out) {
    hipStream_t st = ctx->stream;
    const size_t n = ver->n, na = n + 5;
    const long sv = opt(ctx, "saver_screen_split", SCREEN_SPLIT);
    const size_t split = sv < 2 ? 1 : ((size_t)sv > SCREEN_SPLIT_MAX ? SCREEN_SPLIT_MAX : (size_t)sv);
    std::vector<uint8_t> status, holds;
    // 0. to 2.
    VSP_TRY(saver_piece_prepare(ctx, ver, src, at, c, ctx->screen_timer[0]));
    VSP_TRY(ensure(ctx, ctx->pair_ml, c * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->screen_ws, ScreenWork::bytes(c, split, na)));
    ScreenPiece p{ctx, ver, c, n, na, coeff + 2 * at, nullptr, src.dev != nullptr, ScreenWork(ctx->screen_ws.p, c, split, na)};
    G1Affine *a_pts = (G1Affine *)ctx->pair_g1.p + (n + 4) * c;
    const uint8_t *d_status = (const uint8_t *)ctx->pair_status.p;
    status.resize(c);
    VSP_HIP(hipMemcpyAsync(status.data(), d_status, c, hipMemcpyDeviceToHost, st));
    VSP_HIP(hipEventRecord(ctx->ev_aux, st));
    VSP_HIP(hipMemcpyAsync(p.w.coeff, p.coeff, c * 16, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_screen_scale, dim3((unsigned)((c + SCREEN_THREADS - 1) / SCREEN_THREADS)), dim3(SCREEN_THREADS), 0, st, a_pts, d_status, (const uint64_t *)p.w.coeff, c,
                       p.w.z);
    VSP_LAUNCH_CHECK();
    // the plan of the whole piece goes in front of the Miller loops: the column sums (other streams) wait for the plan alone and
    // run beside them
    VSP_TRY(screen_plan(ctx, p.w.z, c));
    VSP_TRY(ctx->screen_timer[0].mark(ctx, 2, st));
    VSP_TRY(pairing_miller(ctx, a_pts, ctx->pair_g2.p, c, ctx->pair_ml.p));
    VSP_HIP(hipEventSynchronize(ctx->ev_aux));                   // the status bytes alone: the stream runs on
    p.status = status.data();
    // a malformed ballot's verdict is the exact path's own: the status byte of the same kernel
    for (size_t k = 0; k < c; k++) {
        verdict_out[at + k] = status[k] == 0;
        if (reason_out) reason_out[at + k] = status[k] ? 1 : 0;
    }
    VSP_TRY(screen_level(p, c, true, holds));
    if (holds[0]) return VSP_OK;
    // the second level, then the exact path over runs of failed sub-ranges
    size_t len = c;
    if (split > 1 && c > 1) {
        len = (c + split - 1) / split;
        VSP_TRY(screen_level(p, len, false, holds));
    }
    const size_t R = (c + len - 1) / len;
    for (size_t r = 0; r < R;) {
        if (holds[r]) { r++; continue; }
        size_t e = r + 1;
        while (e < R && !holds[e]) e++;
        const size_t lo = at + r * len, hi = e * len < c ? at + e * len : at + c;
        VSP_TRY(saver_verify_source(ctx, ver, src, lo, hi - lo, verdict_out + lo, reason_out ? reason_out + lo : nullptr));
        ctx->stats["saver_screen_exact_ballots"] += (double)(hi - lo);
        r = e;
    }
    return VSP_OK;
}

static int screen_pieces(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t count, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out) {
    if (ver->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch_screened: the verifier belongs to another device");
    if (ctx->prove.active) return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch_screened: a proof is in flight on this context and owns the work slots (finish it first)");
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t piece = screen_piece_ballots(ctx);
    for (size_t at = 0; at < count; at += piece) VSP_TRY(screen_piece(ctx, ver, src, at, count - at < piece ? count - at : piece, coeff, verdict_out, reason_out));
    return VSP_OK;
}
int saver_verify_batch_screened(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *rest, const uint64_t *A, const uint64_t *B, const uint64_t *C,
                                size_t count, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out) {
    BallotSource src;
    src.ct = ct; src.rest = rest; src.A = A; src.B = B; src.C = C;
    const int rc = screen_pieces(ctx, ver, src, count, coeff, verdict_out, reason_out);
    if (rc != VSP_OK) msm_drain_slots(ctx);                         // nothing stays in flight on the work slots after an error
    return rc;
}

}  // namespace vsp
