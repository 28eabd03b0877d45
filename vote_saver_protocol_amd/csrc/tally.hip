// The receiving side of the vote: decode, check and add ciphertext blobs on the GPU (include/vsp.h "tally").
//
// process_encrypted_input_mode_tally_admin_phase (bin/cli/include/nil/vote_saver/common.hpp:1193-1216) deserialises up to
// 1 << tree_depth ciphertexts one after the other and adds them component by component into ct_agg, and every voter who verifies
// the tally repeats it (:1257-1279); the rest of both functions is pairing work on the ONE aggregated ciphertext.  At 2^20 ballots
// of msg_size + 2 = 27 compressed G1 points that is 28 M square roots, subgroup checks and point additions -- the one tally step
// whose cost grows with the number of voters.  Four stages per piece of a call, all on the context's stream:
//   1. k_tally_decode      one lane per point: flag bits, byte order, x < p, Montgomery form, y = sqrt(x^3 + 4) by the fixed
//                          chain of fp_sqrt.h, the sign rule; Montgomery affine point + status byte (rejected: infinity)
//   2. k_subgroup_check    (msm_impl.inc, with its per-point output) the endomorphism test phi(P) = lambda P: bit 2 of the status
//   3. k_tally_ballots     one lane per ballot: the count header against ct_len, OR of the points' status bytes
//      k_tally_colsum      block (b, j): lanes walk the ballots of part b with a stride and add component j of every ACCEPTED
//                          ballot in XYZZ (mixed additions), the lanes' sums are combined in LDS (full additions): one partial
//                          per block
//   4. host                the few partials per component are folded into the handle's running sums (as vsp_fold_jacobian does)
// Every exceptional case of the addition occurs in real data -- the same ballot twice (doubling), a ballot and its negation,
// infinity components, a running sum passing through infinity: curve.h's xyzz_madd / xyzz_add handle all of them.
//
// Proofs (vsp_g2_decompress_batch, vsp_proof_from_blob_batch) reuse stages 1 and 2: a proof blob is A (48) | B (96) | C (48), so A and C
// are records of k_tally_decode at heads 0 and 144 of a 192-byte stride, and B goes through the G2 counterpart
//   1'. k_g2_decode        one lane per point: the same rules on 96-byte records c1 | c0, y = sqrt(x^3 + 4 (1 + u)) by the two fixed
//                          chains of fp2_sqrt.h; Montgomery Affine<Fp2> as k_subgroup_check<Fp2> reads it + status byte
//   2'. k_subgroup_check   over Fp2 (a lane pair per point)
//   3'. k_proof_status     one lane per proof: OR of the three status bytes, and which member was rejected
#include "common.h"
#include "fp2_sqrt.h"

struct vsp_tally {
    size_t ct_len = 0;
    uint64_t ballots = 0;                               // accepted since creation / the last reset
    std::vector<vsp::XYZZ<vsp::HFp>> sums;              // ct_len running sums, host Montgomery
};

namespace vsp {

static constexpr size_t TALLY_MAX_CT_LEN = 1024;
static constexpr size_t TALLY_CHUNK_POINTS = (size_t)1 << 21;      // points of one piece: 192 MiB decoded, 96 MiB raw
static constexpr unsigned TALLY_SUM_THREADS = 64;                  // one wave per block: 12 KiB of LDS for the lanes' sums
static constexpr unsigned TALLY_SUM_PER_LANE = 16;                 // ballots a lane adds before the block combines: 1024 ballots per block
static constexpr size_t TALLY_MAX_PARTIALS = 4096;                 // partial sums of one piece (768 KiB), folded on the host

// point i of the input: ballot i / per of `stride` bytes, `head` bytes of header, then per records of 48 bytes (a plain array of
// points: head = 0, per = 1, stride = 48).  Every record starts at a multiple of 8 bytes.
__global__ __launch_bounds__(256) void k_tally_decode(const uint8_t *__restrict__ src, size_t n, size_t per, size_t stride, size_t head,
                                                      G1Affine *__restrict__ out, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *w = (const uint32_t *)(src + (i / per) * stride + head + (i % per) * 48);
    const uint32_t flags = w[0] & 0xFFu;                          // first byte of the record
    uint32_t rest = w[0] & ~0xE0u;                                // everything but the three flag bits
#pragma unroll
    for (int j = 1; j < 12; j++) rest |= w[j];
    uint32_t st = 0;
    bool finite = false;
    if (!(flags & 0x80u)) st = 1u;                                // not the compressed form
    else if (flags & 0x40u) { if (rest != 0 || (flags & 0x20u)) st = 1u; }      // infinity: every other bit clear
    else finite = true;
    Fp x = fp_from_be(w, true);
    if (finite && !canon_below_p(x)) { st = 1u; finite = false; }
    if (!finite) x = Fp::zero();
    // every lane walks the chain (rejected and infinity lanes on x = 0): the wave runs it anyway
    G1Affine p;
    p.x = to_mont(x);
    const bool on_curve = g1_y_from_x(p.x, (flags & 0x20u) != 0, p.y);
    if (finite && !on_curve) { st = 2u; finite = false; }
    if (!finite) { p.x = Fp::zero(); p.y = Fp::zero(); }
    out[i] = p;
    status[i] = (uint8_t)st;
}

// ballot b: bit 0 when its count header is not ct_len, OR of its points' status bytes
__global__ __launch_bounds__(256) void k_tally_ballots(const uint8_t *__restrict__ src, size_t count, size_t ct_len, const uint8_t *__restrict__ pstatus,
                                                       uint8_t *__restrict__ bstatus) {
    const size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= count) return;
    const uint32_t *h = (const uint32_t *)(src + b * (8 + 48 * ct_len));
    const uint64_t hdr = ((uint64_t)__builtin_bswap32(h[0]) << 32) | __builtin_bswap32(h[1]);
    uint32_t st = hdr == (uint64_t)ct_len ? 0u : 1u;
    for (size_t j = 0; j < ct_len; j++) st |= pstatus[b * ct_len + j];
    bstatus[b] = (uint8_t)st;
}

// Montgomery affine -> canonical affine in place; a point whose status byte is set becomes all zero (vsp_g1/g2_decompress_batch; for
// proofs the byte is the PROOF's: a rejected proof exports none of its members)
template <class F> __global__ __launch_bounds__(256) void k_tally_export(Affine<F> *pts, const uint8_t *__restrict__ status, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = pts[i];
    if (status[i]) { p.x = F::zero(); p.y = F::zero(); }
    else { p.x = from_mont(p.x); p.y = from_mont(p.y); }
    pts[i] = p;
}

// the root as a real call on memory temporaries (see tally_madd below): one copy of the two chains beside the decoding code
__device__ __noinline__ bool tally_g2_y(const Fp2 *x, bool larger, Fp2 *y) { Fp2 t; const bool ok = g2_y_from_x(*x, larger, t); *y = t; return ok; }
// point i of the input as in k_tally_decode, records of 96 bytes: x.c1 | x.c0 big-endian, the flag bits in the first byte
__global__ __launch_bounds__(256) void k_g2_decode(const uint8_t *__restrict__ src, size_t n, size_t per, size_t stride, size_t head,
                                                   G2Affine *__restrict__ out, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *w = (const uint32_t *)(src + (i / per) * stride + head + (i % per) * 96);
    const uint32_t flags = w[0] & 0xFFu;
    uint32_t rest = w[0] & ~0xE0u;
#pragma unroll
    for (int j = 1; j < 24; j++) rest |= w[j];
    uint32_t st = 0;
    bool finite = false;
    if (!(flags & 0x80u)) st = 1u;
    else if (flags & 0x40u) { if (rest != 0 || (flags & 0x20u)) st = 1u; }
    else finite = true;
    Fp2 x;
    x.c1 = fp_from_be(w, true);
    x.c0 = fp_from_be(w + 12, false);
    if (finite && !(canon_below_p(x.c1) && canon_below_p(x.c0))) { st = 1u; finite = false; }
    if (!finite) x = Fp2::zero();
    G2Affine p;
    p.x = to_mont(x);
    const bool on_curve = tally_g2_y(&p.x, (flags & 0x20u) != 0, &p.y);
    if (finite && !on_curve) { st = 2u; finite = false; }
    if (!finite) { p.x = Fp2::zero(); p.y = Fp2::zero(); }
    out[i] = p;
    status[i] = (uint8_t)st;
}

// proof k: OR of the status bytes of A (g1st[k]), C (g1st[m + k]) and B (g2st[k]); bits 4, 5, 6 name the rejected members A, B, C
__global__ __launch_bounds__(256) void k_proof_status(const uint8_t *__restrict__ g1st, const uint8_t *__restrict__ g2st, size_t m, uint8_t *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t a = g1st[k], b = g2st[k], c = g1st[m + k];
    out[k] = (uint8_t)(a | b | c | (a ? 0x10u : 0u) | (b ? 0x20u : 0u) | (c ? 0x40u : 0u));
}

// the two additions as real calls on memory temporaries, as k_subgroup_check makes them (msm_impl.inc sgc_*): the generic formulas
// inlined side by side next to the fixed-register product routine are what this toolchain's backend has tripped over
__device__ __noinline__ void tally_madd(G1XYZZ *a, const G1Affine *p) { G1XYZZ t = *a; xyzz_madd(t, *p); *a = t; }
__device__ __noinline__ void tally_add(G1XYZZ *a, const G1XYZZ *q) { G1XYZZ t = *a; xyzz_add(t, *q); *a = t; }
// grid (parts, ct_len): block (b, j) sums component j over the accepted ballots of part b -- ballots [b * span, (b + 1) * span),
// span = TALLY_SUM_THREADS * TALLY_SUM_PER_LANE -- into partials[j * parts + b]
__global__ __launch_bounds__(TALLY_SUM_THREADS) void k_tally_colsum(const G1Affine *__restrict__ pts, const uint8_t *__restrict__ bstatus, size_t count, size_t ct_len,
                                                                    size_t span, G1XYZZ *__restrict__ partials) {
    __shared__ G1XYZZ sh[TALLY_SUM_THREADS];
    const size_t j = blockIdx.y, first = (size_t)blockIdx.x * span;
    const size_t end = first + span < count ? first + span : count;
    G1XYZZ acc = G1XYZZ::inf();
#pragma unroll 1
    for (size_t b = first + threadIdx.x; b < end; b += TALLY_SUM_THREADS) {
        if (bstatus[b]) continue;                                   // the BALLOT's verdict: a rejected ballot adds none of its components
        G1Affine p = pts[b * ct_len + j];
        tally_madd(&acc, &p);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll 1
    for (unsigned s = TALLY_SUM_THREADS / 2; s >= 1; s >>= 1) {
        if (threadIdx.x < s) { G1XYZZ q = sh[threadIdx.x + s]; tally_add(&acc, &q); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[j * gridDim.x + blockIdx.x] = acc;
}

// the timers of the device stages, created on first use
static int tally_events(vsp_ctx *ctx) {
    for (hipEvent_t &e : ctx->tally_ev) if (!e) VSP_HIP(hipEventCreate(&e));
    for (hipEvent_t &e : ctx->g2_ev) if (!e) VSP_HIP(hipEventCreate(&e));
    return VSP_OK;
}
static void tally_add_times(vsp_ctx *ctx, bool subgroup, bool sum) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->tally_ev[0], ctx->tally_ev[1]) == hipSuccess) ctx->stats["tally_decode_ms"] += ms;
    if (subgroup && hipEventElapsedTime(&ms, ctx->tally_ev[1], ctx->tally_ev[2]) == hipSuccess) ctx->stats["tally_subgroup_ms"] += ms;
    if (sum && hipEventElapsedTime(&ms, ctx->tally_ev[2], ctx->tally_ev[3]) == hipSuccess) ctx->stats["tally_sum_ms"] += ms;
}
// points of one piece: option "tally_chunk_points" (a test hook as well: small pieces at small sizes), 1 .. 2^21
static size_t tally_chunk_points(const vsp_ctx *ctx) {
    const long v = opt(ctx, "tally_chunk_points", (long)TALLY_CHUNK_POINTS);
    return v < 1 ? 1 : ((size_t)v > TALLY_CHUNK_POINTS ? TALLY_CHUNK_POINTS : (size_t)v);
}
// stages 1 and 2 over the G1 points already in ctx->tally_raw: `sets` sets of n points each, set k at heads[k] of the same (per, stride)
// addressing, decoded one after the other into ctx->tally_pts / tally_pstatus; events 0, 1, 2 around the stages
static int tally_decode(vsp_ctx *ctx, size_t n, size_t per, size_t stride, const size_t *heads, size_t sets, int check_subgroup) {
    hipStream_t st = ctx->stream;
    VSP_TRY(ensure(ctx, ctx->tally_pts, sets * n * sizeof(G1Affine)));
    VSP_TRY(ensure(ctx, ctx->tally_pstatus, sets * n));
    VSP_HIP(hipEventRecord(ctx->tally_ev[0], st));
    for (size_t k = 0; k < sets; k++)
        hipLaunchKernelGGL(k_tally_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->tally_raw.p, n, per, stride, heads[k],
                           (G1Affine *)ctx->tally_pts.p + k * n, (uint8_t *)ctx->tally_pstatus.p + k * n);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipEventRecord(ctx->tally_ev[1], st));
    // rejected points are infinity by now, which the check passes over: their bytes keep the decoder's verdict
    if (check_subgroup) VSP_TRY(subgroup_check<G1>(ctx, (const G1Affine *)ctx->tally_pts.p, sets * n, nullptr, (uint8_t *)ctx->tally_pstatus.p));
    VSP_HIP(hipEventRecord(ctx->tally_ev[2], st));
    return VSP_OK;
}
static int tally_decode(vsp_ctx *ctx, size_t n, size_t per, size_t stride, size_t head, int check_subgroup) {
    return tally_decode(ctx, n, per, stride, &head, 1, check_subgroup);
}
// the same two stages over n G2 points of ctx->tally_raw into ctx->g2_pts / g2_pstatus; the events of ctx->g2_ev around them
static int g2_decode(vsp_ctx *ctx, size_t n, size_t per, size_t stride, size_t head, int check_subgroup) {
    hipStream_t st = ctx->stream;
    VSP_TRY(ensure(ctx, ctx->g2_pts, n * sizeof(G2Affine)));
    VSP_TRY(ensure(ctx, ctx->g2_pstatus, n));
    VSP_HIP(hipEventRecord(ctx->g2_ev[0], st));
    hipLaunchKernelGGL(k_g2_decode, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->tally_raw.p, n, per, stride, head,
                       (G2Affine *)ctx->g2_pts.p, (uint8_t *)ctx->g2_pstatus.p);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipEventRecord(ctx->g2_ev[1], st));
    if (check_subgroup) VSP_TRY(subgroup_check<G2>(ctx, (const G2Affine *)ctx->g2_pts.p, n, nullptr, (uint8_t *)ctx->g2_pstatus.p));
    VSP_HIP(hipEventRecord(ctx->g2_ev[2], st));
    return VSP_OK;
}
static void g2_add_times(vsp_ctx *ctx, bool subgroup) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ctx->g2_ev[0], ctx->g2_ev[1]) == hipSuccess) ctx->stats["g2_decode_ms"] += ms;
    if (subgroup && hipEventElapsedTime(&ms, ctx->g2_ev[1], ctx->g2_ev[2]) == hipSuccess) ctx->stats["g2_subgroup_ms"] += ms;
}
// Montgomery -> canonical (zero where `status` is set) and the copy to the host, for n points of either group
template <class F> static int tally_export(vsp_ctx *ctx, Affine<F> *pts, const uint8_t *status, size_t n, uint64_t *out) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_tally_export<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, pts, status, n);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipMemcpyAsync(out, pts, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, ctx->stream));
    return VSP_OK;
}

}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_g1_decompress_batch(vsp_ctx *ctx, const uint8_t *in, size_t n, int check_subgroup, uint64_t *out_affine, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!in || !out_affine || !status_out) return set_error(ctx, VSP_ERR_ARG, "g1_decompress_batch: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(tally_events(ctx));
    hipStream_t st = ctx->stream;
    const size_t piece = tally_chunk_points(ctx);
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        VSP_TRY(ensure(ctx, ctx->tally_raw, 48 * m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, in + 48 * at, 48 * m, hipMemcpyHostToDevice, st));
        VSP_TRY(tally_decode(ctx, m, 1, 48, 0, check_subgroup));
        VSP_TRY(tally_export(ctx, (G1Affine *)ctx->tally_pts.p, (const uint8_t *)ctx->tally_pstatus.p, m, out_affine + 12 * at));
        VSP_HIP(hipMemcpyAsync(status_out + at, ctx->tally_pstatus.p, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        tally_add_times(ctx, check_subgroup != 0, false);
    }
    return VSP_OK;
}

int vsp_g2_decompress_batch(vsp_ctx *ctx, const uint8_t *in, size_t n, int check_subgroup, uint64_t *out_affine, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!in || !out_affine || !status_out) return set_error(ctx, VSP_ERR_ARG, "g2_decompress_batch: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(tally_events(ctx));
    hipStream_t st = ctx->stream;
    const size_t piece = tally_chunk_points(ctx);
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        VSP_TRY(ensure(ctx, ctx->tally_raw, 96 * m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, in + 96 * at, 96 * m, hipMemcpyHostToDevice, st));
        VSP_TRY(g2_decode(ctx, m, 1, 96, 0, check_subgroup));
        VSP_TRY(tally_export(ctx, (G2Affine *)ctx->g2_pts.p, (const uint8_t *)ctx->g2_pstatus.p, m, out_affine + 24 * at));
        VSP_HIP(hipMemcpyAsync(status_out + at, ctx->g2_pstatus.p, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        g2_add_times(ctx, check_subgroup != 0);
    }
    return VSP_OK;
}

int vsp_proof_from_blob_batch(vsp_ctx *ctx, const uint8_t *blobs, size_t n, int check_subgroup, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out,
                              uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!blobs || !status_out) return set_error(ctx, VSP_ERR_ARG, "proof_from_blob_batch: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(tally_events(ctx));
    hipStream_t st = ctx->stream;
    size_t piece = tally_chunk_points(ctx) / 3;                    // proofs of one piece: three points each, at least one proof
    if (piece < 1) piece = 1;
    const size_t heads[2] = {0, 144};                               // A and C; B lies between them
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        VSP_TRY(ensure(ctx, ctx->tally_raw, 192 * m));
        VSP_TRY(ensure(ctx, ctx->tally_bstatus, m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, blobs + 192 * at, 192 * m, hipMemcpyHostToDevice, st));
        VSP_TRY(tally_decode(ctx, m, 1, 192, heads, 2, check_subgroup));          // A: points [0, m), C: [m, 2m)
        VSP_TRY(g2_decode(ctx, m, 1, 192, 48, check_subgroup));
        const uint8_t *pstatus = (const uint8_t *)ctx->tally_bstatus.p;
        hipLaunchKernelGGL(k_proof_status, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->tally_pstatus.p, (const uint8_t *)ctx->g2_pstatus.p, m,
                           (uint8_t *)ctx->tally_bstatus.p);
        VSP_LAUNCH_CHECK();
        if (A_out) VSP_TRY(tally_export(ctx, (G1Affine *)ctx->tally_pts.p, pstatus, m, A_out + 12 * at));
        if (C_out) VSP_TRY(tally_export(ctx, (G1Affine *)ctx->tally_pts.p + m, pstatus, m, C_out + 12 * at));
        if (B_out) VSP_TRY(tally_export(ctx, (G2Affine *)ctx->g2_pts.p, pstatus, m, B_out + 24 * at));
        VSP_HIP(hipMemcpyAsync(status_out + at, pstatus, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        tally_add_times(ctx, check_subgroup != 0, false);
        g2_add_times(ctx, check_subgroup != 0);
    }
    return VSP_OK;
}

vsp_tally *vsp_tally_create(vsp_ctx *ctx, size_t ct_len) {
    if (!ctx) return nullptr;
    if (ct_len < 1 || ct_len > TALLY_MAX_CT_LEN) { set_error(ctx, VSP_ERR_ARG, "tally_create: ct_len outside 1..1024"); return nullptr; }
    vsp_tally *t = new vsp_tally();
    t->ct_len = ct_len;
    t->sums.assign(ct_len, XYZZ<HFp>::inf());
    return t;
}
void vsp_tally_free(vsp_ctx *ctx, vsp_tally *t) { (void)ctx; delete t; }

int vsp_tally_reset(vsp_ctx *ctx, vsp_tally *t) {
    if (!ctx) return VSP_ERR_ARG;
    if (!t) return set_error(ctx, VSP_ERR_ARG, "tally_reset: null handle");
    t->sums.assign(t->ct_len, XYZZ<HFp>::inf());
    t->ballots = 0;
    return VSP_OK;
}

int vsp_tally_add_blobs(vsp_ctx *ctx, vsp_tally *t, const uint8_t *blobs, size_t count, int check_subgroup, uint8_t *status_out, size_t *accepted_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!t || !blobs) return set_error(ctx, VSP_ERR_ARG, "tally_add_blobs: null argument");
    if (accepted_out) *accepted_out = 0;
    if (!count) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(tally_events(ctx));
    hipStream_t st = ctx->stream;
    const size_t L = t->ct_len, ballot_bytes = 8 + 48 * L;
    size_t piece = tally_chunk_points(ctx) / L;                    // ballots of one piece: at least one
    if (piece < 1) piece = 1;
    const size_t span = (size_t)TALLY_SUM_THREADS * TALLY_SUM_PER_LANE;
    std::vector<uint8_t> h_status;
    std::vector<XYZZ<HFp>> h_part;
    size_t accepted = 0;
    for (size_t at = 0; at < count; at += piece) {
        const size_t m = count - at < piece ? count - at : piece;
        // parts of `span` ballots, and wider ones where that would be more partial sums than the host should fold
        size_t parts = (m + span - 1) / span, part_span = span;
        const size_t max_parts = TALLY_MAX_PARTIALS / L ? TALLY_MAX_PARTIALS / L : 1;
        if (parts > max_parts) { part_span = (m + max_parts - 1) / max_parts; parts = (m + part_span - 1) / part_span; }
        VSP_TRY(ensure(ctx, ctx->tally_raw, m * ballot_bytes));
        VSP_TRY(ensure(ctx, ctx->tally_bstatus, m));
        VSP_TRY(ensure(ctx, ctx->tally_partials, parts * L * sizeof(G1XYZZ)));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, blobs + at * ballot_bytes, m * ballot_bytes, hipMemcpyHostToDevice, st));
        VSP_TRY(tally_decode(ctx, m * L, L, ballot_bytes, 8, check_subgroup));
        hipLaunchKernelGGL(k_tally_ballots, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->tally_raw.p, m, L,
                           (const uint8_t *)ctx->tally_pstatus.p, (uint8_t *)ctx->tally_bstatus.p);
        hipLaunchKernelGGL(k_tally_colsum, dim3((unsigned)parts, (unsigned)L), dim3(TALLY_SUM_THREADS), 0, st, (const G1Affine *)ctx->tally_pts.p,
                           (const uint8_t *)ctx->tally_bstatus.p, m, L, part_span, (G1XYZZ *)ctx->tally_partials.p);
        VSP_LAUNCH_CHECK();
        VSP_HIP(hipEventRecord(ctx->tally_ev[3], st));
        h_status.resize(m); h_part.resize(parts * L);
        VSP_HIP(hipMemcpyAsync(h_status.data(), ctx->tally_bstatus.p, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipMemcpyAsync(h_part.data(), ctx->tally_partials.p, parts * L * sizeof(G1XYZZ), hipMemcpyDeviceToHost, st));   // XYZZ<Fp> and XYZZ<HFp>: the same bytes
        VSP_HIP(hipStreamSynchronize(st));
        tally_add_times(ctx, check_subgroup != 0, true);
        // nothing of this piece has touched the handle before this point: an error above leaves the tally as it was
        for (size_t j = 0; j < L; j++)
            for (size_t b = 0; b < parts; b++) xyzz_add(t->sums[j], h_part[j * parts + b]);
        size_t ok = 0;
        for (size_t b = 0; b < m; b++) ok += h_status[b] == 0;
        if (status_out) memcpy(status_out + at, h_status.data(), m);
        accepted += ok;
        t->ballots += ok;
        if (accepted_out) *accepted_out = accepted;
    }
    return VSP_OK;
}

int vsp_tally_result(vsp_ctx *ctx, const vsp_tally *t, uint64_t *ct_out, uint64_t *ballots_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!t || !ct_out) return set_error(ctx, VSP_ERR_ARG, "tally_result: null argument");
    for (size_t j = 0; j < t->ct_len; j++) host_store_affine(ct_out + 12 * j, xyzz_to_affine(t->sums[j]));
    if (ballots_out) *ballots_out = t->ballots;
    return VSP_OK;
}

}  // extern "C"
