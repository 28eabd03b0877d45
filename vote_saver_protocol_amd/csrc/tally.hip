// The receiving side of the vote: decode, check and add ciphertext blobs on the GPU (include/vsp.h "tally").
//
// process_encrypted_input_mode_tally_admin_phase (bin/cli/include/nil/vote_saver/common.hpp:1193-1216) deserialises up to
// 1 << tree_depth ciphertexts one after the other and adds them component by component into ct_agg, and every voter who verifies
// the tally repeats it (:1257-1279); the rest of both functions is pairing work on the ONE aggregated ciphertext.  At 2^20 ballots
// of msg_size + 2 = 27 compressed G1 points that is 28 M square roots, subgroup checks and point additions -- the one tally step
// whose cost grows with the number of voters.  Four stages per piece of a call, all on the context's stream:
//   1. k_point_decode<G1>  (decode.hip) one lane per point: the compressed record -> Montgomery affine point + status byte
//                          (rejected: infinity)
//   2. k_subgroup_check    (msm_impl.inc, with its per-point output) the endomorphism test phi(P) = lambda P: bit 2 of the status
//   3. k_tally_ballots     one lane per ballot: the count header against ct_len, OR of the points' status bytes
//      k_tally_colsum      block (b, j): lanes walk the ballots of part b with a stride and add component j of every ACCEPTED
//                          ballot in XYZZ (mixed additions), the lanes' sums are combined in LDS (full additions): one partial
//                          per block
//   4. host                the few partials per component are folded into the handle's running sums (as vsp_fold_jacobian does)
// Every exceptional case of the addition occurs in real data -- the same ballot twice (doubling), a ballot and its negation,
// infinity components, a running sum passing through infinity: curve.h's xyzz_madd / xyzz_add handle all of them.
#include "common.h"

struct vsp_tally {
    size_t ct_len = 0;
    uint64_t ballots = 0;                               // accepted since creation / the last reset
    std::vector<vsp::XYZZ<vsp::HFp>> sums;              // ct_len running sums, host Montgomery
};

namespace vsp {

static constexpr size_t TALLY_MAX_CT_LEN = 1024;
static constexpr unsigned TALLY_SUM_THREADS = 64;                  // one wave per block: 12 KiB of LDS for the lanes' sums
static constexpr unsigned TALLY_SUM_PER_LANE = 16;                 // ballots a lane adds before the block combines: 1024 ballots per block
static constexpr size_t TALLY_MAX_PARTIALS = 4096;                 // partial sums of one piece (768 KiB), folded on the host

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

size_t tally_ct_len(const vsp_tally *t) { return t->ct_len; }
void tally_ballots_launch(vsp_ctx *ctx, const uint8_t *d_blobs, size_t m, size_t ct_len, const uint8_t *d_pstatus, uint8_t *d_bstatus) {
    hipLaunchKernelGGL(k_tally_ballots, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, d_blobs, m, ct_len, d_pstatus, d_bstatus);
}
int tally_colsum_launch(vsp_ctx *ctx, const void *d_pts, const uint8_t *d_skip, size_t m, size_t ct_len, std::vector<XYZZ<HFp>> &h_part, size_t *parts_out,
                        StageTimer *sum_end) {
    hipStream_t st = ctx->stream;
    const size_t L = ct_len, span = (size_t)TALLY_SUM_THREADS * TALLY_SUM_PER_LANE;
    // parts of `span` ballots, and wider ones where that would be more partial sums than the host should fold
    size_t parts = (m + span - 1) / span, part_span = span;
    const size_t max_parts = TALLY_MAX_PARTIALS / L ? TALLY_MAX_PARTIALS / L : 1;
    if (parts > max_parts) { part_span = (m + max_parts - 1) / max_parts; parts = (m + part_span - 1) / part_span; }
    VSP_TRY(ensure(ctx, ctx->tally_partials, parts * L * sizeof(G1XYZZ)));
    hipLaunchKernelGGL(k_tally_colsum, dim3((unsigned)parts, (unsigned)L), dim3(TALLY_SUM_THREADS), 0, st, (const G1Affine *)d_pts, d_skip, m, L, part_span,
                       (G1XYZZ *)ctx->tally_partials.p);
    VSP_LAUNCH_CHECK();
    if (sum_end) VSP_TRY(sum_end->mark(ctx, 3, st));
    h_part.resize(parts * L);
    VSP_HIP(hipMemcpyAsync(h_part.data(), ctx->tally_partials.p, parts * L * sizeof(G1XYZZ), hipMemcpyDeviceToHost, st));   // XYZZ<Fp> and XYZZ<HFp>: the same bytes
    *parts_out = parts;
    return VSP_OK;
}
void tally_fold(vsp_tally *t, const std::vector<XYZZ<HFp>> &h_part, size_t parts, size_t accepted) {
    for (size_t j = 0; j < t->ct_len; j++)
        for (size_t b = 0; b < parts; b++) xyzz_add(t->sums[j], h_part[j * parts + b]);
    t->ballots += accepted;
}

}  // namespace vsp

using namespace vsp;

extern "C" {

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
    hipStream_t st = ctx->stream;
    const size_t L = t->ct_len, ballot_bytes = 8 + 48 * L, head = 8;
    DecodeWork &w = ctx->decode[0];
    size_t piece = decode_chunk_points(ctx) / L;                    // ballots of one piece: at least one
    if (piece < 1) piece = 1;
    std::vector<uint8_t> h_status;
    std::vector<XYZZ<HFp>> h_part;
    size_t accepted = 0;
    for (size_t at = 0; at < count; at += piece) {
        const size_t m = count - at < piece ? count - at : piece;
        size_t parts = 0;
        VSP_TRY(ensure(ctx, ctx->tally_raw, m * ballot_bytes));
        VSP_TRY(ensure(ctx, ctx->tally_bstatus, m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, blobs + at * ballot_bytes, m * ballot_bytes, hipMemcpyHostToDevice, st));
        VSP_TRY(decode_points<G1>(ctx, m * L, L, ballot_bytes, &head, 1, check_subgroup));
        tally_ballots_launch(ctx, (const uint8_t *)ctx->tally_raw.p, m, L, (const uint8_t *)w.pstatus.p, (uint8_t *)ctx->tally_bstatus.p);
        VSP_TRY(tally_colsum_launch(ctx, w.pts.p, (const uint8_t *)ctx->tally_bstatus.p, m, L, h_part, &parts, &w.timer));
        h_status.resize(m);
        VSP_HIP(hipMemcpyAsync(h_status.data(), ctx->tally_bstatus.p, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        decode_add_times<G1>(ctx, check_subgroup != 0);
        w.timer.add(ctx, 2, "tally_sum_ms");
        // nothing of this piece has touched the handle before this point: an error above leaves the tally as it was
        size_t ok = 0;
        for (size_t b = 0; b < m; b++) ok += h_status[b] == 0;
        tally_fold(t, h_part, parts, ok);
        if (status_out) memcpy(status_out + at, h_status.data(), m);
        accepted += ok;
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
