// Decoding compressed points on the GPU: plain point arrays of either group and proof blobs (include/vsp.h vsp_g1_decompress_batch,
// vsp_g2_decompress_batch, vsp_proof_from_blob_batch), and the first two stages of the tally (tally.hip).  Per piece of a call, all on
// the context's stream:
//   1. k_point_decode<G>   one lane per point: point_decode.h decode_record -- flag bits, byte order, x < p, Montgomery form, the y by
//                          the fixed chains of fp_sqrt.h (G1: y = sqrt(x^3 + 4)) / fp2_sqrt.h (G2: 96-byte records c1 | c0,
//                          y = sqrt(x^3 + 4 (1 + u))), the sign rule; Montgomery affine point + status byte (rejected: infinity)
//   2. k_subgroup_check    (msm_impl.inc, with its per-point output; G2: a lane pair per point) the endomorphism test
//                          phi(P) = lambda P: bit 2 of the status
//   3. k_point_export<F>   Montgomery -> canonical for the copy to the host; a point whose status byte is set leaves all zero
// A proof blob is A (48) | B (96) | C (48): A and C are G1 records at heads 0 and 144 of a 192-byte stride, B a G2 record at head 48, and
//   2'. k_proof_status     one lane per proof: OR of the three status bytes, and which member was rejected
#include "common.h"

namespace vsp {

static constexpr size_t DECODE_CHUNK_POINTS = (size_t)1 << 21;     // points of one piece: 192 MiB decoded, 96 MiB raw (G1)

// point i of the input: ballot i / per of `stride` bytes, `head` bytes of header, then per records of sizeof(G::F) bytes (a plain array
// of points: head = 0, per = 1, stride = the record).  Every record starts at a multiple of 8 bytes.
template <class G>
__global__ __launch_bounds__(256) void k_point_decode(const uint8_t *__restrict__ src, size_t n, size_t per, size_t stride, size_t head,
                                                      typename G::Point *__restrict__ out, uint8_t *__restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename G::Point p;
    const uint32_t st = decode_record((const uint32_t *)(src + (i / per) * stride + head + (i % per) * sizeof(typename G::F)), p);
    out[i] = p;
    status[i] = (uint8_t)st;
}

// Montgomery affine -> canonical affine in place; a point whose status byte is set becomes all zero (vsp_g1/g2_decompress_batch; for
// proofs the byte is the PROOF's: a rejected proof exports none of its members)
template <class F> __global__ __launch_bounds__(256) void k_point_export(Affine<F> *pts, const uint8_t *__restrict__ status, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = pts[i];
    if (status[i]) { p.x = F::zero(); p.y = F::zero(); }
    else { p.x = from_mont(p.x); p.y = from_mont(p.y); }
    pts[i] = p;
}

// proof k: OR of the status bytes of A (g1st[k]), C (g1st[m + k]) and B (g2st[k]); bits 4, 5, 6 name the rejected members A, B, C
__global__ __launch_bounds__(256) void k_proof_status(const uint8_t *__restrict__ g1st, const uint8_t *__restrict__ g2st, size_t m, uint8_t *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const uint32_t a = g1st[k], b = g2st[k], c = g1st[m + k];
    out[k] = (uint8_t)(a | b | c | (a ? 0x10u : 0u) | (b ? 0x20u : 0u) | (c ? 0x40u : 0u));
}

// points of one piece: option "tally_chunk_points" (a test hook as well: small pieces at small sizes), 1 .. 2^21
size_t decode_chunk_points(const vsp_ctx *ctx) {
    const long v = opt(ctx, "tally_chunk_points", (long)DECODE_CHUNK_POINTS);
    return v < 1 ? 1 : ((size_t)v > DECODE_CHUNK_POINTS ? DECODE_CHUNK_POINTS : (size_t)v);
}
template <class G> int decode_points(vsp_ctx *ctx, size_t n, size_t per, size_t stride, const size_t *heads, size_t sets, int check_subgroup, typename G::Point *dst,
                                     uint8_t *dst_status) {
    using Point = typename G::Point;
    hipStream_t st = ctx->stream;
    DecodeWork &w = ctx->decode[G::ID - 1];
    if (!dst) {
        VSP_TRY(ensure(ctx, w.pts, sets * n * sizeof(Point)));
        VSP_TRY(ensure(ctx, w.pstatus, sets * n));
        dst = (Point *)w.pts.p; dst_status = (uint8_t *)w.pstatus.p;
    }
    VSP_TRY(w.timer.mark(ctx, 0, st));
    for (size_t k = 0; k < sets; k++)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_decode<G>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->tally_raw.p, n, per, stride,
                           heads[k], dst + k * n, dst_status + k * n);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer.mark(ctx, 1, st));
    // rejected points are infinity by now, which the check passes over: their bytes keep the decoder's verdict
    if (check_subgroup) VSP_TRY(subgroup_check<G>(ctx, (const Point *)dst, sets * n, nullptr, dst_status));
    VSP_TRY(w.timer.mark(ctx, 2, st));
    return VSP_OK;
}
template int decode_points<G1>(vsp_ctx *, size_t, size_t, size_t, const size_t *, size_t, int, G1Affine *, uint8_t *);
template int decode_points<G2>(vsp_ctx *, size_t, size_t, size_t, const size_t *, size_t, int, G2Affine *, uint8_t *);
template <class G> void decode_add_times(vsp_ctx *ctx, bool subgroup) {
    const StageTimer &t = ctx->decode[G::ID - 1].timer;
    t.add(ctx, 0, G::ID == 1 ? "tally_decode_ms" : "g2_decode_ms");
    if (subgroup) t.add(ctx, 1, G::ID == 1 ? "tally_subgroup_ms" : "g2_subgroup_ms");
}
template void decode_add_times<G1>(vsp_ctx *, bool);
template void decode_add_times<G2>(vsp_ctx *, bool);
int decode_proof_status(vsp_ctx *ctx, size_t m, uint8_t *d_out) {
    hipLaunchKernelGGL(k_proof_status, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const uint8_t *)ctx->decode[0].pstatus.p,
                       (const uint8_t *)ctx->decode[1].pstatus.p, m, d_out);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
// Montgomery -> canonical (zero where `status` is set) and the copy to the host, for n points of either group
template <class F> static int export_points(vsp_ctx *ctx, Affine<F> *pts, const uint8_t *status, size_t n, uint64_t *out) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_point_export<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, pts, status, n);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipMemcpyAsync(out, pts, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, ctx->stream));
    return VSP_OK;
}
// the one body of vsp_g1_decompress_batch / vsp_g2_decompress_batch
template <class G> static int decompress_batch(vsp_ctx *ctx, const uint8_t *in, size_t n, int check_subgroup, uint64_t *out_affine, uint8_t *status_out) {
    using Point = typename G::Point;
    if (!ctx) return VSP_ERR_ARG;
    if (!in || !out_affine || !status_out) return set_error(ctx, VSP_ERR_ARG, G::ID == 1 ? "g1_decompress_batch: null argument" : "g2_decompress_batch: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DecodeWork &w = ctx->decode[G::ID - 1];
    const size_t piece = decode_chunk_points(ctx), rec = sizeof(typename G::F), head = 0;
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        VSP_TRY(ensure(ctx, ctx->tally_raw, rec * m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, in + rec * at, rec * m, hipMemcpyHostToDevice, st));
        VSP_TRY(decode_points<G>(ctx, m, 1, rec, &head, 1, check_subgroup));
        VSP_TRY(export_points(ctx, (Point *)w.pts.p, (const uint8_t *)w.pstatus.p, m, out_affine + G::AFFINE_WORDS * at));
        VSP_HIP(hipMemcpyAsync(status_out + at, w.pstatus.p, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        decode_add_times<G>(ctx, check_subgroup != 0);
    }
    return VSP_OK;
}

}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_g1_decompress_batch(vsp_ctx *ctx, const uint8_t *in, size_t n, int check_subgroup, uint64_t *out_affine, uint8_t *status_out) {
    return decompress_batch<G1>(ctx, in, n, check_subgroup, out_affine, status_out);
}
int vsp_g2_decompress_batch(vsp_ctx *ctx, const uint8_t *in, size_t n, int check_subgroup, uint64_t *out_affine, uint8_t *status_out) {
    return decompress_batch<G2>(ctx, in, n, check_subgroup, out_affine, status_out);
}

int vsp_proof_from_blob_batch(vsp_ctx *ctx, const uint8_t *blobs, size_t n, int check_subgroup, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out,
                              uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!blobs || !status_out) return set_error(ctx, VSP_ERR_ARG, "proof_from_blob_batch: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    size_t piece = decode_chunk_points(ctx) / 3;                    // proofs of one piece: three points each, at least one proof
    if (piece < 1) piece = 1;
    const size_t heads[2] = {0, 144}, head_b = 48;                  // A and C; B lies between them
    DecodeWork &w1 = ctx->decode[0], &w2 = ctx->decode[1];
    for (size_t at = 0; at < n; at += piece) {
        const size_t m = n - at < piece ? n - at : piece;
        VSP_TRY(ensure(ctx, ctx->tally_raw, 192 * m));
        VSP_TRY(ensure(ctx, ctx->tally_bstatus, m));
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, blobs + 192 * at, 192 * m, hipMemcpyHostToDevice, st));
        VSP_TRY(decode_points<G1>(ctx, m, 1, 192, heads, 2, check_subgroup));     // A: points [0, m), C: [m, 2m)
        VSP_TRY(decode_points<G2>(ctx, m, 1, 192, &head_b, 1, check_subgroup));
        const uint8_t *pstatus = (const uint8_t *)ctx->tally_bstatus.p;
        VSP_TRY(decode_proof_status(ctx, m, (uint8_t *)ctx->tally_bstatus.p));
        if (A_out) VSP_TRY(export_points(ctx, (G1Affine *)w1.pts.p, pstatus, m, A_out + 12 * at));
        if (C_out) VSP_TRY(export_points(ctx, (G1Affine *)w1.pts.p + m, pstatus, m, C_out + 12 * at));
        if (B_out) VSP_TRY(export_points(ctx, (G2Affine *)w2.pts.p, pstatus, m, B_out + 24 * at));
        VSP_HIP(hipMemcpyAsync(status_out + at, pstatus, m, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        decode_add_times<G1>(ctx, check_subgroup != 0);
        decode_add_times<G2>(ctx, check_subgroup != 0);
    }
    return VSP_OK;
}

}  // extern "C"
