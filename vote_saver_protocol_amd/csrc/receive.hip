// Ballots received from their blobs (include/vsp.h "ballots received from their blobs"): the ballot box's receiving
// step as one call -- the wire in, verdicts and a running tally out; every point is decoded once and no limb crosses PCIe.  The
// meaning is the composition of vsp_tally_add_blobs, vsp_proof_from_blob_batch, vsp_fr_vector_from_blob and one of the verify calls
// (tests/test_gpu_saver_receive.py computes it).  Stages per piece of a call, on the context's stream:
//   1. the ciphertext blobs: k_point_decode<G1> and k_subgroup_check (decode.hip) into the receive path's own workspace, ballot-major,
//      where the members stay until the piece is finished; k_tally_ballots (tally.hip): wire status byte 0
//   2. the proof blobs, into the same raw buffer behind stage 1: A and C into ctx->decode[0], B into ctx->decode[1]; k_proof_status:
//      wire status byte 1
//   3. k_receive_scalars  one lane per (ballot, scalar): the input blob's 32 big-endian bytes -> canonical words, scalar below r, the
//                         count header (the ballot's first lane): wire status byte 2
//   4. the verdicts: the screened check (screen.hip screen_piece) or the exact path (pairing.hip saver_verify_source) over the source
//      "range [lo, hi) of the decoded piece", which
//      k_receive_prepare  one lane per ballot of the range, the counterpart of k_ballot_prepare over decoded points: gathers the members
//                         column by column, acc, C, A, B; a wire-rejected ballot gets a status byte that is not zero
//      serves as often as the verifiers ask: the whole piece, then the failing sub-ranges on their way to the exact path
//   5. the tally: a byte per ballot "not accepted" in place of the tally's ballot status, k_tally_colsum over the resident members, the
//      partial sums folded on the host (tally.hip tally_fold) -- after the verdicts, so a piece is added whole or not at all
// With a ballot box (vsp_ballot_box_receive_blobs; ballot_box.hip) the same path has three more steps: k_box_screen
// behind stage 3 writes a fourth status row, which k_receive_prepare ORs in -- a ballot of another election or with a spent serial is
// to the verifiers what a wire-rejected one is, and a piece of nothing else never reaches them --; behind the verdicts the accepted
// ballots claim their serials, the losers among equal serials leave the tally's sum, and after the sum the winners are committed.
#include "common.h"
#include "pairing.h"
#include "pairing_g1.h"
#include "receive.h"
#include "ballot_box.h"

namespace vsp {

static constexpr unsigned RECEIVE_THREADS = 64;                    // one wave per block, as the pairing kernels (k_ballot_prepare)

// lane (k, i) of a piece of pc ballots with L rest inputs each: scalar i of ballot k to rest[(k L + i) 8 ..]; status[k] (zeroed by the
// caller, 4-byte aligned) becomes 1 for a wrong count header or a scalar >= r
__global__ __launch_bounds__(256) void k_receive_scalars(const uint8_t *__restrict__ blobs, size_t pc, size_t L, uint32_t *__restrict__ rest, uint8_t *status) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, lanes = recv_scalar_lanes(L);
    if (t >= pc * lanes) return;
    const size_t k = t / lanes, i = t % lanes;
    const uint32_t *w = (const uint32_t *)(blobs + k * recv_input_blob_bytes(L));
    bool bad = i == 0 && !recv_header_ok(w[0], w[1], L);
    if (i < L) {
        uint32_t s[8];
        if (!recv_scalar_decode(w + 2 + 8 * i, s)) bad = true;
        uint4 *out = (uint4 *)(rest + (k * L + i) * 8);
        out[0] = make_uint4(s[0], s[1], s[2], s[3]);
        out[1] = make_uint4(s[4], s[5], s[6], s[7]);
    }
    if (bad) atomicOr((uint32_t *)(status + (k & ~(size_t)3)), 1u << (8 * (unsigned)(k & 3)));
}

// ballot lo + k of a decoded piece of pc ballots becomes ballot k of a verifier's piece of c: what k_ballot_prepare writes, from points
// that are on their curves by construction (receive.h: the index maps).  status[k]: the OR of the three wire status bytes and, where
// a ballot box gave one (box_row not null), of its row
__global__ __launch_bounds__(RECEIVE_THREADS) void k_receive_prepare(const G1Affine *__restrict__ members, const G1Affine *__restrict__ ac, const G2Affine *__restrict__ b_in,
                                                                     const uint32_t *__restrict__ rest, const uint8_t *__restrict__ wire, size_t wire_stride, size_t pc, size_t lo,
                                                                     size_t c, size_t n, size_t n_abc, const G1Affine *__restrict__ tab, G1Affine *__restrict__ pts,
                                                                     G1Affine *__restrict__ a_out, G2Affine *__restrict__ b_out, uint8_t *__restrict__ status,
                                                                     const uint8_t *__restrict__ box_row) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const size_t ballot = lo + k;
    uint32_t st = wire[ballot] | wire[wire_stride + ballot] | wire[2 * wire_stride + ballot];
    if (box_row) st |= box_row[ballot];
    G1Affine P = ac[recv_a_index(pc, ballot)];
    a_out[k] = P;
    b_out[k] = b_in[ballot];
    P = ac[recv_c_index(pc, ballot)];
    pts[recv_column_index(c, n + 3, k)] = P;
    const size_t L = n_abc - 1 - n;
    G1XYZZ acc;
    pr_ballot_acc_start(acc, rest + ballot * L * 8, L, n, tab);
#pragma unroll 1
    for (size_t j = 0; j < n + 2; j++) {
        P = members[recv_member_index(n, ballot, j)];
        pts[recv_column_index(c, j, k)] = P;
        if (j <= n) pr_madd(&acc, &P);                              // psi (j = n + 1) is no summand
    }
    pts[recv_column_index(c, n + 2, k)] = pr_to_affine(acc);
    status[k] = (uint8_t)st;
}

int receive_piece_prepare(vsp_ctx *ctx, const vsp_saver_verifier *ver, const ReceivedPiece &rp, size_t lo, size_t c, void *d_pts, void *d_a, void *d_b, uint8_t *d_status) {
    if (lo > rp.count || c > rp.count - lo) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: a range outside the decoded piece");
    hipLaunchKernelGGL(k_receive_prepare, dim3((unsigned)((c + RECEIVE_THREADS - 1) / RECEIVE_THREADS)), dim3(RECEIVE_THREADS), 0, ctx->stream, (const G1Affine *)rp.members,
                       (const G1Affine *)rp.ac, (const G2Affine *)rp.b, rp.rest, rp.wire, rp.wire_stride, rp.count, lo, c, ver->n, ver->vk->n_abc,
                       ver->vk->d_tab.as<const G1Affine>(), (G1Affine *)d_pts, (G1Affine *)d_a, (G2Affine *)d_b, d_status, rp.box_row);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

namespace {

struct ReceiveCall {
    vsp_ctx *ctx; const vsp_saver_verifier *ver; vsp_tally *tally;
    const uint8_t *ct_blobs, *proof_blobs, *input_blobs;
    size_t count; int check_subgroup; const uint64_t *coeff;
    uint8_t *verdict_out, *reason_out, *wire_status_out; size_t *accepted_out;
    vsp_ballot_box *box; uint64_t *holder_out;                      // vsp_ballot_box_receive_blobs; null: no box
};

int receive_pieces(const ReceiveCall &rc) {
    vsp_ctx *ctx = rc.ctx;
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = rc.ver->n, ct_len = n + 2, L = rc.ver->vk->n_abc - 1 - n;
    const size_t ct_bytes = 8 + 48 * ct_len, in_bytes = recv_input_blob_bytes(L), head_ct = 8, heads_ac[2] = {0, 144}, head_b = 48;
    // ballots of one piece: the verifier's piece and the decoder's, at least one
    size_t piece = rc.coeff ? screen_piece_ballots(ctx) : saver_exact_piece(ctx, n);
    if (piece > decode_chunk_points(ctx) / ct_len) piece = decode_chunk_points(ctx) / ct_len;
    if (piece < 1) piece = 1;
    std::vector<uint8_t> h_wire, h_skip;
    std::vector<XYZZ<HFp>> h_part;
    size_t accepted = 0, wire_rejected = 0;
    for (size_t at = 0; at < rc.count; at += piece) {
        const size_t c = rc.count - at < piece ? rc.count - at : piece, stride = recv_wire_stride(c), rows = rc.box ? 4 : 3;
        VSP_TRY(ensure(ctx, ctx->tally_raw, c * (ct_bytes > 192 ? ct_bytes : 192)));
        VSP_TRY(ensure(ctx, ctx->tally_bstatus, c));
        VSP_TRY(ensure(ctx, ctx->recv_members, c * ct_len * sizeof(G1Affine)));
        VSP_TRY(ensure(ctx, ctx->recv_mstatus, c * ct_len));
        VSP_TRY(ensure(ctx, ctx->recv_wire, rows * stride));
        VSP_TRY(ensure(ctx, ctx->recv_raw, c * in_bytes));
        VSP_TRY(ensure(ctx, ctx->recv_rest, c * L * 32));
        uint8_t *wire = (uint8_t *)ctx->recv_wire.p;
        // 1. the ciphertext members: decoded once, resident until the piece is finished
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, rc.ct_blobs + at * ct_bytes, c * ct_bytes, hipMemcpyHostToDevice, st));
        VSP_TRY(decode_points<G1>(ctx, c * ct_len, ct_len, ct_bytes, &head_ct, 1, rc.check_subgroup, (G1Affine *)ctx->recv_members.p, (uint8_t *)ctx->recv_mstatus.p));
        tally_ballots_launch(ctx, (const uint8_t *)ctx->tally_raw.p, c, ct_len, (const uint8_t *)ctx->recv_mstatus.p, wire);
        VSP_LAUNCH_CHECK();
        VSP_HIP(hipStreamSynchronize(st));                           // the decoder's timers serve the proofs next
        decode_add_times<G1>(ctx, rc.check_subgroup != 0);
        // 2. the proofs, behind k_tally_ballots in the raw buffer
        VSP_HIP(hipMemcpyAsync(ctx->tally_raw.p, rc.proof_blobs + at * 192, c * 192, hipMemcpyHostToDevice, st));
        VSP_TRY(decode_points<G1>(ctx, c, 1, 192, heads_ac, 2, rc.check_subgroup));
        VSP_TRY(decode_points<G2>(ctx, c, 1, 192, &head_b, 1, rc.check_subgroup));
        VSP_TRY(decode_proof_status(ctx, c, wire + stride));
        // 3. the rest inputs
        VSP_HIP(hipMemsetAsync(wire + 2 * stride, 0, stride, st));
        if (rc.input_blobs) VSP_HIP(hipMemcpyAsync(ctx->recv_raw.p, rc.input_blobs + at * in_bytes, c * in_bytes, hipMemcpyHostToDevice, st));
        VSP_TRY(ctx->recv_timer.mark(ctx, 0, st));
        if (rc.input_blobs) {
            hipLaunchKernelGGL(k_receive_scalars, dim3((unsigned)((c * recv_scalar_lanes(L) + 255) / 256)), dim3(256), 0, st, (const uint8_t *)ctx->recv_raw.p, c, L,
                               (uint32_t *)ctx->recv_rest.p, wire + 2 * stride);
            VSP_LAUNCH_CHECK();
        }
        VSP_TRY(ctx->recv_timer.mark(ctx, 1, st));
        if (rc.box) VSP_TRY(box_piece_screen(ctx, rc.box, (const uint32_t *)ctx->recv_rest.p, c, wire + 3 * stride));
        h_wire.resize(rows * stride);
        VSP_HIP(hipMemcpyAsync(h_wire.data(), wire, rows * stride, hipMemcpyDeviceToHost, st));
        // the box's row decides before the verifier: a piece in which it (or the wire) has turned every ballot away is not verified
        bool verify = true;
        if (rc.box) {
            VSP_HIP(hipStreamSynchronize(st));
            verify = false;
            for (size_t k = 0; k < c; k++) verify = verify || !(h_wire[k] | h_wire[stride + k] | h_wire[2 * stride + k] | h_wire[3 * stride + k]);
        }
        // 4. the verdicts, from the decoded piece (every buffer it names stays as it is until the piece is finished)
        ReceivedPiece rp;
        rp.base = at; rp.count = c; rp.wire_stride = stride;
        rp.members = ctx->recv_members.p; rp.ac = ctx->decode[0].pts.p; rp.b = ctx->decode[1].pts.p;
        rp.rest = (const uint32_t *)ctx->recv_rest.p; rp.wire = wire;
        if (rc.box) rp.box_row = wire + 3 * stride;
        BallotSource src;
        src.dev = &rp;
        if (!verify) {
            for (size_t k = 0; k < c; k++) { rc.verdict_out[at + k] = 0; if (rc.reason_out) rc.reason_out[at + k] = 1; }
        } else if (rc.coeff) VSP_TRY(screen_piece(ctx, rc.ver, src, at, c, rc.coeff, rc.verdict_out, rc.reason_out));
        else VSP_TRY(saver_verify_source(ctx, rc.ver, src, at, c, rc.verdict_out + at, rc.reason_out ? rc.reason_out + at : nullptr));
        // (both have waited for the stream)
        decode_add_times<G1>(ctx, rc.check_subgroup != 0);
        decode_add_times<G2>(ctx, rc.check_subgroup != 0);
        ctx->recv_timer.add(ctx, 0, "saver_receive_prepare_ms");
        if (rc.box) {
            // the reasons of the ballots the box turned away (the verifiers called them malformed); the wire's rejection goes first
            size_t mismatched = 0, spent = 0;
            for (size_t k = 0; k < c; k++) {
                if (rc.holder_out) rc.holder_out[at + k] = ~(uint64_t)0;
                const uint8_t row = h_wire[3 * stride + k];
                if (!row || (h_wire[k] | h_wire[stride + k] | h_wire[2 * stride + k])) continue;
                if (rc.reason_out) rc.reason_out[at + k] = row;
                if (row == 16 && rc.holder_out) rc.holder_out[at + k] = rc.box->h_hold[k];
                mismatched += row == 8; spent += row == 16;
            }
            ctx->stats["ballot_box_mismatched"] += (double)mismatched;
            ctx->stats["ballot_box_spent"] += (double)spent;
        }
        size_t ok = 0;
        for (size_t k = 0; k < c; k++) {
            const uint8_t w0 = h_wire[k], w1 = h_wire[stride + k], w2 = h_wire[2 * stride + k];
            if (rc.wire_status_out) { rc.wire_status_out[3 * (at + k)] = w0; rc.wire_status_out[3 * (at + k) + 1] = w1; rc.wire_status_out[3 * (at + k) + 2] = w2; }
            wire_rejected += (w0 | w1 | w2) != 0;
            ok += rc.verdict_out[at + k] != 0;
        }
        // 5. the tally: exactly the accepted ballots, from the members already here
        if (rc.tally || rc.box) {
            size_t parts = 0;
            h_skip.resize(c);
            for (size_t k = 0; k < c; k++) h_skip[k] = rc.verdict_out[at + k] ? 0 : 1;
            // (a ballot the verifier itself refused tells the box so: ballot_box.h BOX_SKIP_REFUSED)
            for (size_t k = 0; rc.box && k < c; k++)
                if (h_skip[k] && !(h_wire[k] | h_wire[stride + k] | h_wire[2 * stride + k] | h_wire[3 * stride + k])) h_skip[k] = BOX_SKIP_REFUSED;
            VSP_HIP(hipMemcpyAsync(ctx->tally_bstatus.p, h_skip.data(), c, hipMemcpyHostToDevice, st));
            // the accepted ballots claim their serials; the losers among equal ones raise their skip bytes
            if (rc.box) VSP_TRY(box_piece_settle(ctx, rc.box, c, (uint8_t *)ctx->tally_bstatus.p));
            StageTimer &t = ctx->decode[0].timer;
            if (rc.tally) {
                VSP_TRY(t.mark(ctx, 2, st));
                VSP_TRY(tally_colsum_launch(ctx, ctx->recv_members.p, (const uint8_t *)ctx->tally_bstatus.p, c, ct_len, h_part, &parts, &t));
            }
            VSP_HIP(hipStreamSynchronize(st));
            if (rc.tally) t.add(ctx, 2, "tally_sum_ms");
            // the box takes the piece first (the last step that can fail), then the handle
            if (rc.box) {
                VSP_TRY(box_piece_commit(ctx, rc.box, c, rc.verdict_out + at, rc.reason_out ? rc.reason_out + at : nullptr, rc.holder_out ? rc.holder_out + at : nullptr, false,
                                         &ok));
                box_add_times(ctx, rc.box, true, true);
            }
            // nothing of this piece has touched the handle before this point
            if (rc.tally) tally_fold(rc.tally, h_part, parts, ok);
        }
        accepted += ok;
        if (rc.accepted_out) *rc.accepted_out = accepted;
        ctx->stats["saver_receive_ballots"] += (double)c;
    }
    ctx->stats["saver_receive_wire_rejected"] += (double)wire_rejected;
    return VSP_OK;
}

}  // anonymous namespace
}  // namespace vsp

using namespace vsp;

extern "C" int vsp_saver_receive_blobs(vsp_ctx *ctx, const vsp_saver_verifier *ver, vsp_tally *tally, const uint8_t *ct_blobs, const uint8_t *proof_blobs,
                                       const uint8_t *input_blobs, size_t count, int check_subgroup, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out,
                                       uint8_t *wire_status_out, size_t *accepted_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (accepted_out) *accepted_out = 0;
    if (!ver || !ct_blobs || !proof_blobs || !verdict_out || (!input_blobs && saver_verifier_n_rest(ver) > 0)) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: null argument");
    if (tally && tally_ct_len(tally) != ver->n + 2) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: the tally's ct_len is not msg_size + 2");
    if (ver->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: the verifier belongs to another device");
    if (coeff) {
        for (size_t k = 0; k < count; k++)
            if (!(coeff[2 * k] | coeff[2 * k + 1])) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: a coefficient is zero");
        if (ctx->prove.active) return set_error(ctx, VSP_ERR_ARG, "saver_receive_blobs: a proof is in flight on this context and owns the work slots (finish it first)");
    }
    if (!count) return VSP_OK;
    const ReceiveCall rc{ctx, ver, tally, ct_blobs, proof_blobs, input_blobs, count, check_subgroup, coeff, verdict_out, reason_out, wire_status_out, accepted_out, nullptr, nullptr};
    const int r = receive_pieces(rc);
    if (r != VSP_OK && coeff) msm_drain_slots(ctx);                  // nothing stays in flight on the work slots after an error
    return r;
}

extern "C" int vsp_ballot_box_receive_blobs(vsp_ctx *ctx, vsp_ballot_box *box, vsp_tally *tally, const uint8_t *ct_blobs, const uint8_t *proof_blobs, const uint8_t *input_blobs,
                                            size_t count, int check_subgroup, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out, uint8_t *wire_status_out,
                                            size_t *accepted_out, uint64_t *holder_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (accepted_out) *accepted_out = 0;
    if (!box || !ct_blobs || !proof_blobs || !input_blobs || !verdict_out) return set_error(ctx, VSP_ERR_ARG, "ballot_box_receive_blobs: null argument");
    const vsp_saver_verifier *ver = box->ver;
    if (tally && tally_ct_len(tally) != ver->n + 2) return set_error(ctx, VSP_ERR_ARG, "ballot_box_receive_blobs: the tally's ct_len is not msg_size + 2");
    if (box->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "ballot_box_receive_blobs: the box belongs to another device");
    if (coeff) {
        for (size_t k = 0; k < count; k++)
            if (!(coeff[2 * k] | coeff[2 * k + 1])) return set_error(ctx, VSP_ERR_ARG, "ballot_box_receive_blobs: a coefficient is zero");
        if (ctx->prove.active) return set_error(ctx, VSP_ERR_ARG, "ballot_box_receive_blobs: a proof is in flight on this context and owns the work slots (finish it first)");
    }
    if (!count) return VSP_OK;
    const ReceiveCall rc{ctx, ver, tally, ct_blobs, proof_blobs, input_blobs, count, check_subgroup, coeff, verdict_out, reason_out, wire_status_out, accepted_out, box, holder_out};
    const int r = receive_pieces(rc);
    if (r != VSP_OK) {
        if (coeff) msm_drain_slots(ctx);
        // the box as it was after the last complete piece: the slots a broken piece claimed go with a rebuilt table
        if (box->dirty) {
            const std::string err = ctx->err;
            if (box_restore(ctx, box) == VSP_OK) ctx->err = err;
        }
    }
    return r;
}
