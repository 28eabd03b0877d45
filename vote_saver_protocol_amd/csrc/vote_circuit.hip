// The voting circuit (include/vsp.h "the voting circuit"): the statement as three CSR matrices built on the host from the
// hash's table, and the witnesses of ballots filled in batches on the device.  The rules -- where every wire and row lies, what every row
// says, what every wire holds -- are vote_circuit.h, which the CPU test build runs too.  Kernels:
//   k_vote_chains   a lane per (ballot, hash): the hash's message is read where it lies (sk, the eid | sk row, two children in the
//                   registry's tree, the pk digest of the launch before); the chain keeps every prefix sum, one inversion makes them
//                   affine (vc_chain); the digest is stored and compared with the registry's node it must equal -- a mismatch is status 1.
//                   Two launches: PK, then every other hash (LEAF reads PK's digest)
//   k_vote_fill_wires / k_vote_fill_chunks   the two halves of vc_fill_item: a lane per (ballot, wire below the chunk region), and a
//                   lane per (ballot, chunk) for the chunk's 2 or 8 wires
// Loop bounds: the chunks of a hash (at most 63 g) twice, the 255 steps of the inversion, 254 steps of a packing or a run wire's position,
// depth + 3 steps to find a chunk's hash.  No kernel waits for another workgroup; there is no spinning; every store is a plain one.
#include <memory>
#include "common.h"
#include "jubjub.h"
#include "vote_circuit.h"

struct vsp_vote_circuit {
    int device = 0;
    vsp::VcParams P{};
    const vsp_pedersen *ped = nullptr;          // the hash (must outlive the circuit): its device table runs the chains
    vsp_r1cs *cs = nullptr;
    vsp::VcCsr csr;                             // the matrices as they were uploaded
    std::vector<vsp::JjEntry<vsp::HFr>> tab;    // the hash's table, read back once
    std::vector<vsp::JjAffine<vsp::HFr>> aff;   // its points (u, v)
    // one piece of witnesses on the device: the affine table; sk | eid | the eid | sk rows | indices | votes; a status word per ballot;
    // digests; the chains' slots; the witnesses
    vsp::DevBuf d_aff, in, status, digests, slots, wit;
    bool wit_live = false;                      // witnesses of a device call stay in `wit` until the next release (vsp_cast_witness_release)
    vsp::StageTimer timer;
};

namespace vsp {
namespace {

static constexpr unsigned VW_PIECE = 64;                    // ballots of one piece
static constexpr unsigned VW_CHAIN_THREADS = 64, VW_FILL_THREADS = 256;

struct VwJob {
    VcParams P;
    uint32_t count;
    const uint64_t *sk, *eid, *sn_rows, *index;
    size_t sn_words;
    const uint32_t *vote;
    uint32_t *status;
    const uint64_t *nodes;
    uint64_t *digests;
    VcSlot<Fr> *slots;
    uint64_t *wit;
};

__global__ __launch_bounds__(VW_CHAIN_THREADS) void k_vote_chains(const JjEntry<Fr> *__restrict__ tab, VwJob job, uint32_t first_hash, uint32_t hashes) {
    const uint32_t t = blockIdx.x * VW_CHAIN_THREADS + threadIdx.x;
    if (t >= job.count * hashes) return;
    const uint32_t k = t / hashes, h = first_hash + t % hashes;
    if (job.status[k] == 2) return;
    const VcParams &P = job.P;
    const uint32_t H = vc_hashes(P);
    const uint64_t x = job.index[k];
    JjMessage m;
    m.nbits = vc_hash_bits(P, h); m.gap = 0;
    const uint64_t *expect = nullptr;
    if (h == vc_hash_sn(P)) m.w = job.sn_rows + (size_t)k * job.sn_words;
    else if (h == 0) m.w = job.sk + 4 * (size_t)k;
    else if (h < vc_hash_node(P, 0)) m.w = job.digests + 4 * (size_t)k * H;
    else {
        const uint32_t l = h - vc_hash_node(P, 0);
        m.w = job.nodes + 4 * jj_level_first(P.depth, l) + 8 * ((x >> l) >> 1);
        m.gap = 1;
        expect = job.nodes + 4 * (jj_level_first(P.depth, l + 1) + (x >> (l + 1)));
    }
    if (h == vc_hash_leaf(P)) expect = job.nodes + 4 * (jj_level_first(P.depth, 0) + x);
    uint64_t d[4];
    vc_chain(tab, m, job.slots + (size_t)k * vc_total_chunks(P) + vc_chunks_before(P, h), d);
    uint64_t *o = job.digests + 4 * ((size_t)k * H + h);
    o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3];
    if (expect && ((d[0] ^ expect[0]) | (d[1] ^ expect[1]) | (d[2] ^ expect[2]) | (d[3] ^ expect[3]))) job.status[k] = 1;
}

__device__ __forceinline__ VcBallot<Fr> vw_ballot(const VwJob &job, uint32_t k) {
    VcBallot<Fr> b;
    b.sk = job.sk + 4 * (size_t)k; b.eid = job.eid; b.index = job.index[k]; b.vote = job.vote[k];
    b.nodes = job.nodes; b.tree = true;
    b.digests = job.digests + 4 * (size_t)k * vc_hashes(job.P);
    b.slots = job.slots + (size_t)k * vc_total_chunks(job.P);
    return b;
}
// the two halves of vc_fill_item: the wires below the chunk region, `per` = vc_w_chunk of them a ballot ...
__global__ __launch_bounds__(VW_FILL_THREADS) void k_vote_fill_wires(VwJob job, uint32_t per) {
    const uint64_t t = (uint64_t)blockIdx.x * VW_FILL_THREADS + threadIdx.x;
    if (t >= (uint64_t)job.count * per) return;
    const uint32_t k = (uint32_t)(t / per), item = (uint32_t)(t % per);
    if (job.status[k] != 0) return;
    uint64_t val[4];
    vc_wire_value(job.P, vw_ballot(job, k), item, val);
    uint64_t *o = job.wit + 4 * ((size_t)k * vc_num_vars(job.P) + item);
    o[0] = val[0]; o[1] = val[1]; o[2] = val[2]; o[3] = val[3];
}
// ... and the chunks, `per` = vc_total_chunks of them a ballot
__global__ __launch_bounds__(VW_FILL_THREADS) void k_vote_fill_chunks(const JjAffine<Fr> *__restrict__ aff, VwJob job, uint32_t per) {
    const uint64_t t = (uint64_t)blockIdx.x * VW_FILL_THREADS + threadIdx.x;
    if (t >= (uint64_t)job.count * per) return;
    const uint32_t k = (uint32_t)(t / per), item = (uint32_t)(t % per);
    if (job.status[k] != 0) return;
    vc_fill_chunk(job.P, aff, vw_ballot(job, k), item, job.wit + 4 * (size_t)k * vc_num_vars(job.P));
}

unsigned vw_blocks(uint64_t lanes, unsigned threads) { return (unsigned)((lanes + threads - 1) / threads); }

void circuit_release(vsp_ctx *ctx, vsp_vote_circuit *c) {
    if (c->wit_live && c->wit.p) { hipMemset(c->wit.p, 0, c->wit.cap); c->wit_live = false; }
    if (c->cs) vsp_r1cs_free(ctx, c->cs);
    delete c;
}

// the stream-ordered zeroing of the witnesses a device call left in the circuit's buffer
void witness_release(vsp_ctx *ctx, vsp_vote_circuit *circ) {
    if (circ->wit_live && circ->wit.p) hipMemsetAsync(circ->wit.p, 0, circ->wit.cap, ctx->stream);
    circ->wit_live = false;
}

// one piece: ballots [at, at + c) of the call.  wit_out null: the device form -- the witnesses stay in the circuit's buffer (member k at
// row k, vc_num_vars values a row), only the status words come to the host, and the buffer is zeroed by the next release, not here
int witness_piece(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const uint64_t *eid, const uint64_t *sks, const uint64_t *indices, const uint32_t *votes,
                  size_t c, uint64_t *wit_out, uint8_t *status_out) {
    const VcParams &P = circ->P;
    hipStream_t st = ctx->stream;
    const size_t H = vc_hashes(P), nv = vc_num_vars(P), chunks = vc_total_chunks(P);
    const size_t eid_words = (P.eid_bits + 63) / 64, sn_words = (vc_sn_bits(P) + 63) / 64 + 1;
    // the host's share: status 2, the eid | sk rows
    std::vector<uint32_t> h_status(c, 0), h_vote(c, 0);
    const size_t in_words = 4 * c + eid_words + c * sn_words + c;
    std::vector<uint64_t> h_in(in_words, 0);
    uint64_t *h_sk = h_in.data(), *h_eid = h_sk + 4 * c, *h_sn = h_eid + eid_words, *h_index = h_sn + c * sn_words;
    for (size_t w = 0; w < eid_words; w++) h_eid[w] = eid[w];
    if (P.eid_bits % 64) h_eid[eid_words - 1] &= ~(uint64_t)0 >> (64 - P.eid_bits % 64);
    size_t live = 0;
    for (size_t k = 0; k < c; k++) {
        const uint64_t *sk = sks + 4 * k;
        if (votes[k] >= P.n || (indices[k] >> P.depth) || (sk[3] >> 63)) { h_status[k] = 2; continue; }
        live++;
        memcpy(h_sk + 4 * k, sk, 4 * sizeof(uint64_t));
        h_index[k] = indices[k]; h_vote[k] = votes[k];
        uint64_t *row = h_sn + k * sn_words;
        for (uint32_t i = 0; i < vc_sn_bits(P); i++) row[i >> 6] |= (uint64_t)(i < P.eid_bits ? vc_word_bit(h_eid, i) : vc_word_bit(sk, i - P.eid_bits)) << (i & 63);
    }
    const size_t wit_bytes = c * nv * 4 * sizeof(uint64_t);
    auto wipe_host = [&]() { volatile uint64_t *p = h_in.data(); for (size_t i = 0; i < in_words; i++) p[i] = 0; };
    witness_release(ctx, circ);
    if (!live) {
        if (wit_out) memset(wit_out, 0, wit_bytes);
        else {                                  // no member reaches the kernels: all-zero rows, as the host form returns them
            VSP_TRY(ensure(ctx, circ->wit, wit_bytes));
            VSP_HIP(hipMemsetAsync(circ->wit.p, 0, wit_bytes, st));
        }
        for (size_t k = 0; k < c; k++) status_out[k] = (uint8_t)h_status[k];
        wipe_host();
        return VSP_OK;
    }
    const size_t slot_bytes = c * chunks * sizeof(VcSlot<Fr>), digest_bytes = c * H * 4 * sizeof(uint64_t);
    auto run = [&]() -> int {
        VSP_TRY(ensure(ctx, circ->in, in_words * sizeof(uint64_t) + c * sizeof(uint32_t)));
        VSP_TRY(ensure(ctx, circ->status, c * sizeof(uint32_t)));
        VSP_TRY(ensure(ctx, circ->digests, digest_bytes));
        VSP_TRY(ensure(ctx, circ->slots, slot_bytes));
        VSP_TRY(ensure(ctx, circ->wit, wit_bytes));
        uint64_t *d_in = (uint64_t *)circ->in.p;
        VwJob job;
        job.P = P; job.count = (uint32_t)c;
        job.sk = d_in; job.eid = d_in + 4 * c; job.sn_rows = job.eid + eid_words; job.index = job.sn_rows + c * sn_words; job.sn_words = sn_words;
        job.vote = (const uint32_t *)(d_in + in_words);
        job.status = (uint32_t *)circ->status.p;
        job.nodes = (const uint64_t *)reg->nodes.p;
        job.digests = (uint64_t *)circ->digests.p; job.slots = (VcSlot<Fr> *)circ->slots.p; job.wit = (uint64_t *)circ->wit.p;
        VSP_HIP(hipMemcpyAsync(d_in, h_in.data(), in_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemcpyAsync(d_in + in_words, h_vote.data(), c * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemcpyAsync(circ->status.p, h_status.data(), c * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemsetAsync(circ->wit.p, 0, wit_bytes, st));
        VSP_TRY(circ->timer.mark(ctx, 0, st));
        const JjEntry<Fr> *tab = (const JjEntry<Fr> *)circ->ped->table.p;
        hipLaunchKernelGGL(k_vote_chains, dim3(vw_blocks(c, VW_CHAIN_THREADS)), dim3(VW_CHAIN_THREADS), 0, st, tab, job, 0u, 1u);
        VSP_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_vote_chains, dim3(vw_blocks(c * (H - 1), VW_CHAIN_THREADS)), dim3(VW_CHAIN_THREADS), 0, st, tab, job, 1u, (uint32_t)(H - 1));
        VSP_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_vote_fill_wires, dim3(vw_blocks((uint64_t)c * vc_w_chunk(P), VW_FILL_THREADS)), dim3(VW_FILL_THREADS), 0, st, job, vc_w_chunk(P));
        VSP_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_vote_fill_chunks, dim3(vw_blocks((uint64_t)c * chunks, VW_FILL_THREADS)), dim3(VW_FILL_THREADS), 0, st, (const JjAffine<Fr> *)circ->d_aff.p, job,
                           (uint32_t)chunks);
        VSP_LAUNCH_CHECK();
        VSP_TRY(circ->timer.mark(ctx, 1, st));
        VSP_HIP(hipMemcpyAsync(h_status.data(), circ->status.p, c * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (wit_out) {
            VSP_HIP(hipMemcpyAsync(wit_out, circ->wit.p, wit_bytes, hipMemcpyDeviceToHost, st));
            ctx->stats["vote_witness_d2h_bytes"] += (double)wit_bytes;
        }
        VSP_HIP(hipStreamSynchronize(st));
        circ->timer.add(ctx, 0, "vote_witness_ms");
        return VSP_OK;
    };
    const int r = run();
    // the call's device copies of sk and of everything derived from it are zeroed before it returns, whatever happened
    hipStreamSynchronize(st);
    if (circ->in.p) hipMemsetAsync(circ->in.p, 0, circ->in.cap, st);
    if (circ->digests.p) hipMemsetAsync(circ->digests.p, 0, circ->digests.cap, st);
    if (circ->slots.p) hipMemsetAsync(circ->slots.p, 0, circ->slots.cap, st);
    if (circ->wit.p && (wit_out || r != VSP_OK)) hipMemsetAsync(circ->wit.p, 0, circ->wit.cap, st);
    hipStreamSynchronize(st);
    wipe_host();
    if (r != VSP_OK) { if (wit_out) memset(wit_out, 0, wit_bytes); return r; }
    circ->wit_live = !wit_out;
    for (size_t k = 0; k < c; k++) status_out[k] = (uint8_t)h_status[k];
    return VSP_OK;
}

}  // anonymous namespace
}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_vote_circuit_create(vsp_ctx *ctx, const vsp_pedersen *ped, size_t msg_size, size_t eid_bits, unsigned depth, int hash_leaves, vsp_vote_circuit **out) {
    if (!ctx) return VSP_ERR_ARG;
    if (out) *out = nullptr;
    if (!ped || !out) return set_error(ctx, VSP_ERR_ARG, "vote_circuit_create: null argument");
    if (ped->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "vote_circuit_create: the hash's tables belong to another device");
    if (ped->g < JJ_NODE_GENERATORS) return set_error(ctx, VSP_ERR_ARG, "vote_circuit_create: a node hashes 510 bits: at least 3 generators are needed");
    if (depth > JJ_MAX_DEPTH) return set_error(ctx, VSP_ERR_UNSUPPORTED, "vote_circuit_create: depth above 24");
    if (msg_size == 0 || msg_size > ((size_t)1 << 20)) return set_error(ctx, VSP_ERR_ARG, "vote_circuit_create: msg_size of 1 to 2^20 expected");
    if (eid_bits == 0 || eid_bits + JJ_DIGEST_BITS > jj_max_bits(ped->g)) return set_error(ctx, VSP_ERR_ARG, "vote_circuit_create: eid | sk has 256 to 189 g bits");
    VSP_HIP(hipSetDevice(ctx->device));
    vsp_vote_circuit *c = new vsp_vote_circuit();
    c->device = ctx->device; c->ped = ped;
    c->P.n = (uint32_t)msg_size; c->P.eid_bits = (uint32_t)eid_bits; c->P.depth = depth; c->P.hash_leaves = hash_leaves ? 1 : 0;
    auto setup = [&]() -> int {
        const size_t entries = ped->g * JJ_GEN_ENTRIES;
        c->tab.resize(entries); c->aff.resize(entries);
        VSP_HIP(hipMemcpyAsync(c->tab.data(), ped->table.p, entries * sizeof(JjEntry<HFr>), hipMemcpyDeviceToHost, ctx->stream));      // the same bytes on either limb width
        VSP_HIP(hipStreamSynchronize(ctx->stream));
        vc_affine_table(c->tab.data(), entries, c->aff.data());
        VSP_TRY(ensure(ctx, c->d_aff, entries * sizeof(JjAffine<Fr>)));
        VSP_HIP(hipMemcpyAsync(c->d_aff.p, c->aff.data(), entries * sizeof(JjAffine<Fr>), hipMemcpyHostToDevice, ctx->stream));
        VSP_HIP(hipStreamSynchronize(ctx->stream));
        vc_build_csr(c->P, c->aff.data(), c->csr);
        c->cs = vsp_r1cs_upload(ctx, vc_num_constraints(c->P), vc_num_inputs(c->P), vc_num_vars(c->P), c->csr.row_ptr[0].data(), c->csr.col[0].data(), c->csr.coef[0].data(),
                                c->csr.row_ptr[1].data(), c->csr.col[1].data(), c->csr.coef[1].data(), c->csr.row_ptr[2].data(), c->csr.col[2].data(), c->csr.coef[2].data());
        return c->cs ? VSP_OK : VSP_ERR_HIP;
    };
    const int r = setup();
    if (r != VSP_OK) { circuit_release(ctx, c); return r; }
    *out = c;
    return VSP_OK;
}

void vsp_vote_circuit_free(vsp_ctx *ctx, vsp_vote_circuit *circ) {
    if (!circ) return;
    hipSetDevice(circ->device);
    if (ctx) hipStreamSynchronize(ctx->stream);
    circuit_release(ctx, circ);
}

const vsp_r1cs *vsp_vote_circuit_r1cs(const vsp_vote_circuit *circ) { return circ ? circ->cs : nullptr; }

int vsp_vote_circuit_sizes(const vsp_vote_circuit *circ, size_t *num_constraints_out, size_t *num_inputs_out, size_t *num_vars_out, size_t nnz_out[3]) {
    if (!circ) return VSP_ERR_ARG;
    if (num_constraints_out) *num_constraints_out = vc_num_constraints(circ->P);
    if (num_inputs_out) *num_inputs_out = vc_num_inputs(circ->P);
    if (num_vars_out) *num_vars_out = vc_num_vars(circ->P);
    if (nnz_out) for (int k = 0; k < 3; k++) nnz_out[k] = circ->csr.col[k].size();
    return VSP_OK;
}

int vsp_vote_circuit_csr(const vsp_vote_circuit *circ, int matrix, uint32_t *row_ptr_out, uint32_t *col_out, uint64_t *coef_out) {
    if (!circ || !row_ptr_out || !col_out || !coef_out || matrix < 0 || matrix > 2) return VSP_ERR_ARG;
    const VcCsr &m = circ->csr;
    memcpy(row_ptr_out, m.row_ptr[matrix].data(), m.row_ptr[matrix].size() * sizeof(uint32_t));
    memcpy(col_out, m.col[matrix].data(), m.col[matrix].size() * sizeof(uint32_t));
    memcpy(coef_out, m.coef[matrix].data(), m.coef[matrix].size() * sizeof(uint64_t));
    return VSP_OK;
}

int vsp_vote_circuit_wires(const vsp_vote_circuit *circ, int block, size_t *first_out, size_t *count_out) {
    if (!circ || !first_out || !count_out) return VSP_ERR_ARG;
    uint32_t first, count;
    if (!vc_block(circ->P, block, &first, &count)) return VSP_ERR_ARG;
    *first_out = first; *count_out = count;
    return VSP_OK;
}

int vsp_vote_witness_host(const vsp_vote_circuit *circ, const uint64_t *eid_bits_words, const uint64_t sk[4], uint64_t index, uint32_t vote, const uint64_t *copath,
                          uint64_t *witness_out, uint64_t leaf_out[4]) {
    if (!circ || !eid_bits_words || !sk || !witness_out || (circ->P.depth && !copath)) return VSP_ERR_ARG;
    if (vote >= circ->P.n || (index >> circ->P.depth) || (sk[3] >> 63)) return VSP_ERR_ARG;
    vc_witness_host<HFr>(circ->P, circ->tab.data(), circ->aff.data(), eid_bits_words, sk, index, vote, copath, witness_out, leaf_out);
    return VSP_OK;
}

int vsp_vote_witness_batch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const uint64_t *eid_bits_words, const uint64_t *sks, const uint64_t *indices,
                           const uint32_t *votes, size_t count, uint64_t *witnesses_out, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!circ || !reg || !eid_bits_words || !sks || !indices || !votes || !witnesses_out || !status_out) return set_error(ctx, VSP_ERR_ARG, "vote_witness_batch: null argument");
    if (circ->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "vote_witness_batch: the circuit belongs to another device");
    if (reg->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "vote_witness_batch: the registry belongs to another device");
    if (reg->depth != circ->P.depth) return set_error(ctx, VSP_ERR_ARG, "vote_witness_batch: the registry's depth is not the circuit's");
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t nv = vc_num_vars(circ->P);
    for (size_t at = 0; at < count; at += VW_PIECE) {
        const size_t c = count - at < VW_PIECE ? count - at : VW_PIECE;
        VSP_TRY(witness_piece(ctx, circ, reg, eid_bits_words, sks + 4 * at, indices + at, votes + at, c, witnesses_out + at * nv * 4, status_out + at));
    }
    return VSP_OK;
}

// option "vote_cast_device" = 0: the witnesses travel through host memory -- to the host, compacted there, and back into the batch prover
static int cast_through_host(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const vsp_saver_pk *spk, const vsp_pk *pk, const uint64_t *eid_bits_words,
                        const uint64_t *sks, const uint64_t *indices, const uint32_t *votes, size_t count, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s,
                        uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!circ || !reg || !spk || !pk || !eid_bits_words || !sks || !indices || !votes || !r_enc || !r || !s || !status_out)
        return set_error(ctx, VSP_ERR_ARG, "vote_cast_batch: null argument");
    if (count == 0 || count > VW_PIECE) return set_error(ctx, VSP_ERR_ARG, "vote_cast_batch: 1 to 64 ballots expected");
    const size_t n = circ->P.n, nv = vc_num_vars(circ->P), ct_words = (n + 2) * 12, blob_bytes = 8 + 48 * (n + 2);
    const size_t wit_words = count * nv * 4;
    std::unique_ptr<uint64_t[]> wit_buf(new uint64_t[wit_words]);       // every word is written by the witness call: no zeroing first
    uint64_t *wit = wit_buf.get();
    auto wipe = [&]() { memset(wit, 0, wit_words * sizeof(uint64_t)); __asm__ __volatile__("" : : "r"(wit) : "memory"); };
    int rc = vsp_vote_witness_batch(ctx, circ, reg, eid_bits_words, sks, indices, votes, count, wit, status_out);
    if (rc != VSP_OK) { wipe(); return rc; }
    // the members that have a witness, packed to the front
    std::vector<size_t> live;
    for (size_t k = 0; k < count; k++) if (status_out[k] == 0) live.push_back(k);
    const size_t L = live.size();
    if (ct_out) memset(ct_out, 0, count * ct_words * sizeof(uint64_t));
    if (A_out) memset(A_out, 0, count * 12 * sizeof(uint64_t));
    if (B_out) memset(B_out, 0, count * 24 * sizeof(uint64_t));
    if (C_out) memset(C_out, 0, count * 12 * sizeof(uint64_t));
    if (proofs_out) memset(proofs_out, 0, count * 192);
    if (ct_blobs_out) memset(ct_blobs_out, 0, count * blob_bytes);
    if (!L) { wipe(); return VSP_OK; }
    std::vector<uint64_t> msgs(L * n * 4, 0), rnd(3 * L * 4);
    for (size_t i = 0; i < L; i++) {
        const size_t k = live[i];
        if (i != k) memmove(wit + i * nv * 4, wit + k * nv * 4, nv * 4 * sizeof(uint64_t));
        msgs[(i * n + votes[k]) * 4] = 1;
        memcpy(&rnd[4 * i], r_enc + 4 * k, 32); memcpy(&rnd[4 * (L + i)], r + 4 * k, 32); memcpy(&rnd[4 * (2 * L + i)], s + 4 * k, 32);
    }
    std::vector<uint64_t> ct(ct_out ? L * ct_words : 0), A(A_out ? L * 12 : 0), B(B_out ? L * 24 : 0), Cc(C_out ? L * 12 : 0);
    std::vector<uint8_t> proofs(proofs_out ? L * 192 : 0), blobs(ct_blobs_out ? L * blob_bytes : 0);
    rc = vsp_saver_encrypt_batch(ctx, spk, circ->cs, pk, msgs.data(), wit, L, &rnd[0], &rnd[4 * L], &rnd[8 * L], ct_out ? ct.data() : nullptr, A_out ? A.data() : nullptr,
                                 B_out ? B.data() : nullptr, C_out ? Cc.data() : nullptr, proofs_out ? proofs.data() : nullptr, ct_blobs_out ? blobs.data() : nullptr);
    wipe();
    if (rc != VSP_OK && rc != VSP_ERR_UNSATISFIED) return rc;
    for (size_t i = 0; i < L; i++) {
        const size_t k = live[i];
        if (ct_out) memcpy(ct_out + k * ct_words, &ct[i * ct_words], ct_words * sizeof(uint64_t));
        if (A_out) memcpy(A_out + k * 12, &A[i * 12], 12 * sizeof(uint64_t));
        if (B_out) memcpy(B_out + k * 24, &B[i * 24], 24 * sizeof(uint64_t));
        if (C_out) memcpy(C_out + k * 12, &Cc[i * 12], 12 * sizeof(uint64_t));
        if (proofs_out) memcpy(proofs_out + k * 192, &proofs[i * 192], 192);
        if (ct_blobs_out) memcpy(ct_blobs_out + k * blob_bytes, &blobs[i * blob_bytes], blob_bytes);
    }
    return rc;
}


// the circuit, the registry and the context belong together (the checks of vsp_vote_witness_batch, under the caller's name)
static int cast_check_handles(vsp_ctx *ctx, const char *who, const vsp_vote_circuit *circ, const vsp_registry *reg) {
    char m[160];
    const char *what = circ->device != ctx->device ? "the circuit belongs to another device" : reg->device != ctx->device ? "the registry belongs to another device" :
                       reg->depth != circ->P.depth ? "the registry's depth is not the circuit's" : nullptr;
    if (!what) return VSP_OK;
    snprintf(m, sizeof m, "%s: %s", who, what);
    return set_error(ctx, VSP_ERR_ARG, m);
}

int vsp_cast_witness_batch_device(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const uint64_t *eid_bits_words, const uint64_t *sks, const uint64_t *indices,
                                  const uint32_t *votes, size_t count, const void **d_witnesses_out, size_t *stride_out, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!circ || !reg || !eid_bits_words || !sks || !indices || !votes || !d_witnesses_out || !stride_out || !status_out)
        return set_error(ctx, VSP_ERR_ARG, "cast_witness_batch_device: null argument");
    if (count == 0 || count > VW_PIECE) return set_error(ctx, VSP_ERR_ARG, "cast_witness_batch_device: 1 to 64 ballots expected");
    VSP_TRY(cast_check_handles(ctx, "cast_witness_batch_device", circ, reg));
    VSP_HIP(hipSetDevice(ctx->device));
    *d_witnesses_out = nullptr; *stride_out = 0;
    VSP_TRY(witness_piece(ctx, circ, reg, eid_bits_words, sks, indices, votes, count, nullptr, status_out));
    *d_witnesses_out = circ->wit.p; *stride_out = vc_num_vars(circ->P);
    return VSP_OK;
}

int vsp_cast_witness_release(vsp_ctx *ctx, vsp_vote_circuit *circ) {
    if (!ctx) return VSP_ERR_ARG;
    if (!circ) return set_error(ctx, VSP_ERR_ARG, "cast_witness_release: null argument");
    if (circ->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "cast_witness_release: the circuit belongs to another device");
    VSP_HIP(hipSetDevice(ctx->device));
    witness_release(ctx, circ);
    return VSP_OK;
}

int vsp_cast_batch_launch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const vsp_saver_pk *spk, const vsp_pk *pk, const uint64_t *eid_bits_words,
                          const uint64_t *sks, const uint64_t *indices, const uint32_t *votes, size_t count, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s,
                          uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!circ || !reg || !spk || !pk || !eid_bits_words || !sks || !indices || !votes || !r_enc || !r || !s || !status_out)
        return set_error(ctx, VSP_ERR_ARG, "cast_batch_launch: null argument");
    if (count == 0 || count > VW_PIECE) return set_error(ctx, VSP_ERR_ARG, "cast_batch_launch: 1 to 64 ballots expected");
    if (ctx->cast.active || ctx->prove.active) return set_error(ctx, VSP_ERR_ARG, "cast_batch_launch: a batch is already in flight on this context (finish it first)");
    if (spk->n != circ->P.n) return set_error(ctx, VSP_ERR_ARG, "cast_batch_launch: the SAVER key's msg_size is not the circuit's");
    VSP_TRY(cast_check_handles(ctx, "cast_batch_launch", circ, reg));
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(witness_piece(ctx, circ, reg, eid_bits_words, sks, indices, votes, count, nullptr, status_out));      // blocks for the status words alone
    auto &f = ctx->cast;
    f.live.clear();
    for (size_t k = 0; k < count; k++) if (status_out[k] == 0) f.live.push_back((uint32_t)k);
    const size_t L = f.live.size();
    int rc = VSP_OK;
    if (L) {
        // the live members are the map; their randomness packed to the front, as the host path packs it
        std::vector<uint64_t> rnd(3 * L * 4);
        for (size_t i = 0; i < L; i++) {
            const size_t k = f.live[i];
            memcpy(&rnd[4 * i], r_enc + 4 * k, 32); memcpy(&rnd[4 * (L + i)], r + 4 * k, 32); memcpy(&rnd[4 * (2 * L + i)], s + 4 * k, 32);
        }
        rc = vsp_saver_encrypt_batch_launch_device(ctx, spk, circ->cs, pk, circ->wit.p, vc_num_vars(circ->P), count, f.live.data(), L, &rnd[0], &rnd[4 * L], &rnd[8 * L]);
    }
    witness_release(ctx, circ);                 // right behind the launch, whose gather is the only reader: stream-ordered
    if (rc != VSP_OK) return rc;
    f.active = true; f.count = count; f.n = circ->P.n;
    return VSP_OK;
}

int vsp_cast_batch_finish(vsp_ctx *ctx, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out) {
    if (!ctx) return VSP_ERR_ARG;
    auto &f = ctx->cast;
    if (!f.active) return set_error(ctx, VSP_ERR_ARG, "cast_batch_finish: no batch of cast ballots in flight on this context");
    f.active = false;
    const size_t count = f.count, n = f.n, L = f.live.size(), ct_words = (n + 2) * 12, blob_bytes = 8 + 48 * (n + 2);
    std::vector<uint64_t> ct(ct_out ? L * ct_words : 0), A(A_out ? L * 12 : 0), B(B_out ? L * 24 : 0), Cc(C_out ? L * 12 : 0);
    std::vector<uint8_t> proofs(proofs_out ? L * 192 : 0), blobs(ct_blobs_out ? L * blob_bytes : 0);
    int rc = VSP_OK;
    // the finish runs whatever the outputs are: nothing of the batch stays in flight
    if (L) rc = vsp_saver_encrypt_batch_finish(ctx, ct_out ? ct.data() : nullptr, A_out ? A.data() : nullptr, B_out ? B.data() : nullptr, C_out ? Cc.data() : nullptr,
                                               proofs_out ? proofs.data() : nullptr, ct_blobs_out ? blobs.data() : nullptr);
    if (ct_out) memset(ct_out, 0, count * ct_words * sizeof(uint64_t));
    if (A_out) memset(A_out, 0, count * 12 * sizeof(uint64_t));
    if (B_out) memset(B_out, 0, count * 24 * sizeof(uint64_t));
    if (C_out) memset(C_out, 0, count * 12 * sizeof(uint64_t));
    if (proofs_out) memset(proofs_out, 0, count * 192);
    if (ct_blobs_out) memset(ct_blobs_out, 0, count * blob_bytes);
    if (rc != VSP_OK && rc != VSP_ERR_UNSATISFIED) return rc;
    for (size_t i = 0; i < L; i++) {            // the scatter to the members' slots
        const size_t k = f.live[i];
        if (ct_out) memcpy(ct_out + k * ct_words, &ct[i * ct_words], ct_words * sizeof(uint64_t));
        if (A_out) memcpy(A_out + k * 12, &A[i * 12], 12 * sizeof(uint64_t));
        if (B_out) memcpy(B_out + k * 24, &B[i * 24], 24 * sizeof(uint64_t));
        if (C_out) memcpy(C_out + k * 12, &Cc[i * 12], 12 * sizeof(uint64_t));
        if (proofs_out) memcpy(proofs_out + k * 192, &proofs[i * 192], 192);
        if (ct_blobs_out) memcpy(ct_blobs_out + k * blob_bytes, &blobs[i * blob_bytes], blob_bytes);
    }
    return rc;
}

int vsp_vote_cast_batch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const vsp_saver_pk *spk, const vsp_pk *pk, const uint64_t *eid_bits_words,
                        const uint64_t *sks, const uint64_t *indices, const uint32_t *votes, size_t count, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s,
                        uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out, uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!opt(ctx, "vote_cast_device", 1))
        return cast_through_host(ctx, circ, reg, spk, pk, eid_bits_words, sks, indices, votes, count, r_enc, r, s, ct_out, A_out, B_out, C_out, proofs_out, ct_blobs_out, status_out);
    if (!circ || !reg || !spk || !pk || !eid_bits_words || !sks || !indices || !votes || !r_enc || !r || !s || !status_out)
        return set_error(ctx, VSP_ERR_ARG, "vote_cast_batch: null argument");
    if (count == 0 || count > VW_PIECE) return set_error(ctx, VSP_ERR_ARG, "vote_cast_batch: 1 to 64 ballots expected");
    VSP_TRY(vsp_cast_batch_launch(ctx, circ, reg, spk, pk, eid_bits_words, sks, indices, votes, count, r_enc, r, s, status_out));
    return vsp_cast_batch_finish(ctx, ct_out, A_out, B_out, C_out, proofs_out, ct_blobs_out);
}

}  // extern "C"
