// Internal definitions shared by the translation units of libvsp_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <initializer_list>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/vsp.h"
#include <atomic>
#include <mutex>
#include <thread>
#include "curve.h"
#include "point_decode.h"
#include "saver_ct.h"
#include "saver_rerand.h"
#include "lds_sort_map.h"

struct vsp_ctx;
namespace vsp {

// ---- the two groups: G1 over Fp, G2 over Fp2 (y^2 = x^3 + b, curve_b below) ----
struct Affine28; struct Affine28x2;         // rows of the 28-bit-limb tables (fp28.h)
template <int N> struct Group;
template <> struct Group<1> {
    static constexpr int ID = 1;
    using F = Fp; using HF = HFp; using Point = Affine<Fp>; using Row28 = Affine28;     // device field, host field, device affine point, table row
    static constexpr size_t AFFINE_WORDS = 12, JACOBIAN_WORDS = 18;                    // canonical 64-bit words of x | y and of X | Y | Z
    static constexpr uint64_t GEN[12] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL, 0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL,
                                         0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL, 0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
};
template <> struct Group<2> {
    static constexpr int ID = 2;
    using F = Fp2; using HF = HFp2; using Point = Affine<Fp2>; using Row28 = Affine28x2;
    static constexpr size_t AFFINE_WORDS = 24, JACOBIAN_WORDS = 36;
    static constexpr uint64_t GEN[24] = {0xd48056c8c121bdb8ULL, 0x0bac0326a805bbefULL, 0xb4510b647ae3d177ULL, 0xc6e47ad4fa403b02ULL, 0x260805272dc51051ULL, 0x024aa2b2f08f0a91ULL,
                                         0xe5ac7d055d042b7eULL, 0x334cf11213945d57ULL, 0xb5da61bbdc7f5049ULL, 0x596bd0d09920b61aULL, 0x7dacd3a088274f65ULL, 0x13e02b6052719f60ULL,
                                         0xe193548608b82801ULL, 0x923ac9cc3baca289ULL, 0x6d429a695160d12cULL, 0xadfd9baa8cbdd3a7ULL, 0x8cc9cdc6da2e351aULL, 0x0ce5d527727d6e11ULL,
                                         0xaaa9075ff05f79beULL, 0x3f370d275cec1da1ULL, 0x267492ab572e99abULL, 0xcb3e287e85a763afULL, 0x32acd2b02bc28b99ULL, 0x0606c4a02ea734ccULL};
};
using G1 = Group<1>;
using G2 = Group<2>;
// f(G1{}) for group 1, f(G2{}) otherwise: the one place a group number becomes a type
template <class Fn> inline decltype(auto) with_group(int group, Fn &&f) {
    if (group == 1) return f(G1{});
    return f(G2{});
}
// bytes of one device affine point of a group
inline size_t point_bytes(int group) { return with_group(group, [](auto g) { return sizeof(typename decltype(g)::Point); }); }

// The owners of the library's memory: DevBuf (hipMalloc) and PinnedBuf (hipHostMalloc).  Move-only; the destructor frees, so a struct
// that holds one frees it when the struct goes and a local frees it on every return.  Nothing waits here: whoever lets a buffer go
// has waited for the work that uses it.  live() counts the allocations of a kind in the process ("device_allocations_live",
// "pinned_allocations_live" of vsp_get_stat)
template <bool PINNED> struct OwnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~OwnedBuf() { reset(); }
    static std::atomic<long> &live() { static std::atomic<long> n{0}; return n; }
    // exactly `bytes` (not zero) in place of what it held
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes; live()++;
        return hipSuccess;
    }
    void reset() {
        if (p) { if (PINNED) hipHostFree(p); else hipFree(p); live()--; }
        p = nullptr; cap = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};
using DevBuf = OwnedBuf<false>;
using PinnedBuf = OwnedBuf<true>;
// the timers around the device stages of one kind of call: up to four events, created on first use, destroyed with the timer
struct StageTimer {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    StageTimer() = default;
    StageTimer(const StageTimer &) = delete;
    StageTimer &operator=(const StageTimer &) = delete;
    ~StageTimer() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    int event(vsp_ctx *ctx, int i, hipEvent_t *out);                // event i, created on first use
    int mark(vsp_ctx *ctx, int i, hipStream_t st);                  // record event i on st
    void add(vsp_ctx *ctx, int i, const char *name) const;          // ctx->stats[name] += the time from event i to event i + 1; an error is ignored
};
// the decoded points of one piece of a group (decode.hip): Montgomery affine points, a status byte per point, and the timer around
// the decoding and the subgroup check (G1: event 3 closes the tally's sum)
struct DecodeWork {
    DevBuf pts, pstatus;
    StageTimer timer;
};
// a piece of ballots decoded from their blobs and resident on the device until the piece is finished (receive.hip): `count` ballots
// of which the first is ballot `base` of the call.  Montgomery affine points as the decoder leaves them: the ciphertext members
// ballot-major, members[k (n + 2) + j]; A of ballot k at ac[k], C at ac[count + k]; B at b[k]; the rest inputs as canonical words,
// rest[(k n_rest + i) 8 ..]; the three wire status bytes of ballot k at wire[k], wire[stride + k], wire[2 stride + k]
// With a ballot box (ballot_box.hip) a fourth status row, box_row[k]: not zero for a ballot the box has turned away before the verifier
struct ReceivedPiece {
    size_t base = 0, count = 0, wire_stride = 0;
    const void *members = nullptr, *ac = nullptr, *b = nullptr;
    const uint32_t *rest = nullptr;
    const uint8_t *wire = nullptr;
    const uint8_t *box_row = nullptr;
};
// where the verifiers take the ballots of a piece from (pairing.hip saver_piece_prepare): canonical limbs of the whole call in host
// memory -- ballots [at, at + c) are uploaded and checked by k_ballot_prepare -- or, with `dev` set, a range of a decoded piece, which
// k_receive_prepare gathers.  Ballot indices are the call's in both
struct BallotSource {
    const uint64_t *ct = nullptr, *rest = nullptr, *A = nullptr, *B = nullptr, *C = nullptr;
    const ReceivedPiece *dev = nullptr;
};

// stage [s0, s1) split of one NTT (see ntt.hip)
struct NttTables {
    DevBuf fwd, inv;        // omega^j and omega^-j, j < 2^(log-1), Montgomery form
    unsigned log = 0;       // domain log the tables were generated for (serves every smaller domain)
    // two-level coset power tables for the cached coset generator
    DevBuf pw_lo_f, pw_hi_f, pw_lo_i, pw_hi_i;
    unsigned pw_log = 0;    // log_m the hi tables were sized for
    uint64_t pw_g[4] = {0, 0, 0, 0};
    bool pw_valid = false;
    // the same tables for the 9 x 29-bit butterflies (fr29.h): Montgomery form for R' = 2^261, three planes per table (16 + 16 + 4 bytes per entry)
    DevBuf fwd29, inv29, pw29[4];   // pw29: lo_f, hi_f, lo_i, hi_i
    unsigned log29 = 0;             // log the fwd29 / inv29 tables were converted for (0 = none)
    unsigned pw29_log = 0; uint64_t pw29_g[4] = {0, 0, 0, 0}; bool pw29_valid = false;
};

// digit-window geometry of one MSM
struct MsmGeom {
    unsigned c;         // window bits
    unsigned W;         // windows
    unsigned B;         // buckets per window = 2^(c-1)
    unsigned q0, q1, q2;  // bucket index bit split, q0+q1+q2 = c-1
    unsigned T;         // split threshold (max points per bucket part)
    size_t n;
    size_t G;           // Wr * B buckets in total
    unsigned Wr;        // bucket sets: W (one per window) or 1 (precomputed window multiples, all windows share one set)
    unsigned single;    // 1 in the shared-set mode
    uint32_t idx_stride, idx_first;   // shared-set mode: sorted entry of digit w of scalar i = w * idx_stride + idx_first + i
    unsigned sbits;     // bits of a scalar the windows must cover: 255, or 128 for the two halves of an endomorphism-split scalar
    unsigned lb;        // windows wider than 16 bits: the low bits of the bucket index that the second sort pass orders (c - 16); 0 otherwise
    unsigned fold;      // 255-bit scalars are read as min(k, r - k) < 2^254 with the sign flipped: one window fewer where c divides 255 (c = 15, 17)
    unsigned bd;        // slots per digit in the k_dimbits result layout: 8 (digits of up to 8 bits, three of them) or 12 (two digits of up to 12 bits)
    // a BATCH of K scalar vectors over one set of bases (round 4: vsp_groth16_prove_batch): vector k starts kstride elements after vector
    // k - 1, its Wk windows are the windows k Wk .. (k + 1) Wk - 1 of the W = K Wk the rest of the pipeline sees -- separate bucket sets per
    // (vector, window), the same base rows: the sort, the accumulation and the bucket reduction run ONCE, K times as wide.  K = 1: Wk = W.
    unsigned K, Wk;
    size_t kstride;
};
// reference to the precomputed window multiples of resident bases
struct MsmPre { size_t stride; size_t first; unsigned c; const void *table28; bool glv; };   // table28: the same table on 14 x 28-bit limbs (fp28.h), or null;
                                                                                             // glv: table28 holds (2^(cw) P_i, phi(2^(cw) P_i)) interleaved for the 128 / c windows of split scalars

// one in-flight MSM: its stream, device workspaces (grow only) and the pinned landing buffer of its window results
struct MsmWork {
    static constexpr size_t PINNED_BYTES = 256 * 1024;       // window results land here (25 records of 192 / 384 bytes per window at most); a batch grows it
    bool inited = false, own_stream = false, active = false, empty = false;
    bool dimbits = false;                  // layout of the window results of the last launch (msm_impl.inc k_dimbits / k_dimweight)
    hipStream_t stream = nullptr;          // the stream launches queue on: the slot's own one, or a borrowed one (msm_slot_use_stream)
    hipStream_t own = nullptr;             // the slot's own stream (slots 1..), created when first needed
    hipEvent_t ev0 = nullptr, ev1 = nullptr, done = nullptr, plan_ready = nullptr;
    DevBuf cnt, off, cursor, nsub, suboff, blocksum, sorted, heavy, counters, digits, blockhist, partbucket, perm, sizehist;
    DevBuf buckets, partials, dims, winres, medium, redo;
    DevBuf buckets28, partials28;          // G1: bucket sums in the 14 x 28-bit form (fp28.h XYZZ<Fp28>)
    DevBuf pairs_a, pairs_b, ms_h1, ms_h1s, ms_h2, ms_h2s;      // staged sort of large wide-window problems (msm_sort.hip k_ms_*)
    DevBuf tmp_sorted, tmp_lo, off_hi, cnt_hi;      // windows wider than 16 bits: the entries ordered by the high 15 bits of the bucket index, their low bits, the segment offsets
    DevBuf glv_scalars;                  // endomorphism split: 2n half-length scalars k1_i, k2_i (interleaved)
    bool glv = false;                    // this launch runs over the split scalars and the interleaved (P, phi(P)) table
    PinnedBuf h_pinned;
    // vsp_msm_finish_jacobian_device: the Jacobian record leaves through a small pinned ring (REC_RING entries of 288 bytes) so that the
    // copy into the caller's device buffer is an asynchronous DMA; rec_ev[k] marks the copy out of entry k as done
    static constexpr unsigned REC_RING = 4;
    PinnedBuf h_rec; hipEvent_t rec_ev[REC_RING] = {nullptr, nullptr, nullptr, nullptr}; unsigned rec_idx = 0;
    PinnedBuf h_census;                  // count of scalars that are neither 0 nor 1
    hipEvent_t census_done = nullptr;
    bool census_pending = false; size_t census_n = 0; const void *census_scalars = nullptr;
    bool check_pending = false;          // this launch's census (count + non-canonical flag) is to be read at finish
    size_t neff_cache_n = 0, neff_cache = 0;   // count of the last census over a vector of neff_cache_n scalars
    MsmGeom g;
    size_t n = 0, n_eff = 0;
};
static constexpr unsigned VSP_MSM_SLOTS = 6;
// what options "msm_window_bits", "msm_split" and "msm_dimbits" choose, pinned for one launch: window bits (0 = automatic), bucket part
// length (0 = automatic), the bucket reduction's last step (1 = k_dimbits, 0 = k_dimweight, -1 = by group)
struct MsmTuning { long window_bits = 0, split = 0, dimbits = -1; };
// one multi-exponentiation queued on a work slot (msm_slot_launch)
struct MsmRequest {
    const void *bases = nullptr;        // Affine<Fp> / Affine<Fp2>, Montgomery form: the points, or with `pre` the table of window multiples
    const Fr *scalars = nullptr;
    size_t n = 0;
    int plan_from = -1;                 // a slot whose digit sort and bucket plan over the SAME scalars this launch reuses (the prover's
                                        // A_query, B_query(G1) and B_query(G2) all multiply by the same witness vector), or -1
    bool dense = false;                 // the scalars are known to be dense: skip the 0/1 census
    bool plan_only = false;             // queue the digit sort and the bucket plan only; a later launch on the SAME slot with plan_from = that
                                        // slot queues the accumulation and the reduction over it
    const MsmPre *pre = nullptr;
    const void *table28 = nullptr;      // plain bases: the same points on 28-bit limbs, or null
    bool glv = false;                   // table28 (or pre->table28) holds (P_i, phi(P_i)) interleaved: split the scalars k = k1 + k2 lambda
    unsigned batch = 0;                 // 0: one scalar vector; K >= 1: a batch (MsmGeom.K), vector k at scalars + k * stride, one result each
    size_t stride = 0;
    const MsmTuning *tuning = nullptr;  // null: the options
    MsmRequest(const Fr *scalars_ = nullptr, size_t n_ = 0) : scalars(scalars_), n(n_) {}
};
// what the stages of one msm_launch share: the request as the kernels see it and the sizes its geometry gives
struct MsmLaunch {
    MsmRequest rq;                      // the caller's, with batch >= 1 and glv only where the interleaved table is there
    hipStream_t st;
    const MsmWork *plan_from;           // the work whose digit sort / bucket plan this launch reuses, or null
    const void *table28;                // the bases (or table) on 28-bit limbs, or null
    const Fr *scalars; size_t n;        // what the sort reads: with the endomorphism split 2 rq.n half-length scalars (k_glv_split)
    long sort_mode;                     // option "msm_sort": 1 never staged, 2 staged whenever c >= 17
    MsmTuning tune;                     // the request's, or the options'
    bool fused_split, fused_scans, dimbits;      // dimbits: the bucket reduction's last step is k_dimbits (which decides how wide a digit may be)
    size_t M, Smax;                     // upper bounds on sorted entries and on bucket parts
    unsigned per_w, nblk, gblk, ablk;
};
// what the sort / plan side (msm_sort.hip) and the group side (msm_impl.inc) of the pipeline both use: threads per workgroup; bins of the
// counting sort of bucket parts by size (k_partinfo .. k_partsort); points per part of a bucket of s points cut into `parts` parts
static constexpr unsigned MSM_THREADS = 256;
static constexpr unsigned SZ_BINS = 1024;
__device__ __forceinline__ uint32_t part_len(uint32_t s, uint32_t parts) { return (s + parts - 1) / parts; }

// which butterflies run a transform: the 29-bit ones when ntt29_in_use says so, else the 8 x 32-bit ones; or one of the two forced
enum NttPath { NTT_AUTO, NTT_FR29, NTT_FR32 };
// `count` radix-2 transforms of 2^log_m canonical values in one launch per pass (ntt_launch).  Pointer form (strides 0): transform b
// reads in[b] and writes out[b], count <= 3.  Strided form: transform b reads in[0] + b in_stride and writes out[0] + b out_stride,
// count <= 65535.  Several transforms, out of place or fused, need the 29-bit butterflies.
struct NttRequest {
    const Fr *in[3] = {nullptr, nullptr, nullptr};
    Fr *out[3] = {nullptr, nullptr, nullptr};
    unsigned count = 1;
    size_t in_stride = 0, out_stride = 0;
    const Fr *fuse_b = nullptr, *fuse_c = nullptr;      // non-null: the first pass loads (in b - c) 2^-261, b and c following in_stride
    unsigned log_m = 0;
    int inverse = 0;
    const uint64_t *coset_g = nullptr;                  // canonical coset generator (forward: a[i] g^i before; inverse: ginv^i after), or null
    const HFr *extra_scale = nullptr;                   // host Montgomery: a constant multiplied into every output, or null
    NttPath path = NTT_AUTO;
    // one transform of d_a in place
    NttRequest(Fr *d_a, unsigned log_m_, int inverse_ = 0, const uint64_t *coset_g_ = nullptr, const HFr *extra_scale_ = nullptr)
        : log_m(log_m_), inverse(inverse_), coset_g(coset_g_), extra_scale(extra_scale_) { in[0] = d_a; out[0] = d_a; }
};

}  // namespace vsp

struct vsp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;       // stream in use
    hipStream_t own_stream = nullptr;   // created by vsp_create
    hipStream_t prove_streams[2] = {nullptr, nullptr};      // the prover's two witness chains (prover.hip), created on first use
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_aux = nullptr;
    std::string err;
    std::map<std::string, double> stats;
    std::map<std::string, long> opts;
    vsp::NttTables ntt;
    vsp::DevBuf ntt_scratch;
    vsp::DevBuf dom_scratch;            // step-domain transforms: the d / partial-sum vectors
    // MSM work slots (slot 0 runs on the context's stream; the others own a stream each)
    vsp::MsmWork msm_work[vsp::VSP_MSM_SLOTS];
    int slot_group[vsp::VSP_MSM_SLOTS] = {1, 1, 1, 1, 1, 1};
    bool lds_attr_set = false;
    bool ntt_attr_set = false;
    int ntt29_checked = 0;              // known-answer check of k_ntt29_pass: 0 not yet (or could not run), 1 passed, -1 failed (8 x 32-bit kernel in use)
    vsp::DevBuf msm_scalars;
    vsp::PinnedBuf h_fold;              // landing buffer of vsp_fold_jacobian_device (the ranks' records)
    vsp::DevBuf val_flag;               // one word: validation result of the last bases upload
    int fp28_checked[2] = {0, 0};       // known-answer check of the 28-bit-limb accumulation kernels, per group: 0 not yet, 1 passed, -1 failed (kernel disabled)
    // fixed-base tables of the generators (fb_table[group - 1]), built lazily, and the scratch of the batch exponentiation
    vsp::DevBuf fb_table[2], fb_tmp, fb_pre;
    // the receiving side's piece: raw blobs (decode.hip, tally.hip), the decoded points of either group (decode[G::ID - 1]), a status
    // byte per ballot or proof, the tally's partial sums
    vsp::DevBuf tally_raw, tally_bstatus, tally_partials;
    vsp::DecodeWork decode[2];
    // the pairings' piece (pairing.hip): canonical inputs, Montgomery pairs, status bytes (pairs | products | results), Miller values, their
    // products, GT values; the timers around the Miller stage and the final exponentiation, and around the three stages of
    // vsp_saver_verify_batch (prepare, Miller, final exponentiation)
    vsp::DevBuf pair_raw, pair_g1, pair_g2, pair_status, pair_ml, pair_prod, pair_gt;
    vsp::StageTimer pair_timer, saver_timer;
    // the screened ballot check (screen.hip): coefficients, range arguments, their Miller values and the product tree's levels in one
    // workspace; the timers around prepare | scale | Miller and tree, and around column sums | fixed-argument Miller | final exponentiation
    vsp::DevBuf screen_ws;
    vsp::StageTimer screen_timer[2];
    // ballots received from their blobs (receive.hip): the decoded ciphertext members of a piece with their status bytes, the raw input
    // blobs, the decoded rest inputs, the wire status bytes (3 x a stride); the timer around k_receive_scalars
    vsp::DevBuf recv_members, recv_mstatus, recv_raw, recv_rest, recv_wire;
    vsp::StageTimer recv_timer;
    // SAVER decryption (decrypt.hip): a result word per (ciphertext, slot) item and the pending count of the giant search; the timer around
    // the stages of vsp_saver_decrypt_batch / vsp_saver_verify_decryption_batch (prepare, values, search or powers) and around the table build
    vsp::DevBuf dec_out;
    vsp::StageTimer dec_timer;
    // Pedersen hashes and the registry (pedersen.hip): a piece's messages, keys or indices; its digests, points, copaths or blob words;
    // the all-zero row that absent keys read; the timer around the kernels of one call
    vsp::DevBuf ped_in, ped_out, ped_zero;
    vsp::StageTimer ped_timer;
    // prover workspaces for K witnesses (a single proof: K = 1): z [K][num_vars + 1], A z, B z, C z [K][3][m], H [K][m], the packed witness
    vsp::DevBuf pr_z, pr_abc, pr_h, pr_pack;
    // the witness check (prover.hip k_r1cs_verdict): per member of a piece of at most VERDICT_MEMBERS witnesses three 32-bit words --
    // first_bad_row [64] | bad_rows [64] | a value >= r [64] -- on the device and in the pinned buffer the asynchronous copy lands in
    static constexpr size_t VERDICT_MEMBERS = 64, VERDICT_BYTES = 3 * VERDICT_MEMBERS * sizeof(uint32_t);
    vsp::DevBuf pr_verdict;
    vsp::PinnedBuf h_verdict;
    vsp::StageTimer check_timer;          // vsp_r1cs_check_batch: around its front half and around its verdict kernels
    // the proof or the batch of K proofs in flight between a launch and its finish (one per context): the key, r and s (K x 4 words), the
    // SAVER term (single proofs only), the bytes of z the launch wrote
    struct {
        bool active = false, batch = false; const vsp_pk *pk = nullptr; size_t count = 0, z_bytes = 0; std::vector<uint64_t> r, s;
        bool has_saver = false; uint64_t P1[12], r_enc[4];
        std::vector<uint64_t> addend;      // a batch's SAVER terms, K canonical affine points added to C (saver_batch.hip sets them before the finish); empty: none
        bool check = false;      // option "prove_check_witness": the verdict records are on their way to h_verdict
    } prove;
    // ballots in batches (saver_batch.hip): the ciphertext kernels' stream, their device workspace (a piece's scalars, column sums and
    // canonical points), the pinned staging of the scalars and of the points with the event behind the copy back, the timer around the
    // kernels; and the batch between vsp_saver_encrypt_batch_launch and its finish
    struct {
        hipStream_t stream = nullptr;
        vsp::DevBuf scalars, sums, points;
        vsp::PinnedBuf h_scalars, h_points;
        hipEvent_t done = nullptr;
        vsp::StageTimer timer;
        bool active = false, gpu = false, device_src = false; const vsp_saver_pk *spk = nullptr; size_t count = 0;
    } saver_ct;
    // a batch of cast ballots between vsp_cast_batch_launch and its finish (vote_circuit.hip): the members' count, the live ones' slots in
    // member order, the key's msg_size.  Every prover launch refuses a context with a cast in flight, a cast without a live member included
    struct {
        bool active = false; size_t count = 0, n = 0; std::vector<uint32_t> live;
    } cast;
    // rerandomization in batches (saver_rerand.hip): a piece's device workspace -- canonical words in and out (one buffer), scalar records,
    // Montgomery points, column sums of both groups, a status word per ballot --, the pinned staging of both directions, the timers
    // around check | columns | affine and around the G1 | G2 multiplications
    struct {
        vsp::DevBuf words, scalars, given, b_in, sums, sums2, status;
        vsp::PinnedBuf h_in, h_out;
        vsp::StageTimer timer[2];
    } saver_rr;
    // vsp_groth16_prove_batch_verdicts: status byte and first failing row of every member of the last finished batch that was checked
    std::vector<uint8_t> batch_status;
    std::vector<uint64_t> batch_first_bad;
};

struct vsp_bases {
    int group = 1;          // 1 = G1, 2 = G2
    size_t n = 0;
    vsp::DevBuf d;          // device array of Affine<Fp> / Affine<Fp2>, Montgomery form; with pre_c != 0 it is the table
                            // [W][n]: slice w holds 2^(pre_c * w) * P  (vsp_bases_precompute)
    unsigned pre_c = 0;
    int in_subgroup = 0;    // 1: every point satisfies phi(P) = lambda P (checked at upload, or the library's own multiples of a generator); -1: the check
                            // found a point that does not; 0: not checked.  The endomorphism layout below needs 1 (or option "msm_glv" = 2)
    bool glv = false;       // d28 holds (P_i, phi(P_i)) interleaved, phi(x, y) = (beta x, y) = lambda * P (the curve's endomorphism): a scalar
                            // k = k1 + k2 lambda then needs windows over 128 bits only.  Plain bases: 2n rows, half the bucket sets to reduce.
                            // Window multiples (pre_split): 2n rows for each of the ceil(128 / pre_c) windows -- the split over ONE bucket set
    bool pre_split = false; // vsp_bases_precompute_split: the table of window multiples is meant for dense scalars and carries the endomorphism rows
    vsp::DevBuf d28;        // the same array (or table) once more on 14 x 28-bit limbs (fp28.h: 112-byte rows G1, 224-byte rows G2) for the accumulation kernel
};

// math::evaluation_domain<Fr>: the basic radix-2 domain (step = 0, m = big_m = 2^log_big) or the step radix-2 domain
// (m = big_m + small_m, both powers of two, small_m < big_m) that make_evaluation_domain(min_size) selects
struct vsp_domain {
    size_t m = 0, big_m = 0, small_m = 0;
    unsigned log_big = 0, log_small = 0;
    int step = 0;
    // divide_by_z_on_coset for the coset generator 7: 1 / Z(7 x_i).  Basic domain: one constant.  Step domain: a table of period
    // compr = big_m / small_m over the first big_m elements (device, Montgomery form) and one constant for the last small_m.
    vsp::DevBuf zinv;
    vsp::HFr zinv_const;
};

struct vsp_r1cs {
    size_t num_constraints = 0, num_inputs = 0, num_vars = 0;
    vsp_domain dom;          // make_evaluation_domain(num_constraints + num_inputs + 1)
    vsp::DevBuf rp[3], ci[3];       // row pointers, column indices (uint32_t)
    vsp::DevBuf co[3];              // Fr Montgomery
    // column-major copy (for the generator's per-variable accumulation): col_ptr [num_vars+2], row index, coefficient
    vsp::DevBuf cp[3], ri[3];       // uint32_t
    vsp::DevBuf cot[3];             // Fr Montgomery
};

struct vsp_keypair {
    vsp_pk *pk = nullptr;
    vsp_bases *q[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // A, B_g1, B_g2, H, L, gamma_ABC_g1
    uint64_t alpha_g1[12], beta_g1[12], delta_g1[12], beta_g2[24], delta_g2[24], gamma_g2[24];
    uint64_t gamma_g1[12];          // extended verification key (the SAVER key generation needs gamma in G1)
};

struct vsp_pk {
    vsp::Affine<vsp::HFp> alpha_g1, beta_g1, delta_g1;     // host, Montgomery
    vsp::Affine<vsp::HFp2> beta_g2, delta_g2;
    const vsp_bases *A = nullptr, *B1 = nullptr, *B2 = nullptr, *H = nullptr, *L = nullptr;
    // every proof multiplies delta (G1: by r, s, r s; G2: by s): fixed-base tables of d 2^(8 w) delta, d = 1..255, w = 0..31, built by the
    // first proof over this key (prover.hip delta_tables; contexts on several threads share a key: built once, under the mutex)
    mutable std::mutex tab_mu;
    mutable std::atomic<bool> tab_ready{false};
    mutable std::vector<vsp::XYZZ<vsp::HFp>> tab1;
    mutable std::vector<vsp::XYZZ<vsp::HFp2>> tab2;
};

// k * P for a fixed P: table[w][d - 1] = d * 16^w * P (affine), 64 windows x 15 entries; a product is <= 64 mixed additions
namespace vsp {
struct FixedBase {
    std::vector<Affine<HFp>> tab;
    bool inf = false;
    void build(const Affine<HFp> &p) {
        inf = is_inf(p);
        if (inf) return;
        std::vector<XYZZ<HFp>> pts(64 * 15);
        XYZZ<HFp> base = xyzz_from_affine(p);
        for (int w = 0; w < 64; w++) {
            XYZZ<HFp> acc = base;
            for (int d = 1; d <= 15; d++) { pts[w * 15 + d - 1] = acc; xyzz_add(acc, base); }
            base = acc;                                            // 16 * base
        }
        // batch normalisation (one inversion): prefix products of ZZZ
        std::vector<HFp> pre(pts.size());
        HFp run = HFp::one();
        for (size_t i = 0; i < pts.size(); i++) { pre[i] = run; run = mul(run, pts[i].ZZZ); }
        HFp ri = inv(run);
        tab.resize(pts.size());
        for (size_t i = pts.size(); i-- > 0;) {
            HFp zi3 = mul(ri, pre[i]);                               // 1 / ZZZ_i
            ri = mul(ri, pts[i].ZZZ);
            HFp zi = mul(zi3, pts[i].ZZ), zi2 = sqr(zi);
            tab[i].x = mul(pts[i].X, zi2); tab[i].y = mul(pts[i].Y, zi3);
        }
    }
    XYZZ<HFp> mul_scalar(const uint64_t k[4]) const {
        XYZZ<HFp> acc = XYZZ<HFp>::inf();
        if (inf) return acc;
        for (int w = 0; w < 64; w++) {
            unsigned d = (unsigned)(k[w >> 4] >> ((w & 15) * 4)) & 15u;
            if (d) xyzz_madd(acc, tab[w * 15 + d - 1]);
        }
        return acc;
    }
};
}  // namespace vsp
// the SAVER public key (saver.hip); saver_batch.hip adds the tables of ALL its 3 n + 3 fixed points in the order of saver_ct.h, on the
// host (`flat`) and on one device, built once by the first vsp_saver_pk_upload under the mutex (contexts on several threads share a key)
struct vsp_saver_pk {
    size_t n = 0;
    std::vector<uint64_t> words;                   // the flat public key
    std::vector<uint64_t> gabc;                    // G_0 .. G_n (canonical)
    std::vector<vsp::FixedBase> X;                 // delta_g1, delta_s_g1[0..n), delta_sum_s_g1   (n + 2 tables: the bases of the ciphertext)
    vsp::FixedBase P2;                             // gamma_inverse_sum_s_g1
    std::vector<vsp::Affine<vsp::HFp>> G, Y;       // message bases G_i (i = 1..n) and t_g1[i]
    mutable std::mutex up_mu;
    mutable std::atomic<bool> uploaded{false};
    mutable int device = -1;
    mutable std::vector<vsp::Affine<vsp::HFp>> flat;      // (3 n + 3) x 960 points; the table of a base at infinity is all zero
    mutable vsp::SaverPlan plan;                          // which scalars meet which bases in which column, and the lanes of a ballot
    mutable vsp::DevBuf d_tab, d_desc;                    // the table and the plan (columns | pairs | lane_col) on the device
    mutable size_t device_bytes = 0;
};

// a Groth16 verification key resident on the device (pairing.hip)
struct vsp_vk {
    size_t n_abc = 0;
    uint8_t alpha_beta[576];            // e(alpha, beta), canonical tower order
    vsp::DevBuf d_expect;               // the same value, Fp12 in Montgomery form
    vsp::DevBuf d_neg;                  // two G2Affine, Montgomery: -gamma_g2, -delta_g2
    vsp::DevBuf d_tab;                  // n_abc rows of 16 G1Affine, Montgomery: d * gamma_ABC[i], d = 0..15 (d = 0: infinity)
};
// A SAVER verifier: the Groth16 key as above, and the prepared lines (pairing.h) of the election key's G2 members in the order of the
// pairs of a ballot: t_g2[0..n] | -H | -gamma_g2 | -delta_g2, then beta_g2 and alpha_g1 for the screened check's e(alpha, beta)^Z (screen.hip)
struct vsp_saver_verifier {
    int device = 0;
    size_t n = 0;                       // msg_size
    std::unique_ptr<vsp_vk> vk;
    vsp::DevBuf d_lines;                // (n + 5) x MILLER_LINES LineCoeffs, Montgomery
    vsp::Affine<vsp::HFp> alpha_g1;     // host, Montgomery
};

// A ballot box (ballot_box.hip; the rules: ballot_box.h): the roles and the FIXED values of the rest inputs, the serials of the accepted
// ballots in ordinal order (`store`, count x words) and the open-addressing table over them (`table`, `slots` 64-bit slots, at most half
// full), all on the verifier's device; the workspace of one piece -- its serials (`pend`), per ballot the holder found before the
// verifier (`hold`), the slot's value and position after the claim (`win`, `pos`), the ordinals of the winners (`ord`) -- and the
// device-side error word.  dirty: a piece has claimed slots and is not committed; the table is rebuilt from the store before its next use
struct vsp_ballot_box {
    int device = 0;
    const vsp_saver_verifier *ver = nullptr;
    size_t L = 0, S = 0, words = 0;     // rest inputs, SERIAL inputs, 8 S
    std::vector<uint8_t> role;
    vsp::DevBuf d_role, d_expected, store, table, pend, hold, win, pos, ord, flag;
    uint64_t slots = 0, count = 0;
    bool dirty = false;
    std::vector<uint64_t> h_hold, h_win, h_ord;
    uint32_t h_flag[2] = {0, 0};
    vsp::StageTimer timer[2];           // [0] 0-1 the screening; [1] 0-1 growth, claim and resolve, 2-3 the commit
};

// The hash's tables and a registry's tree (pedersen.hip), which the voting circuit's witnesses read in place (vote_circuit.hip)
struct vsp_pedersen {
    int device = 0;
    size_t g = 0;
    vsp::DevBuf table;              // g x 252 entries of 96 bytes
};
struct vsp_registry {
    int device = 0;
    unsigned depth = 0;
    vsp::DevBuf nodes;              // 2^(depth + 1) - 1 digests of four words, leaves first, root last
};

namespace vsp {

// option `name` of the context (vsp_set_option), or dflt when it was never set
inline long opt(const vsp_ctx *ctx, const char *name, long dflt) { auto it = ctx->opts.find(name); return it != ctx->opts.end() ? it->second : dflt; }
// the verdict of a known-answer check (bases.hip fp28_known_answer_check, ntt.hip ntt29_known_answer_check): state and stat 1 when the
// results matched, -1 when not -- option `fault` (a test hook) makes a match a mismatch.  A mismatch sets option `off` to 0 (the generic
// kernels for the context's lifetime: beside vsp_set_option, the only write to the option map) and the error text to msg
inline bool record_verdict(vsp_ctx *ctx, int &state, bool same, const char *fault, const std::string &stat, const char *off, const char *msg) {
    if (opt(ctx, fault, 0)) same = false;
    state = same ? 1 : -1;
    ctx->stats[stat] = same ? 1.0 : -1.0;
    if (!same) { ctx->opts[off] = 0; ctx->err = msg; }
    return same;
}
// splitmix64: the known-answer checks' inputs
struct SplitMix64 {
    uint64_t x;
    uint64_t operator()() { x += 0x9E3779B97F4A7C15ULL; uint64_t z = x; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
};
int set_hip_error(vsp_ctx *ctx, hipError_t e, const char *what, const char *file, int line);
// f(0) .. f(n - 1) on up to `max_threads` host threads (the host steps of a BATCH: the Horner chains over the window results of K
// multi-exponentiations and the assembly of K proofs are independent pieces of a few hundred group operations each)
template <class Fn> inline void host_parallel_for(size_t n, Fn f, unsigned max_threads = 16) {
    unsigned hw = std::thread::hardware_concurrency(); if (hw == 0) hw = 4;
    size_t T = n < hw ? n : hw; if (T > max_threads) T = max_threads;
    if (T <= 1) { for (size_t i = 0; i < n; i++) f(i); return; }
    std::vector<std::thread> th;
    th.reserve(T - 1);
    for (size_t t = 1; t < T; t++) th.emplace_back([=]() { for (size_t i = t; i < n; i += T) f(i); });
    for (size_t i = 0; i < n; i += T) f(i);
    for (auto &x : th) x.join();
}
int set_error(vsp_ctx *ctx, int code, const char *msg);
// b holds at least `bytes`: grow only, with an eighth of headroom so that a slightly larger call does not allocate again; nothing of
// the old contents is kept.  The device form waits for `wait` (the stream whose work may still use b) before it frees
int ensure(vsp_ctx *ctx, DevBuf &b, size_t bytes, hipStream_t wait);
inline int ensure(vsp_ctx *ctx, DevBuf &b, size_t bytes) { return ensure(ctx, b, bytes, ctx->stream); }
int ensure_pinned(vsp_ctx *ctx, PinnedBuf &b, size_t bytes);

#define VSP_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return vsp::set_hip_error(ctx, e_, #call, __FILE__, __LINE__); \
    } while (0)
#define VSP_TRY(call)                \
    do {                             \
        int rc_ = (call);            \
        if (rc_ != VSP_OK) return rc_; \
    } while (0)
#define VSP_LAUNCH_CHECK() VSP_HIP(hipGetLastError())

inline int StageTimer::event(vsp_ctx *ctx, int i, hipEvent_t *out) {
    if (!ev[i]) VSP_HIP(hipEventCreate(&ev[i]));
    *out = ev[i];
    return VSP_OK;
}
inline int StageTimer::mark(vsp_ctx *ctx, int i, hipStream_t st) {
    hipEvent_t e;
    VSP_TRY(event(ctx, i, &e));
    VSP_HIP(hipEventRecord(e, st));
    return VSP_OK;
}
inline void StageTimer::add(vsp_ctx *ctx, int i, const char *name) const {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) ctx->stats[name] += ms;
}

// ---- internal entry points (each implemented in its own .hip) ----
int ntt_launch(vsp_ctx *ctx, const NttRequest &rq);
bool ntt29_in_use(vsp_ctx *ctx);                                // runs the 29-bit butterflies' known-answer check first: before any table set-up
int ntt_ensure_twiddles(vsp_ctx *ctx, unsigned log_m);
int ntt_ensure_coset_tables(vsp_ctx *ctx, unsigned log_m, const uint64_t *g4);
// evaluation domains (domain.hip)
int domain_init(vsp_ctx *ctx, vsp_domain *d, size_t min_size);      // make_evaluation_domain's choice + the coset divisors
void domain_basic(vsp_domain *d, unsigned log_m);                   // the basic radix-2 domain of size 2^log_m (log_m = 0 allowed)
int fr_from_mont_device(vsp_ctx *ctx, Fr *d_a, size_t n);
int domain_fft_device(vsp_ctx *ctx, const vsp_domain *d, Fr *d_a, int inverse, const uint64_t *coset_g, const HFr *extra_scale);
int domain_divide_by_z_device(vsp_ctx *ctx, const vsp_domain *d, Fr *d_p);
int domain_lagrange_device(vsp_ctx *ctx, const vsp_domain *d, const HFr &t, Fr *d_u /* m, Montgomery form */);
HFr domain_vanishing(const vsp_domain *d, const HFr &t);
HFr domain_element(const vsp_domain *d, size_t idx);
// K witnesses: member k's A z, B z, C z at dA, dB, dC + k abc_stride (overwritten), its H at dH + k h_stride (domain.hip)
int witness_map_device(vsp_ctx *ctx, const vsp_domain *d, Fr *dA, Fr *dB, Fr *dC, size_t abc_stride, unsigned K, Fr *dH, size_t h_stride);
// the witness as the caller hands it over (prover.hip prove_front_half): plain (num_vars x 4 canonical words a witness, host memory), packed
// (vsp_witness_pack), or rows of a device buffer -- dev: rows of `stride` values of 4 words, stride >= num_vars; member k of a piece is
// row members[k], or row first + k where members is null (members: host memory, read before the launch returns)
struct WitnessSrc {
    const uint64_t *plain; const uint64_t *class_words; const uint32_t *word_offsets; const uint64_t *dense; size_t n_dense;
    const uint64_t *dev = nullptr; size_t stride = 0, first = 0; const uint32_t *members = nullptr;
};
// the checks every entry point with a device source makes before anything is queued, and the source they yield (prover.hip)
int witness_src_device(vsp_ctx *ctx, const char *who, const vsp_r1cs *cs, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members, size_t count,
                       WitnessSrc *out);
// vsp_groth16_prove_batch_launch over either kind of source (prover.hip); a device source leaves ctx->ev_aux recorded behind its last read
int prove_batch_launch_src(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &w, size_t count, const uint64_t *r, const uint64_t *s);
// vsp_groth16_prove with a hook (prover.hip): `overlap` runs on the host after every kernel is queued and before the first wait
int prove_with_overlap(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness, const uint64_t r[4], const uint64_t s[4],
                       const uint64_t *saver_P1, const uint64_t *saver_r_enc, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12],
                       uint8_t proof_out[192], const std::function<void()> *overlap);

// ballots in batches (saver_batch.hip): the stream and the event vsp_destroy lets go, the device half of a key vsp_saver_pk_free does
void saver_ct_release(vsp_ctx *ctx);
void saver_pk_release_device(vsp_saver_pk *spk);
// a plan's columns | pairs | lane_col in one device buffer
int upload_plan(vsp_ctx *ctx, const SaverPlan &p, DevBuf &out);

// MSM on device-resident Montgomery bases; result as host XYZZ (Montgomery, 64-bit limbs).  The templates over the group: msm_impl.inc,
// instantiated by msm_g1.hip / msm_g2.hip.  Everything without a template parameter is group-independent and defined once, in
// msm_sort.hip (but msm_diag_clock: msm_g1.hip, beside the kernel whose stamps it reads).
inline MsmWork &slot(vsp_ctx *ctx, unsigned i) { return ctx->msm_work[i]; }
// the stages of one launch that msm_sort.hip owns; msm_launch<F> (msm_impl.inc) calls them between its own
int work_init(vsp_ctx *ctx, MsmWork &wk, hipStream_t stream_or_null);
int msm_census(vsp_ctx *ctx, MsmWork &wk, const Fr *d_scalars, size_t n, hipStream_t on_stream = nullptr, unsigned batch = 1, size_t batch_stride = 0);
int msm_split_scalars(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g);
int msm_digit_sort(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g);
int msm_bucket_plan(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g);
template <class G> int msm_slot_launch(vsp_ctx *ctx, unsigned slot, const MsmRequest &rq);
template <class G> int msm_precompute(vsp_ctx *ctx, typename G::Point *table, size_t n, unsigned c);
// count (glv: 2 count) rows of sizeof(G::Row28) bytes
template <class G> int msm_table28(vsp_ctx *ctx, const typename G::Point *table, size_t count, void *d_out, bool glv);
// the results of a launch: `count` of them, one per vector of its batch (1 for a launch without a batch)
template <class G> int msm_slot_finish(vsp_ctx *ctx, unsigned slot, XYZZ<typename G::HF> *out, unsigned count = 1);
// a finish in two halves: the wait (context state: caller's thread) and the fold of the window results (pure host arithmetic over the slot: any thread)
template <class G> int msm_slot_finish_wait(vsp_ctx *ctx, unsigned slot, unsigned count, bool *empty);
template <class G> void msm_slot_fold(vsp_ctx *ctx, unsigned slot, XYZZ<typename G::HF> *out);
// rq over points [first, first + rq.n) of resident bases: fills in rq's bases, pre, table28 and glv
int launch_on_bases(vsp_ctx *ctx, unsigned slot, const vsp_bases *bases, size_t first, MsmRequest rq);
int msm_slot_stream(vsp_ctx *ctx, unsigned slot, hipStream_t *out);
int msm_slot_census(vsp_ctx *ctx, unsigned slot, const Fr *d_scalars, size_t n);
void msm_free_slots(vsp_ctx *ctx);
int msm_slot_use_stream(vsp_ctx *ctx, unsigned slot, hipStream_t stream_or_null);
int msm_make_slot_stream(vsp_ctx *ctx, hipStream_t *out);
void msm_drain_slots(vsp_ctx *ctx);
// d_flag: one device word, zeroed by the caller; bit 0 = coordinate >= p, bit 1 = point off the curve (only when check_curve)
template <class G> int bases_to_mont(vsp_ctx *ctx, const void *d_canon, typename G::Point *d_out, size_t n, int check_curve, uint32_t *d_flag);
// raises bit 2 of *d_flag when some point fails phi(P) = lambda P (the endomorphism split's precondition; msm_impl.inc k_subgroup_check).
// With d_status (n bytes, one per point) the verdict is per point instead: bit 2 of d_status[i] is raised and *d_flag is not touched
template <class G> int subgroup_check(vsp_ctx *ctx, const typename G::Point *d_mont, size_t n, uint32_t *d_flag, uint8_t *d_status = nullptr);
int msm_diag_clock(vsp_ctx *ctx, int reset, double *ghz, double *waves);
int ntt_diag_clock(vsp_ctx *ctx, int reset, double *ghz, double *waves);
// resident bases from canonical points into *out; trust: BASES_CALLER = caller data (validated; the split only after the subgroup check),
// BASES_OWN = points this library computed as multiples of a generator (in the subgroup by construction: no check),
// BASES_TRANSIENT = bases of one host-buffer call, or bases about to get window multiples (no split, so no check: exact for any curve point)
enum { BASES_CALLER = 0, BASES_OWN = 1, BASES_TRANSIENT = 2 };
int bases_create(vsp_ctx *ctx, int group, const void *src, bool src_on_device, size_t n, int trust, vsp_bases **out);
// out[i] = scalars[i] * the group's generator, canonical affine (fixedbase_impl.inc, instantiated by fixedbase_g1.hip / fixedbase_g2.hip)
template <class G> int fixed_base_mul(vsp_ctx *ctx, const Fr *d_scalars, size_t n, void *d_out);
// point decoding (decode.hip).  Stages 1 and 2 over the points of group G already in ctx->tally_raw: `sets` sets of n points each, set k
// at heads[k] of the same (per, stride) addressing, decoded one after the other into ctx->decode[G::ID - 1]; events 0, 1, 2 of its
// timer around the stages, which decode_add_times adds to the stats ("tally_*" for G1, "g2_*" for G2; the subgroup stage on request)
// With dst / dst_status the points and their status bytes go there instead (room for sets n of each): a piece that needs more than
// one decode of a group keeps the first (receive.hip)
template <class G> int decode_points(vsp_ctx *ctx, size_t n, size_t per, size_t stride, const size_t *heads, size_t sets, int check_subgroup,
                                     typename G::Point *dst = nullptr, uint8_t *dst_status = nullptr);
template <class G> void decode_add_times(vsp_ctx *ctx, bool subgroup);
size_t decode_chunk_points(const vsp_ctx *ctx);                 // points of one piece: option "tally_chunk_points"
// k_proof_status over the m proofs just decoded into ctx->decode (A, C: decode[0], sets of m; B: decode[1]): a byte per proof to d_out
int decode_proof_status(vsp_ctx *ctx, size_t m, uint8_t *d_out);
// the tally's sum stage (tally.hip) over m resident ballots of ct_len members each, ballot-major; d_skip[b] not zero: ballot b adds
// nothing.  tally_colsum_launch queues k_tally_colsum, event 3 of *sum_end behind it, and the copy of its partial sums into h_part
// (parts x ct_len; valid once the stream is waited for); tally_fold adds them to the handle's running sums and `accepted` to its
// ballot count.  tally_ballots_launch: k_tally_ballots, a status byte per ballot from its count header and its points' bytes
int tally_colsum_launch(vsp_ctx *ctx, const void *d_pts, const uint8_t *d_skip, size_t m, size_t ct_len, std::vector<XYZZ<HFp>> &h_part, size_t *parts_out,
                        StageTimer *sum_end);
void tally_fold(vsp_tally *t, const std::vector<XYZZ<HFp>> &h_part, size_t parts, size_t accepted);
size_t tally_ct_len(const vsp_tally *t);
void tally_ballots_launch(vsp_ctx *ctx, const uint8_t *d_blobs, size_t m, size_t ct_len, const uint8_t *d_pstatus, uint8_t *d_bstatus);
// pairings and Groth16 verdicts (pairing.hip); the arguments are checked by the exports in capi.hip
int pairing_multi_batch(vsp_ctx *ctx, const uint64_t *g1, const uint64_t *g2, size_t m, size_t n, uint8_t *gt_out, uint8_t *is_one_out);
vsp_vk *pairing_vk_create(vsp_ctx *ctx, const uint64_t *alpha_g1, const uint64_t *beta_g2, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *gamma_abc_g1,
                          size_t n_abc);
const uint8_t *pairing_vk_alpha_beta(const vsp_vk *vk);
size_t pairing_vk_n_abc(const vsp_vk *vk);
void pairing_vk_free(vsp_ctx *ctx, vsp_vk *vk);
int pairing_verify_batch(vsp_ctx *ctx, const vsp_vk *vk, const uint64_t *inputs, const uint64_t *A, const uint64_t *B, const uint64_t *C, size_t n, uint8_t *verdict_out);
// SAVER ballot verdicts (pairing.hip): a verification key with the prepared lines of the election key's G2 members
vsp_saver_verifier *saver_verifier_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_pk_words, const uint64_t *alpha_g1, const uint64_t *beta_g2,
                                          const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *gamma_abc_g1, size_t n_abc);
void saver_verifier_free(vsp_ctx *ctx, vsp_saver_verifier *ver);
size_t saver_verifier_msg_size(const vsp_saver_verifier *ver);
size_t saver_verifier_n_rest(const vsp_saver_verifier *ver);
int saver_verify_batch(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *inputs_rest, const uint64_t *A, const uint64_t *B,
                       const uint64_t *C, size_t n, uint8_t *verdict_out, uint8_t *reason_out);
// the same over ballots [first, first + n) of a source: verdict_out[i], reason_out[i] belong to ballot first + i
int saver_verify_source(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t first, size_t n, uint8_t *verdict_out, uint8_t *reason_out);
size_t saver_exact_piece(const vsp_ctx *ctx, size_t msg_size);  // ballots of one piece of the exact path: "pairing_chunk" and the 2^19-argument bound
// one piece of ballots (pairing.hip): the c ballots from ballot `at` of the source on, prepared between events 0 and 1 of `timer` --
// host limbs uploaded and k_ballot_prepare run, or a range of a decoded piece gathered by k_receive_prepare (receive.hip).
// Leaves the arguments c_0 .. c_n | psi | acc | C column by column and A in ctx->pair_g1 ((n + 5) c points), B in ctx->pair_g2, the
// status bytes in ctx->pair_status (room for 3 c)
int saver_piece_prepare(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t at, size_t c, StageTimer &timer);
// the device half of it for a decoded piece (receive.hip): ballots [lo, lo + c) of the piece
int receive_piece_prepare(vsp_ctx *ctx, const vsp_saver_verifier *ver, const ReceivedPiece &rp, size_t lo, size_t c, void *d_pts, void *d_a, void *d_b, uint8_t *d_status);
// the ballot box's share of a received piece of c ballots (ballot_box.hip).  Each queues its kernels and copies on the context's stream;
// the host arrays they fill are valid once the stream is waited for.
//   screen   k_box_screen over the decoded rest inputs: d_row[k] = 0, 8 (a FIXED input differs) or 16 (the serial is committed);
//            box->h_hold[k] the holder's ordinal for 16
//   settle   grows the table where the piece could pass half its slots; k_box_claim and k_box_resolve over the ballots with
//            d_skip[k] = 0; a ballot whose serial a lower index of the piece holds gets d_skip[k] = 1; box->h_win, box->h_flag
//   commit   after the wait: the losers' verdicts (0, reason 16, holder) and the winners' ordinals, k_box_commit, the wait for it;
//            *accepted_out the ballots of the piece that remain accepted.  verdict / reason / holder: the piece's own (reason, holder
//            may be null; for vsp_ballot_box_add_serials verdict is a status array: 1 = already held)
//   restore  the table rebuilt from the store (after an error between settle and commit)
int box_piece_screen(vsp_ctx *ctx, vsp_ballot_box *box, const uint32_t *d_rest, size_t c, uint8_t *d_row);
int box_piece_settle(vsp_ctx *ctx, vsp_ballot_box *box, size_t c, uint8_t *d_skip);
int box_piece_commit(vsp_ctx *ctx, vsp_ballot_box *box, size_t c, uint8_t *verdict, uint8_t *reason, uint64_t *holder, bool as_status, size_t *accepted_out);
int box_restore(vsp_ctx *ctx, vsp_ballot_box *box);
void box_add_times(vsp_ctx *ctx, vsp_ballot_box *box, bool screen, bool settle);
// the screened check (screen.hip); coeff: count x 2 words, none zero (capi.hip checks)
int saver_verify_batch_screened(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *inputs_rest, const uint64_t *A, const uint64_t *B,
                                const uint64_t *C, size_t n, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out);
// one piece of it: ballots [at, at + c) of the source, c at most screen_piece_ballots; coeff, verdict_out, reason_out are the call's
// (indexed by ballot).  The caller drains the work slots after an error
int screen_piece(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t at, size_t c, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out);
size_t screen_piece_ballots(const vsp_ctx *ctx);                // option "saver_screen_chunk"
// stage 1 of pairing.hip on its own: the Miller values of n device pairs (Montgomery affine points; infinity gives one)
int pairing_miller(vsp_ctx *ctx, const void *d_g1, const void *d_g2, size_t n, void *d_out);
// the final exponentiation of n Miller values on the device (stage 3 of pairing.hip on its own): canonical GT values and is-one bytes
int pairing_final_exp(vsp_ctx *ctx, const void *d_miller, size_t n, void *d_gt_out, uint8_t *d_is_one_out);
// one tower operation on n device values of 6 * level words, canonical in and out (vsp_selftest_tower; level and op already checked):
// pairing.hip runs everything but the power of level 12, which is decrypt.hip's (e: the first four words of each b)
int pairing_selftest_tower(vsp_ctx *ctx, int level, int op, const void *d_a, const void *d_b, void *d_out, size_t n);
int decrypt_selftest_gt_pow(vsp_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
// SAVER decryption and its verification (decrypt.hip): the baby-step tables of a key, resident
vsp_saver_decryptor *saver_decryptor_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_vk_words, const uint64_t *gamma_abc_g1, uint64_t max_value);
void saver_decryptor_free(vsp_ctx *ctx, vsp_saver_decryptor *dec);
size_t saver_decryptor_msg_size(const vsp_saver_decryptor *dec);
uint64_t saver_decryptor_max_value(const vsp_saver_decryptor *dec);
unsigned saver_decryptor_baby_bits(const vsp_saver_decryptor *dec);
const uint8_t *saver_decryptor_base(const vsp_saver_decryptor *dec, size_t slot);
int saver_decrypt_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t rho[4], const uint64_t *ct, size_t count, uint64_t *msgs_out, uint64_t *nu_out,
                        uint8_t *status_out);
int saver_verify_decryption_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t *ct, const uint64_t *msgs, const uint64_t *nu, size_t count,
                                  uint8_t *verdict_out, uint8_t *reason_out, uint32_t *first_bad_slot_out);
int upload_power_tables(vsp_ctx *ctx, const HFr &base, size_t hi_count, DevBuf &lo, DevBuf &hi);
HFr host_omega(unsigned log_m);

// canonical <-> host Montgomery helpers: one field element, an affine point (x | y) and a Jacobian record (X | Y | Z); HFp2 values
// are c0 | c1, 6 words each
template <class F> inline F host_load_canon(const uint64_t *p) { F t; memcpy(&t, p, sizeof(F)); return to_mont(t); }
template <class F> inline void host_store_canon(uint64_t *p, const F &m) { F t = from_mont(m); memcpy(p, &t, sizeof(F)); }
template <class HF> inline Affine<HF> host_load_affine(const uint64_t *p) {
    constexpr size_t w = sizeof(HF) / 8;
    Affine<HF> a; a.x = host_load_canon<HF>(p); a.y = host_load_canon<HF>(p + w); return a;
}
template <class HF> inline void host_store_affine(uint64_t *p, const Affine<HF> &a) {
    constexpr size_t w = sizeof(HF) / 8;
    host_store_canon(p, a.x); host_store_canon(p + w, a.y);
}
template <class HF> inline Jacobian<HF> host_load_jacobian(const uint64_t *p) {
    constexpr size_t w = sizeof(HF) / 8;
    Jacobian<HF> j; j.X = host_load_canon<HF>(p); j.Y = host_load_canon<HF>(p + w); j.Z = host_load_canon<HF>(p + 2 * w); return j;
}
template <class HF> inline void host_store_jacobian(uint64_t *p, const Jacobian<HF> &j) {
    constexpr size_t w = sizeof(HF) / 8;
    host_store_canon(p, j.X); host_store_canon(p + w, j.Y); host_store_canon(p + 2 * w, j.Z);
}

// ---- host codec helpers: canonical values as little-endian 64-bit limbs
// nl limbs <-> nl * 8 big-endian bytes
inline void be_from_limbs(uint8_t *o, const uint64_t *l, int nl) { for (int i = 0; i < nl; i++) for (int b = 0; b < 8; b++) o[nl * 8 - 1 - (i * 8 + b)] = (uint8_t)(l[i] >> (8 * b)); }
inline void limbs_from_be(uint64_t *l, const uint8_t *p, int nl) {
    for (int i = 0; i < nl; i++) { uint64_t v = 0; for (int b = 0; b < 8; b++) v |= (uint64_t)p[nl * 8 - 1 - (i * 8 + b)] << (8 * b); l[i] = v; }
}
inline bool limbs_zero(const uint64_t *l, int n) { uint64_t o = 0; for (int i = 0; i < n; i++) o |= l[i]; return o == 0; }
// P::N limbs below the modulus P::MOD (FpP64: a coordinate below p; FrP64: a scalar below r)
template <class P> inline bool below_mod(const uint64_t *l) {
    for (int i = P::N - 1; i >= 0; i--) { if (l[i] < P::MOD[i]) return true; if (l[i] > P::MOD[i]) return false; }
    return false;
}
// a host scalar as the kernels take it (the same Montgomery value on 32-bit limbs)
inline Fr to_dev(const HFr &h) { Fr d; memcpy(&d, &h, sizeof(Fr)); return d; }
inline HFr host_from_u64(uint64_t v) { uint64_t c[4] = {v, 0, 0, 0}; return host_load_canon<HFr>(c); }
// the curve constant b of y^2 = x^3 + b: 4 (G1), 4 (1 + u) (G2)
template <class HF> inline HF curve_b();
template <> inline HFp curve_b<HFp>() { return dbl(dbl(HFp::one())); }
template <> inline HFp2 curve_b<HFp2>() { HFp2 b; b.c0 = curve_b<HFp>(); b.c1 = b.c0; return b; }
// `words` canonical words (whole Fp values) all below p
inline bool coords_below_p(const uint64_t *l, size_t words) { for (size_t k = 0; k < words; k += 6) if (!below_mod<FpP64>(l + k)) return false; return true; }
// canonical affine words of group G: every coordinate below p, and the point on the curve or all zero (infinity)
template <class G> inline bool affine_valid(const uint64_t *p) {
    if (!coords_below_p(p, G::AFFINE_WORDS)) return false;
    const Affine<typename G::HF> a = host_load_affine<typename G::HF>(p);
    return is_inf(a) || eq(sqr(a.y), add(mul(sqr(a.x), a.x), curve_b<typename G::HF>()));
}

// a canonical scalar (two 16-byte halves of its eight 32-bit words) below r: the multi-exponentiations' census (msm_sort.hip k_classify) and
// the witness check (prover.hip k_witness_canonical) refuse the same values
__device__ __forceinline__ bool scalar_below_r(const uint4 &lo, const uint4 &hi) {
    // r = 0x73eda753299d7d48 3339d80809a1d805 53bda402fffe5bfe ffffffff00000001, compared from the top 32-bit word down
    const uint32_t k[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const uint32_t r[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    bool lt = false, gt = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt = lt || (!gt && k[i] < r[i]);
        gt = gt || (!lt && k[i] > r[i]);
    }
    return lt;
}

static inline unsigned ceil_log2(size_t n) { unsigned l = 0; while (((size_t)1 << l) < n) l++; return l; }

}  // namespace vsp
