// SAVER ballots in batches (include/vsp.h "SAVER ballots in batches"): the ciphertexts of many votes of one election on
// the GPU, beside the batch prover's proofs.
//
// A ciphertext is msg_size + 2 sums of scalar multiples of the election key's FIXED points, so over tables of window multiples it is a
// sum of table entries and nothing else: no doubling, and no chain longer than the lanes of a group make it (saver_ct.h has the
// columns, the split into lanes and the fold; this file has the tables' upload, the two launches and the calls).  The kernels run on a
// stream of the context's own, so beside a batch proof they fill the gaps between the prover's kernels; the proof's SAVER term
// r_enc P2 is one more column and reaches the batch assembly (prover.hip) as a per-member addend.
#include <chrono>

#include "common.h"

namespace vsp {
namespace {

static constexpr unsigned CT_BLOCK = 256;
// Each lane of a ballot's span sums its share of its column's terms; the groups then fold through LDS (a group lies inside one wave, the
// barriers are the block's: every thread reaches every one of them).  sums[ballot][column] = the column in XYZZ
__global__ __launch_bounds__(CT_BLOCK) void k_saver_ct(const G1Affine *tab, const SaverColumn *cols, const SaverPair *pairs, const uint32_t *lane_col, unsigned ballot_lanes,
                                                       unsigned n_cols, unsigned n_scalars, const uint64_t *scalars, size_t count, G1XYZZ *sums) {
    __shared__ G1XYZZ part[CT_BLOCK];
    const size_t g = (size_t)blockIdx.x * CT_BLOCK + threadIdx.x, ballot = g / ballot_lanes;
    const uint32_t c = ballot < count ? lane_col[g % ballot_lanes] : SAVER_NO_COLUMN;
    unsigned lane = 0, lanes = 0;
    G1XYZZ acc = G1XYZZ::inf();
    if (c != SAVER_NO_COLUMN) {
        const SaverColumn col = cols[c];
        lanes = col.lanes; lane = (unsigned)(g % ballot_lanes) - col.lane0;
        saver_lane_sum(acc, tab, scalars + ballot * n_scalars * 4, col, pairs, lane, lanes, [](G1XYZZ *a, const G1Affine *q) { xyzz_madd(*a, *q); });
    }
    saver_fold_lds(acc, part, lane, lanes);
    if (lanes && lane == 0) sums[ballot * n_cols + c] = acc;
}
// canonical affine words of every sum (infinity: all zero), one inversion per point
__global__ __launch_bounds__(64) void k_saver_ct_affine(const G1XYZZ *sums, size_t points, G1Affine *out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= points) return;
    const G1Affine a = xyzz_to_affine(sums[i]);
    G1Affine r; r.x = from_mont(a.x); r.y = from_mont(a.y);
    out[i] = r;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// the tables of the key on the host (`flat`) and on the context's device, and the plan behind them; once per key
static int tables_ready(vsp_ctx *ctx, const vsp_saver_pk *spk) {
    if (spk->uploaded.load(std::memory_order_acquire)) {
        if (spk->device != ctx->device) return set_error(ctx, VSP_ERR_UNSUPPORTED, "saver_pk_upload: the key's tables are resident on another device");
        return VSP_OK;
    }
    std::lock_guard<std::mutex> lock(spk->up_mu);
    if (spk->uploaded.load(std::memory_order_relaxed)) return tables_ready(ctx, spk);
    VSP_HIP(hipSetDevice(ctx->device));
    const double t0 = now_ms();
    const size_t n = spk->n, nb = saver_bases(n);
    // the G and Y tables do not exist yet; X and P2 are the key's own
    std::vector<FixedBase> gy(2 * n);
    host_parallel_for(2 * n, [&](size_t j) { gy[j].build(j < n ? spk->G[j] : spk->Y[j - n]); });
    std::vector<uint8_t> base_inf(nb, 0);
    spk->flat.assign(nb * SAVER_TABLE_POINTS, Affine<HFp>{HFp::zero(), HFp::zero()});
    auto place = [&](size_t b, const FixedBase &f) {
        base_inf[b] = f.inf;
        if (!f.inf) std::copy(f.tab.begin(), f.tab.end(), spk->flat.begin() + b * SAVER_TABLE_POINTS);
    };
    for (size_t i = 0; i < n + 2; i++) place(saver_base_X(i), spk->X[i]);
    place(saver_base_P2(n), spk->P2);
    for (size_t i = 1; i <= n; i++) { place(saver_base_G(n, i), gy[i - 1]); place(saver_base_Y(n, i), gy[n + i - 1]); }
    spk->plan = saver_plan(n, base_inf.data());
    const SaverPlan &pl = spk->plan;
    // host Montgomery points and device ones are the same bytes (fixedbase_impl.inc build_fixed_table)
    static_assert(sizeof(Affine<HFp>) == sizeof(G1Affine), "one table for the host and the device");
    const size_t tab_bytes = spk->flat.size() * sizeof(G1Affine);
    DevBuf d_tab, d_desc;
    int rc = VSP_OK;
    if (d_tab.alloc(tab_bytes) != hipSuccess) rc = set_error(ctx, VSP_ERR_NOMEM, "saver_pk_upload: hipMalloc of the key's tables failed");
    else if (const hipError_t e = hipMemcpy(d_tab.p, spk->flat.data(), tab_bytes, hipMemcpyHostToDevice); e != hipSuccess) rc = set_hip_error(ctx, e, "hipMemcpy of the key's tables", __FILE__, __LINE__);
    else rc = upload_plan(ctx, pl, d_desc);
    if (rc != VSP_OK) { spk->flat.clear(); return rc; }
    spk->device = ctx->device; spk->device_bytes = d_tab.cap + d_desc.cap;
    spk->d_tab = std::move(d_tab); spk->d_desc = std::move(d_desc);
    ctx->stats["saver_ct_table_ms"] += now_ms() - t0;
    spk->uploaded.store(true, std::memory_order_release);
    return VSP_OK;
}

// THE PIECE.  At most "saver_ct_chunk" ballots (option, default and maximum 1024) go through the kernels at a time, so the workspace is
// bounded whatever `count` is: per ballot 32 (n + 1) bytes of scalars, 192 (n + 3) of column sums and 96 (n + 3) of points on the device
// and the scalars and points once more in pinned memory -- 9.1 MB + 3.6 MB at msg_size 25.
static size_t piece_ballots(const vsp_ctx *ctx) { const long c = opt(ctx, "saver_ct_chunk", 1024); return c < 1 ? 1 : (c > 1024 ? 1024 : (size_t)c); }

// the ciphertext stream and the event behind a piece, made on first use
static int ct_stream_ready(vsp_ctx *ctx) {
    auto &w = ctx->saver_ct;
    VSP_HIP(hipSetDevice(ctx->device));
    if (!w.stream) VSP_HIP(hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    if (!w.done) VSP_HIP(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    return VSP_OK;
}
// c ballots (msgs: c x n x 4, r_enc: c x 4) onto the ciphertext stream: scalars up, the two kernels between events 0 and 1 of the timer,
// the points back to pinned memory, the event `done` behind them
//
// msgs null: the device form -- the batch prover's front half has gathered z_k = (1, row of member k) into pr_z, with ctx->ev_aux recorded
// behind the gather; the message, the first msg_size values of each row, is copied from there, device to device, beside r_enc from the host
static int ct_queue(vsp_ctx *ctx, const vsp_saver_pk *spk, const uint64_t *msgs, const uint64_t *r_enc, size_t c, size_t z_stride = 0) {
    auto &w = ctx->saver_ct;
    const size_t n = spk->n, ns = n + 1, nc = saver_columns(n);
    VSP_TRY(ct_stream_ready(ctx));
    VSP_TRY(ensure(ctx, w.scalars, c * ns * 32, w.stream));
    VSP_TRY(ensure(ctx, w.sums, c * nc * sizeof(G1XYZZ), w.stream));
    VSP_TRY(ensure(ctx, w.points, c * nc * sizeof(G1Affine), w.stream));
    VSP_TRY(ensure_pinned(ctx, w.h_scalars, c * ns * 32));
    VSP_TRY(ensure_pinned(ctx, w.h_points, c * nc * sizeof(G1Affine)));
    uint64_t *hs = w.h_scalars.as<uint64_t>();
    if (msgs) {
        for (size_t k = 0; k < c; k++) { memcpy(hs + k * ns * 4, r_enc + 4 * k, 32); memcpy(hs + k * ns * 4 + 4, msgs + k * n * 4, n * 32); }
        VSP_HIP(hipMemcpyAsync(w.scalars.p, hs, c * ns * 32, hipMemcpyHostToDevice, w.stream));
    } else {
        memcpy(hs, r_enc, c * 32);
        VSP_HIP(hipMemcpy2DAsync(w.scalars.p, ns * 32, hs, 32, 32, c, hipMemcpyHostToDevice, w.stream));
        VSP_HIP(hipStreamWaitEvent(w.stream, ctx->ev_aux, 0));
        VSP_HIP(hipMemcpy2DAsync((uint64_t *)w.scalars.p + 4, ns * 32, (const uint64_t *)ctx->pr_z.p + 4, z_stride * 32, n * 32, c, hipMemcpyDeviceToDevice, w.stream));
    }
    const SaverColumn *d_cols = spk->d_desc.as<const SaverColumn>();
    const SaverPair *d_pairs = (const SaverPair *)(d_cols + spk->plan.cols.size());
    const uint32_t *d_lane_col = (const uint32_t *)(d_pairs + spk->plan.pairs.size());
    const unsigned ballot_lanes = (unsigned)spk->plan.lane_col.size();
    VSP_TRY(w.timer.mark(ctx, 0, w.stream));
    hipLaunchKernelGGL(k_saver_ct, dim3((unsigned)((c * ballot_lanes + CT_BLOCK - 1) / CT_BLOCK)), dim3(CT_BLOCK), 0, w.stream, spk->d_tab.as<const G1Affine>(), d_cols, d_pairs,
                       d_lane_col, ballot_lanes, (unsigned)nc, (unsigned)ns, (const uint64_t *)w.scalars.p, c, (G1XYZZ *)w.sums.p);
    VSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_saver_ct_affine, dim3((unsigned)((c * nc + 63) / 64)), dim3(64), 0, w.stream, (const G1XYZZ *)w.sums.p, c * nc, (G1Affine *)w.points.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(w.timer.mark(ctx, 1, w.stream));
    VSP_HIP(hipMemcpyAsync(w.h_points.p, w.points.p, c * nc * sizeof(G1Affine), hipMemcpyDeviceToHost, w.stream));
    VSP_HIP(hipEventRecord(w.done, w.stream));
    return VSP_OK;
}
// ballot k's columns -> its row of each output (any may be null)
static void ct_store(size_t n, const uint64_t *cols, size_t k, uint64_t *ct_out, uint64_t *addend_out, uint8_t *blobs_out) {
    const size_t ctw = (n + 2) * 12;
    if (ct_out) memcpy(ct_out + k * ctw, cols, ctw * 8);
    if (addend_out) memcpy(addend_out + 12 * k, cols + ctw, 96);
    if (blobs_out) vsp_g1_vector_to_blob(cols, n + 2, blobs_out + k * vsp_g1_vector_blob_size(n + 2));
}
// the wait for a queued piece and its results
static int ct_collect(vsp_ctx *ctx, size_t n, size_t c, size_t at, uint64_t *ct_out, uint64_t *addend_out, uint8_t *blobs_out) {
    auto &w = ctx->saver_ct;
    VSP_HIP(hipEventSynchronize(w.done));
    w.timer.add(ctx, 0, "saver_ct_ms");
    for (size_t k = 0; k < c; k++) ct_store(n, w.h_points.as<const uint64_t>() + k * saver_columns(n) * 12, at + k, ct_out, addend_out, blobs_out);
    return VSP_OK;
}
// the host leg (option "saver_encrypt_gpu" = 0): the same columns over the same tables, one lane per column, a ballot per task
static void ct_host(const vsp_saver_pk *spk, const uint64_t *msgs, const uint64_t *r_enc, size_t count, uint64_t *ct_out, uint64_t *addend_out, uint8_t *blobs_out) {
    const size_t n = spk->n, nc = saver_columns(n);
    const SaverPlan &pl = spk->plan;
    host_parallel_for(count, [&](size_t k) {
        std::vector<uint64_t> scal(4 * (n + 1)), cols(nc * 12);
        memcpy(scal.data(), r_enc + 4 * k, 32); memcpy(scal.data() + 4, msgs + k * n * 4, n * 32);
        for (size_t c = 0; c < nc; c++) {
            XYZZ<HFp> acc;
            saver_lane_sum(acc, spk->flat.data(), scal.data(), pl.cols[c], pl.pairs.data(), 0, 1, [](XYZZ<HFp> *a, const Affine<HFp> *q) { xyzz_madd(*a, *q); });
            host_store_affine(cols.data() + 12 * c, xyzz_to_affine(acc));
        }
        ct_store(n, cols.data(), k, ct_out, addend_out, blobs_out);
    });
}
// every scalar of the batch canonical; the refusal names the member.  msgs null (the device form): r_enc alone is host data
static int scalars_canonical(vsp_ctx *ctx, const char *who, size_t n, const uint64_t *msgs, const uint64_t *r_enc, size_t count) {
    char m[160];
    for (size_t k = 0; k < count; k++) {
        if (!below_mod<FrP64>(r_enc + 4 * k)) { snprintf(m, sizeof m, "%s: r_enc of member %zu is not canonical (>= r)", who, k); return set_error(ctx, VSP_ERR_ARG, m); }
        for (size_t i = 0; msgs && i < n; i++)
            if (!below_mod<FrP64>(msgs + (k * n + i) * 4)) { snprintf(m, sizeof m, "%s: message block %zu of member %zu is not canonical (>= r)", who, i, k); return set_error(ctx, VSP_ERR_ARG, m); }
    }
    return VSP_OK;
}

// a batch of ballots is in flight: launched (every prover launch clears the mark, the ballot launch sets it afterwards), and its proofs
// not finished behind its back by vsp_groth16_prove_batch_finish
static bool ballots_in_flight(const vsp_ctx *ctx) { return ctx->saver_ct.active && ctx->prove.active && ctx->prove.batch; }

// the launch both forms share, behind their checks: the batch prover over the source, then the ciphertexts -- msgs from the host, or
// (msgs null, a device source) the first msg_size values of each member's z in pr_z
static int ballots_launch(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &src, const uint64_t *msgs, size_t count,
                          const uint64_t *r_enc, const uint64_t *r, const uint64_t *s) {
    const size_t n = spk->n, zs = cs->num_vars + 1;
    VSP_TRY(prove_batch_launch_src(ctx, cs, pk, src, count, r, s));
    auto &w = ctx->saver_ct;
    w.gpu = opt(ctx, "saver_encrypt_gpu", 1) != 0;
    w.device_src = msgs == nullptr;
    int rc = VSP_OK;
    if (w.gpu) rc = ct_queue(ctx, spk, msgs, r_enc, count, zs);
    else {
        // the host leg computes in the finish, inside the wait for the proofs: it keeps the scalars until then
        rc = ensure_pinned(ctx, w.h_scalars, count * (n + 1) * 32);
        if (rc == VSP_OK) memcpy(w.h_scalars.p, r_enc, count * 32);
        if (rc == VSP_OK && msgs) memcpy(w.h_scalars.as<uint64_t>() + count * 4, msgs, count * n * 32);
        // the device form: the count x msg_size message scalars, and nothing else, come to the host, behind the gather; the finish waits for them
        if (rc == VSP_OK && !msgs) rc = [&]() -> int {
            VSP_TRY(ct_stream_ready(ctx));
            VSP_HIP(hipStreamWaitEvent(w.stream, ctx->ev_aux, 0));
            VSP_HIP(hipMemcpy2DAsync(w.h_scalars.as<uint64_t>() + count * 4, n * 32, (const uint64_t *)ctx->pr_z.p + 4, zs * 32, n * 32, count, hipMemcpyDeviceToHost, w.stream));
            VSP_HIP(hipEventRecord(w.done, w.stream));
            return VSP_OK;
        }();
    }
    if (rc != VSP_OK) {
        // the proofs are queued and cannot be recalled: finish them into nothing, keep this call's error
        const std::string keep = ctx->err;
        if (w.stream) hipStreamSynchronize(w.stream);      // nothing of this call still reads pr_z when the finish zeroes it
        (void)vsp_groth16_prove_batch_finish(ctx, nullptr, nullptr, nullptr, nullptr);
        ctx->err = keep;
        return rc;
    }
    w.active = true; w.spk = spk; w.count = count;
    return VSP_OK;
}

}  // anonymous namespace

int upload_plan(vsp_ctx *ctx, const SaverPlan &pl, DevBuf &out) {
    const size_t cb = pl.cols.size() * sizeof(SaverColumn), pb = pl.pairs.size() * sizeof(SaverPair), lb = pl.lane_col.size() * sizeof(uint32_t);
    DevBuf d;
    if (d.alloc(cb + pb + lb) != hipSuccess) return set_error(ctx, VSP_ERR_NOMEM, "hipMalloc of a plan failed");
    hipError_t e = hipMemcpy(d.p, pl.cols.data(), cb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.as<char>() + cb, pl.pairs.data(), pb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.as<char>() + cb + pb, pl.lane_col.data(), lb, hipMemcpyHostToDevice);
    if (e != hipSuccess) return set_hip_error(ctx, e, "hipMemcpy of a plan", __FILE__, __LINE__);
    out = std::move(d);
    return VSP_OK;
}
void saver_ct_release(vsp_ctx *ctx) {
    auto &w = ctx->saver_ct;
    if (w.stream) hipStreamSynchronize(w.stream);
    if (w.done) hipEventDestroy(w.done);
    w.done = nullptr;
    if (w.stream) hipStreamDestroy(w.stream);
    w.stream = nullptr;
}
void saver_pk_release_device(vsp_saver_pk *spk) {
    if (!spk->uploaded.load()) return;
    hipSetDevice(spk->device);
    hipDeviceSynchronize();                  // a context may still be reading the tables
    spk->d_tab.reset(); spk->d_desc.reset();
    spk->device_bytes = 0;
    spk->uploaded.store(false);
}

}  // namespace vsp

using namespace vsp;
extern "C" {

int vsp_saver_pk_upload(vsp_ctx *ctx, vsp_saver_pk *spk) {
    if (!ctx) return VSP_ERR_ARG;
    if (!spk) return set_error(ctx, VSP_ERR_ARG, "saver_pk_upload: null argument");
    return tables_ready(ctx, spk);
}
size_t vsp_saver_pk_device_bytes(const vsp_saver_pk *spk) { return spk && spk->uploaded.load() ? spk->device_bytes : 0; }

int vsp_saver_ciphertext_batch(vsp_ctx *ctx, const vsp_saver_pk *spk, const uint64_t *msgs, const uint64_t *r_enc, size_t count, uint64_t *ct_out, uint64_t *addend_out,
                               uint8_t *ct_blobs_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!spk || !ct_out || (count && (!msgs || !r_enc))) return set_error(ctx, VSP_ERR_ARG, "saver_ciphertext_batch: null argument");
    if (ballots_in_flight(ctx)) return set_error(ctx, VSP_ERR_ARG, "saver_ciphertext_batch: a batch of ballots is in flight on this context and owns the workspace (finish it first)");
    VSP_TRY(scalars_canonical(ctx, "saver_ciphertext_batch", spk->n, msgs, r_enc, count));
    VSP_TRY(tables_ready(ctx, spk));
    if (!opt(ctx, "saver_encrypt_gpu", 1)) { ct_host(spk, msgs, r_enc, count, ct_out, addend_out, ct_blobs_out); return VSP_OK; }
    const size_t n = spk->n, piece = piece_ballots(ctx);
    for (size_t at = 0; at < count; at += piece) {
        const size_t c = count - at < piece ? count - at : piece;
        VSP_TRY(ct_queue(ctx, spk, msgs + at * n * 4, r_enc + at * 4, c));
        VSP_TRY(ct_collect(ctx, n, c, at, ct_out, addend_out, ct_blobs_out));
    }
    return VSP_OK;
}

int vsp_saver_encrypt_batch_launch(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *msgs, const uint64_t *witnesses, size_t count,
                                   const uint64_t *r_enc, const uint64_t *r, const uint64_t *s) {
    if (!ctx) return VSP_ERR_ARG;
    if (!spk || !cs || !pk || !msgs || !witnesses || !r_enc || !r || !s || count < 1 || count > 64) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch: null argument or a batch outside 1..64");
    if (ballots_in_flight(ctx)) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch: a batch of ballots is already in flight on this context (finish it first)");
    const size_t n = spk->n;
    if (cs->num_inputs < n) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch: the constraint system has fewer public inputs than message blocks");
    VSP_TRY(scalars_canonical(ctx, "saver_encrypt_batch", n, msgs, r_enc, count));
    for (size_t k = 0; k < count; k++)      // the message IS the first msg_size public inputs (vsp_saver_encrypt)
        if (memcmp(msgs + k * n * 4, witnesses + k * cs->num_vars * 4, n * 32) != 0) {
            char m[160]; snprintf(m, sizeof m, "saver_encrypt_batch: the message of member %zu differs from the first public inputs of its witness", k);
            return set_error(ctx, VSP_ERR_ARG, m);
        }
    VSP_TRY(tables_ready(ctx, spk));
    const WitnessSrc src{witnesses, nullptr, nullptr, nullptr, 0};
    return ballots_launch(ctx, spk, cs, pk, src, msgs, count, r_enc, r, s);
}

int vsp_saver_encrypt_batch_launch_device(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows,
                                          const uint32_t *members, size_t count, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s) {
    if (!ctx) return VSP_ERR_ARG;
    if (!spk || !cs || !pk || !d_witnesses || !r_enc || !r || !s || count < 1 || count > 64)
        return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch_device: null argument or a batch outside 1..64");
    if (ballots_in_flight(ctx)) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch_device: a batch of ballots is already in flight on this context (finish it first)");
    if (cs->num_inputs < spk->n) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch_device: the constraint system has fewer public inputs than message blocks");
    WitnessSrc src;
    VSP_TRY(witness_src_device(ctx, "saver_encrypt_batch_device", cs, d_witnesses, stride, rows, members, count, &src));
    VSP_TRY(scalars_canonical(ctx, "saver_encrypt_batch_device", spk->n, nullptr, r_enc, count));
    VSP_TRY(tables_ready(ctx, spk));
    return ballots_launch(ctx, spk, cs, pk, src, nullptr, count, r_enc, r, s);
}

int vsp_saver_encrypt_batch_finish(vsp_ctx *ctx, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out) {
    if (!ctx) return VSP_ERR_ARG;
    auto &w = ctx->saver_ct;
    if (!ballots_in_flight(ctx)) return set_error(ctx, VSP_ERR_ARG, "saver_encrypt_batch_finish: no batch of ballots in flight on this context");
    w.active = false;
    const size_t n = w.spk->n, K = w.count, ctw = (n + 2) * 12, blob = vsp_g1_vector_blob_size(n + 2);
    ctx->prove.addend.assign(12 * K, 0);
    int rc;
    if (w.gpu) rc = ct_collect(ctx, n, K, 0, ct_out, ctx->prove.addend.data(), ct_blobs_out);
    else {
        rc = w.device_src ? [&]() -> int { VSP_HIP(hipEventSynchronize(w.done)); return VSP_OK; }() : VSP_OK;
        if (rc == VSP_OK) ct_host(w.spk, w.h_scalars.as<const uint64_t>() + K * 4, w.h_scalars.as<const uint64_t>(), K, ct_out, ctx->prove.addend.data(), ct_blobs_out);
    }
    if (rc != VSP_OK) {
        const std::string keep = ctx->err;
        (void)vsp_groth16_prove_batch_finish(ctx, nullptr, nullptr, nullptr, nullptr);
        ctx->err = keep;
        return rc;
    }
    rc = vsp_groth16_prove_batch_finish(ctx, A_out, B_out, C_out, proofs_out);
    if (rc == VSP_OK || rc == VSP_ERR_UNSATISFIED) ctx->stats["saver_encrypt_batches"] += 1;
    // option "prove_check_witness": no ciphertext leaves for a statement that has no proof
    if (rc == VSP_ERR_UNSATISFIED)
        for (size_t k = 0; k < K; k++)
            if (ctx->batch_status[k]) {
                if (ct_out) memset(ct_out + k * ctw, 0, ctw * 8);
                if (ct_blobs_out) memset(ct_blobs_out + k * blob, 0, blob);
            }
    // the device form met its messages only on the device: where the proofs' census refuses the batch (a value >= r), no ciphertext leaves either
    if (w.device_src && rc != VSP_OK && rc != VSP_ERR_UNSATISFIED) {
        if (ct_out) memset(ct_out, 0, K * ctw * 8);
        if (ct_blobs_out) memset(ct_blobs_out, 0, K * blob);
    }
    return rc;
}

int vsp_saver_encrypt_batch(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *msgs, const uint64_t *witnesses, size_t count,
                            const uint64_t *r_enc, const uint64_t *r, const uint64_t *s, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out,
                            uint8_t *proofs_out, uint8_t *ct_blobs_out) {
    int rc = vsp_saver_encrypt_batch_launch(ctx, spk, cs, pk, msgs, witnesses, count, r_enc, r, s);
    if (rc != VSP_OK) return rc;
    return vsp_saver_encrypt_batch_finish(ctx, ct_out, A_out, B_out, C_out, proofs_out, ct_blobs_out);
}

int vsp_saver_encrypt_batch_device(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows,
                                   const uint32_t *members, size_t count, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s, uint64_t *ct_out, uint64_t *A_out,
                                   uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out) {
    int rc = vsp_saver_encrypt_batch_launch_device(ctx, spk, cs, pk, d_witnesses, stride, rows, members, count, r_enc, r, s);
    if (rc != VSP_OK) return rc;
    return vsp_saver_encrypt_batch_finish(ctx, ct_out, A_out, B_out, C_out, proofs_out, ct_blobs_out);
}

}  // extern "C"
