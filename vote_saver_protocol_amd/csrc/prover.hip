// Groth16 prover orchestration (r1cs_gg_ppzksnark_prover::process), the sparse R1CS mat-vec that feeds
// r1cs_to_qap::witness_map, and the generator-side fixed-base batch exponentiation.
//
// Replaces, for the hot path, crypto3-zk r1cs_gg_ppzksnark/prover.hpp + reductions/r1cs_to_qap.hpp
// (absent submodule, /root/reference/.gitmodules:11-12; README.md:272-273 points at prover.hpp#L73),
// reached from bin/cli/include/nil/vote_saver/common.hpp:1132-1135; the generator's batch_exp is
// reached from common.hpp:916-917.
//
//   A = alpha + sum z_i A_i + r delta          (G1)
//   B = beta  + sum z_i B_i + s delta          (G2, and the same in G1 for C)
//   C = sum h_i H_i + sum_{aux} z_i L_i + s A + r B_g1 - r s delta  (+ r_enc P1 in SAVER mode)
#include <chrono>

#include "common.h"

namespace vsp {

// ---- sparse mat-vec: out[row] = sum_e coef[e] * z[col[e]],  z canonical, coef Montgomery -> canonical out
__global__ __launch_bounds__(256) void k_csr_matvec(const uint32_t *rp, const uint32_t *ci, const Fr *co, const Fr *z, size_t rows, Fr *out,
                                                    size_t z_stride = 0, size_t out_stride = 0) {
    z += (size_t)blockIdx.y * z_stride; out += (size_t)blockIdx.y * out_stride;      // grid.y: the witnesses of a batch
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    Fr acc = Fr::zero();
    for (uint32_t e = rp[i]; e < rp[i + 1]; e++) acc = add(acc, mul(z[ci[e]], co[e]));
    out[i] = acc;
}
// ---- the witness check: does member k's z satisfy (A z)[i] (B z)[i] = (C z)[i] on the rows i < rows of the constraint system?
// abc: member k's A z, B z, C z at abc + k stride, m values each, canonical as k_csr_matvec leaves them (rows .. m - 1 -- the
// "input_i * 0 = 0" rows, the padding, a step domain's tail -- belong to the domain, not to the system, and are not read).  One thread per
// (row, member): one conversion to Montgomery form and one product give the canonical a b, compared word for word with c.  The failing
// lanes of a wave are counted by a ballot, and the lowest of them -- the wave's lowest failing row -- issues one atomicMin into
// first_bad[k] (preset to `rows`) and one atomicAdd into bad_rows[k] (preset to 0): both results are independent of the order in which
// waves arrive, and a satisfied witness issues no atomic at all.
__global__ __launch_bounds__(256) void k_r1cs_verdict(const Fr *abc, size_t rows, size_t m, size_t stride, uint32_t *first_bad, uint32_t *bad_rows) {
    const Fr *a = abc + (size_t)blockIdx.y * stride, *b = a + m, *c = b + m;      // grid.y: the witnesses of a batch, as in k_csr_matvec
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < rows) bad = !eq(mul(to_mont(a[i]), b[i]), c[i]);
    const unsigned long long failing = __ballot(bad);
    if (failing == 0) return;
    if ((threadIdx.x & 63u) == (unsigned)__ffsll(failing) - 1u) {
        atomicMin(&first_bad[blockIdx.y], (uint32_t)i);
        atomicAdd(&bad_rows[blockIdx.y], (uint32_t)__popcll(failing));
    }
}
// flag[k] != 0: member k's z = (1, witness) holds a value that is not canonical (>= r), in a wire of a constraint or not -- the mat-vec
// reduces such a value, so the rows alone would not show it.  The comparison is the census' (common.h scalar_below_r).
__global__ __launch_bounds__(256) void k_witness_canonical(const Fr *z, size_t n, size_t z_stride, uint32_t *flag) {
    z += (size_t)blockIdx.y * z_stride;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint4 *w = (const uint4 *)z[i].l;
        const uint4 lo = w[0], hi = w[1];
        bad = hi.w >= 0x73eda753u && !scalar_below_r(lo, hi);
    }
    const unsigned long long failing = __ballot(bad);
    if (failing != 0 && (threadIdx.x & 63u) == (unsigned)__ffsll(failing) - 1u) atomicOr(&flag[blockIdx.y], 1u);
}
__global__ __launch_bounds__(256) void k_fr_to_mont(Fr *a, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = to_mont(a[i]);
}


}  // namespace vsp

using namespace vsp;

// ------------------------------------------------------------------------------------------------ C ABI: r1cs / pk / prove
extern "C" {

vsp_r1cs *vsp_r1cs_upload(vsp_ctx *ctx, size_t num_constraints, size_t num_inputs, size_t num_vars,
                          const uint32_t *row_ptr_a, const uint32_t *col_a, const uint64_t *coef_a,
                          const uint32_t *row_ptr_b, const uint32_t *col_b, const uint64_t *coef_b,
                          const uint32_t *row_ptr_c, const uint32_t *col_c, const uint64_t *coef_c) {
    if (!ctx) return nullptr;
    if (!row_ptr_a || !row_ptr_b || !row_ptr_c || num_inputs > num_vars) { set_error(ctx, VSP_ERR_ARG, "r1cs_upload: bad argument"); return nullptr; }
    hipSetDevice(ctx->device);
    std::unique_ptr<vsp_r1cs> cs(new vsp_r1cs());            // a failure below lets it go with what it holds
    cs->num_constraints = num_constraints; cs->num_inputs = num_inputs; cs->num_vars = num_vars;
    if (domain_init(ctx, &cs->dom, num_constraints + num_inputs + 1) != VSP_OK) return nullptr;
    const uint32_t *rp[3] = {row_ptr_a, row_ptr_b, row_ptr_c}, *ci[3] = {col_a, col_b, col_c};
    const uint64_t *co[3] = {coef_a, coef_b, coef_c};
    for (int m = 0; m < 3; m++) {                             // every matrix before anything is allocated: row pointers monotone from 0, arrays present
        const size_t nnz = rp[m][num_constraints];
        bool mono = rp[m][0] == 0;
        for (size_t r = 0; r < num_constraints && mono; r++) mono = rp[m][r] <= rp[m][r + 1];
        if (!mono || (nnz && (!ci[m] || !co[m]))) {
            set_error(ctx, VSP_ERR_ARG, !mono ? "r1cs_upload: row pointers must start at 0 and not decrease" : "r1cs_upload: null column / coefficient array with nnz > 0");
            return nullptr;
        }
    }
    for (int m = 0; m < 3; m++) {
        size_t nnz = rp[m][num_constraints];
        for (size_t e = 0; e < nnz; e++) if (ci[m][e] > num_vars) { set_error(ctx, VSP_ERR_ARG, "r1cs_upload: column out of range"); return nullptr; }
        for (size_t e = 0; e < nnz; e++) if (!below_mod<FrP64>(co[m] + 4 * e)) { set_error(ctx, VSP_ERR_ARG, "r1cs_upload: a coefficient is not canonical (>= r)"); return nullptr; }
        bool ok = cs->rp[m].alloc((num_constraints + 1) * 4) == hipSuccess && cs->ci[m].alloc((nnz ? nnz : 1) * 4) == hipSuccess &&
                  cs->co[m].alloc((nnz ? nnz : 1) * sizeof(Fr)) == hipSuccess;
        if (!ok) { set_error(ctx, VSP_ERR_NOMEM, "r1cs_upload: hipMalloc"); return nullptr; }
        if (hipMemcpyAsync(cs->rp[m].p, rp[m], (num_constraints + 1) * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(cs->ci[m].p, ci[m], nnz * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipMemcpyAsync(cs->co[m].p, co[m], nnz * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            set_error(ctx, VSP_ERR_HIP, "r1cs_upload: host-to-device copy failed"); return nullptr;
        }
        if (nnz) hipLaunchKernelGGL(k_fr_to_mont, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, cs->co[m].as<Fr>(), nnz);
        // column-major copy by a counting sort over the column index
        std::vector<uint32_t> colptr(num_vars + 2, 0), rows(nnz ? nnz : 1);
        std::vector<uint64_t> cot((nnz ? nnz : 1) * 4);
        for (size_t e = 0; e < nnz; e++) colptr[ci[m][e] + 1]++;
        for (size_t c = 0; c <= num_vars; c++) colptr[c + 1] += colptr[c];
        std::vector<uint32_t> cur(colptr.begin(), colptr.end() - 1);
        for (size_t r = 0; r < num_constraints; r++)
            for (uint32_t e = rp[m][r]; e < rp[m][r + 1]; e++) {
                uint32_t pos = cur[ci[m][e]]++;
                rows[pos] = (uint32_t)r; memcpy(&cot[4 * (size_t)pos], co[m] + 4 * (size_t)e, 32);
            }
        ok = cs->cp[m].alloc((num_vars + 2) * 4) == hipSuccess && cs->ri[m].alloc((nnz ? nnz : 1) * 4) == hipSuccess &&
             cs->cot[m].alloc((nnz ? nnz : 1) * sizeof(Fr)) == hipSuccess;
        if (!ok) { set_error(ctx, VSP_ERR_NOMEM, "r1cs_upload: hipMalloc"); return nullptr; }
        if (hipMemcpy(cs->cp[m].p, colptr.data(), (num_vars + 2) * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(cs->ri[m].p, rows.data(), nnz * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(cs->cot[m].p, cot.data(), nnz * sizeof(Fr), hipMemcpyHostToDevice) != hipSuccess) {
            set_error(ctx, VSP_ERR_HIP, "r1cs_upload: host-to-device copy failed"); return nullptr;
        }
        if (nnz) hipLaunchKernelGGL(k_fr_to_mont, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, ctx->stream, cs->cot[m].as<Fr>(), nnz);
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error(ctx, VSP_ERR_HIP, "r1cs_upload: sync"); return nullptr; }
    return cs.release();
}

void vsp_r1cs_free(vsp_ctx *ctx, vsp_r1cs *cs) {
    if (!cs) return;
    if (ctx) hipSetDevice(ctx->device);
    delete cs;
}

vsp_pk *vsp_pk_create(vsp_ctx *ctx, const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                      const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                      const vsp_bases *A_query, const vsp_bases *B_query_g1, const vsp_bases *B_query_g2,
                      const vsp_bases *H_query, const vsp_bases *L_query) {
    if (!ctx) return nullptr;
    if (!alpha_g1 || !beta_g1 || !beta_g2 || !delta_g1 || !delta_g2 || !A_query || !B_query_g1 || !B_query_g2 || !H_query || !L_query ||
        A_query->group != 1 || B_query_g1->group != 1 || B_query_g2->group != 2 || H_query->group != 1 || L_query->group != 1) {
        set_error(ctx, VSP_ERR_ARG, "pk_create: bad argument"); return nullptr;
    }
    vsp_pk *pk = new vsp_pk();
    pk->alpha_g1 = host_load_affine<HFp>(alpha_g1); pk->beta_g1 = host_load_affine<HFp>(beta_g1); pk->delta_g1 = host_load_affine<HFp>(delta_g1);
    pk->beta_g2 = host_load_affine<HFp2>(beta_g2); pk->delta_g2 = host_load_affine<HFp2>(delta_g2);
    pk->A = A_query; pk->B1 = B_query_g1; pk->B2 = B_query_g2; pk->H = H_query; pk->L = L_query;
    return pk;
}
void vsp_pk_free(vsp_ctx *, vsp_pk *pk) { delete pk; }
}  // extern "C"
namespace vsp {
// the fixed-base tables of delta (common.h vsp_pk): built by the first proof over the key, 32 x 255 additions per group (~5 ms G1, ~15 ms G2);
// option "prove_fixed_base" = 0 keeps the double-and-add multiplications of rounds 1-3
static bool delta_tables(vsp_ctx *ctx, const vsp_pk *pk) {
    if (opt(ctx, "prove_fixed_base", 1) == 0) return false;
    if (pk->tab_ready.load(std::memory_order_acquire)) return true;
    std::lock_guard<std::mutex> lock(pk->tab_mu);
    if (!pk->tab_ready.load(std::memory_order_relaxed)) {
        std::thread t2([&]() { xyzz_fixed_base_table(xyzz_from_affine(pk->delta_g2), pk->tab2); });
        xyzz_fixed_base_table(xyzz_from_affine(pk->delta_g1), pk->tab1);
        t2.join();
        pk->tab_ready.store(true, std::memory_order_release);
    }
    return true;
}

// host time since the previous lap (or the construction), added to the vsp_get_stat counter the lap names
struct HostLap {
    vsp_ctx *ctx; double t = now();
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void operator()(const char *name) { const double t1 = now(); ctx->stats[name] += t1 - t; t = t1; }
};

// ---- the Groth16 algebra of one proof on the host: the single prover and the batch call these, so their proofs agree byte for byte
// k delta in G1 / G2: over the key's fixed-base tables (delta_tables; round 4: at most 32 additions per multiple instead of 255 doublings
// + ~127 additions), or by double-and-add without them
struct DeltaMul {
    const vsp_pk *pk; bool fixed; XYZZ<HFp> d1; XYZZ<HFp2> d2;
    DeltaMul(vsp_ctx *ctx, const vsp_pk *pk_) : pk(pk_), fixed(delta_tables(ctx, pk_)), d1(xyzz_from_affine(pk_->delta_g1)), d2(xyzz_from_affine(pk_->delta_g2)) {}
    XYZZ<HFp> g1(const uint64_t k[4]) const { return fixed ? xyzz_mul_fixed(pk->tab1, k) : xyzz_mul_scalar(d1, k, 255); }
    XYZZ<HFp2> g2(const uint64_t k[4]) const { return fixed ? xyzz_mul_fixed(pk->tab2, k) : xyzz_mul_scalar(d2, k, 255); }
};
static void rs_product(const uint64_t r[4], const uint64_t s[4], uint64_t rs[4]) { host_store_canon(rs, mul(host_load_canon<HFr>(r), host_load_canon<HFr>(s))); }
// A = alpha + sum z_i A_i + r delta, B = beta + sum z_i B_i + s delta (G1 and G2) from the multi-exponentiations' results eA, eB1, eB2
static XYZZ<HFp> proof_a(const vsp_pk *pk, XYZZ<HFp> eA, const XYZZ<HFp> &r_delta) { xyzz_madd(eA, pk->alpha_g1); xyzz_add(eA, r_delta); return eA; }
static XYZZ<HFp> proof_b1(const vsp_pk *pk, XYZZ<HFp> eB1, const XYZZ<HFp> &s_delta) { xyzz_madd(eB1, pk->beta_g1); xyzz_add(eB1, s_delta); return eB1; }
static XYZZ<HFp2> proof_b2(const vsp_pk *pk, XYZZ<HFp2> eB2, const XYZZ<HFp2> &s_delta2) { xyzz_madd(eB2, pk->beta_g2); xyzz_add(eB2, s_delta2); return eB2; }
// C = sum h_i H_i + sum_{aux} z_i L_i + s A + r B1 - r s delta (+ r_enc P1; `saver` is infinity outside SAVER mode)
static XYZZ<HFp> proof_c(XYZZ<HFp> eH, const XYZZ<HFp> &eL, const XYZZ<HFp> &s_gA, const XYZZ<HFp> &r_gB1, const XYZZ<HFp> &neg_rs_delta, const XYZZ<HFp> &saver) {
    xyzz_add(eH, eL); xyzz_add(eH, s_gA); xyzz_add(eH, r_gB1); xyzz_add(eH, neg_rs_delta); xyzz_add(eH, saver);
    return eH;
}
// proof k into the outputs (any may be null): A, B, C as canonical affine words, and the 192 compressed bytes
static void store_proof(size_t k, const XYZZ<HFp> &gA, const XYZZ<HFp2> &gB2, const XYZZ<HFp> &gC, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out) {
    uint64_t A12[12], B24[24], C12[12];
    host_store_affine(A12, xyzz_to_affine(gA)); host_store_affine(B24, xyzz_to_affine(gB2)); host_store_affine(C12, xyzz_to_affine(gC));
    if (A_out) memcpy(A_out + 12 * k, A12, sizeof A12);
    if (B_out) memcpy(B_out + 24 * k, B24, sizeof B24);
    if (C_out) memcpy(C_out + 12 * k, C12, sizeof C12);
    if (proofs_out) { uint8_t *p = proofs_out + 192 * k; vsp_g1_compress(A12, p); vsp_g2_compress(B24, p + 48); vsp_g1_compress(C12, p + 144); }
}

// ---- the proof or the batch in flight on a context (ctx->prove), between a launch and its finish
// the start both launches share: the checks, made before anything is queued (arguments present, nothing in flight, the K pairs (r, s) and
// r_enc canonical, the key made for the constraint system), then the record the finish reads -- active once the launch body has succeeded
static int prove_begin(vsp_ctx *ctx, bool batch, bool args_present, const vsp_r1cs *cs, const vsp_pk *pk, size_t K, const uint64_t *r, const uint64_t *s,
                       const uint64_t *saver_P1, const uint64_t *saver_r_enc) {
    if (!ctx) return VSP_ERR_ARG;
    if (!args_present) return set_error(ctx, VSP_ERR_ARG, batch ? "prove_batch: null argument or a batch outside 1..64" : "prove: null argument");
    if (ctx->prove.active) return set_error(ctx, VSP_ERR_ARG, "prove: a proof is already in flight on this context (finish it first)");
    if (ctx->cast.active) return set_error(ctx, VSP_ERR_ARG, "prove: a batch of cast ballots is in flight on this context (finish it first)");
    for (size_t k = 0; k < K; k++)
        if (!below_mod<FrP64>(r + 4 * k) || !below_mod<FrP64>(s + 4 * k) || (saver_r_enc && !below_mod<FrP64>(saver_r_enc)))
            return set_error(ctx, VSP_ERR_ARG, batch ? "prove: r and s must be canonical (< r)" : "prove: r, s and r_enc must be canonical (< r)");
    const size_t nv = cs->num_vars;
    if (pk->A->n != nv + 1 || pk->B1->n != nv + 1 || pk->B2->n != nv + 1 || pk->H->n + 1 != cs->dom.m || pk->L->n != nv - cs->num_inputs)
        return set_error(ctx, VSP_ERR_ARG, "prove: proving key does not match the constraint system");
    auto &p = ctx->prove;
    p.batch = batch; p.pk = pk; p.count = K; p.z_bytes = K * (nv + 1) * sizeof(Fr);
    p.r.assign(r, r + 4 * K); p.s.assign(s, s + 4 * K);
    p.has_saver = saver_P1 && saver_r_enc;
    p.addend.clear();                      // a batch of ballots sets its members' terms before its finish (saver_batch.hip)
    ctx->saver_ct.active = false;          // and marks itself after this launch: a ballot batch finished as a plain one does not outlive it
    if (p.has_saver) { memcpy(p.P1, saver_P1, 96); memcpy(p.r_enc, saver_r_enc, 32); }
    return VSP_OK;
}
// the end of a failed launch and of every finish
static void prove_cleanup(vsp_ctx *ctx, int rc) {
    if (rc != VSP_OK) {
        // an early return leaves multi-exponentiations in flight on their own streams, still reading the witness and H vectors:
        // wait for all of them before the caller (or the next call's workspace growth) can touch those buffers
        std::string keep = ctx->err;
        msm_drain_slots(ctx);
        ctx->err = keep;
    }
    for (unsigned k = 1; k <= 4; k++) (void)msm_slot_use_stream(ctx, k, nullptr);      // the slots go back to their own streams
    // the call's copy of its witnesses, z = (1, witness) for each of the K, is zeroed; what was derived from them -- A z, B z, C z
    // (pr_abc), the H coefficients (pr_h), the packed witness (pr_pack) -- stays resident until the next call overwrites it
    const size_t zb = ctx->prove.z_bytes < ctx->pr_z.cap ? ctx->prove.z_bytes : ctx->pr_z.cap;
    if (ctx->pr_z.p && zb) hipMemsetAsync(ctx->pr_z.p, 0, zb, ctx->stream);
    ctx->prove.active = false;
}
// the four witness multi-exponentiations as two chains on the prover's two low-priority streams: slots 1, 2 on one, 3, 4 on the other
static int prove_use_streams(vsp_ctx *ctx) {
    for (int k = 0; k < 2; k++) if (!ctx->prove_streams[k]) VSP_TRY(msm_make_slot_stream(ctx, &ctx->prove_streams[k]));
    VSP_TRY(msm_slot_use_stream(ctx, 1, ctx->prove_streams[0])); VSP_TRY(msm_slot_use_stream(ctx, 2, ctx->prove_streams[0]));
    VSP_TRY(msm_slot_use_stream(ctx, 3, ctx->prove_streams[1])); VSP_TRY(msm_slot_use_stream(ctx, 4, ctx->prove_streams[1]));
    return VSP_OK;
}
}  // namespace vsp
extern "C" {

static int prove_launch_impl(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &w);
static int prove_finish_impl(vsp_ctx *ctx, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192], const std::function<void()> *overlap);

}  // extern "C"
namespace vsp {
static int prove_launch_checked(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &w, const uint64_t r[4], const uint64_t s[4],
                                const uint64_t *saver_P1, const uint64_t *saver_r_enc) {
    const bool args = cs && pk && r && s && (w.plain || (w.class_words && w.word_offsets && (w.dense || !w.n_dense)));
    VSP_TRY(prove_begin(ctx, false, args, cs, pk, 1, r, s, saver_P1, saver_r_enc));
    int rc = prove_launch_impl(ctx, cs, pk, w);
    if (rc != VSP_OK) prove_cleanup(ctx, rc); else ctx->prove.active = true;
    return rc;
}
// the prover with a hook: `overlap` runs on the host after every kernel is queued and before the first wait -- the window in which
// the host has nothing to do but wait for the GPU (vsp_saver_encrypt computes its ciphertext there)
int prove_with_overlap(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness, const uint64_t r[4], const uint64_t s[4],
                       const uint64_t *saver_P1, const uint64_t *saver_r_enc, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12],
                       uint8_t proof_out[192], const std::function<void()> *overlap) {
    WitnessSrc w{witness, nullptr, nullptr, nullptr, 0};
    int rc = prove_launch_checked(ctx, cs, pk, w, r, s, saver_P1, saver_r_enc);
    if (rc != VSP_OK) return rc;
    rc = prove_finish_impl(ctx, A_out, B_out, C_out, proof_out, overlap);
    prove_cleanup(ctx, rc);
    return rc;
}
}  // namespace vsp
extern "C" {

int vsp_groth16_prove(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness,
                      const uint64_t r[4], const uint64_t s[4], const uint64_t *saver_P1, const uint64_t *saver_r_enc,
                      uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192]) {
    return prove_with_overlap(ctx, cs, pk, witness, r, s, saver_P1, saver_r_enc, A_out, B_out, C_out, proof_out, nullptr);
}
// The same call in two halves, so that ONE host thread keeps several proofs in flight (one per context, all over one resident key): launch
// queues every kernel of the proof and returns; finish does the host-side scalar multiplications, waits and assembles.
int vsp_groth16_prove_launch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness, const uint64_t r[4], const uint64_t s[4],
                             const uint64_t *saver_P1, const uint64_t *saver_r_enc) {
    WitnessSrc w{witness, nullptr, nullptr, nullptr, 0};
    return prove_launch_checked(ctx, cs, pk, w, r, s, saver_P1, saver_r_enc);
}
int vsp_groth16_prove_launch_packed(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *class_words, const uint32_t *word_offsets,
                                    const uint64_t *dense, size_t n_dense, const uint64_t r[4], const uint64_t s[4],
                                    const uint64_t *saver_P1, const uint64_t *saver_r_enc) {
    if (!ctx) return VSP_ERR_ARG;
    if (!cs || !class_words || !word_offsets || (!dense && n_dense)) return set_error(ctx, VSP_ERR_ARG, "prove: null argument");
    // the class map indexes the dense values on the device: refuse a map whose offsets or count do not add up (a read outside the buffer)
    {
        const size_t nv = cs->num_vars, words = (nv + 31) / 32;
        size_t run = 0;
        for (size_t wd = 0; wd < words; wd++) {
            uint64_t cw = class_words[wd];
            if (wd == words - 1 && (nv & 31) && (cw >> (2 * (nv & 31)))) return set_error(ctx, VSP_ERR_ARG, "prove: packed witness has class bits beyond num_vars");
            if ((cw >> 1) & cw & 0x5555555555555555ull) return set_error(ctx, VSP_ERR_ARG, "prove: packed witness uses the reserved class 3");
            if (word_offsets[wd] != run) return set_error(ctx, VSP_ERR_ARG, "prove: packed witness offsets do not match its class map");
            run += (size_t)__builtin_popcountll((cw >> 1) & 0x5555555555555555ull);
        }
        if (run != n_dense) return set_error(ctx, VSP_ERR_ARG, "prove: packed witness dense count does not match its class map");
    }
    WitnessSrc w{nullptr, class_words, word_offsets, dense, n_dense};
    return prove_launch_checked(ctx, cs, pk, w, r, s, saver_P1, saver_r_enc);
}
int vsp_groth16_prove_finish(vsp_ctx *ctx, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ctx->prove.active || ctx->prove.batch) return set_error(ctx, VSP_ERR_ARG, "prove_finish: no proof in flight on this context");
    int rc = prove_finish_impl(ctx, A_out, B_out, C_out, proof_out, nullptr);
    prove_cleanup(ctx, rc);
    return rc;
}
// Packed witness.  A Groth16 witness is mostly wires equal to 0 or 1, and its 32 bytes per wire cross PCIe in front of every proof with
// the GPU idle (0.8 ms at 2^20 constraints).  Packed form: two bits per wire (0 = zero, 1 = one, 2 = a dense value), 32 wires per 64-bit
// word; per word the index of its first dense value; the dense values (4 words each) in wire order.  A witness generator can emit this
// directly; vsp_witness_pack converts a plain witness (one pass over it on the host).  Sizes: words = (n + 31) / 32.
size_t vsp_witness_pack_words(size_t n) { return (n + 31) / 32; }
int vsp_witness_pack(const uint64_t *witness, size_t n, uint64_t *class_words, uint32_t *word_offsets, uint64_t *dense_out, size_t dense_capacity, size_t *n_dense_out) {
    if ((!witness && n) || !class_words || !word_offsets || !n_dense_out) return VSP_ERR_ARG;
    size_t nd = 0;
    const size_t words = (n + 31) / 32;
    for (size_t wd = 0; wd < words; wd++) {
        uint64_t cw = 0;
        word_offsets[wd] = (uint32_t)nd;
        const size_t lim = n - 32 * wd < 32 ? n - 32 * wd : 32;
        for (size_t j = 0; j < lim; j++) {
            const uint64_t *v = witness + 4 * (32 * wd + j);
            const bool small = (v[1] | v[2] | v[3]) == 0 && v[0] <= 1;
            if (small) cw |= (uint64_t)v[0] << (2 * j);
            else {
                cw |= (uint64_t)2 << (2 * j);
                if (dense_out) { if (nd >= dense_capacity) return VSP_ERR_ARG; memcpy(dense_out + 4 * nd, v, 32); }
                nd++;
            }
        }
        class_words[wd] = cw;
    }
    *n_dense_out = nd;
    return nd > 0xFFFFFFFFull ? VSP_ERR_UNSUPPORTED : VSP_OK;
}

// z[1 + i] of the packed witness: 0, 1 or the next dense value (canonical words either way)
__global__ __launch_bounds__(256) void k_witness_expand(const uint64_t *class_words, const uint32_t *word_offsets, const uint4 *dense, size_t n, uint4 *z) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t cw = class_words[i >> 5];
    const unsigned j = (unsigned)(i & 31), cls = (unsigned)(cw >> (2 * j)) & 3u;
    uint4 lo = make_uint4(cls == 1 ? 1u : 0u, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
    if (cls >= 2) {
        // dense values before this wire inside the word: the even bits of the class pairs above... class 2 = binary 10: count the high bits below j
        const uint64_t highs = (cw >> 1) & 0x5555555555555555ull & ((j ? ((uint64_t)1 << (2 * j)) : 1ull) - 1ull);
        const size_t k = (size_t)word_offsets[i >> 5] + (size_t)__popcll(highs);
        lo = dense[2 * k]; hi = dense[2 * k + 1];
    }
    z[2 * i] = lo; z[2 * i + 1] = hi;
}

// z_k = (1, row map.row[k] of the source) for the K members of a batch whose witnesses lie in device memory (WitnessSrc::dev): grid.y the
// member, a lane per 16 bytes of z_k -- two of them a value, so consecutive lanes load and store consecutive 16 bytes of one row.  The
// map travels by value: 64 row indices are 256 bytes of kernel argument.  No loop; every store is a plain one.
struct GatherMap { uint32_t row[vsp_ctx::VERDICT_MEMBERS]; };
__global__ __launch_bounds__(256) void k_witness_gather(const uint4 *src, size_t stride, GatherMap map, size_t nv, uint4 *z) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
    if (i >= 2 * (nv + 1)) return;
    uint4 v = make_uint4(i == 0 ? 1u : 0u, 0, 0, 0);
    if (i >= 2) v = src[2 * (size_t)map.row[k] * stride + (i - 2)];
    z[2 * k * (nv + 1) + i] = v;
}

// ---- the front half of every proof, and the whole device side of the stand-alone witness check (vsp_r1cs_check_batch): z_k = (1, witness_k)
// canonical into pr_z for the K members, then A z, B z, C z of each into pr_abc (member k at pr_abc + k 3 m: A z | B z | C z, m values each,
// zero beyond the constraint rows) and the rows "input_i * 0 = 0" of A.  There is one copy of it, so what the check approves is, word for
// word, what witness_map_device consumes.  strided: the batch form -- K plain witnesses one after the other, copied from pageable memory
// and waited for; else K = 1, plain or packed, nothing waited for.
static int prove_front_half(vsp_ctx *ctx, const vsp_r1cs *cs, const WitnessSrc &wsrc, size_t K, bool strided) {
    const size_t nv = cs->num_vars, ni = cs->num_inputs, nc = cs->num_constraints, m = cs->dom.m, zs = nv + 1;
    hipStream_t st = ctx->stream;
    VSP_TRY(ensure(ctx, ctx->pr_z, K * zs * sizeof(Fr)));
    VSP_TRY(ensure(ctx, ctx->pr_abc, K * 3 * m * sizeof(Fr)));
    Fr *dz = (Fr *)ctx->pr_z.p, *abc = (Fr *)ctx->pr_abc.p;
    std::vector<uint64_t> ones;
    const uint64_t one4[4] = {1, 0, 0, 0};
    if (wsrc.dev) {
        GatherMap map{};
        for (size_t k = 0; k < K; k++) map.row[k] = wsrc.members ? wsrc.members[k] : (uint32_t)(wsrc.first + k);
        hipLaunchKernelGGL(k_witness_gather, dim3((unsigned)((2 * zs + 255) / 256), (unsigned)K), dim3(256), 0, st, (const uint4 *)wsrc.dev, wsrc.stride, map, nv, (uint4 *)dz);
        VSP_LAUNCH_CHECK();
        VSP_HIP(hipEventRecord(ctx->ev_aux, st));
    } else if (strided) {
        // the K ones from a small host array, the witnesses by one strided copy
        ctx->stats["prove_witness_h2d_bytes"] += (double)(K * nv * 32);
        ones.assign(K * 4, 0); for (size_t k = 0; k < K; k++) ones[4 * k] = 1;
        VSP_HIP(hipMemcpy2DAsync(dz, zs * 32, ones.data(), 32, 32, K, hipMemcpyHostToDevice, st));
        if (nv) VSP_HIP(hipMemcpy2DAsync(dz + 1, zs * 32, wsrc.plain, nv * 32, nv * 32, K, hipMemcpyHostToDevice, st));
    } else {
        VSP_HIP(hipMemcpyAsync(dz, one4, 32, hipMemcpyHostToDevice, st));
        ctx->stats["prove_witness_h2d_bytes"] += (double)(wsrc.plain ? nv * 32 : ((nv + 31) / 32) * 12 + wsrc.n_dense * 32);
        if (wsrc.plain) VSP_HIP(hipMemcpyAsync(dz + 1, wsrc.plain, nv * 32, hipMemcpyHostToDevice, st));
        else {
            // packed witness: class map, per-word offsets and the dense values cross PCIe (a tenth of the plain witness for a 90 % boolean one); a kernel expands
            const size_t words = (nv + 31) / 32;
            VSP_TRY(ensure(ctx, ctx->pr_pack, words * 12 + wsrc.n_dense * 32 + 64));
            uint64_t *d_cw = (uint64_t *)ctx->pr_pack.p; uint32_t *d_off = (uint32_t *)(d_cw + words);
            uint4 *d_dense = (uint4 *)(((uintptr_t)(d_off + words) + 15) & ~(uintptr_t)15);
            VSP_HIP(hipMemcpyAsync(d_cw, wsrc.class_words, words * 8, hipMemcpyHostToDevice, st));
            VSP_HIP(hipMemcpyAsync(d_off, wsrc.word_offsets, words * 4, hipMemcpyHostToDevice, st));
            if (wsrc.n_dense) VSP_HIP(hipMemcpyAsync(d_dense, wsrc.dense, wsrc.n_dense * 32, hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_witness_expand, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, st, (const uint64_t *)d_cw, (const uint32_t *)d_off, (const uint4 *)d_dense, nv, (uint4 *)(dz + 1));
            VSP_LAUNCH_CHECK();
        }
    }
    // evaluation vectors (witness_map part 1): A z, B z, C z, plus the rows "input_i * 0 = 0" in A
    VSP_HIP(hipMemsetAsync(abc, 0, K * 3 * m * sizeof(Fr), st));
    if (nc) for (int j = 0; j < 3; j++) {
        hipLaunchKernelGGL(k_csr_matvec, dim3((unsigned)((nc + 255) / 256), (unsigned)K), dim3(256), 0, st, cs->rp[j].as<const uint32_t>(), cs->ci[j].as<const uint32_t>(),
                           cs->co[j].as<const Fr>(), (const Fr *)dz, nc, abc + (size_t)j * m, zs, 3 * m);
        VSP_LAUNCH_CHECK();
    }
    if (strided) {
        VSP_HIP(hipMemcpy2DAsync(abc + nc, 3 * m * sizeof(Fr), dz, zs * sizeof(Fr), (ni + 1) * sizeof(Fr), K, hipMemcpyDeviceToDevice, st));
        if (!wsrc.dev) VSP_HIP(hipStreamSynchronize(st));                   // `ones` goes out of scope; the copies above are queued from pageable memory anyway
    } else VSP_HIP(hipMemcpyAsync(abc + nc, dz, (ni + 1) * sizeof(Fr), hipMemcpyDeviceToDevice, st));
    return VSP_OK;
}
// ---- the verdict pass over the K members the front half left in pr_z / pr_abc, queued behind it on the context's stream and before
// witness_map_device overwrites pr_abc: the records are preset (first_bad_row = num_constraints, the rest 0), k_r1cs_verdict fills
// first_bad_row and bad_rows, with_canonical also raises the flag of a value >= r (inside the prover the multi-exponentiations' census
// makes that check, as before); an asynchronous copy takes the records to the context's pinned buffer.  t0 / t1 (or null): events
// around the kernels.  ctx->h_verdict is valid once everything queued here has run.
static int verdict_queue(vsp_ctx *ctx, const vsp_r1cs *cs, size_t K, bool with_canonical, hipEvent_t t0, hipEvent_t t1) {
    constexpr size_t M = vsp_ctx::VERDICT_MEMBERS;
    const size_t nc = cs->num_constraints, m = cs->dom.m, zs = cs->num_vars + 1;
    hipStream_t st = ctx->stream;
    if (K > M) return set_error(ctx, VSP_ERR_ARG, "r1cs_check: more members than the verdict records hold");
    VSP_TRY(ensure(ctx, ctx->pr_verdict, vsp_ctx::VERDICT_BYTES));
    if (!ctx->h_verdict.p) VSP_HIP(ctx->h_verdict.alloc(vsp_ctx::VERDICT_BYTES));
    uint32_t *first_bad = (uint32_t *)ctx->pr_verdict.p, *bad_rows = first_bad + M, *flag = first_bad + 2 * M;
    if (t0) VSP_HIP(hipEventRecord(t0, st));
    VSP_HIP(hipMemsetD32Async((hipDeviceptr_t)first_bad, (int)(uint32_t)nc, M, st));
    VSP_HIP(hipMemsetAsync(bad_rows, 0, 2 * M * sizeof(uint32_t), st));
    if (nc) {
        hipLaunchKernelGGL(k_r1cs_verdict, dim3((unsigned)((nc + 255) / 256), (unsigned)K), dim3(256), 0, st, (const Fr *)ctx->pr_abc.p, nc, m, 3 * m, first_bad, bad_rows);
        VSP_LAUNCH_CHECK();
    }
    if (with_canonical) {
        hipLaunchKernelGGL(k_witness_canonical, dim3((unsigned)((zs + 255) / 256), (unsigned)K), dim3(256), 0, st, (const Fr *)ctx->pr_z.p, zs, zs, flag);
        VSP_LAUNCH_CHECK();
    }
    if (t1) VSP_HIP(hipEventRecord(t1, st));
    VSP_HIP(hipMemcpyAsync(ctx->h_verdict.p, first_bad, vsp_ctx::VERDICT_BYTES, hipMemcpyDeviceToHost, st));
    return VSP_OK;
}
// option "prove_check_witness" (default 0): every prover entry point queues the verdict pass between its front half and witness_map_device;
// the finish reads the records after its own waits -- the copy sits on the context's stream in front of the H chain the finish waits for
static int prove_queue_check(vsp_ctx *ctx, const vsp_r1cs *cs, size_t K) {
    ctx->prove.check = opt(ctx, "prove_check_witness", 0) != 0;
    return ctx->prove.check ? verdict_queue(ctx, cs, K, false, nullptr, nullptr) : VSP_OK;
}
// member k's record in the pinned buffer
struct Verdict { uint32_t first_bad_row, bad_rows, not_canonical; };
static Verdict verdict_of(const vsp_ctx *ctx, size_t k) {
    const volatile uint32_t *h = ctx->h_verdict.as<const volatile uint32_t>();
    return Verdict{h[k], h[vsp_ctx::VERDICT_MEMBERS + k], h[2 * vsp_ctx::VERDICT_MEMBERS + k]};
}

static int prove_launch_impl(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &wsrc) {
    const size_t nv = cs->num_vars, ni = cs->num_inputs;
    const size_t m = cs->dom.m;
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HostLap lap{ctx};
    // z = (1, witness) canonical on device; the workspace of a batch of one: A z, B z, C z one after the other in pr_abc
    VSP_TRY(prove_front_half(ctx, cs, wsrc, 1, false));
    VSP_TRY(ensure(ctx, ctx->pr_h, m * sizeof(Fr)));
    Fr *dz = (Fr *)ctx->pr_z.p, *dA = (Fr *)ctx->pr_abc.p, *dB = dA + m, *dC = dA + 2 * m, *dH = (Fr *)ctx->pr_h.p;
    VSP_TRY(prove_queue_check(ctx, cs, 1));
    // Order of queueing: (1) the two scalar censuses, tiny, on the context's stream; (2) witness_map (7 NTTs) and the H
    // multi-exponentiation, the longest dependent chain, on the context's stream; (3) the four multi-exponentiations over the
    // witness -- independent of witness_map -- on the low-priority slots 1-4, filling the GPU around (2).  A_query, B_query(G1)
    // and B_query(G2) share one digit sort / bucket plan (same scalars) when their bases are precomputed alike.
    // The four witness multi-exponentiations run as TWO chains, on two streams the prover owns (lowest priority, like the work slots' own
    // streams, which stay free for callers that pipeline independent multi-exponentiations): A_query then B_query(G1) on one, B_query(G2)
    // -- which waits for A_query's digit sort, the plan the three share -- then L_query on the other.  Measured at 2^20 constraints on one
    // box: 6.5 ms per proof against 7.2-7.6 ms with one stream per multi-exponentiation, the same 170 / 190 proofs/s with two / three
    // contexts; the other pairings lose (A,B2 | B1,L: 7.8 ms; all four on one stream: 7.3 ms).  Fewer concurrent witness chains leave the
    // transforms and the H accumulation -- the critical chain -- alone for longer.  Option "prove_witness_streams" = 0: the
    // slots' own streams.
    if (opt(ctx, "prove_witness_streams", 1)) VSP_TRY(prove_use_streams(ctx));
    VSP_TRY(msm_slot_census(ctx, 1, dz, nv + 1));
    VSP_TRY(msm_slot_census(ctx, 4, dz + ni + 1, nv - ni));
    VSP_HIP(hipEventRecord(ctx->ev_aux, st));          // z resident and censuses queued
    // option "prove_h_first" (default 1): queue witness_map + H before the witness multi-exponentiations, or after (0)
    const long h_first = opt(ctx, "prove_h_first", 1);
    {
        hipStream_t s1, s2, s3, s4;
        VSP_TRY(msm_slot_stream(ctx, 1, &s1)); VSP_TRY(msm_slot_stream(ctx, 2, &s2));
        VSP_TRY(msm_slot_stream(ctx, 3, &s3)); VSP_TRY(msm_slot_stream(ctx, 4, &s4));
        VSP_HIP(hipStreamWaitEvent(s1, ctx->ev_aux, 0)); VSP_HIP(hipStreamWaitEvent(s2, ctx->ev_aux, 0));
        VSP_HIP(hipStreamWaitEvent(s3, ctx->ev_aux, 0)); VSP_HIP(hipStreamWaitEvent(s4, ctx->ev_aux, 0));
    }
    // option "prove_plan_first" (default 0): queue the digit sorts and bucket plans of the two witness vectors BEFORE witness_map.
    // Their counting sort needs 128 KiB of LDS per workgroup; queued after the transforms it finds every CU's LDS taken by NTT tiles and
    // then every wave slot taken by the H accumulation, and waits ~2 ms (kernel timeline).  Queued first it runs while the
    // GPU is idle -- measured: no gain (9.10 against 9.02 ms): the proof is bound by the sum of its kernels, not by that wait.
    const long plan_first = opt(ctx, "prove_plan_first", 0);
    MsmRequest a(dz, nv + 1), l(dz + ni + 1, nv - ni), h(dH, m - 1);      // A_query (B_query G1 / G2 alike), L_query, H_query
    h.dense = true;                                           // H coefficients are dense
    if (h_first && plan_first) {
        MsmRequest plan_a = a, plan_l = l; plan_a.plan_only = plan_l.plan_only = true;
        VSP_TRY(launch_on_bases(ctx, 1, pk->A, 0, plan_a)); a.plan_from = 1;
        VSP_TRY(launch_on_bases(ctx, 4, pk->L, 0, plan_l)); l.plan_from = 4;
    }
    if (h_first) {
        VSP_TRY(witness_map_device(ctx, &cs->dom, dA, dB, dC, 3 * m, 1, dH, m));
        VSP_TRY(launch_on_bases(ctx, 0, pk->H, 0, h));
    }
    VSP_TRY(launch_on_bases(ctx, 1, pk->A, 0, a));
    MsmRequest b = a;
    b.plan_from = pk->B2->pre_c == pk->A->pre_c ? 1 : -1; VSP_TRY(launch_on_bases(ctx, 3, pk->B2, 0, b));
    b.plan_from = pk->B1->pre_c == pk->A->pre_c ? 1 : -1; VSP_TRY(launch_on_bases(ctx, 2, pk->B1, 0, b));
    VSP_TRY(launch_on_bases(ctx, 4, pk->L, 0, l));
    if (!h_first) {
        VSP_TRY(witness_map_device(ctx, &cs->dom, dA, dB, dC, 3 * m, 1, dH, m));
        VSP_TRY(launch_on_bases(ctx, 0, pk->H, 0, h));
    }
    lap("prove_launch_ms");
    return VSP_OK;
}

static int prove_finish_impl(vsp_ctx *ctx, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192], const std::function<void()> *overlap) {
    const vsp_pk *pk = ctx->prove.pk;
    const uint64_t *r = ctx->prove.r.data(), *s = ctx->prove.s.data();
    VSP_HIP(hipSetDevice(ctx->device));
    HostLap lap{ctx};
    // host work that needs no MSM result, done while the GPU runs: the four multiples of delta on four host threads (round 4: at the real
    // circuit's size the HOST was the critical path of a proof -- 0.85 ms of scalar multiplications here and ~1 ms of Horner chains in the
    // five finishes below, one after the other, against ~1.5 ms of GPU work; tools/prove_phases.py)
    uint64_t rs4[4]; rs_product(r, s, rs4);
    XYZZ<HFp> r_delta, s_delta, neg_rs_delta, saver = XYZZ<HFp>::inf();
    XYZZ<HFp2> s_delta2;
    const unsigned T = opt(ctx, "prove_host_threads", 1) ? 8u : 1u;
    const DeltaMul delta(ctx, pk);
    host_parallel_for(5, [&](size_t j) {
        if (j == 0) s_delta2 = delta.g2(s);                   // the G2 one is the longest: first
        else if (j == 1) r_delta = delta.g1(r);
        else if (j == 2) s_delta = delta.g1(s);
        else if (j == 3) neg_rs_delta = xyzz_neg(delta.g1(rs4));
        else if (ctx->prove.has_saver) saver = xyzz_mul_scalar_w4(xyzz_from_affine(host_load_affine<HFp>(ctx->prove.P1)), ctx->prove.r_enc);
    }, T);
    if (overlap && *overlap) (*overlap)();
    lap("prove_host_overlap_ms");
    // The witness multi-exponentiations finish long before the H chain (witness_map, then the dense H query).  Each finish is a wait (this
    // thread: it touches the context) and a fold of the window results -- a Horner chain of a few hundred host group operations, 0.2 ms in G1,
    // 0.6 ms in G2 -- which runs on a thread of its own while this one waits for the next slot; s * A and r * B1, the two 255-bit scalar
    // multiplications of the assembly, follow their folds on the same threads.  Option "prove_host_threads" = 0: everything on this thread.
    XYZZ<HFp> eA = XYZZ<HFp>::inf(), eB1 = XYZZ<HFp>::inf(), eH = XYZZ<HFp>::inf(), eL = XYZZ<HFp>::inf(); XYZZ<HFp2> eB2 = XYZZ<HFp2>::inf();
    XYZZ<HFp> gA, s_gA, r_gB1;
    XYZZ<HFp2> gB2;
    std::vector<std::thread> workers;
    auto run = [&](std::function<void()> f) { if (T > 1) workers.emplace_back(std::move(f)); else f(); };
    int rc = VSP_OK; bool empty = false;
    if ((rc = msm_slot_finish_wait<G1>(ctx, 1, 1, &empty)) == VSP_OK)
        run([&, e = empty]() { if (!e) msm_slot_fold<G1>(ctx, 1, &eA); gA = proof_a(pk, eA, r_delta); s_gA = xyzz_mul_scalar_w4(gA, s); });
    if (rc == VSP_OK && (rc = msm_slot_finish_wait<G1>(ctx, 2, 1, &empty)) == VSP_OK)
        run([&, e = empty]() { if (!e) msm_slot_fold<G1>(ctx, 2, &eB1); r_gB1 = xyzz_mul_scalar_w4(proof_b1(pk, eB1, s_delta), r); });
    if (rc == VSP_OK && (rc = msm_slot_finish_wait<G1>(ctx, 4, 1, &empty)) == VSP_OK)
        run([&, e = empty]() { if (!e) msm_slot_fold<G1>(ctx, 4, &eL); });
    if (rc == VSP_OK && (rc = msm_slot_finish_wait<G2>(ctx, 3, 1, &empty)) == VSP_OK)
        run([&, e = empty]() { if (!e) msm_slot_fold<G2>(ctx, 3, &eB2); gB2 = proof_b2(pk, eB2, s_delta2); });
    if (rc == VSP_OK && (rc = msm_slot_finish_wait<G1>(ctx, 0, 1, &empty)) == VSP_OK && !empty) msm_slot_fold<G1>(ctx, 0, &eH);
    for (auto &w : workers) w.join();
    if (rc != VSP_OK) return rc;
    lap("prove_wait_ms");
    if (ctx->prove.check) {
        // the records' copy was queued on the context's stream in front of the H chain, whose end the last wait above saw
        const Verdict v = verdict_of(ctx, 0);
        ctx->stats["prove_first_bad_row"] = (double)v.first_bad_row;
        if (v.bad_rows) {
            if (A_out) memset(A_out, 0, 12 * 8);
            if (B_out) memset(B_out, 0, 24 * 8);
            if (C_out) memset(C_out, 0, 12 * 8);
            if (proof_out) memset(proof_out, 0, 192);
            char msg[160];
            snprintf(msg, sizeof msg, "prove: the witness does not satisfy the constraint system: constraint %u is the first of %u that fail", v.first_bad_row, v.bad_rows);
            return set_error(ctx, VSP_ERR_UNSATISFIED, msg);
        }
    }
    store_proof(0, gA, gB2, proof_c(eH, eL, s_gA, r_gB1, neg_rs_delta, saver), A_out, B_out, C_out, proof_out);      // a handful of group operations
    lap("prove_assembly_ms");
    ctx->stats["prove_calls"] += 1;
    return VSP_OK;
}


// ---- a BATCH of proofs over one key (round 4).  Proofs of the real circuit's size (2^15..2^16 constraints) are bound by
// the latency of their dependent chains -- a few hundred small launches, each a fraction of the GPU -- not by work: 2.1 ms per proof, 465 / s
// from one context, ~900 / s from twelve.  K witnesses proved TOGETHER run the same number of launches K times as wide: one matvec, one
// witness_map over 3 K transforms, and each of the five multi-exponentiations once over K scalar vectors (MsmGeom.K: separate bucket sets
// per witness, the same base rows).  Every proof is byte-identical to vsp_groth16_prove's for the same (witness, r, s).
// The key is plain (vsp_groth16_generate with precompute = 0, or vsp_pk_create over plain bases) or has tables of window multiples of at
// most 16 bits (pre_c <= 16: one bucket set per witness and query -- worth it where the tables are small, i.e. at the real circuit's size);
// other tables, or any table with option "msm_batch_tables" = 0, are refused with VSP_ERR_UNSUPPORTED.
static int prove_batch_launch_impl(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &w, size_t K) {
    const size_t nv = cs->num_vars, ni = cs->num_inputs, m = cs->dom.m, zs = nv + 1;
    VSP_HIP(hipSetDevice(ctx->device));
    HostLap lap{ctx};                                         // vsp_get_stat "prove_batch_*_ms": where a batch's time goes on the host
    VSP_TRY(prove_front_half(ctx, cs, w, K, true));          // z_k = (1, witness_k) and A z, B z, C z of the K members
    VSP_TRY(ensure(ctx, ctx->pr_h, K * m * sizeof(Fr)));
    Fr *dz = (Fr *)ctx->pr_z.p, *abc = (Fr *)ctx->pr_abc.p, *dH = (Fr *)ctx->pr_h.p;
    VSP_TRY(prove_queue_check(ctx, cs, K));
    VSP_TRY(prove_use_streams(ctx));                         // the H chain on the context's stream (prove_launch_impl)
    // the device form waited for nothing: the witness chains' streams start behind the gather, as prove_launch_impl's behind its copy
    if (w.dev) for (int k = 0; k < 2; k++) VSP_HIP(hipStreamWaitEvent(ctx->prove_streams[k], ctx->ev_aux, 0));
    VSP_TRY(witness_map_device(ctx, &cs->dom, abc, abc + m, abc + 2 * m, 3 * m, (unsigned)K, dH, m));
    MsmRequest h(dH, m - 1), a(dz, nv + 1), l(dz + ni + 1, nv - ni);      // as in prove_launch_impl, K vectors each
    h.dense = true; h.batch = a.batch = l.batch = (unsigned)K; h.stride = m; a.stride = l.stride = zs;      // H coefficients are dense
    VSP_TRY(launch_on_bases(ctx, 0, pk->H, 0, h));
    VSP_TRY(launch_on_bases(ctx, 1, pk->A, 0, a));
    // A, B1 and B2 multiply by the same K witness vectors: one digit sort and bucket plan (A's) serves the three (option "prove_batch_share_plan")
    const long share = opt(ctx, "prove_batch_share_plan", 1);
    const bool same_shape = pk->A->glv == pk->B1->glv && pk->A->glv == pk->B2->glv && (pk->A->d28.p != nullptr) == (pk->B1->d28.p != nullptr) && (pk->A->d28.p != nullptr) == (pk->B2->d28.p != nullptr) &&
                            pk->A->pre_c == pk->B1->pre_c && pk->A->pre_c == pk->B2->pre_c && pk->A->n == pk->B1->n && pk->A->n == pk->B2->n;
    MsmRequest b = a; b.plan_from = share && same_shape && nv + 1 > 0 ? 1 : -1;
    VSP_TRY(launch_on_bases(ctx, 3, pk->B2, 0, b));
    VSP_TRY(launch_on_bases(ctx, 2, pk->B1, 0, b));
    VSP_TRY(launch_on_bases(ctx, 4, pk->L, 0, l));
    lap("prove_batch_launch_ms");
    return VSP_OK;
}
static int prove_batch_finish_impl(vsp_ctx *ctx, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out) {
    const vsp_pk *pk = ctx->prove.pk;
    const size_t K = ctx->prove.count;
    const uint64_t *r = ctx->prove.r.data(), *s = ctx->prove.s.data();
    ctx->batch_status.clear(); ctx->batch_first_bad.clear();      // vsp_groth16_prove_batch_verdicts speaks of THIS batch, once it has finished with the check on
    HostLap lap{ctx};
    VSP_HIP(hipSetDevice(ctx->device));
    // host work that needs no result: the delta multiples of every proof
    std::vector<XYZZ<HFp>> r_delta(K), s_delta(K), neg_rs_delta(K);
    std::vector<XYZZ<HFp2>> s_delta2(K);
    const DeltaMul delta(ctx, pk);
    host_parallel_for(K, [&](size_t k) {
        const uint64_t *rk = r + 4 * k, *sk = s + 4 * k;
        uint64_t rs4[4]; rs_product(rk, sk, rs4);
        r_delta[k] = delta.g1(rk); s_delta[k] = delta.g1(sk);
        neg_rs_delta[k] = xyzz_neg(delta.g1(rs4));
        s_delta2[k] = delta.g2(sk);
    });
    lap("prove_batch_delta_ms");
    std::vector<XYZZ<HFp>> eA(K), eB1(K), eH(K), eL(K);
    std::vector<XYZZ<HFp2>> eB2(K);
    VSP_TRY(msm_slot_finish<G1>(ctx, 1, eA.data(), (unsigned)K));
    VSP_TRY(msm_slot_finish<G1>(ctx, 2, eB1.data(), (unsigned)K));
    VSP_TRY(msm_slot_finish<G1>(ctx, 4, eL.data(), (unsigned)K));
    VSP_TRY(msm_slot_finish<G2>(ctx, 3, eB2.data(), (unsigned)K));
    lap("prove_batch_witness_finishes_ms");
    // s * A and r * B1 of every proof inside the wait for the H chain, as prove_finish_impl does them
    std::vector<XYZZ<HFp>> gA(K), s_gA(K), r_gB1(K);
    host_parallel_for(K, [&](size_t k) {
        gA[k] = proof_a(pk, eA[k], r_delta[k]);
        s_gA[k] = xyzz_mul_scalar_w4(gA[k], s + 4 * k);
        r_gB1[k] = xyzz_mul_scalar_w4(proof_b1(pk, eB1[k], s_delta[k]), r + 4 * k);
    });
    lap("prove_batch_sA_rB1_ms");
    VSP_TRY(msm_slot_finish<G1>(ctx, 0, eH.data(), (unsigned)K));
    lap("prove_batch_h_finish_ms");
    // the members' verdicts (option "prove_check_witness"; the records' copy sits in front of the H chain the finish above waited for):
    // an unsatisfied member gets all-zero outputs -- its GPU work above was not skipped -- and every other member its proof as without the check
    size_t unsatisfied = 0, first_member = 0;
    if (ctx->prove.check) {
        ctx->batch_status.assign(K, 0); ctx->batch_first_bad.assign(K, 0);
        for (size_t k = K; k-- > 0;) {
            const Verdict v = verdict_of(ctx, k);
            ctx->batch_first_bad[k] = v.first_bad_row;
            if (v.bad_rows) { ctx->batch_status[k] = 2; unsatisfied++; first_member = k; }
        }
    }
    host_parallel_for(K, [&](size_t k) {
        if (ctx->prove.check && ctx->batch_status[k]) {
            if (A_out) memset(A_out + 12 * k, 0, 12 * 8);
            if (B_out) memset(B_out + 24 * k, 0, 24 * 8);
            if (C_out) memset(C_out + 12 * k, 0, 12 * 8);
            if (proofs_out) memset(proofs_out + 192 * k, 0, 192);
            return;
        }
        const XYZZ<HFp> saver = ctx->prove.addend.empty() ? XYZZ<HFp>::inf() : xyzz_from_affine(host_load_affine<HFp>(ctx->prove.addend.data() + 12 * k));
        store_proof(k, gA[k], proof_b2(pk, eB2[k], s_delta2[k]), proof_c(eH[k], eL[k], s_gA[k], r_gB1[k], neg_rs_delta[k], saver), A_out, B_out, C_out, proofs_out);
    });
    lap("prove_batch_assembly_ms");
    ctx->stats["prove_calls"] += (double)K;
    ctx->stats["prove_batches"] += 1;
    if (unsatisfied) {
        char msg[200];
        snprintf(msg, sizeof msg, "prove_batch: %zu of %zu witnesses do not satisfy the constraint system (the first is member %zu, at constraint %llu); their outputs are zero",
                 unsatisfied, K, first_member, (unsigned long long)ctx->batch_first_bad[first_member]);
        return set_error(ctx, VSP_ERR_UNSATISFIED, msg);
    }
    return VSP_OK;
}
}  // extern "C"
namespace vsp {
// the batch launch over a witness source the caller has checked: K host witnesses one after the other, or rows of a device buffer
int prove_batch_launch_src(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const WitnessSrc &w, size_t count, const uint64_t *r, const uint64_t *s) {
    VSP_TRY(prove_begin(ctx, true, cs && pk && (w.plain || w.dev) && r && s && count >= 1 && count <= 64, cs, pk, count, r, s, nullptr, nullptr));
    int rc = prove_batch_launch_impl(ctx, cs, pk, w, count);
    if (rc != VSP_OK) prove_cleanup(ctx, rc); else ctx->prove.active = true;
    return rc;
}
// the checks of a device source (include/vsp.h "witnesses in device memory"), made before anything is queued; `out` is the source
int witness_src_device(vsp_ctx *ctx, const char *who, const vsp_r1cs *cs, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members, size_t count,
                       WitnessSrc *out) {
    char m[200];
    auto refuse = [&](const char *what) { snprintf(m, sizeof m, "%s: %s", who, what); return set_error(ctx, VSP_ERR_ARG, m); };
    if (!cs || !d_witnesses) return refuse("null argument");
    if (stride < cs->num_vars) return refuse("the stride of the device witnesses is below num_vars");
    if ((uintptr_t)d_witnesses & 15) return refuse("the device witnesses are not 16-byte aligned");
    if (rows > 0xFFFFFFFFull) return refuse("more than 2^32 - 1 rows of device witnesses");
    if (!members && count > rows) return refuse("members is NULL and count exceeds the rows of the device witnesses");
    for (size_t k = 0; members && k < count; k++)
        if (members[k] >= rows) {
            snprintf(m, sizeof m, "%s: members[%zu] = %u is not a row of the device witnesses (%zu rows)", who, k, members[k], rows);
            return set_error(ctx, VSP_ERR_ARG, m);
        }
    *out = WitnessSrc{};
    out->dev = (const uint64_t *)d_witnesses; out->stride = stride; out->members = members;
    return VSP_OK;
}
}  // namespace vsp
extern "C" {
int vsp_groth16_prove_batch_launch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witnesses, size_t count, const uint64_t *r, const uint64_t *s) {
    const WitnessSrc w{witnesses, nullptr, nullptr, nullptr, 0};
    return prove_batch_launch_src(ctx, cs, pk, w, count, r, s);
}
int vsp_groth16_prove_batch_launch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members,
                                          size_t count, const uint64_t *r, const uint64_t *s) {
    if (!ctx) return VSP_ERR_ARG;
    if (!cs || !pk || !d_witnesses || !r || !s || count < 1 || count > 64) return set_error(ctx, VSP_ERR_ARG, "prove_batch_device: null argument or a batch outside 1..64");
    WitnessSrc w;
    VSP_TRY(witness_src_device(ctx, "prove_batch_device", cs, d_witnesses, stride, rows, members, count, &w));
    return prove_batch_launch_src(ctx, cs, pk, w, count, r, s);
}
int vsp_groth16_prove_batch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members,
                                   size_t count, const uint64_t *r, const uint64_t *s, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out) {
    int rc = vsp_groth16_prove_batch_launch_device(ctx, cs, pk, d_witnesses, stride, rows, members, count, r, s);
    if (rc != VSP_OK) return rc;
    return vsp_groth16_prove_batch_finish(ctx, A_out, B_out, C_out, proofs_out);
}
int vsp_groth16_prove_batch_finish(vsp_ctx *ctx, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ctx->prove.active || !ctx->prove.batch) return set_error(ctx, VSP_ERR_ARG, "prove_batch_finish: no batch in flight on this context");
    int rc = prove_batch_finish_impl(ctx, A_out, B_out, C_out, proofs_out);
    prove_cleanup(ctx, rc);
    return rc;
}
int vsp_groth16_prove_batch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witnesses, size_t count, const uint64_t *r, const uint64_t *s,
                            uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out) {
    int rc = vsp_groth16_prove_batch_launch(ctx, cs, pk, witnesses, count, r, s);
    if (rc != VSP_OK) return rc;
    return vsp_groth16_prove_batch_finish(ctx, A_out, B_out, C_out, proofs_out);
}
int vsp_groth16_prove_batch_verdicts(vsp_ctx *ctx, uint8_t *status_out, uint64_t *first_bad_row_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!status_out) return set_error(ctx, VSP_ERR_ARG, "prove_batch_verdicts: null argument");
    if (ctx->batch_status.empty()) return set_error(ctx, VSP_ERR_ARG, "prove_batch_verdicts: no batch has finished on this context with option prove_check_witness = 1");
    memcpy(status_out, ctx->batch_status.data(), ctx->batch_status.size());
    if (first_bad_row_out) memcpy(first_bad_row_out, ctx->batch_first_bad.data(), ctx->batch_first_bad.size() * sizeof(uint64_t));
    return VSP_OK;
}

// ---- the stand-alone witness check: bp.is_satisfied() (common.hpp:1109-1128).  The prover's front half and the verdict pass, in pieces
// of at most 64 witnesses -- the batch prover's limit, so its workspaces pr_z / pr_abc serve and nothing new is allocated
}  // extern "C"
// the pieces of either source: piece `first` of a host source starts at witness `first`, of a device source at member `first` of the map
static int r1cs_check_pieces(vsp_ctx *ctx, const vsp_r1cs *cs, const WitnessSrc &all, size_t count, uint8_t *status_out, uint64_t *first_bad_row_out, uint64_t *bad_rows_out) {
    if (ctx->prove.active || ctx->cast.active) return set_error(ctx, VSP_ERR_ARG, "r1cs_check: a proof is in flight on this context and owns the workspace (finish it first)");
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t nv = cs->num_vars;
    size_t z_bytes = 0;
    int rc = VSP_OK;
    for (size_t first = 0; first < count && rc == VSP_OK; first += vsp_ctx::VERDICT_MEMBERS) {
        const size_t K = count - first < vsp_ctx::VERDICT_MEMBERS ? count - first : vsp_ctx::VERDICT_MEMBERS;
        WitnessSrc w = all;
        if (all.dev) { w.first = first; if (all.members) w.members = all.members + first; }
        else w.plain = all.plain + first * nv * 4;
        rc = [&]() -> int {
            hipEvent_t t0, t1;                                                            // around the verdict kernels
            VSP_TRY(ctx->check_timer.event(ctx, 1, &t0));
            VSP_TRY(ctx->check_timer.event(ctx, 2, &t1));
            VSP_TRY(ctx->check_timer.mark(ctx, 0, ctx->stream));
            VSP_TRY(prove_front_half(ctx, cs, w, K, true));
            VSP_TRY(verdict_queue(ctx, cs, K, true, t0, t1));
            VSP_HIP(hipStreamSynchronize(ctx->stream));
            return VSP_OK;
        }();
        if (K * (nv + 1) * sizeof(Fr) > z_bytes) z_bytes = K * (nv + 1) * sizeof(Fr);
        if (rc != VSP_OK) break;
        ctx->check_timer.add(ctx, 0, "r1cs_check_front_ms");
        ctx->check_timer.add(ctx, 1, "r1cs_check_ms");
        for (size_t k = 0; k < K; k++) {
            const Verdict v = verdict_of(ctx, k);
            status_out[first + k] = (uint8_t)((v.not_canonical ? 1 : 0) | (v.bad_rows ? 2 : 0));
            if (first_bad_row_out) first_bad_row_out[first + k] = v.first_bad_row;
            if (bad_rows_out) bad_rows_out[first + k] = v.bad_rows;
        }
    }
    // the call's copy of the witnesses is zeroed, as after a proof (prove_cleanup)
    if (ctx->pr_z.p && z_bytes) hipMemsetAsync(ctx->pr_z.p, 0, z_bytes < ctx->pr_z.cap ? z_bytes : ctx->pr_z.cap, ctx->stream);
    if (rc == VSP_OK) ctx->stats["r1cs_check_witnesses"] += (double)count;
    return rc;
}
extern "C" {
int vsp_r1cs_check_batch(vsp_ctx *ctx, const vsp_r1cs *cs, const uint64_t *witnesses, size_t count, uint8_t *status_out, uint64_t *first_bad_row_out,
                         uint64_t *bad_rows_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!cs || !witnesses || !status_out) return set_error(ctx, VSP_ERR_ARG, "r1cs_check: null argument");
    const WitnessSrc w{witnesses, nullptr, nullptr, nullptr, 0};
    return r1cs_check_pieces(ctx, cs, w, count, status_out, first_bad_row_out, bad_rows_out);
}
int vsp_r1cs_check_batch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members, size_t count,
                                uint8_t *status_out, uint64_t *first_bad_row_out, uint64_t *bad_rows_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!cs || !d_witnesses || !status_out) return set_error(ctx, VSP_ERR_ARG, "r1cs_check_device: null argument");
    WitnessSrc w;
    VSP_TRY(witness_src_device(ctx, "r1cs_check_device", cs, d_witnesses, stride, rows, members, count, &w));
    return r1cs_check_pieces(ctx, cs, w, count, status_out, first_bad_row_out, bad_rows_out);
}
int vsp_r1cs_is_satisfied(vsp_ctx *ctx, const vsp_r1cs *cs, const uint64_t *witness, int *satisfied_out, uint64_t *first_bad_row_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!satisfied_out) return set_error(ctx, VSP_ERR_ARG, "r1cs_is_satisfied: null argument");
    uint8_t status = 0;
    VSP_TRY(vsp_r1cs_check_batch(ctx, cs, witness, 1, &status, first_bad_row_out, nullptr));
    *satisfied_out = status == 0;
    return VSP_OK;
}

}  // extern "C"
