// SAVER decrypt and verify_decryption on the GPU (include/vsp.h "SAVER decryption"): the last step of the election,
// decrypt<elgamal_verifiable> / verify_decryption<elgamal_verifiable> of the reference (common.hpp:1220-1223, 1282-1283) on the
// aggregated ciphertext that vsp_tally_result returns.
//
//     nu      = rho c_0
//     value_i = fexp( ml(c_i, W_i) ml(-nu, V_i) )                 i = 1..n        V_i = rho_sv_g2[i-1], W_i = rho_rhov_g2[i-1]
//     base_i  = e(G_i, W_i)                                                        G_i = gamma_abc_g1[i]
//     m_i     = the m in [0, max_value] with base_i^m = value_i                    (gt_dlog.h: baby-step / giant-step)
//     verify_decryption:   equation 0   e(nu, H) e(c_0, -rho_g2) = 1        equation i   value_i = base_i^(m_i)
//
// The conventions of pairing.hip: one lane per item, 64-lane blocks, tower values in memory behind __noinline__ wrappers.  Stages per
// piece of a call, all on the context's stream:
//   1. k_dec_prepare          one lane per ciphertext: c_0..c_n checked and in Montgomery form, nu = rho c_0 by double-and-add with the
//                             generic additions, one inversion, -nu
//      k_dec_prepare_verify   (verification) the same checks on the stated nu and the scalars m_i < r instead of the multiplication
//   2. k_dec_values           one lane per (ciphertext, slot): miller_multi of the two pairs over the prepared lines of W_i, V_i --
//                             and for verification one more item per ciphertext, equation 0 over the lines of -rho_g2, H --
//                             then pairing.hip's final exponentiation (pairing_final_exp)
//   3. k_dlog_search          one lane per run of DLOG_RUN_STEPS giant steps of one (ciphertext, slot), launched over the giant range in
//                             pieces until every item of the piece has a result (k_dlog_pending: one word read between launches)
//      k_dec_power            (verification) one lane per (ciphertext, slot): base_i^(m_i) for the full-width m_i, compared with value_i
// and, once per key, k_dlog_table: one lane per run of DLOG_RUN_STEPS baby steps of one slot.
#include <chrono>

#include "common.h"
#include "gt_dlog.h"
#include "pairing_g1.h"

// Public data only (the secret rho is an argument of decrypt alone): the prepared lines in the order W_1 V_1 .. W_n V_n | -rho_g2 | H,
// base_i and g_i = base_i^(-B) in Montgomery form, and per slot the B = 2^b baby steps sorted by fingerprint
struct vsp_saver_decryptor {
    int device = 0;
    size_t n = 0;                       // msg_size
    uint64_t max_value = 0, giants = 0; // giant steps: ceil((max_value + 1) / B)
    unsigned b = 0, fp_bits = 64;
    std::vector<uint8_t> base;          // n x 576: base_i, canonical tower order
    vsp::DevBuf d_lines;                // (2 n + 2) x MILLER_LINES LineCoeffs
    vsp::DevBuf d_base, d_g;            // n Fp12 each
    vsp::DevBuf d_keys, d_js;           // n x B fingerprints (8 bytes) and exponents (4 bytes)
};

namespace vsp {

static constexpr size_t DECRYPT_MAX_ITEMS = 65535;             // (ciphertext, slot) items of one piece: a grid dimension of the search

struct Scalar256 { uint32_t w[8]; };

static __device__ __noinline__ void dc_miller2(Fp12 *f, const G1Affine *P, size_t stride, const LineCoeffs<Fp> *lines) {
    *f = miller_multi<Fp>(P, stride, lines, 2, nullptr, nullptr);
}
static __device__ __noinline__ void dc_pow(Fp12 *out, const Fp12 *a, const uint64_t *e, int nwords) { *out = gt_pow(*a, e, nwords); }
static __device__ __noinline__ void dc_baby_run(const Fp12 *base, uint64_t j0, unsigned steps, unsigned fp_bits, uint64_t *keys_out) {
    dlog_baby_run(*base, j0, steps, fp_bits, keys_out);
}
static __device__ __noinline__ uint64_t dc_giant_run(const Fp12 *value, const Fp12 *base, const Fp12 *g, uint64_t k0, unsigned steps, const uint64_t *keys, const uint32_t *js,
                                                     unsigned b, unsigned fp_bits, uint64_t max_value) {
    return dlog_giant_run(*value, *base, *g, k0, steps, keys, js, b, fp_bits, max_value);
}

// The points of a piece of c ciphertexts: member j of ciphertext k at pts[j c + k] -- c_0 .. c_n, then -nu (j = n + 1) and, for
// verification, nu (j = n + 2).  status[k]: not zero = malformed, and then every point of the ciphertext is infinity (its values are one)
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dec_prepare(const uint64_t *__restrict__ ct, Scalar256 rho, size_t c, size_t n, G1Affine *__restrict__ pts,
                                                                  G1Affine *__restrict__ nu_out, uint8_t *__restrict__ status) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    G1Affine P;
    uint32_t st = 0;
#pragma unroll 1
    for (size_t j = 0; j <= n; j++) { st |= pr_load_g1(ct + (k * (n + 2) + j) * 12, &P); pts[j * c + k] = P; }
    G1Affine zero; zero.x = Fp::zero(); zero.y = Fp::zero();
    if (st) {
#pragma unroll 1
        for (size_t j = 0; j <= n; j++) pts[j * c + k] = zero;
    }
    // nu = rho c_0: rho < r < 2^255; c_0 = infinity (or a malformed ciphertext) leaves infinity
    G1Affine c0 = pts[k];
    G1XYZZ acc = G1XYZZ::inf();
#pragma unroll 1
    for (int i = 254; i >= 0; i--) {
        pr_dbl(&acc);
        if ((rho.w[i >> 5] >> (i & 31)) & 1) pr_madd(&acc, &c0);
    }
    G1Affine nu = pr_to_affine(acc);                                 // infinity comes out as x = y = 0
    G1Affine canon; canon.x = from_mont(nu.x); canon.y = from_mont(nu.y);
    nu_out[k] = canon;
    nu.y = neg(nu.y);
    pts[(n + 1) * c + k] = nu;
    status[k] = (uint8_t)st;
}

__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dec_prepare_verify(const uint64_t *__restrict__ ct, const uint32_t *__restrict__ msgs, const uint64_t *__restrict__ nu_in,
                                                                         size_t c, size_t n, G1Affine *__restrict__ pts, uint8_t *__restrict__ status) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    G1Affine P;
    uint32_t st = 0;
#pragma unroll 1
    for (size_t j = 0; j <= n; j++) { st |= pr_load_g1(ct + (k * (n + 2) + j) * 12, &P); pts[j * c + k] = P; }
    st |= pr_load_g1(nu_in + k * 12, &P);
    pts[(n + 2) * c + k] = P;
    P.y = neg(P.y);
    pts[(n + 1) * c + k] = P;
#pragma unroll 1
    for (size_t i = 0; i < n; i++) {
        const uint32_t *s = msgs + (k * n + i) * 8;
        const uint4 lo = *(const uint4 *)s, hi = *(const uint4 *)(s + 4);
        if (!scalar_below_r(lo, hi)) st |= 1u;
    }
    if (st) {
        G1Affine zero; zero.x = Fp::zero(); zero.y = Fp::zero();
#pragma unroll 1
        for (size_t j = 0; j <= n + 2; j++) pts[j * c + k] = zero;
    }
    status[k] = (uint8_t)st;
}

// lane = ciphertext, blockIdx.y = slot: every lane of a wave reads the same line coefficients.  Slot i < n: the pairs (c_{i+1}, W_{i+1})
// (-nu, V_{i+1}); slot n (verification only): (c_0, -rho_g2) (nu, H).  out[slot c + k]
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dec_values(const G1Affine *__restrict__ pts, const LineCoeffs<Fp> *__restrict__ lines, size_t c, size_t n,
                                                                 Fp12 *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const size_t slot = blockIdx.y;
    Fp12 f;
    if (slot < n) dc_miller2(&f, pts + (slot + 1) * c + k, (n - slot) * c, lines + 2 * slot * MILLER_LINES);
    else dc_miller2(&f, pts + k, (n + 2) * c, lines + 2 * n * MILLER_LINES);
    out[slot * c + k] = f;
}

// blockIdx.y = slot; lane l of a slot walks baby steps l S .. l S + S - 1, S = DLOG_RUN_STEPS: keys[slot B + j] = fingerprint(base^j)
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dlog_table(const Fp12 *__restrict__ base, unsigned b, unsigned fp_bits, uint64_t *__restrict__ keys) {
    const uint64_t B = (uint64_t)1 << b, j0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * DLOG_RUN_STEPS;
    if (j0 >= B) return;
    const size_t slot = blockIdx.y;
    Fp12 bs = base[slot];
    dc_baby_run(&bs, j0, (unsigned)(B - j0 < DLOG_RUN_STEPS ? B - j0 : DLOG_RUN_STEPS), fp_bits, keys + slot * B + j0);
}

// blockIdx.y = item (slot c + k); lane l of this launch owns run lane0 + l of the item's giant range: steps (lane0 + l) S .. + S - 1.
// A confirmed m goes out by atomicMin on the item's word (all ones = none yet); an item that has its result is skipped
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dlog_search(const Fp12 *__restrict__ vals, const Fp12 *__restrict__ base, const Fp12 *__restrict__ g,
                                                                  const uint64_t *__restrict__ keys, const uint32_t *__restrict__ js, size_t c, unsigned b, unsigned fp_bits,
                                                                  uint64_t max_value, uint64_t giants, uint64_t lane0, uint64_t lanes, unsigned long long *result) {
    const uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= lanes) return;
    const uint64_t k0 = (lane0 + l) * DLOG_RUN_STEPS;
    if (k0 >= giants) return;
    const size_t item = blockIdx.y, slot = item / c;
    if (result[item] != DLOG_NONE) return;
    Fp12 v = to_mont(vals[item]), bs = base[slot], gs = g[slot];
    const uint64_t m = dc_giant_run(&v, &bs, &gs, k0, (unsigned)(giants - k0 < DLOG_RUN_STEPS ? giants - k0 : DLOG_RUN_STEPS), keys + ((size_t)slot << b),
                                    js + ((size_t)slot << b), b, fp_bits, max_value);
    if (m != DLOG_NONE) atomicMin(&result[item], (unsigned long long)m);
}
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dlog_pending(const unsigned long long *__restrict__ result, size_t items, uint32_t *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < items && result[i] == DLOG_NONE) atomicAdd(flag, 1u);
}

// lane = ciphertext, blockIdx.y = slot: ok[slot c + k] = (base_slot^(m) = value), m the canonical scalar msgs[k n + slot]
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_dec_power(const Fp12 *__restrict__ vals, const Fp12 *__restrict__ base, const uint64_t *__restrict__ msgs, size_t c,
                                                                size_t n, const uint8_t *__restrict__ status, uint8_t *__restrict__ ok) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const size_t slot = blockIdx.y, item = slot * c + k;
    if (status[k]) { ok[item] = 0; return; }
    uint64_t e[4];
    for (int w = 0; w < 4; w++) e[w] = msgs[(k * n + slot) * 4 + w];
    Fp12 bs = base[slot], pw;
    dc_pow(&pw, &bs, e, 4);
    const Fp12 v = to_mont(vals[item]);
    ok[item] = eq(pw, v) ? 1 : 0;
}

// the power on its own (include/vsp.h vsp_selftest_tower, level 12 op 12): canonical a, the exponent in the first four words of b,
// through the dc_pow that k_dec_power calls
__global__ __launch_bounds__(DLOG_BLOCK_LANES) void k_selftest_gt_pow(const Fp12 *__restrict__ a, const Fp12 *__restrict__ b, Fp12 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t *src = (const uint64_t *)(b + i);
    uint64_t e[4];
    for (int w = 0; w < 4; w++) e[w] = src[w];
    Fp12 bs = to_mont(a[i]), pw;
    dc_pow(&pw, &bs, e, 4);
    out[i] = from_mont(pw);
}
int decrypt_selftest_gt_pow(vsp_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n) {
    hipLaunchKernelGGL(k_selftest_gt_pow, dim3((unsigned)((n + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES)), dim3(DLOG_BLOCK_LANES), 0, ctx->stream, (const Fp12 *)d_a,
                       (const Fp12 *)d_b, (Fp12 *)d_out, n);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

void saver_decryptor_free(vsp_ctx *ctx, vsp_saver_decryptor *dec) {
    if (!dec) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    delete dec;
}
size_t saver_decryptor_msg_size(const vsp_saver_decryptor *dec) { return dec->n; }
uint64_t saver_decryptor_max_value(const vsp_saver_decryptor *dec) { return dec->max_value; }
unsigned saver_decryptor_baby_bits(const vsp_saver_decryptor *dec) { return dec->b; }
const uint8_t *saver_decryptor_base(const vsp_saver_decryptor *dec, size_t slot) { return slot < dec->n ? dec->base.data() + 576 * slot : nullptr; }

static int decryptor_build(vsp_ctx *ctx, vsp_saver_decryptor *dec, const uint64_t *vk_words, const uint64_t *gamma_abc_g1) {
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = dec->n, B = (size_t)1 << dec->b;
    const uint64_t *rho_g2 = vk_words, *V = vk_words + 24, *W = vk_words + 24 + 24 * n;
    // the prepared lines: W_1 V_1 .. W_n V_n | -rho_g2 | H
    std::vector<Affine<HFp2>> q(2 * n + 2);
    for (size_t i = 0; i < n; i++) { q[2 * i] = host_load_affine<HFp2>(W + 24 * i); q[2 * i + 1] = host_load_affine<HFp2>(V + 24 * i); }
    q[2 * n] = host_load_affine<HFp2>(rho_g2);
    q[2 * n].y = neg(q[2 * n].y);                                                                       // infinity stays x = y = 0
    q[2 * n + 1] = host_load_affine<HFp2>(G2::GEN);
    std::vector<LineCoeffs<HFp>> lines(q.size() * MILLER_LINES);                                        // LineCoeffs<HFp> and <Fp>: the same bytes
    host_parallel_for(q.size(), [&](size_t j) { prepare_g2(q[j], lines.data() + j * MILLER_LINES); });
    const size_t line_bytes = lines.size() * sizeof(LineCoeffs<HFp>);
    VSP_HIP(dec->d_lines.alloc(line_bytes));
    VSP_HIP(hipMemcpyAsync(dec->d_lines.p, lines.data(), line_bytes, hipMemcpyHostToDevice, st));
    VSP_HIP(hipStreamSynchronize(st));
    // base_i = e(G_i, W_i) by the pairing kernels; one means a degenerate key
    dec->base.resize(576 * n);
    std::vector<uint8_t> is_one(n);
    VSP_TRY(pairing_multi_batch(ctx, gamma_abc_g1 + 12, W, 1, n, dec->base.data(), is_one.data()));
    std::vector<HFp12> bg(2 * n);                                                                       // HFp12 and Fp12: the same bytes
    for (size_t i = 0; i < n; i++) {
        if (is_one[i]) return set_error(ctx, VSP_ERR_ARG, "saver_decryptor_create: degenerate key: e(G_i, rho_rhov_g2[i]) is one");
        HFp12 e; memcpy(&e, dec->base.data() + 576 * i, sizeof e);
        bg[i] = to_mont(e);
    }
    host_parallel_for(n, [&](size_t i) { bg[n + i] = dlog_giant_stride(bg[i], dec->b); });
    VSP_HIP(dec->d_base.alloc(n * sizeof(HFp12)));
    VSP_HIP(dec->d_g.alloc(n * sizeof(HFp12)));
    VSP_HIP(hipMemcpyAsync(dec->d_base.p, bg.data(), n * sizeof(HFp12), hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemcpyAsync(dec->d_g.p, bg.data() + n, n * sizeof(HFp12), hipMemcpyHostToDevice, st));
    VSP_HIP(hipStreamSynchronize(st));
    // the baby tables: fingerprints on the GPU, the sort by fingerprint on the host, once
    VSP_HIP(dec->d_keys.alloc(n * B * sizeof(uint64_t)));
    VSP_HIP(dec->d_js.alloc(n * B * sizeof(uint32_t)));
    const size_t runs = (B + DLOG_RUN_STEPS - 1) / DLOG_RUN_STEPS;
    VSP_TRY(ctx->dec_timer.mark(ctx, 0, st));
    hipLaunchKernelGGL(k_dlog_table, dim3((unsigned)((runs + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES), (unsigned)n), dim3(DLOG_BLOCK_LANES), 0, st, dec->d_base.as<const Fp12>(),
                       dec->b, dec->fp_bits, dec->d_keys.as<uint64_t>());
    VSP_LAUNCH_CHECK();
    VSP_TRY(ctx->dec_timer.mark(ctx, 1, st));
    std::vector<uint64_t> keys(n * B);
    std::vector<uint32_t> js(n * B);
    VSP_HIP(hipMemcpyAsync(keys.data(), dec->d_keys.p, keys.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    ctx->dec_timer.add(ctx, 0, "saver_decrypt_table_ms");
    const auto t0 = std::chrono::steady_clock::now();
    host_parallel_for(n, [&](size_t i) { dlog_sort_table(keys.data() + i * B, js.data() + i * B, B); });
    ctx->stats["saver_decrypt_sort_ms"] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    VSP_HIP(hipMemcpyAsync(dec->d_keys.p, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemcpyAsync(dec->d_js.p, js.data(), js.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    VSP_HIP(hipStreamSynchronize(st));
    return VSP_OK;
}

vsp_saver_decryptor *saver_decryptor_create(vsp_ctx *ctx, size_t n, const uint64_t *vk_words, const uint64_t *gamma_abc_g1, uint64_t max_value) {
    auto refuse = [&](const char *msg) { set_error(ctx, VSP_ERR_ARG, msg); return (vsp_saver_decryptor *)nullptr; };
    const long ob = opt(ctx, "saver_decrypt_baby_bits", 0), of = opt(ctx, "saver_decrypt_fp_bits", 64);
    if (ob < 0 || ob > (long)DLOG_MAX_BABY_BITS) return refuse("saver_decryptor_create: option saver_decrypt_baby_bits outside 0..20");
    if (of < 1 || of > 64) return refuse("saver_decryptor_create: option saver_decrypt_fp_bits outside 1..64");
    const unsigned b = ob ? (unsigned)ob : dlog_auto_baby_bits(max_value);
    if (dlog_giant_steps(max_value, b) > DLOG_MAX_GIANT_STEPS) return refuse("saver_decryptor_create: max_value needs more than 2^24 giant steps at these baby bits");
    for (size_t j = 0; j < 2 * n + 1; j++)
        if (!affine_valid<G2>(vk_words + 24 * j)) return refuse("saver_decryptor_create: a verification key point is not canonical or not on its curve");
    for (size_t i = 0; i <= n; i++)
        if (!affine_valid<G1>(gamma_abc_g1 + 12 * i)) return refuse("saver_decryptor_create: a gamma_ABC point is not canonical or not on the curve");
    for (size_t i = 0; i < n; i++)
        if (limbs_zero(gamma_abc_g1 + 12 * (i + 1), 12) || limbs_zero(vk_words + 24 + 24 * i, 24) || limbs_zero(vk_words + 24 + 24 * n + 24 * i, 24))
            return refuse("saver_decryptor_create: degenerate key: a G_i, rho_sv_g2[i] or rho_rhov_g2[i] is infinity");
    vsp_saver_decryptor *dec = new vsp_saver_decryptor();
    dec->device = ctx->device; dec->n = n; dec->max_value = max_value; dec->b = b; dec->fp_bits = (unsigned)of; dec->giants = dlog_giant_steps(max_value, b);
    if (decryptor_build(ctx, dec, vk_words, gamma_abc_g1) != VSP_OK) { saver_decryptor_free(ctx, dec); return nullptr; }
    return dec;
}

// ciphertexts of one piece: "pairing_chunk" as for the pairings, and at most DECRYPT_MAX_ITEMS (ciphertext, slot) items, equation 0 counted
static size_t decrypt_piece(const vsp_ctx *ctx, size_t n) {
    const long v = opt(ctx, "pairing_chunk", (long)1 << 14);
    size_t piece = v < 1 ? 1 : ((size_t)v > ((size_t)1 << 14) ? (size_t)1 << 14 : (size_t)v);
    if (piece * (n + 1) > DECRYPT_MAX_ITEMS) piece = DECRYPT_MAX_ITEMS / (n + 1);
    return piece ? piece : 1;
}
// what both calls need of the context for a piece of c ciphertexts with `slots` items each and `raw` canonical input words
static int decrypt_workspace(vsp_ctx *ctx, size_t c, size_t n, size_t slots, size_t raw_words) {
    VSP_TRY(ensure(ctx, ctx->pair_raw, raw_words * sizeof(uint64_t)));
    VSP_TRY(ensure(ctx, ctx->pair_g1, (n + 3) * c * sizeof(G1Affine)));
    VSP_TRY(ensure(ctx, ctx->pair_status, c + 2 * slots * c));                                           // malformed | is-one bytes | power bytes
    VSP_TRY(ensure(ctx, ctx->pair_ml, slots * c * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->pair_gt, slots * c * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->dec_out, slots * c * sizeof(uint64_t) + 16));                               // a result word per item | the pending count
    return VSP_OK;
}
// stage 2 over the points in ctx->pair_g1: the values of `slots` items per ciphertext, canonical in ctx->pair_gt, their is-one bytes at
// pair_status + c
static int decrypt_values(vsp_ctx *ctx, const vsp_saver_decryptor *dec, size_t c, size_t slots) {
    hipLaunchKernelGGL(k_dec_values, dim3((unsigned)((c + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES), (unsigned)slots), dim3(DLOG_BLOCK_LANES), 0, ctx->stream,
                       (const G1Affine *)ctx->pair_g1.p, dec->d_lines.as<const LineCoeffs<Fp>>(), c, dec->n, (Fp12 *)ctx->pair_ml.p);
    VSP_LAUNCH_CHECK();
    return pairing_final_exp(ctx, ctx->pair_ml.p, slots * c, ctx->pair_gt.p, (uint8_t *)ctx->pair_status.p + c);
}

int saver_decrypt_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t rho[4], const uint64_t *ct, size_t count, uint64_t *msgs_out, uint64_t *nu_out,
                        uint8_t *status_out) {
    if (dec->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "saver_decrypt_batch: the decryptor belongs to another device");
    if (!below_mod<FrP64>(rho)) return set_error(ctx, VSP_ERR_ARG, "saver_decrypt_batch: rho is not canonical (>= r)");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = dec->n, piece = decrypt_piece(ctx, n);
    Scalar256 k;
    memcpy(k.w, rho, sizeof k.w);
    const uint64_t runs = (dec->giants + DLOG_RUN_STEPS - 1) / DLOG_RUN_STEPS;                           // lanes an item's whole giant range takes
    std::vector<uint64_t> found;
    std::vector<uint8_t> bad;
    for (size_t at = 0; at < count; at += piece) {
        const size_t c = count - at < piece ? count - at : piece, items = n * c, ct_words = c * (n + 2) * 12;
        VSP_TRY(decrypt_workspace(ctx, c, n, n, ct_words + c * 12));
        uint64_t *d_ct = (uint64_t *)ctx->pair_raw.p;
        G1Affine *d_nu = (G1Affine *)(d_ct + ct_words);
        uint8_t *status = (uint8_t *)ctx->pair_status.p;
        unsigned long long *result = (unsigned long long *)ctx->dec_out.p;
        uint32_t *flag = (uint32_t *)(result + items);
        VSP_HIP(hipMemcpyAsync(d_ct, ct + at * (n + 2) * 12, ct_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_TRY(ctx->dec_timer.mark(ctx, 0, st));
        hipLaunchKernelGGL(k_dec_prepare, dim3((unsigned)((c + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES)), dim3(DLOG_BLOCK_LANES), 0, st, (const uint64_t *)d_ct, k, c, n,
                           (G1Affine *)ctx->pair_g1.p, d_nu, status);
        VSP_LAUNCH_CHECK();
        VSP_TRY(ctx->dec_timer.mark(ctx, 1, st));
        VSP_TRY(decrypt_values(ctx, dec, c, n));
        VSP_TRY(ctx->dec_timer.mark(ctx, 2, st));
        // the giant range in launches of about DLOG_LAUNCH_LANES lanes (whole blocks per item), until no item of the piece is pending
        VSP_HIP(hipMemsetAsync(result, 0xff, items * sizeof(uint64_t), st));
        const uint64_t lanes = dlog_launch_lanes(items, runs);
        for (uint64_t lane0 = 0; lane0 < runs; lane0 += lanes) {
            ctx->stats["saver_decrypt_dlog_launches"] += 1;
            hipLaunchKernelGGL(k_dlog_search, dim3((unsigned)((lanes + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES), (unsigned)items), dim3(DLOG_BLOCK_LANES), 0, st,
                               (const Fp12 *)ctx->pair_gt.p, dec->d_base.as<const Fp12>(), dec->d_g.as<const Fp12>(), dec->d_keys.as<const uint64_t>(), dec->d_js.as<const uint32_t>(), c,
                               dec->b, dec->fp_bits, dec->max_value, dec->giants, lane0, lanes, result);
            VSP_LAUNCH_CHECK();
            if (lane0 + lanes >= runs) break;                                                            // the last launch: nothing left to decide
            VSP_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), st));
            hipLaunchKernelGGL(k_dlog_pending, dim3((unsigned)((items + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES)), dim3(DLOG_BLOCK_LANES), 0, st, result, items, flag);
            VSP_LAUNCH_CHECK();
            uint32_t pending = 0;
            VSP_HIP(hipMemcpyAsync(&pending, flag, sizeof pending, hipMemcpyDeviceToHost, st));
            VSP_HIP(hipStreamSynchronize(st));
            if (!pending) break;
        }
        VSP_TRY(ctx->dec_timer.mark(ctx, 3, st));
        found.resize(items); bad.resize(c);
        VSP_HIP(hipMemcpyAsync(found.data(), result, items * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VSP_HIP(hipMemcpyAsync(bad.data(), status, c, hipMemcpyDeviceToHost, st));
        if (nu_out) VSP_HIP(hipMemcpyAsync(nu_out + at * 12, d_nu, c * 12 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        for (size_t j = 0; j < c; j++)
            for (size_t i = 0; i < n; i++) {
                const uint64_t m = bad[j] ? DLOG_NONE : found[i * c + j];
                msgs_out[(at + j) * n + i] = m;
                status_out[(at + j) * n + i] = bad[j] ? 2 : (m == DLOG_NONE ? 1 : 0);
            }
        static const char *const names[3] = {"saver_decrypt_prepare_ms", "saver_decrypt_values_ms", "saver_decrypt_dlog_ms"};
        for (int i = 0; i < 3; i++) ctx->dec_timer.add(ctx, i, names[i]);
    }
    return VSP_OK;
}

int saver_verify_decryption_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t *ct, const uint64_t *msgs, const uint64_t *nu, size_t count,
                                  uint8_t *verdict_out, uint8_t *reason_out, uint32_t *first_bad_slot_out) {
    if (dec->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "saver_verify_decryption_batch: the decryptor belongs to another device");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t n = dec->n, piece = decrypt_piece(ctx, n);
    std::vector<uint8_t> flags;
    for (size_t at = 0; at < count; at += piece) {
        const size_t c = count - at < piece ? count - at : piece, items = (n + 1) * c, ct_words = c * (n + 2) * 12;
        VSP_TRY(decrypt_workspace(ctx, c, n, n + 1, ct_words + c * n * 4 + c * 12));
        uint64_t *d_ct = (uint64_t *)ctx->pair_raw.p, *d_msgs = d_ct + ct_words, *d_nu = d_msgs + c * n * 4;
        uint8_t *status = (uint8_t *)ctx->pair_status.p, *is_one = status + c, *power_ok = is_one + items;
        VSP_HIP(hipMemcpyAsync(d_ct, ct + at * (n + 2) * 12, ct_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemcpyAsync(d_msgs, msgs + at * n * 4, c * n * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemcpyAsync(d_nu, nu + at * 12, c * 12 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        const unsigned blocks = (unsigned)((c + DLOG_BLOCK_LANES - 1) / DLOG_BLOCK_LANES);
        VSP_TRY(ctx->dec_timer.mark(ctx, 0, st));
        hipLaunchKernelGGL(k_dec_prepare_verify, dim3(blocks), dim3(DLOG_BLOCK_LANES), 0, st, (const uint64_t *)d_ct, (const uint32_t *)d_msgs, (const uint64_t *)d_nu, c, n,
                           (G1Affine *)ctx->pair_g1.p, status);
        VSP_LAUNCH_CHECK();
        VSP_TRY(ctx->dec_timer.mark(ctx, 1, st));
        VSP_TRY(decrypt_values(ctx, dec, c, n + 1));
        VSP_TRY(ctx->dec_timer.mark(ctx, 2, st));
        hipLaunchKernelGGL(k_dec_power, dim3(blocks, (unsigned)n), dim3(DLOG_BLOCK_LANES), 0, st, (const Fp12 *)ctx->pair_gt.p, dec->d_base.as<const Fp12>(),
                           (const uint64_t *)d_msgs, c, n, (const uint8_t *)status, power_ok);
        VSP_LAUNCH_CHECK();
        VSP_TRY(ctx->dec_timer.mark(ctx, 3, st));
        flags.resize(c + 2 * items);
        VSP_HIP(hipMemcpyAsync(flags.data(), status, c + 2 * items, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        const uint8_t *h_one = flags.data() + c, *h_ok = h_one + items;
        for (size_t j = 0; j < c; j++) {
            uint8_t reason = 0;
            uint32_t first = UINT32_MAX;
            if (flags[j]) reason = 1;
            else {
                if (!h_one[n * c + j]) reason |= 2;
                for (size_t i = 0; i < n; i++) if (!h_ok[i * c + j]) { reason |= 4; first = (uint32_t)i; break; }
            }
            verdict_out[at + j] = reason == 0;
            if (reason_out) reason_out[at + j] = reason;
            if (first_bad_slot_out) first_bad_slot_out[at + j] = first;
        }
        static const char *const names[3] = {"saver_decrypt_prepare_ms", "saver_decrypt_values_ms", "saver_decrypt_power_ms"};
        for (int i = 0; i < 3; i++) ctx->dec_timer.add(ctx, i, names[i]);
    }
    return VSP_OK;
}

}  // namespace vsp
