// Batched BLS12-381 pairings and exact per-proof Groth16 verdicts on the GPU (include/vsp.h "pairings").
//
// The verifying side of the reference (zk::verify, tvm.vergrth16) is a product of pairings per proof; the pairs of a batch are
// independent, so the work has the shape of the decoding kernel of decode.hip: one lane per item, straight-line field arithmetic from
// the headers fp12.h / pairing.h, which the CPU test build checks against the test oracle.  Stages per piece of a call, all on the
// context's stream:
//   0. k_pair_check        one lane per pair: coordinates below p, Montgomery form, on the curve (or all zero: infinity); status byte
//      k_verify_prepare    (proofs) one lane per proof: the same checks on A, B, C, scalars below r, acc = G_0 + sum x_i G_i over the
//                          key's table of 4-bit multiples, and the three pairs (A, B), (acc, -gamma), (C, -delta)
//   1. k_miller            one lane per pair: the Miller value f_{|x|,Q}(P), one where a point is infinity (or was rejected)
//   2. k_gt_product        one lane per product: the m Miller values of a product multiplied, their status bytes ORed (m > 1 only)
//   3. k_final_exp         one lane per product: the final exponentiation; 576 canonical bytes, and a byte: equal to one -- or, for
//                          proofs, equal to the key's e(alpha, beta) and no member rejected
// An Fp12 value is 144 registers: the kernels keep their tower values in scratch and call the out-of-line products of fp12.h.
#include "common.h"
#include "pairing.h"
#include "pairing_g1.h"

// vsp_vk, vsp_saver_verifier: common.h
namespace vsp {

static constexpr size_t PAIRING_CHUNK = (size_t)1 << 14;       // products of one piece (option "pairing_chunk")
static constexpr size_t PAIRING_MAX_PAIRS = (size_t)1 << 16;   // pairs of one piece, whatever m is (a piece holds at least one product)
static constexpr size_t SAVER_MAX_ARGS = (size_t)1 << 19;      // G1 arguments of one piece of ballots (msg_size <= 1022: at least 510 ballots)
static constexpr unsigned PAIRING_THREADS = 64;                // one wave per block: 2^14 lanes spread over every compute unit

// the tower work as real calls on memory temporaries (see point_decode.h record_y): one copy of each loop in a kernel
__device__ __noinline__ void pr_miller(Fp12 *f, const G1Affine *P, const G2Affine *Q) { *f = miller_loop(*P, *Q); }
__device__ __noinline__ void pr_final_exp(Fp12 *f) { const Fp12 t = final_exp(*f); *f = t; }
__device__ __noinline__ void pr_mul(Fp12 *f, const Fp12 *g) { const Fp12 t = mul(*f, *g); *f = t; }

// pr_load_g1, pr_dbl, pr_madd, pr_to_affine: pairing_g1.h
__device__ __noinline__ uint32_t pr_load_g2(const uint64_t *src, G2Affine *out) {
    G2Affine c = *(const G2Affine *)src;
    uint32_t st = (canon_below_p(c.x.c0) && canon_below_p(c.x.c1) && canon_below_p(c.y.c0) && canon_below_p(c.y.c1)) ? 0u : 1u;
    G2Affine p; p.x = to_mont(c.x); p.y = to_mont(c.y);
    Fp2 b; b.c0 = dbl(dbl(Fp::one())); b.c1 = b.c0;
    if (!st && !is_inf(c) && !eq(f2sqr(p.y), add(f2mul(f2sqr(p.x), p.x), b))) st = 2u;
    if (st) { p.x = Fp2::zero(); p.y = Fp2::zero(); }
    *out = p;
    return st;
}
// pr_scalars_below_r, pr_input_sum, pr_ballot_acc_start: pairing_g1.h

__global__ __launch_bounds__(PAIRING_THREADS) void k_pair_check(const uint64_t *__restrict__ g1, const uint64_t *__restrict__ g2, size_t n, G1Affine *__restrict__ p_out,
                                                                G2Affine *__restrict__ q_out, uint8_t *__restrict__ status, uint32_t *__restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine P; G2Affine Q;
    const uint32_t st = pr_load_g1(g1 + 12 * i, &P) | pr_load_g2(g2 + 24 * i, &Q);
    p_out[i] = P; q_out[i] = Q;
    status[i] = (uint8_t)st;
    if (st) atomicOr(flag, st);
}

// proof k of a piece: pairs 3k .. 3k + 2.  inputs: n x (n_abc - 1) canonical scalars; tab: the key's multiples, neg: -gamma, -delta
__global__ __launch_bounds__(PAIRING_THREADS) void k_verify_prepare(const uint64_t *__restrict__ A, const uint64_t *__restrict__ B, const uint64_t *__restrict__ C,
                                                                    const uint32_t *__restrict__ inputs, size_t n, size_t n_abc, const G1Affine *__restrict__ tab,
                                                                    const G2Affine *__restrict__ neg_gd, G1Affine *__restrict__ p_out, G2Affine *__restrict__ q_out,
                                                                    uint8_t *__restrict__ status) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    G1Affine P; G2Affine Q;
    uint32_t st = pr_load_g1(A + 12 * k, &P) | pr_load_g2(B + 24 * k, &Q);
    p_out[3 * k] = P; q_out[3 * k] = Q;
    status[3 * k] = (uint8_t)st;
    st = pr_load_g1(C + 12 * k, &P);
    p_out[3 * k + 2] = P; q_out[3 * k + 2] = neg_gd[1];
    status[3 * k + 2] = (uint8_t)st;
    // the public-input combination G_0 + sum x_i G_i
    const size_t L = n_abc - 1;
    const uint32_t *s = inputs + k * L * 8;
    st = pr_scalars_below_r(s, L) ? 0u : 1u;
    G1XYZZ acc;
    pr_input_sum(acc, s, L, tab + 16);
    { G1Affine g0 = tab[1]; pr_madd(&acc, &g0); }
    P = pr_to_affine(acc);
    if (st) { P.x = Fp::zero(); P.y = Fp::zero(); }
    p_out[3 * k + 1] = P; q_out[3 * k + 1] = neg_gd[0];
    status[3 * k + 1] = (uint8_t)st;
}

__global__ __launch_bounds__(PAIRING_THREADS) void k_miller(const G1Affine *__restrict__ g1, const G2Affine *__restrict__ g2, size_t n, Fp12 *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    G1Affine P = g1[i]; G2Affine Q = g2[i];
    Fp12 f;
    pr_miller(&f, &P, &Q);
    out[i] = f;
}

__global__ __launch_bounds__(PAIRING_THREADS) void k_gt_product(const Fp12 *__restrict__ ml, const uint8_t *__restrict__ status, size_t m, size_t n, Fp12 *__restrict__ out,
                                                                uint8_t *__restrict__ pstatus) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp12 f = ml[i * m];
    uint32_t st = status[i * m];
#pragma unroll 1
    for (size_t j = 1; j < m; j++) { Fp12 g = ml[i * m + j]; pr_mul(&f, &g); st |= status[i * m + j]; }
    out[i] = f;
    pstatus[i] = (uint8_t)st;
}

// the byte of item i < n_one says "is one"; that of the others "equals *expect (one Fp12 in Montgomery form)" and, where pstatus is
// given, "no member was rejected".  gt_out: the canonical values, or null
__global__ __launch_bounds__(PAIRING_THREADS) void k_final_exp(const Fp12 *__restrict__ in, const uint8_t *__restrict__ pstatus, size_t n, size_t n_one,
                                                               const Fp12 *__restrict__ expect, Fp12 *__restrict__ gt_out, uint8_t *__restrict__ flag_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp12 f = in[i];
    pr_final_exp(&f);
    bool ok;
    if (i < n_one) ok = is_one(f);
    else { const Fp12 e = *expect; ok = eq(f, e) && (!pstatus || pstatus[i] == 0); }
    flag_out[i] = ok ? 1 : 0;
    if (gt_out) gt_out[i] = from_mont(f);
}

// ---- SAVER ballots (include/vsp.h "SAVER ballot verdicts").  A ballot of a piece of c has n + 4 G1 arguments whose G2
// partner is a key member with prepared lines -- c_0 .. c_n, psi, acc, C: argument j of ballot k at pts[j c + k], its lines at
// lines[j MILLER_LINES] -- and the pair (A, B)
__device__ __noinline__ void pr_miller_multi(Fp12 *f, const G1Affine *P, size_t stride, const LineCoeffs<Fp> *lines, size_t g, const G1Affine *Pv, const G2Affine *Qv) {
    *f = miller_multi<Fp>(P, stride, lines, g, Pv, Qv);
}

// ballot k of a piece: every limb vector checked and in Montgomery form, acc = G_0 + c_0 + .. + c_n + sum x_i G_{n+1+i} (the additions
// generic: equal, opposite and infinity summands are legal ciphertexts; the scalar part by pr_input_sum as in k_verify_prepare).
// status[k]: not zero = malformed.  rest: c x n_rest canonical scalars, n_rest = n_abc - 1 - n
__global__ __launch_bounds__(PAIRING_THREADS) void k_ballot_prepare(const uint64_t *__restrict__ ct, const uint32_t *__restrict__ rest, const uint64_t *__restrict__ A,
                                                                    const uint64_t *__restrict__ B, const uint64_t *__restrict__ C, size_t c, size_t n, size_t n_abc,
                                                                    const G1Affine *__restrict__ tab, G1Affine *__restrict__ pts, G1Affine *__restrict__ a_out,
                                                                    G2Affine *__restrict__ b_out, uint8_t *__restrict__ status) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    G1Affine P; G2Affine Q;
    uint32_t st = pr_load_g1(A + 12 * k, &P) | pr_load_g2(B + 24 * k, &Q);
    a_out[k] = P; b_out[k] = Q;
    st |= pr_load_g1(C + 12 * k, &P);
    pts[(n + 3) * c + k] = P;
    const size_t L = n_abc - 1 - n;
    const uint32_t *s = rest + k * L * 8;
    if (!pr_scalars_below_r(s, L)) st |= 1u;
    G1XYZZ acc;
    pr_ballot_acc_start(acc, s, L, n, tab);
#pragma unroll 1
    for (size_t j = 0; j < n + 2; j++) {
        st |= pr_load_g1(ct + (k * (n + 2) + j) * 12, &P);
        pts[j * c + k] = P;
        if (j <= n) pr_madd(&acc, &P);                              // psi (j = n + 1) is no summand
    }
    pts[(n + 2) * c + k] = pr_to_affine(acc);
    status[k] = (uint8_t)st;
}

// lane = ballot, blockIdx.y = group: every lane of a wave reads the same line coefficients.  Groups 0 .. ng - 1 cut the n + 2 pairs of
// the ciphertext equation into runs of G (the last may be shorter); group ng is the Groth16 side (acc, -gamma) (C, -delta) (A, B).
// out[group c + k]
__global__ __launch_bounds__(PAIRING_THREADS) void k_miller_ballot(const G1Affine *__restrict__ pts, const G1Affine *__restrict__ a_in, const G2Affine *__restrict__ b_in,
                                                                   const LineCoeffs<Fp> *__restrict__ lines, size_t c, size_t n, size_t G, size_t ng, Fp12 *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const size_t grp = blockIdx.y;
    Fp12 f;
    if (grp < ng) {
        const size_t first = grp * G, g = first + G <= n + 2 ? G : n + 2 - first;
        pr_miller_multi(&f, pts + first * c + k, c, lines + first * MILLER_LINES, g, nullptr, nullptr);
    } else {
        G1Affine Pa = a_in[k]; G2Affine Qb = b_in[k];
        pr_miller_multi(&f, pts + (n + 2) * c + k, c, lines + (n + 2) * MILLER_LINES, 2, &Pa, &Qb);
    }
    out[grp * c + k] = f;
}

// the two Miller values of ballot k: out[k] = the product of groups 0 .. ng - 1, out[c + k] = group ng
__global__ __launch_bounds__(PAIRING_THREADS) void k_ballot_product(const Fp12 *__restrict__ ml, size_t c, size_t ng, Fp12 *__restrict__ out) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    Fp12 f = ml[k];
#pragma unroll 1
    for (size_t j = 1; j < ng; j++) { Fp12 g = ml[j * c + k]; pr_mul(&f, &g); }
    out[k] = f;
    out[c + k] = ml[ng * c + k];
}

// ---- the tower on its own (include/vsp.h vsp_selftest_tower): one operation per lane on canonical values.  Levels 6 and 12 go through
// wrappers of the kind above on memory temporaries, so the out-of-line bodies they reach (fp12.h VSP_HD_CALL) are this translation
// unit's copies, the ones k_miller and k_final_exp run
__device__ __noinline__ void pr_sqr(Fp12 *f) { const Fp12 t = sqr(*f); *f = t; }
__device__ __noinline__ void pr_inv(Fp12 *f) { const Fp12 t = inv(*f); *f = t; }
__device__ __noinline__ void pr_frobenius(Fp12 *f) { const Fp12 t = frobenius(*f); *f = t; }
__device__ __noinline__ void pr_frobenius2(Fp12 *f) { const Fp12 t = frobenius2(*f); *f = t; }
__device__ __noinline__ void pr_cyclotomic_sqr(Fp12 *f) { const Fp12 t = cyclotomic_sqr(*f); *f = t; }
__device__ __noinline__ void pr_mul_by_014(Fp12 *f, const Fp2 *l0, const Fp2 *l1, const Fp2 *l4) { const Fp12 t = mul_by_014(*f, *l0, *l1, *l4); *f = t; }
__device__ __noinline__ void pr6_mul(Fp6 *f, const Fp6 *g) { const Fp6 t = mul(*f, *g); *f = t; }
__device__ __noinline__ void pr6_inv(Fp6 *f) { const Fp6 t = inv(*f); *f = t; }
__device__ __noinline__ void pr6_mul_by_01(Fp6 *f, const Fp2 *b0, const Fp2 *b1) { const Fp6 t = mul_by_01(*f, *b0, *b1); *f = t; }
__device__ __noinline__ void pr6_mul_by_1(Fp6 *f, const Fp2 *b1) { const Fp6 t = mul_by_1(*f, *b1); *f = t; }
__device__ __forceinline__ Fp6 to_mont(const Fp6 &a) { Fp6 r; r.c0 = to_mont(a.c0); r.c1 = to_mont(a.c1); r.c2 = to_mont(a.c2); return r; }
__device__ __forceinline__ Fp6 from_mont(const Fp6 &a) { Fp6 r; r.c0 = from_mont(a.c0); r.c1 = from_mont(a.c1); r.c2 = from_mont(a.c2); return r; }

__global__ __launch_bounds__(PAIRING_THREADS) void k_selftest_fp12(int op, const Fp12 *__restrict__ a, const Fp12 *__restrict__ b, Fp12 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp12 x = to_mont(a[i]), y = to_mont(b[i]);
    switch (op) {
        case 0: pr_mul(&x, &y); break;
        case 1: pr_sqr(&x); break;
        case 2: pr_inv(&x); break;
        case 3: x = conj(x); break;
        case 4: pr_frobenius(&x); break;
        case 5: pr_frobenius2(&x); break;
        case 6: pr_cyclotomic_sqr(&x); break;
        case 7: x = add(x, y); break;
        case 8: x = sub(x, y); break;
        case 9: pr_final_exp(&x); break;
        case 10: pr_mul_by_014(&x, &y.c0.c0, &y.c0.c1, &y.c1.c1); break;
        default: {                                                  // op 11: the answer in the first word, not a field value
            Fp12 flag = Fp12::zero();
            flag.c0.c0.c0.l[0] = is_one(x) ? 1u : 0u;
            out[i] = flag;
            return;
        }
    }
    out[i] = from_mont(x);
}
__global__ __launch_bounds__(PAIRING_THREADS) void k_selftest_fp6(int op, const Fp6 *__restrict__ a, const Fp6 *__restrict__ b, Fp6 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp6 x = to_mont(a[i]), y = to_mont(b[i]);
    switch (op) {
        case 0: pr6_mul(&x, &y); break;
        case 1: x = mul_v(x); break;
        case 2: pr6_inv(&x); break;
        case 3: pr6_mul_by_01(&x, &y.c0, &y.c1); break;
        case 4: pr6_mul_by_1(&x, &y.c1); break;
        case 7: x = add(x, y); break;
        default: x = sub(x, y); break;                              // op 8
    }
    out[i] = from_mont(x);
}
// Fp2T<Fp> with the whole value in one lane, as decoding, the pairing and decryption use it
__global__ __launch_bounds__(PAIRING_THREADS) void k_selftest_fp2(int op, const Fp2 *__restrict__ a, const Fp2 *__restrict__ b, Fp2 *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fp2 x = to_mont(a[i]), y = to_mont(b[i]);
    Fp2 r;
    switch (op) {
        case 0: r = mul(x, y); break;
        case 1: r = sqr(x); break;
        case 2: r = inv(x); break;
        case 3: r = conj(x); break;
        case 4: r = f2inv(x); break;
        case 5: r = mul_xi(x); break;
        case 6: r = f2half(x); break;
        case 7: r = add(x, y); break;
        case 8: r = sub(x, y); break;
        case 9: r = mul_fp(x, y.c0); break;
        case 10: r = neg(x); break;
        case 11: r = dbl(x); break;
        case 12: r.c0 = fp_half(x.c0); r.c1 = fp_half(x.c1); break;
        default: r.c0 = fp_inv_chain(x.c0); r.c1 = fp_inv_chain(x.c1); break;      // op 13
    }
    out[i] = from_mont(r);
}
int pairing_selftest_tower(vsp_ctx *ctx, int level, int op, const void *d_a, const void *d_b, void *d_out, size_t n) {
    const dim3 blocks((unsigned)((n + PAIRING_THREADS - 1) / PAIRING_THREADS)), threads(PAIRING_THREADS);
    if (level == 12) hipLaunchKernelGGL(k_selftest_fp12, blocks, threads, 0, ctx->stream, op, (const Fp12 *)d_a, (const Fp12 *)d_b, (Fp12 *)d_out, n);
    else if (level == 6) hipLaunchKernelGGL(k_selftest_fp6, blocks, threads, 0, ctx->stream, op, (const Fp6 *)d_a, (const Fp6 *)d_b, (Fp6 *)d_out, n);
    else hipLaunchKernelGGL(k_selftest_fp2, blocks, threads, 0, ctx->stream, op, (const Fp2 *)d_a, (const Fp2 *)d_b, (Fp2 *)d_out, n);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// products of one piece: option "pairing_chunk" (a test hook as well), 1 .. 2^14, and at most 2^16 pairs (m <= 2^16: the export refuses more)
static size_t pairing_piece(const vsp_ctx *ctx, size_t m) {
    const long v = opt(ctx, "pairing_chunk", (long)PAIRING_CHUNK);
    size_t piece = v < 1 ? 1 : ((size_t)v > PAIRING_CHUNK ? PAIRING_CHUNK : (size_t)v);
    if (piece * m > PAIRING_MAX_PAIRS) piece = PAIRING_MAX_PAIRS / m ? PAIRING_MAX_PAIRS / m : 1;
    return piece;
}
static int pairing_workspace(vsp_ctx *ctx, size_t m, size_t n) {
    VSP_TRY(ensure(ctx, ctx->pair_g1, n * m * sizeof(G1Affine)));
    VSP_TRY(ensure(ctx, ctx->pair_g2, n * m * sizeof(G2Affine)));
    VSP_TRY(ensure(ctx, ctx->pair_status, n * m + n + n));          // pairs | products | result bytes
    VSP_TRY(ensure(ctx, ctx->pair_ml, n * m * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->pair_prod, n * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->pair_gt, n * sizeof(Fp12)));
    return VSP_OK;
}
// stages 1 to 3 over the n products of m pairs in ctx->pair_g1 / pair_g2 / pair_status; the result bytes land at pair_status + n m + n,
// the GT values (when want_gt) in ctx->pair_gt
static int pairing_stages(vsp_ctx *ctx, size_t m, size_t n, const Fp12 *d_expect, bool want_gt) {
    hipStream_t st = ctx->stream;
    const size_t pairs = n * m;
    uint8_t *status = (uint8_t *)ctx->pair_status.p, *pstatus = status + pairs, *result = pstatus + n;
    VSP_TRY(ctx->pair_timer.mark(ctx, 0, st));
    hipLaunchKernelGGL(k_miller, dim3((unsigned)((pairs + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, st, (const G1Affine *)ctx->pair_g1.p,
                       (const G2Affine *)ctx->pair_g2.p, pairs, (Fp12 *)ctx->pair_ml.p);
    VSP_LAUNCH_CHECK();
    const Fp12 *prod = (const Fp12 *)ctx->pair_ml.p;
    const uint8_t *ps = status;
    const unsigned blocks = (unsigned)((n + PAIRING_THREADS - 1) / PAIRING_THREADS);
    if (m > 1) {
        hipLaunchKernelGGL(k_gt_product, dim3(blocks), dim3(PAIRING_THREADS), 0, st, prod, (const uint8_t *)status, m, n, (Fp12 *)ctx->pair_prod.p, pstatus);
        VSP_LAUNCH_CHECK();
        prod = (const Fp12 *)ctx->pair_prod.p; ps = pstatus;
    }
    VSP_TRY(ctx->pair_timer.mark(ctx, 1, st));
    hipLaunchKernelGGL(k_final_exp, dim3(blocks), dim3(PAIRING_THREADS), 0, st, prod, ps, n, d_expect ? (size_t)0 : n, d_expect, want_gt ? (Fp12 *)ctx->pair_gt.p : (Fp12 *)nullptr, result);
    VSP_LAUNCH_CHECK();
    VSP_TRY(ctx->pair_timer.mark(ctx, 2, st));
    return VSP_OK;
}
static void pairing_add_times(vsp_ctx *ctx) {
    ctx->pair_timer.add(ctx, 0, "pairing_miller_ms");
    ctx->pair_timer.add(ctx, 1, "pairing_finalexp_ms");
}
int pairing_miller(vsp_ctx *ctx, const void *d_g1, const void *d_g2, size_t n, void *d_out) {
    hipLaunchKernelGGL(k_miller, dim3((unsigned)((n + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, ctx->stream, (const G1Affine *)d_g1,
                       (const G2Affine *)d_g2, n, (Fp12 *)d_out);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
int pairing_final_exp(vsp_ctx *ctx, const void *d_miller, size_t n, void *d_gt_out, uint8_t *d_is_one_out) {
    hipLaunchKernelGGL(k_final_exp, dim3((unsigned)((n + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, ctx->stream, (const Fp12 *)d_miller,
                       (const uint8_t *)nullptr, n, n, (const Fp12 *)nullptr, (Fp12 *)d_gt_out, d_is_one_out);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
// the proof members of a piece: c proofs from proof `at` on, with L scalars each, laid out A | B | C | scalars at dst (device words)
struct ProofArgs { uint64_t *A, *B, *C; uint32_t *scalars; };
static size_t proof_words(size_t c, size_t L) { return c * (48 + 4 * L); }
static int upload_proofs(vsp_ctx *ctx, uint64_t *dst, const uint64_t *A, const uint64_t *B, const uint64_t *C, const uint64_t *scalars, size_t at, size_t c, size_t L,
                         ProofArgs &d) {
    hipStream_t st = ctx->stream;
    d.A = dst; d.B = d.A + c * 12; d.C = d.B + c * 24; d.scalars = (uint32_t *)(d.C + c * 12);
    VSP_HIP(hipMemcpyAsync(d.A, A + at * 12, c * 12 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemcpyAsync(d.B, B + at * 24, c * 24 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VSP_HIP(hipMemcpyAsync(d.C, C + at * 12, c * 12 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    if (L) VSP_HIP(hipMemcpyAsync(d.scalars, scalars + at * L * 4, c * L * 4 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    return VSP_OK;
}

int pairing_multi_batch(vsp_ctx *ctx, const uint64_t *g1, const uint64_t *g2, size_t m, size_t n, uint8_t *gt_out, uint8_t *is_one_out) {
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t piece = pairing_piece(ctx, m);
    for (size_t at = 0; at < n; at += piece) {
        const size_t c = n - at < piece ? n - at : piece, pairs = c * m;
        VSP_TRY(pairing_workspace(ctx, m, c));
        VSP_TRY(ensure(ctx, ctx->pair_raw, pairs * 36 * sizeof(uint64_t) + 16));
        uint64_t *raw1 = (uint64_t *)ctx->pair_raw.p, *raw2 = raw1 + pairs * 12;
        uint32_t *flag = (uint32_t *)(raw2 + pairs * 24);
        VSP_HIP(hipMemcpyAsync(raw1, g1 + at * m * 12, pairs * 12 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemcpyAsync(raw2, g2 + at * m * 24, pairs * 24 * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemsetAsync(flag, 0, sizeof(uint32_t), st));
        hipLaunchKernelGGL(k_pair_check, dim3((unsigned)((pairs + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, st, raw1, raw2, pairs,
                           (G1Affine *)ctx->pair_g1.p, (G2Affine *)ctx->pair_g2.p, (uint8_t *)ctx->pair_status.p, flag);
        VSP_LAUNCH_CHECK();
        uint32_t h_flag = 0;
        VSP_HIP(hipMemcpyAsync(&h_flag, flag, sizeof h_flag, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        if (h_flag) return set_error(ctx, VSP_ERR_ARG, h_flag & 1u ? "multi_pairing_batch: a coordinate is not below p" : "multi_pairing_batch: a point is not on its curve");
        VSP_TRY(pairing_stages(ctx, m, c, nullptr, gt_out != nullptr));
        if (gt_out) VSP_HIP(hipMemcpyAsync(gt_out + at * 576, ctx->pair_gt.p, c * 576, hipMemcpyDeviceToHost, st));
        if (is_one_out) VSP_HIP(hipMemcpyAsync(is_one_out + at, (const uint8_t *)ctx->pair_status.p + pairs + c, c, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        pairing_add_times(ctx);
    }
    return VSP_OK;
}

void pairing_vk_free(vsp_ctx *ctx, vsp_vk *vk) {
    if (!vk) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    delete vk;
}

vsp_vk *pairing_vk_create(vsp_ctx *ctx, const uint64_t *alpha_g1, const uint64_t *beta_g2, const uint64_t *gamma_g2, const uint64_t *delta_g2, const uint64_t *gamma_abc_g1,
                          size_t n_abc) {
    if (!affine_valid<G1>(alpha_g1) || !affine_valid<G2>(beta_g2) || !affine_valid<G2>(gamma_g2) || !affine_valid<G2>(delta_g2)) {
        set_error(ctx, VSP_ERR_ARG, "vk_create: a point is not canonical or not on its curve"); return nullptr;
    }
    for (size_t i = 0; i < n_abc; i++)
        if (!affine_valid<G1>(gamma_abc_g1 + 12 * i)) { set_error(ctx, VSP_ERR_ARG, "vk_create: a gamma_ABC point is not canonical or not on the curve"); return nullptr; }
    std::unique_ptr<vsp_vk> vk(new vsp_vk());               // every failure below is behind a wait for the stream, or before anything is queued over vk
    vk->n_abc = n_abc;
    auto fail = [&](const char *msg) { set_error(ctx, VSP_ERR_HIP, msg); return (vsp_vk *)nullptr; };
    if (pairing_multi_batch(ctx, alpha_g1, beta_g2, 1, 1, vk->alpha_beta, nullptr) != VSP_OK) return nullptr;
    HFp12 e; memcpy(&e, vk->alpha_beta, sizeof e); e = to_mont(e);                       // HFp12 and Fp12: the same bytes
    Affine<HFp2> ng[2] = {host_load_affine<HFp2>(gamma_g2), host_load_affine<HFp2>(delta_g2)};
    for (auto &q : ng) q.y = neg(q.y);                                                   // infinity stays x = y = 0
    // d * G_i for d = 0 .. 15
    std::vector<Affine<HFp>> tab(n_abc * 16);
    host_parallel_for(n_abc, [&](size_t i) {
        const Affine<HFp> g = host_load_affine<HFp>(gamma_abc_g1 + 12 * i);
        XYZZ<HFp> acc = XYZZ<HFp>::inf();
        tab[i * 16].x = HFp::zero(); tab[i * 16].y = HFp::zero();
        for (int d = 1; d < 16; d++) { xyzz_madd(acc, g); tab[i * 16 + d] = xyzz_to_affine(acc); }
    });
    if (vk->d_expect.alloc(sizeof e) != hipSuccess || vk->d_neg.alloc(sizeof ng) != hipSuccess ||
        vk->d_tab.alloc(tab.size() * sizeof(Affine<HFp>)) != hipSuccess) return fail("vk_create: hipMalloc failed");
    if (hipMemcpyAsync(vk->d_expect.p, &e, sizeof e, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(vk->d_neg.p, ng, sizeof ng, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(vk->d_tab.p, tab.data(), tab.size() * sizeof(Affine<HFp>), hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) return fail("vk_create: upload failed");
    return vk.release();
}
const uint8_t *pairing_vk_alpha_beta(const vsp_vk *vk) { return vk->alpha_beta; }
size_t pairing_vk_n_abc(const vsp_vk *vk) { return vk->n_abc; }

int pairing_verify_batch(vsp_ctx *ctx, const vsp_vk *vk, const uint64_t *inputs, const uint64_t *A, const uint64_t *B, const uint64_t *C, size_t n, uint8_t *verdict_out) {
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t L = vk->n_abc - 1, piece = pairing_piece(ctx, 3);
    for (size_t at = 0; at < n; at += piece) {
        const size_t c = n - at < piece ? n - at : piece;
        VSP_TRY(pairing_workspace(ctx, 3, c));
        VSP_TRY(ensure(ctx, ctx->pair_raw, proof_words(c, L) * sizeof(uint64_t)));
        ProofArgs d;
        VSP_TRY(upload_proofs(ctx, (uint64_t *)ctx->pair_raw.p, A, B, C, inputs, at, c, L, d));
        hipLaunchKernelGGL(k_verify_prepare, dim3((unsigned)((c + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, st, d.A, d.B, d.C, d.scalars, c,
                           vk->n_abc, vk->d_tab.as<const G1Affine>(), vk->d_neg.as<const G2Affine>(), (G1Affine *)ctx->pair_g1.p, (G2Affine *)ctx->pair_g2.p,
                           (uint8_t *)ctx->pair_status.p);
        VSP_LAUNCH_CHECK();
        VSP_TRY(pairing_stages(ctx, 3, c, vk->d_expect.as<const Fp12>(), false));
        VSP_HIP(hipMemcpyAsync(verdict_out + at, (const uint8_t *)ctx->pair_status.p + 3 * c + c, c, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        pairing_add_times(ctx);
    }
    return VSP_OK;
}

// ---- SAVER ballot verdicts
void saver_verifier_free(vsp_ctx *ctx, vsp_saver_verifier *ver) {
    if (!ver) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    delete ver;
}
size_t saver_verifier_msg_size(const vsp_saver_verifier *ver) { return ver->n; }
size_t saver_verifier_n_rest(const vsp_saver_verifier *ver) { return ver->vk->n_abc - 1 - ver->n; }

vsp_saver_verifier *saver_verifier_create(vsp_ctx *ctx, size_t n, const uint64_t *pk_words, const uint64_t *alpha_g1, const uint64_t *beta_g2, const uint64_t *gamma_g2,
                                          const uint64_t *delta_g2, const uint64_t *gamma_abc_g1, size_t n_abc) {
    const uint64_t *t_g2 = pk_words + 12 + 24 * n;                   // delta_g1 | delta_s_g1 [n] | t_g1 [n] | t_g2 [n + 1] | two sums (saver.hip)
    for (size_t j = 0; j <= n; j++)
        if (!affine_valid<G2>(t_g2 + 24 * j)) { set_error(ctx, VSP_ERR_ARG, "saver_verifier_create: a t_g2 point is not canonical or not on its curve"); return nullptr; }
    vsp_vk *vk = pairing_vk_create(ctx, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc);      // validates the Groth16 key
    if (!vk) return nullptr;
    std::unique_ptr<vsp_saver_verifier> ver(new vsp_saver_verifier());
    ver->device = ctx->device; ver->n = n; ver->vk.reset(vk);
    ver->alpha_g1 = host_load_affine<HFp>(alpha_g1);
    std::vector<Affine<HFp2>> q(n + 5);
    for (size_t j = 0; j <= n; j++) q[j] = host_load_affine<HFp2>(t_g2 + 24 * j);
    q[n + 1] = host_load_affine<HFp2>(G2::GEN);
    q[n + 2] = host_load_affine<HFp2>(gamma_g2);
    q[n + 3] = host_load_affine<HFp2>(delta_g2);
    q[n + 4] = host_load_affine<HFp2>(beta_g2);
    for (size_t j = n + 1; j < n + 4; j++) q[j].y = neg(q[j].y);                                        // infinity stays x = y = 0
    std::vector<LineCoeffs<HFp>> lines(q.size() * MILLER_LINES);                                        // LineCoeffs<HFp> and <Fp>: the same bytes
    host_parallel_for(q.size(), [&](size_t j) { prepare_g2(q[j], lines.data() + j * MILLER_LINES); });
    const size_t bytes = lines.size() * sizeof(LineCoeffs<HFp>);
    if (ver->d_lines.alloc(bytes) != hipSuccess || hipMemcpyAsync(ver->d_lines.p, lines.data(), bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
        set_error(ctx, VSP_ERR_HIP, "saver_verifier_create: the prepared lines could not be uploaded");
        hipStreamSynchronize(ctx->stream);                               // `lines` and the handle go
        return nullptr;
    }
    return ver.release();
}

int saver_piece_prepare(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t at, size_t c, StageTimer &timer) {
    hipStream_t st = ctx->stream;
    const size_t n = ver->n, L = ver->vk->n_abc - 1 - n;
    VSP_TRY(ensure(ctx, ctx->pair_g1, (n + 5) * c * sizeof(G1Affine)));                              // n + 4 prepared-side arguments, then A
    VSP_TRY(ensure(ctx, ctx->pair_g2, c * sizeof(G2Affine)));
    VSP_TRY(ensure(ctx, ctx->pair_status, 3 * c));                                                   // malformed | equation 1 | equation 2
    G1Affine *pts = (G1Affine *)ctx->pair_g1.p, *a_pts = pts + (n + 4) * c;
    if (src.dev) {
        // a range of a decoded piece: nothing to upload
        VSP_TRY(timer.mark(ctx, 0, st));
        VSP_TRY(receive_piece_prepare(ctx, ver, *src.dev, at - src.dev->base, c, pts, a_pts, ctx->pair_g2.p, (uint8_t *)ctx->pair_status.p));
        VSP_TRY(timer.mark(ctx, 1, st));
        return VSP_OK;
    }
    const size_t ct_words = c * (n + 2) * 12;
    VSP_TRY(ensure(ctx, ctx->pair_raw, (ct_words + proof_words(c, L)) * sizeof(uint64_t)));
    uint64_t *d_ct = (uint64_t *)ctx->pair_raw.p;
    VSP_HIP(hipMemcpyAsync(d_ct, src.ct + at * (n + 2) * 12, ct_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    ProofArgs d;
    VSP_TRY(upload_proofs(ctx, d_ct + ct_words, src.A, src.B, src.C, src.rest, at, c, L, d));
    VSP_TRY(timer.mark(ctx, 0, st));
    hipLaunchKernelGGL(k_ballot_prepare, dim3((unsigned)((c + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, st, d_ct, d.scalars, d.A, d.B, d.C, c, n,
                       ver->vk->n_abc, ver->vk->d_tab.as<const G1Affine>(), pts, a_pts, (G2Affine *)ctx->pair_g2.p, (uint8_t *)ctx->pair_status.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(timer.mark(ctx, 1, st));
    return VSP_OK;
}

// the exact verdicts of a prepared piece of c ballots (what saver_piece_prepare left, events 0 and 1 of ctx->saver_timer around it):
// the Miller groups of G pairs, their products, both final exponentiations in one launch and the read-back
static int saver_piece_judge(vsp_ctx *ctx, const vsp_saver_verifier *ver, size_t c, size_t G, size_t ng, bool from_device, std::vector<uint8_t> &flags, uint8_t *verdict_out,
                             uint8_t *reason_out) {
    hipStream_t st = ctx->stream;
    const size_t n = ver->n;
    VSP_TRY(ensure(ctx, ctx->pair_ml, (ng + 1) * c * sizeof(Fp12)));
    VSP_TRY(ensure(ctx, ctx->pair_prod, 2 * c * sizeof(Fp12)));
    G1Affine *pts = (G1Affine *)ctx->pair_g1.p, *a_pts = pts + (n + 4) * c;
    uint8_t *status = (uint8_t *)ctx->pair_status.p;
    const unsigned blocks = (unsigned)((c + PAIRING_THREADS - 1) / PAIRING_THREADS);
    hipLaunchKernelGGL(k_miller_ballot, dim3(blocks, (unsigned)(ng + 1)), dim3(PAIRING_THREADS), 0, st, (const G1Affine *)pts, (const G1Affine *)a_pts,
                       (const G2Affine *)ctx->pair_g2.p, ver->d_lines.as<const LineCoeffs<Fp>>(), c, n, G, ng, (Fp12 *)ctx->pair_ml.p);
    VSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_ballot_product, dim3(blocks), dim3(PAIRING_THREADS), 0, st, (const Fp12 *)ctx->pair_ml.p, c, ng, (Fp12 *)ctx->pair_prod.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(ctx->saver_timer.mark(ctx, 2, st));
    // both final exponentiations of a piece in one launch: flag[i] for i < c says "equation 1 of ballot i holds" (the value is one),
    // for i >= c "equation 2 of ballot i - c holds" (the value is the key's e(alpha, beta))
    hipLaunchKernelGGL(k_final_exp, dim3((unsigned)((2 * c + PAIRING_THREADS - 1) / PAIRING_THREADS)), dim3(PAIRING_THREADS), 0, st, (const Fp12 *)ctx->pair_prod.p,
                       (const uint8_t *)nullptr, 2 * c, c, ver->vk->d_expect.as<const Fp12>(), (Fp12 *)nullptr, status + c);
    VSP_LAUNCH_CHECK();
    VSP_TRY(ctx->saver_timer.mark(ctx, 3, st));
    flags.resize(3 * c);
    VSP_HIP(hipMemcpyAsync(flags.data(), status, 3 * c, hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < c; k++) {
        const uint8_t reason = flags[k] ? 1 : (uint8_t)((flags[c + k] ? 0 : 2) | (flags[2 * c + k] ? 0 : 4));
        verdict_out[k] = reason == 0;
        if (reason_out) reason_out[k] = reason;
    }
    static const char *const names[3] = {"saver_verify_prepare_ms", "saver_verify_miller_ms", "saver_verify_finalexp_ms"};
    for (int i = 0; i < 3; i++) ctx->saver_timer.add(ctx, i, names[i]);
    if (from_device) ctx->saver_timer.add(ctx, 0, "saver_receive_prepare_ms");
    return VSP_OK;
}

// ballots of one piece: "pairing_chunk" as for the pairings, and at most 2^19 G1 arguments (a ballot has n + 5; never split)
size_t saver_exact_piece(const vsp_ctx *ctx, size_t n) {
    size_t piece = pairing_piece(ctx, 1);
    if (piece * (n + 5) > SAVER_MAX_ARGS) piece = SAVER_MAX_ARGS / (n + 5);
    return piece;
}

int saver_verify_source(vsp_ctx *ctx, const vsp_saver_verifier *ver, const BallotSource &src, size_t first, size_t count, uint8_t *verdict_out, uint8_t *reason_out) {
    if (ver->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch: the verifier belongs to another device");
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t n = ver->n, piece = saver_exact_piece(ctx, n);
    // groups of the ciphertext equation: option "saver_verify_group" pairs each
    const long gv = opt(ctx, "saver_verify_group", 9);
    const size_t G = gv < 1 ? 1 : ((size_t)gv > n + 2 ? n + 2 : (size_t)gv), ng = (n + 2 + G - 1) / G;
    std::vector<uint8_t> flags;
    for (size_t at = 0; at < count; at += piece) {
        const size_t c = count - at < piece ? count - at : piece;
        VSP_TRY(saver_piece_prepare(ctx, ver, src, first + at, c, ctx->saver_timer));
        VSP_TRY(saver_piece_judge(ctx, ver, c, G, ng, src.dev != nullptr, flags, verdict_out + at, reason_out ? reason_out + at : nullptr));
    }
    return VSP_OK;
}
int saver_verify_batch(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *rest, const uint64_t *A, const uint64_t *B, const uint64_t *C, size_t count,
                       uint8_t *verdict_out, uint8_t *reason_out) {
    BallotSource src;
    src.ct = ct; src.rest = rest; src.A = A; src.B = B; src.C = C;
    return saver_verify_source(ctx, ver, src, 0, count, verdict_out, reason_out);
}

}  // namespace vsp
