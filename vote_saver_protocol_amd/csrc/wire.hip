// Wire formats of the artefacts that cross the prover's boundary: the big-endian blobs of the reference's
// marshaling_policy (bin/cli/include/nil/vote_saver/common.hpp:168-203: option::big_endian; proof / primary input / ciphertext
// written at :462-485, the proving key read INSIDE the timed vote phase at :749-754 and :1002-1004).
//
// The marshalling code itself lives in absent submodules (crypto3-marshalling-*, /root/reference/.gitmodules:35-44), so only what the
// reference's own files show is pinned; everything else is a stated guess kept in ONE place (this file):
//   pinned    * proof = A | B | C, ZCash-compressed, 48 + 96 + 48 bytes                      bin/cli/src/data.bin[0:192)
//             * scalar vectors = 8-byte count, then 32-byte field elements                     protocol_exec.ipynb cell 0 / 20 (fr_size = 32,
//               (eid / sn / rt blobs: "eid[std_size_t_size * 2:]", sizes eid_len * fr_size)    std_size_t_size = 8) -- big-endian per common.hpp:180
//             * extended verification key starts: 4 bytes, then a GT element as 12 x 48-byte   data.bin[192:196), [196:772): satisfies g^r = 1
//               LITTLE-endian Fp (tower order c0.c0.c0, c0.c0.c1, c0.c1.c0, ...), then two      under the test-side pairing; [772:868), [868:964)
//               compressed G2 points and one compressed G1 point                               decode as G2, [964:1012) as G1, all in the subgroup
//   guesses   * the roles gamma_g2, delta_g2, delta_g1 of those three points; the tail of the key (gamma_ABC_g1 as a counted vector of
//               compressed G1, then gamma_g1): data.bin is zero from byte 1012 on
//             * ciphertext = counted vector of compressed G1 (by analogy with the scalar vectors)
//             * "fast" proving key = UNCOMPRESSED big-endian affine points (ZCash uncompressed form: no square root on load, which is
//               what makes it fast), fixed elements alpha_g1 beta_g1 beta_g2 delta_g1 delta_g2, then A_query, B_query (pairs G2 | G1),
//               H_query, L_query as counted vectors.  Upstream's key also embeds the constraint system; here it travels separately
//               (vsp_r1cs_upload), because circuit construction is out of scope.
// The proving-key loader is the part with a cost: the reference parses ~0.6 GB per vote at 2^20 constraints.  vsp_pk_from_blob copies the
// raw bytes to the GPU once and converts there (byte order, infinity flags, curve check, Montgomery form, the 28-bit-limb table).
// The ZCash point compression every compressed element goes through (vsp_g1/g2_compress, vsp_g1/g2_decompress) is here too, written
// once for both groups.
#include "common.h"

namespace vsp {

// ZCash uncompressed records -> canonical affine points (infinity flag -> all zero).  flag bit 2: a record is malformed -- it claims to be
// compressed (0x80), carries the sign bit that only the compressed form has (0x20), or is an infinity record (0x40) with a non-zero payload
__device__ __forceinline__ bool record_rest_zero(const uint32_t *w, unsigned words) {
    uint32_t acc = w[0] & ~0xFFu;                              // everything but the flag byte
    for (unsigned j = 1; j < words; j++) acc |= w[j];
    return acc == 0 && (w[0] & 0x3Fu) == 0;
}
__global__ __launch_bounds__(256) void k_g1_from_be(const uint8_t *src, size_t stride, size_t n, G1Affine *out, uint32_t *flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *w = (const uint32_t *)(src + i * stride);
    const uint32_t head = w[0] & 0xFFu;                       // first byte of the record
    G1Affine p;
    if (head & 0xA0u) atomicOr(flag, 4u);
    if (head & 0x40u) { p.x = Fp::zero(); p.y = Fp::zero(); if (!record_rest_zero(w, 24)) atomicOr(flag, 4u); }
    else { p.x = fp_from_be(w, true); p.y = fp_from_be(w + 12, false); }
    out[i] = p;
}
__global__ __launch_bounds__(256) void k_g2_from_be(const uint8_t *src, size_t stride, size_t n, G2Affine *out, uint32_t *flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t *w = (const uint32_t *)(src + i * stride);
    const uint32_t head = w[0] & 0xFFu;
    G2Affine p;
    if (head & 0xA0u) atomicOr(flag, 4u);
    if (head & 0x40u) { p.x.c0 = p.x.c1 = p.y.c0 = p.y.c1 = Fp::zero(); if (!record_rest_zero(w, 48)) atomicOr(flag, 4u); }
    else { p.x.c1 = fp_from_be(w, true); p.x.c0 = fp_from_be(w + 12, false); p.y.c1 = fp_from_be(w + 24, false); p.y.c0 = fp_from_be(w + 36, false); }
    out[i] = p;
}

static void put_be64(uint8_t *o, uint64_t v) { for (int i = 0; i < 8; i++) o[i] = (uint8_t)(v >> (56 - 8 * i)); }
static uint64_t get_be64(const uint8_t *p) { uint64_t v = 0; for (int i = 0; i < 8; i++) v = (v << 8) | p[i]; return v; }
// one coordinate of group G (G::AFFINE_WORDS / 2 canonical words; G2: c0 | c1) <-> its big-endian bytes, the highest coefficient first (G2: c1 | c0)
template <class G> static void coord_to_be(uint8_t *o, const uint64_t *l) {
    constexpr int m = (int)G::AFFINE_WORDS / 12;
    for (int c = 0; c < m; c++) be_from_limbs(o + 48 * c, l + 6 * (m - 1 - c), 6);
}
template <class G> static void coord_from_be(uint64_t *l, const uint8_t *o) {
    constexpr int m = (int)G::AFFINE_WORDS / 12;
    for (int c = 0; c < m; c++) limbs_from_be(l + 6 * (m - 1 - c), o + 48 * c, 6);
}
// ZCash uncompressed record: x | y big-endian, infinity = the flag 0x40 and nothing else
template <class G> static void uncompressed(uint8_t *o, const uint64_t *p) {
    constexpr size_t half = G::AFFINE_WORDS / 2;
    if (limbs_zero(p, (int)G::AFFINE_WORDS)) { memset(o, 0, 16 * half); o[0] = 0x40; return; }
    coord_to_be<G>(o, p); coord_to_be<G>(o + 8 * half, p + half);
}

// ---- ZCash compressed encoding (the wire format of reference bin/cli/src/data.bin[0:192)): x big-endian with three flag bits in its
// first byte -- 0x80 compressed, 0x40 infinity (every other bit clear), 0x20 y is the larger of y and -y
static const uint64_t HALF_P[6] = {0xdcff7fffffffd555ULL, 0x0f55ffff58a9ffffULL, 0xb39869507b587b12ULL, 0xb23ba5c279c2895fULL, 0x258dd3db21a5d66bULL, 0x0d0088f51cbff34dULL};
static bool fp_lex_larger(const uint64_t *y) {      // y > (p-1)/2
    for (int i = 5; i >= 0; i--) { if (y[i] > HALF_P[i]) return true; if (y[i] < HALF_P[i]) return false; }
    return false;
}
// y larger than -y: its highest non-zero coefficient (G1: y itself) above (p - 1) / 2
template <class G> static bool y_larger(const uint64_t *y) {
    int c = (int)G::AFFINE_WORDS / 12 - 1;
    while (c > 0 && limbs_zero(y + 6 * c, 6)) c--;
    return fp_lex_larger(y + 6 * c);
}
// VSP_ERR_ARG for a null pointer or a coordinate that is not canonical (>= p: its top bits would collide with the flag bits)
template <class G> static int compress(const uint64_t *affine, uint8_t *out) {
    constexpr size_t half = G::AFFINE_WORDS / 2;
    if (!affine || !out) return VSP_ERR_ARG;
    if (limbs_zero(affine, (int)G::AFFINE_WORDS)) { memset(out, 0, 8 * half); out[0] = 0xC0; return VSP_OK; }
    if (!coords_below_p(affine, G::AFFINE_WORDS)) return VSP_ERR_ARG;
    coord_to_be<G>(out, affine);
    out[0] |= 0x80;
    if (y_larger<G>(affine + half)) out[0] |= 0x20;
    return VSP_OK;
}

// ---- decompression (the inverse of the above): x from the big-endian bytes, y = sqrt(x^3 + b) with the sign the flag names ----
// a^((p+1)/4) -- the square root when a is a quadratic residue (p = 3 mod 4); returns false when it is not
static bool fp_sqrt(const HFp &a, HFp &out) {
    uint64_t e[6]; uint64_t carry = 1;                         // e = (p + 1) / 4
    for (int i = 0; i < 6; i++) { uint64_t v = FpP64::MOD[i] + carry; carry = (v < carry) ? 1 : 0; e[i] = v; }
    for (int i = 0; i < 6; i++) e[i] = (e[i] >> 2) | (i < 5 ? e[i + 1] << 62 : 0);
    out = pow_limbs(a, e, 6);
    return eq(sqr(out), a);
}
// square root in Fp2 = Fp[u]/(u^2+1) by the norm: returns false when a is not a square
static bool fp_sqrt(const HFp2 &a, HFp2 &out) {
    if (is_zero(a.c1)) {
        HFp r;
        if (fp_sqrt(a.c0, r)) { out.c0 = r; out.c1 = HFp::zero(); return true; }
        if (fp_sqrt(neg(a.c0), r)) { out.c0 = HFp::zero(); out.c1 = r; return true; }   // (r u)^2 = -r^2
        return false;
    }
    HFp s;
    if (!fp_sqrt(add(sqr(a.c0), sqr(a.c1)), s)) return false;
    uint64_t two4[6] = {2, 0, 0, 0, 0, 0};
    HFp half = inv(host_load_canon<HFp>(two4));
    HFp t = mul(add(a.c0, s), half), x0;
    if (!fp_sqrt(t, x0)) { t = mul(sub(a.c0, s), half); if (!fp_sqrt(t, x0)) return false; }
    out.c0 = x0; out.c1 = mul(mul(a.c1, half), inv(x0));
    return eq(sqr(out), a);
}
template <class G> static int decompress(const uint8_t *in, int check_subgroup, uint64_t *out_affine, int *out_is_inf) {
    using HF = typename G::HF;
    constexpr size_t half = G::AFFINE_WORDS / 2, bytes = 8 * half;
    if (!in || !out_affine) return VSP_ERR_ARG;
    if (!(in[0] & 0x80)) return VSP_ERR_ARG;                       // uncompressed form is not accepted
    uint8_t buf[bytes]; memcpy(buf, in, bytes); buf[0] &= 0x1f;
    if (in[0] & 0x40) {                                            // infinity: every other bit must be clear
        for (size_t i = 0; i < bytes; i++) if (buf[i]) return VSP_ERR_ARG;
        if (in[0] & 0x20) return VSP_ERR_ARG;
        memset(out_affine, 0, 2 * bytes); if (out_is_inf) *out_is_inf = 1; return VSP_OK;
    }
    uint64_t xy[G::AFFINE_WORDS];                                  // canonical x | y
    coord_from_be<G>(xy, buf);
    if (!coords_below_p(xy, half)) return VSP_ERR_ARG;
    Affine<HF> p; p.x = host_load_canon<HF>(xy);
    if (!fp_sqrt(add(mul(sqr(p.x), p.x), curve_b<HF>()), p.y)) return VSP_ERR_ARG;      // not on the curve
    host_store_canon(xy + half, p.y);
    if (y_larger<G>(xy + half) != ((in[0] & 0x20) != 0)) { p.y = neg(p.y); host_store_canon(xy + half, p.y); }
    if (check_subgroup && !is_inf(xyzz_mul_scalar(xyzz_from_affine(p), FrP64::MOD, 255))) return VSP_ERR_ARG;
    memcpy(out_affine, xy, 2 * bytes);
    if (out_is_inf) *out_is_inf = 0;
    return VSP_OK;
}

}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_g1_compress(const uint64_t affine[12], uint8_t out[48]) { return compress<G1>(affine, out); }
int vsp_g2_compress(const uint64_t affine[24], uint8_t out[96]) { return compress<G2>(affine, out); }
int vsp_g1_decompress(const uint8_t in[48], int check_subgroup, uint64_t out_affine[12], int *out_is_inf) { return decompress<G1>(in, check_subgroup, out_affine, out_is_inf); }
int vsp_g2_decompress(const uint8_t in[96], int check_subgroup, uint64_t out_affine[24], int *out_is_inf) { return decompress<G2>(in, check_subgroup, out_affine, out_is_inf); }

// ---- scalar vectors (primary input, eid / sn / rt, voting result): common.hpp:476-485, 529-535 --------------------------------------
size_t vsp_fr_vector_blob_size(size_t count) { return 8 + 32 * count; }
int vsp_fr_vector_to_blob(const uint64_t *vals, size_t count, uint8_t *out) {
    if ((!vals && count) || !out) return VSP_ERR_ARG;
    for (size_t i = 0; i < count; i++) if (!below_mod<FrP64>(vals + 4 * i)) return VSP_ERR_ARG;
    put_be64(out, count);
    for (size_t i = 0; i < count; i++) be_from_limbs(out + 8 + 32 * i, vals + 4 * i, 4);
    return VSP_OK;
}
int vsp_fr_vector_from_blob(const uint8_t *blob, size_t len, uint64_t *vals_out, size_t capacity, size_t *count_out) {
    if (!blob || len < 8 || !count_out) return VSP_ERR_ARG;
    uint64_t n = get_be64(blob);
    if (n > (len - 8) / 32 || len != 8 + 32 * n) return VSP_ERR_ARG;
    *count_out = (size_t)n;
    if (!vals_out) return VSP_OK;                                  // size query
    if (capacity < n) return VSP_ERR_ARG;
    for (size_t i = 0; i < n; i++) { limbs_from_be(vals_out + 4 * i, blob + 8 + 32 * i, 4); if (!below_mod<FrP64>(vals_out + 4 * i)) return VSP_ERR_ARG; }
    return VSP_OK;
}

// ---- G1 vectors (the ciphertext, r1cs_gg_ppzksnark_encrypted_primary_input: common.hpp:471-474, 773-781) ----------------------------
size_t vsp_g1_vector_blob_size(size_t count) { return 8 + 48 * count; }
int vsp_g1_vector_to_blob(const uint64_t *pts, size_t count, uint8_t *out) {
    if ((!pts && count) || !out) return VSP_ERR_ARG;
    put_be64(out, count);
    for (size_t i = 0; i < count; i++) if (vsp_g1_compress(pts + 12 * i, out + 8 + 48 * i) != VSP_OK) return VSP_ERR_ARG;
    return VSP_OK;
}
int vsp_g1_vector_from_blob(const uint8_t *blob, size_t len, int check_subgroup, uint64_t *pts_out, size_t capacity, size_t *count_out) {
    if (!blob || len < 8 || !count_out) return VSP_ERR_ARG;
    uint64_t n = get_be64(blob);
    if (n > (len - 8) / 48 || len != 8 + 48 * n) return VSP_ERR_ARG;
    *count_out = (size_t)n;
    if (!pts_out) return VSP_OK;
    if (capacity < n) return VSP_ERR_ARG;
    for (size_t i = 0; i < n; i++) { int inf; if (vsp_g1_decompress(blob + 8 + 48 * i, check_subgroup, pts_out + 12 * i, &inf) != VSP_OK) return VSP_ERR_ARG; }
    return VSP_OK;
}

// ---- proof (r1cs_gg_ppzksnark_proof: common.hpp:467-469) -- the layout of data.bin[0:192) ------------------------------------------
int vsp_proof_from_blob(const uint8_t blob[192], int check_subgroup, uint64_t A[12], uint64_t B[24], uint64_t C[12]) {
    if (!blob || !A || !B || !C) return VSP_ERR_ARG;
    int inf;
    if (vsp_g1_decompress(blob, check_subgroup, A, &inf) != VSP_OK || vsp_g2_decompress(blob + 48, check_subgroup, B, &inf) != VSP_OK ||
        vsp_g1_decompress(blob + 144, check_subgroup, C, &inf) != VSP_OK) return VSP_ERR_ARG;
    return VSP_OK;
}
int vsp_proof_to_blob(const uint64_t A[12], const uint64_t B[24], const uint64_t C[12], uint8_t out[192]) {
    if (!A || !B || !C || !out) return VSP_ERR_ARG;
    if (vsp_g1_compress(A, out) != VSP_OK || vsp_g2_compress(B, out + 48) != VSP_OK || vsp_g1_compress(C, out + 144) != VSP_OK) return VSP_ERR_ARG;
    return VSP_OK;
}

// ---- extended verification key (r1cs_gg_ppzksnark_extended_verification_key: common.hpp:183-185) -----------------------------------
// head (4) | alpha_g1_beta_g2 (576, opaque here: the pairing lives on the verifier side) | gamma_g2 (96) | delta_g2 (96) | delta_g1 (48) |
// count (8) | gamma_ABC_g1 (count x 48) | gamma_g1 (48)
size_t vsp_vk_blob_size(size_t n_abc) { return 4 + 576 + 96 + 96 + 48 + 8 + 48 * n_abc + 48; }
int vsp_vk_to_blob(uint32_t head, const uint8_t gt[576], const uint64_t gamma_g2[24], const uint64_t delta_g2[24], const uint64_t delta_g1[12],
                   const uint64_t *gamma_abc_g1, size_t n_abc, const uint64_t gamma_g1[12], uint8_t *out) {
    if (!gt || !gamma_g2 || !delta_g2 || !delta_g1 || (!gamma_abc_g1 && n_abc) || !gamma_g1 || !out) return VSP_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = (uint8_t)(head >> (24 - 8 * i));
    memcpy(out + 4, gt, 576);
    uint8_t *p = out + 580;
    if (vsp_g2_compress(gamma_g2, p) != VSP_OK || vsp_g2_compress(delta_g2, p + 96) != VSP_OK || vsp_g1_compress(delta_g1, p + 192) != VSP_OK) return VSP_ERR_ARG;
    put_be64(p + 240, n_abc);
    for (size_t i = 0; i < n_abc; i++) if (vsp_g1_compress(gamma_abc_g1 + 12 * i, p + 248 + 48 * i) != VSP_OK) return VSP_ERR_ARG;
    if (vsp_g1_compress(gamma_g1, p + 248 + 48 * n_abc) != VSP_OK) return VSP_ERR_ARG;
    return VSP_OK;
}
int vsp_vk_from_blob(const uint8_t *blob, size_t len, int check_subgroup, uint32_t *head, uint8_t gt[576], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                     uint64_t delta_g1[12], uint64_t *gamma_abc_g1, size_t capacity, size_t *n_abc, uint64_t gamma_g1[12]) {
    if (!blob || len < vsp_vk_blob_size(0) || !n_abc) return VSP_ERR_ARG;
    const uint8_t *p = blob + 580;
    uint64_t n = get_be64(p + 240);
    if (n > (len - vsp_vk_blob_size(0)) / 48 || len != vsp_vk_blob_size((size_t)n)) return VSP_ERR_ARG;
    *n_abc = (size_t)n;
    if (head) *head = ((uint32_t)blob[0] << 24) | ((uint32_t)blob[1] << 16) | ((uint32_t)blob[2] << 8) | blob[3];
    if (gt) memcpy(gt, blob + 4, 576);
    int inf;
    if (gamma_g2 && vsp_g2_decompress(p, check_subgroup, gamma_g2, &inf) != VSP_OK) return VSP_ERR_ARG;
    if (delta_g2 && vsp_g2_decompress(p + 96, check_subgroup, delta_g2, &inf) != VSP_OK) return VSP_ERR_ARG;
    if (delta_g1 && vsp_g1_decompress(p + 192, check_subgroup, delta_g1, &inf) != VSP_OK) return VSP_ERR_ARG;
    if (gamma_abc_g1) {
        if (capacity < n) return VSP_ERR_ARG;
        for (size_t i = 0; i < n; i++) if (vsp_g1_decompress(p + 248 + 48 * i, check_subgroup, gamma_abc_g1 + 12 * i, &inf) != VSP_OK) return VSP_ERR_ARG;
    }
    if (gamma_g1 && vsp_g1_decompress(p + 248 + 48 * n, check_subgroup, gamma_g1, &inf) != VSP_OK) return VSP_ERR_ARG;
    return VSP_OK;
}

// ---- proving key (r1cs_gg_ppzksnark_fast_proving_key: common.hpp:186-188, read at :749-754 inside the timed vote phase) -------------
// alpha_g1 (96) beta_g1 (96) beta_g2 (192) delta_g1 (96) delta_g2 (192) | count A (8) A_query (x 96) | count B (8) B_query (x (192 + 96)) |
// count H (8) H_query (x 96) | count L (8) L_query (x 96)
static const size_t PK_FIXED = 96 + 96 + 192 + 96 + 192;
size_t vsp_pk_blob_size(const vsp_keypair *kp) {
    if (!kp) return 0;
    return PK_FIXED + 8 + 96 * kp->q[0]->n + 8 + 288 * kp->q[2]->n + 8 + 96 * kp->q[3]->n + 8 + 96 * kp->q[4]->n;
}
int vsp_pk_to_blob(vsp_ctx *ctx, const vsp_keypair *kp, uint8_t *out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!kp || !out) return set_error(ctx, VSP_ERR_ARG, "pk_to_blob: null argument");
    if (kp->q[1]->n != kp->q[2]->n) return set_error(ctx, VSP_ERR_ARG, "pk_to_blob: B_query halves differ in length");
    uint8_t *p = out;
    uncompressed<G1>(p, kp->alpha_g1); uncompressed<G1>(p + 96, kp->beta_g1); uncompressed<G2>(p + 192, kp->beta_g2);
    uncompressed<G1>(p + 384, kp->delta_g1); uncompressed<G2>(p + 480, kp->delta_g2);
    p += PK_FIXED;
    std::vector<uint64_t> a, b;
    auto g1_section = [&](int which) -> int {
        size_t n = kp->q[which]->n;
        a.resize(12 * (n ? n : 1));
        VSP_TRY(vsp_keypair_export(ctx, kp, which, a.data()));
        put_be64(p, n); p += 8;
        for (size_t i = 0; i < n; i++) uncompressed<G1>(p + 96 * i, a.data() + 12 * i);
        p += 96 * n;
        return VSP_OK;
    };
    VSP_TRY(g1_section(0));
    {
        size_t n = kp->q[2]->n;
        a.resize(12 * (n ? n : 1)); b.resize(24 * (n ? n : 1));
        VSP_TRY(vsp_keypair_export(ctx, kp, 1, a.data())); VSP_TRY(vsp_keypair_export(ctx, kp, 2, b.data()));
        put_be64(p, n); p += 8;
        for (size_t i = 0; i < n; i++) { uncompressed<G2>(p + 288 * i, b.data() + 24 * i); uncompressed<G1>(p + 288 * i + 192, a.data() + 12 * i); }
        p += 288 * n;
    }
    VSP_TRY(g1_section(3));
    VSP_TRY(g1_section(4));
    return VSP_OK;
}

vsp_keypair *vsp_pk_from_blob(vsp_ctx *ctx, const uint8_t *blob, size_t len, int precompute) {
    if (!ctx) return nullptr;
    auto fail = [&](const char *msg) -> vsp_keypair * { if (msg) set_error(ctx, VSP_ERR_ARG, msg); return nullptr; };
    if (!blob || len < PK_FIXED + 32) return fail("pk_from_blob: blob too short");
    // section table from the counts (all offsets are multiples of 8)
    size_t off = PK_FIXED, cnt[4], at[4];
    const size_t rec[4] = {96, 288, 96, 96};
    for (int s = 0; s < 4; s++) {
        if (off + 8 > len) return fail("pk_from_blob: truncated");
        uint64_t n = get_be64(blob + off); off += 8;
        if (n > (len - off) / rec[s]) return fail("pk_from_blob: a count exceeds the blob");
        cnt[s] = (size_t)n; at[s] = off; off += rec[s] * cnt[s];
    }
    if (off != len) return fail("pk_from_blob: trailing bytes");
    if (hipSetDevice(ctx->device) != hipSuccess) return fail("pk_from_blob: device");
    hipStream_t st = ctx->stream;
    DevBuf raw, pts;
    size_t maxn = 1; for (int s = 0; s < 4; s++) if (cnt[s] > maxn) maxn = cnt[s];
    if (raw.alloc(len) != hipSuccess || pts.alloc(maxn * sizeof(G2Affine)) != hipSuccess || ensure(ctx, ctx->val_flag, 16) != VSP_OK) {
        set_error(ctx, VSP_ERR_NOMEM, "pk_from_blob: hipMalloc failed"); return nullptr;
    }
    void *d_raw = raw.p, *d_pts = pts.p;
    vsp_keypair *kp = new vsp_keypair();
    memset(kp->gamma_g2, 0, sizeof kp->gamma_g2); memset(kp->gamma_g1, 0, sizeof kp->gamma_g1);
    bool ok = hipMemcpyAsync(d_raw, blob, len, hipMemcpyHostToDevice, st) == hipSuccess && hipMemsetAsync(ctx->val_flag.p, 0, 16, st) == hipSuccess;
    // which query each section feeds: A -> q0, B -> q2 (G2, record offset 0) and q1 (G1, record offset 192), H -> q3, L -> q4
    struct Part { int sec; size_t shift; int group; int q; } parts[5] = {{0, 0, 1, 0}, {1, 192, 1, 1}, {1, 0, 2, 2}, {2, 0, 1, 3}, {3, 0, 1, 4}};
    for (int k = 0; k < 5 && ok; k++) {
        const Part &pt = parts[k];
        size_t n = cnt[pt.sec];
        unsigned blk = (unsigned)((n + 255) / 256);
        const uint8_t *src = (const uint8_t *)d_raw + at[pt.sec] + pt.shift;
        if (n) {
            if (pt.group == 1) hipLaunchKernelGGL(k_g1_from_be, dim3(blk), dim3(256), 0, st, src, rec[pt.sec], n, (G1Affine *)d_pts, (uint32_t *)ctx->val_flag.p);
            else hipLaunchKernelGGL(k_g2_from_be, dim3(blk), dim3(256), 0, st, src, rec[pt.sec], n, (G2Affine *)d_pts, (uint32_t *)ctx->val_flag.p);
            uint32_t h_flag = 0;
            ok = hipMemcpyAsync(&h_flag, ctx->val_flag.p, 4, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
            if (ok && h_flag) { set_error(ctx, VSP_ERR_ARG, "pk_from_blob: a point record is not a well-formed uncompressed record (compressed form, stray flag bits, or an infinity record with a payload)"); ok = false; break; }
        }
        if (ok) {
            // curve check, Montgomery form, 28-bit table; wire bytes are caller data: the endomorphism layout only after the subgroup check
            // (a query that gets window multiples below never uses that layout: BASES_TRANSIENT skips the layout and its check)
            const bool pre_this = ((precompute & 1) && pt.q != 3) || ((precompute >> (pt.q + 1)) & 1);
            ok = bases_create(ctx, pt.group, d_pts, true, n, pre_this ? BASES_TRANSIENT : BASES_CALLER, &kp->q[pt.q]) == VSP_OK;
        }
    }
    hipStreamSynchronize(st);
    raw.reset(); pts.reset();               // before the window multiples are built: the raw blob (0.6 GB at 2^20 constraints) is no longer needed
    // precompute: the bit mask of vsp_groth16_generate -- bit 0 = the recommended set A, B(G1), B(G2), L (H stays plain); bits 1..5 = A, B(G1), B(G2), H, L
    for (int i = 0; i < 5 && ok; i++) {
        const bool pre_this = ((precompute & 1) && i != 3) || ((precompute >> (i + 1)) & 1);
        if (pre_this) ok = vsp_bases_precompute(ctx, kp->q[i], 0) == VSP_OK;
    }
    if (ok) {
        // the five single elements on the host (uncompressed records; infinity is not a valid key element)
        // (each validated: coordinates below p, on the curve)
        auto load = [&](auto g, const uint8_t *p, uint64_t *o) {
            using G = decltype(g);
            if (p[0] & 0xC0) return false;
            coord_from_be<G>(o, p); coord_from_be<G>(o + G::AFFINE_WORDS / 2, p + 4 * G::AFFINE_WORDS);
            return affine_valid<G>(o);
        };
        ok = load(G1{}, blob, kp->alpha_g1) && load(G1{}, blob + 96, kp->beta_g1) && load(G2{}, blob + 192, kp->beta_g2) && load(G1{}, blob + 384, kp->delta_g1) &&
             load(G2{}, blob + 480, kp->delta_g2);
        if (!ok) set_error(ctx, VSP_ERR_ARG, "pk_from_blob: a fixed key element is not a curve point in uncompressed form");
    }
    if (ok) {
        kp->pk = vsp_pk_create(ctx, kp->alpha_g1, kp->beta_g1, kp->beta_g2, kp->delta_g1, kp->delta_g2, kp->q[0], kp->q[1], kp->q[2], kp->q[3], kp->q[4]);
        ok = kp->pk != nullptr;
    }
    if (!ok) { vsp_keypair_free(ctx, kp); return nullptr; }
    return kp;
}

}  // extern "C"
