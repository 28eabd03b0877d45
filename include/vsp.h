/* vsp.h -- C ABI of the MI355X-native Groth16 prover hot path (libvsp_hip.so).
 *
 * Drop-in boundary for the one compute-heavy path of NilFoundation/vote-saver-protocol: the
 * r1cs_gg_ppzksnark prover that runs below
 *     bin/cli/include/nil/vote_saver/common.hpp:1132-1135   (encrypt<elgamal_verifiable<bls12_381>, ...>)
 * whose two hot loops are crypto3-algebra `multiexp` (included via common.hpp:38) and crypto3-math
 * `evaluation_domain` (absent submodules, .gitmodules:8-9,47-48).  The reference has no FFI for
 * this path (header-only C++ templates); its only C ABI convention is the WASM shell
 * (bin/cli/src/wasm.cpp:32-44,62-201): POD pointer+size buffers, blocking calls.  This header keeps
 * that convention, with two deliberate differences: every buffer is CALLER-owned,
 * and failures are returned as negative status codes instead of aborting the process
 * (reference: BOOST_ASSERT -> std::exit(1), bin/cli/src/main.cpp:24-33).
 *
 * Data layout at the boundary (host or device memory, see each function):
 *   Fr scalar        4 x uint64  canonical (non-Montgomery) little-endian limbs, value < r
 *   Fp element       6 x uint64  canonical little-endian limbs, value < p
 *   G1 affine point 12 x uint64  x, y                      -- infinity = all 96 bytes zero
 *   G2 affine point 24 x uint64  x.c0, x.c1, y.c0, y.c1    -- infinity = all 192 bytes zero
 *   G1 Jacobian     18 x uint64  X, Y, Z (x = X/Z^2, y = Y/Z^3; Z = 0 infinity); G2: 36 x uint64
 * No torch types, no C++ types: plain pointers and sizes.
 *
 * Threading: a vsp_ctx is used by one thread at a time (the reference is single-threaded,
 * bin/cli/CMakeLists.txt:114-116); different contexts are independent.  All calls block until the
 * result is in the caller's buffer unless the name ends in _async.
 */
#ifndef VSP_H
#define VSP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsp_ctx vsp_ctx;
typedef struct vsp_bases vsp_bases;     /* device-resident MSM bases (a slice of the proving key) */
typedef struct vsp_r1cs vsp_r1cs;       /* device-resident constraint system (three CSR matrices) */
typedef struct vsp_pk vsp_pk;           /* device-resident Groth16 proving key */

enum {
    VSP_OK = 0,
    VSP_ERR_ARG = -1,        /* null pointer, size out of range, scalar/coordinate layout violated: a scalar >= r (reported when the
                              * multi-exponentiation / proof finishes), a base coordinate >= p or a base off the curve (at upload) */
    VSP_ERR_HIP = -2,        /* a HIP runtime call failed; vsp_last_error() has the text */
    VSP_ERR_NOMEM = -3,
    VSP_ERR_UNSUPPORTED = -4, /* e.g. log_m > 28 */
    VSP_ERR_UNSATISFIED = -5  /* option "prove_check_witness": a witness does not satisfy the constraint system; no proof was written for it */
};

/* ---- context ------------------------------------------------------------------------------- */
/* One context = one GPU (device_ordinal) + one HIP stream + grow-only device workspaces. */
vsp_ctx *vsp_create(int device_ordinal);
void vsp_destroy(vsp_ctx *ctx);
const char *vsp_last_error(vsp_ctx *ctx);
/* Run on a caller-provided hipStream_t (e.g. torch.cuda.Stream().cuda_stream); NULL = context's own. */
int vsp_set_stream(vsp_ctx *ctx, void *hip_stream);
int vsp_synchronize(vsp_ctx *ctx);
/* Named timing/diagnostic values of the last calls, e.g. "msm_accum_ms" (HIP-event time of the bucket
 * accumulation kernel, summed since the last vsp_stats_reset), "msm_accum_launches", "msm_window_bits". */
double vsp_get_stat(vsp_ctx *ctx, const char *name);
void vsp_stats_reset(vsp_ctx *ctx);
/* options: "bases_check_curve" (default 1: uploads verify y^2 = x^3 + b for every point; coordinates < p are always checked),
 * "bases_check_subgroup" (the endomorphism split below relies on phi(P) = lambda P, which holds only in the order-r subgroup, while
 * the curve equation also admits points with a cofactor component.  1, the default: an upload that would use the split checks
 * phi(P) = lambda P for every point on the GPU (126 doublings + 11 additions per point, 20-30 ms for 2^20 G1 points, once per key);
 * bases that fail keep the plain layout, over which sum k_i P_i is exact for ANY curve point -- as the reference's generic multiexp is
 * -- and vsp_get_stat("bases_outside_subgroup") counts them.  2: every upload is checked and one that fails is refused with
 * VSP_ERR_ARG.  0: never checked, and then never split unless "msm_glv" = 2.  Keys made by vsp_groth16_generate are multiples of the
 * generators and need no check; the bases of one vsp_msm_g1 / vsp_msm_g2 call are never split, hence never checked),
 * "msm_census_sync" (1: every multi-exponentiation waits for its own 0/1 census before planning; default 0: a slot plans from the
 * count it saw for the previous vector of the same length -- the count steers window size and part length, never the result);
 * "msm_glv" (default 1: plain resident bases keep phi(P) = (beta x, y) = lambda P beside every P in the 28-bit-limb table -- 2 x 128
 * (G1) / 2 x 256 (G2) bytes per point -- and every scalar is split k = k1 + k2 lambda into two signed 127-bit halves: half as many windows,
 * i.e. half the bucket sets to reduce -- applied while the doubled table stays within 256 MB for G1 (2^20 points) / 128 MB for G2
 * (2^18 points): beyond that the measurements favour the plain layout; 2 forces it for any size AND skips the subgroup check -- the caller
 * vouches that every base is in the order-r subgroup, else results are wrong; 0 before an upload keeps the plain layout);
 * tuning knobs: "msm_window_bits" (0 = automatic), "msm_split" (bucket split threshold), "prove_h_first" (1: queue witness_map and
 * the H multi-exponentiation before the witness ones), "msm_fp28" (1: bases are kept a second time on 14 x 28-bit limbs for the
 * accumulation kernel -- 128 (G1) / 256 (G2) bytes per point (cache-line rows) on top of the 96 / 192; 0 before an upload / precomputation leaves that copy out and the
 * 12 x 32-bit kernel runs), "prove_plan_first" (1: the witness vectors' digit sorts are queued before witness_map),
 * "prove_host_threads" (default 1: the prover's host steps -- the four multiples of delta, the Horner chain over each multi-exponentiation's
 * window results, s*A and r*B1 -- run on host threads of their own inside the wait for the GPU; 0: on the calling thread, one after the other),
 * "generate_precompute_window" (8..22; 0 = by the query's size: the window of the tables vsp_groth16_generate builds when `precompute` asks for them),
 * "prove_fixed_base" (default 1: the multiples of delta every proof needs come from fixed-base tables of 32 x 255 multiples per group,
 * built on the host by the first proof over a key -- at most 32 additions per multiple; 0: double-and-add),
 * "prove_batch_share_plan" (default 1: in vsp_groth16_prove_batch the B1 and B2 multi-exponentiations take A's digit sort and bucket plan --
 * the three multiply by the same witness vectors; 0: each sorts for itself),
 * "witness_map_batched" (default 1: the three transforms of every step of witness_map -- 3 K in a batch of K proofs -- in one launch per
 * pass and the pointwise step inside the last transform's first pass, basic domains on the 29-bit butterflies; 0: transform by transform,
 * proof by proof), "msm_dimsum_lanes" (8/16/32/64 lanes per bucket-digit sum; 0 = chosen by the library),
 * "msm_dimsum_maxw" (256..4096, default 1024: waves the per-digit lane plan of the bucket reduction may fill; 2048 = two per SIMD),
 * "msm_dimsum_prefetch" (1: the bucket reduction requests the next bucket before the current addition; default 0, it spills),
 * "msm_dimsum_dense" (default 1: one-lane fields fold the bucket-digit sums in 256-thread blocks whose tree levels are packed onto the
 * waves that have live additions; 0: one wave per block, masked tree levels; vsp_get_stat "msm_dimsum_dense_launches" counts the launches
 * of the packed kernel), "msm_dimbits" (1 / 0: the last
 * step of the bucket reduction as plain subset sums folded by the host's doubling chain / as weighted sums on the GPU; default by group),
 * "msm_slot_normal_priority" (1 before the first use of a work slot: its stream gets the context's priority instead of the lowest --
 * faster single proofs, slower independent multi-exponentiations in flight), "ntt_fr29" (default 1: butterflies on
 * 9 x 29-bit limbs; 0: the 8 x 32-bit kernel); diagnostics: every context checks its hand-laid-out field routines THROUGH the kernels
 * that use them, against the generic kernels, on data the library generates itself -- vsp_get_stat "msm_fp28_selfcheck_g1" / "_g2"
 * (first 28-bit table of a group) and "ntt_fr29_selfcheck" (first transform): 1 passed, -1 failed (the context then runs the generic
 * kernels for its lifetime and vsp_last_error says so), 0 could not run; "msm_fp28_selfcheck_detail_g1" / "_g2": which leg of the check
 * differed (bit 0 the default pipeline, 1 split buckets / the other last step, 4 / 5 the 6-bit / 12-bit window legs, 2 an unexpected
 * infinity, 3 a failed launch); "msm_fp28" = 2 (diagnostics only: bisecting a failed check) builds the 28-bit table WITHOUT the check;
 * "msm_debug_counts" (1: vsp_get_stat reports "msm_buckets", "msm_parts", "msm_medium_buckets", "msm_heavy_buckets" of the last
 * multi-exponentiation -- a blocking read-back); "msm_sort" (0: by size; 1: never the staged sort of large wide-window problems;
 * 2: the staged sort for every window of 12 bits and more), "msm_wide_windows" (0: never more than 16 bits per window), "msm_fold" (0: 255-bit
 * scalars are not folded to min(k, r - k) where the window width divides 255), "msm_fused_split" (0: the endomorphism split and the digit
 * extraction run as two kernels over the scalars instead of one; vsp_get_stat "msm_glv_split_launches" counts the launches of the split as
 * a kernel of its own -- small problems and windows wider than 16 bits take it under either value), "msm_fused_scans" (0: the bucket
 * scans take three kernels each, as they do above 2^20 buckets; vsp_get_stat "msm_scan3_launches" counts the bucket scans queued that way),
 * "msm_accum28_asm" (default 1: the G1 accumulation over the 28-bit table runs the generated gfx950 loop; 0: its C++ twin k_accum28_cxx,
 * the same additions in the same order -- the only 28-bit accumulation of the portable diagnostic build; vsp_get_stat
 * "msm_accum28_cxx_launches" counts the twin's launches),
 * "prove_witness_streams" (default 1: the prover's four witness multi-exponentiations run as two chains on the two streams the context
 * created first, ahead of every work slot's, so that each chain has a hardware queue to itself; 0: each on its work slot's own stream),
 * "msm_scatter_rounds" (the LDS counting sort places its entries one range of buckets at a time, so that the lines it writes are
 * completed in L2: 0 = as many rounds as the size asks for, n = n rounds, rounded down to a power of two, 32 at most; 1 = a single pass;
 * vsp_get_stat "msm_scatter_rounds": the rounds of the last sort),
 * "prove_check_witness" (default 0; 1: every prover entry point checks its witnesses against the constraint system and refuses the ones
 * that fail -- "witness check" below).
 * Test hooks, never for a caller: "msm_fp28_selfcheck_fault" and "ntt_fr29_selfcheck_fault" (1: the self-check above reports a mismatch
 * it did not find, so that the suite can watch the context fall back to the generic kernels).
 * The names above and the ones the later sections of this header introduce are all there are: vsp_set_option returns VSP_ERR_ARG for any
 * other name, vsp_last_error quotes it, nothing is stored and the context stays usable.  (A name that nothing reads would otherwise be
 * accepted in silence and leave its caller on the default path.)
 *
 * Runtime environment.  Results never depend on it.  GPU_MAX_HW_QUEUES (HIP runtime, read once when the runtime starts; default 4
 * hardware queues per stream priority): one proof's latency does not depend on it (the prover's two chains take their queues when the
 * context is created), but independent multi-exponentiations kept IN FLIGHT TOGETHER over the work slots overlap better with 8
 * (2^20 G1 points, four in flight: 2.86 ms per multi-exponentiation against 3.03 with the default 4; MI355X, ROCm 7.2).  A service that
 * pipelines proofs or multi-exponentiations should export GPU_MAX_HW_QUEUES=8 before the process's first HIP call;
 * vsp_get_stat("runtime_hw_queues_env") is the value this process saw (0: not set).
 *
 * Memory.  vsp_get_stat("device_allocations_live") and ("pinned_allocations_live") are the device and the page-locked host
 * allocations the library holds at this moment, over every context and handle of the process (vsp_dmalloc's are the caller's and not
 * counted).  Diagnostics: a handle that is freed, or a context that is destroyed, takes the counts back to what they were before it. */
int vsp_set_option(vsp_ctx *ctx, const char *name, long value);
/* Diagnostic build only (libvsp_hip_diag.so, `make -C vote_saver_protocol_amd/csrc diag`: the same sources with stamps around the G1
 * accumulation loop -- in the shipped library no stamp executes and this returns VSP_ERR_UNSUPPORTED): the clock the chip held inside
 * that loop since the last reset, delta s_memtime / delta s_memrealtime x 100 MHz summed over waves, and the number of waves. */
int vsp_diag_clock(vsp_ctx *ctx, int reset, double *ghz_out, double *waves_out);
/* The same for the passes of the radix-2 transform on 29-bit limbs (k_ntt29_pass; stamps around a whole pass of every wave). */
int vsp_diag_clock_ntt(vsp_ctx *ctx, int reset, double *ghz_out, double *waves_out);

/* ---- raw device memory helpers (for callers without torch) --------------------------------- */
void *vsp_dmalloc(vsp_ctx *ctx, size_t bytes);
void vsp_dfree(vsp_ctx *ctx, void *dptr);
int vsp_h2d(vsp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int vsp_d2h(vsp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* Page-lock / release caller memory: host buffers the library copies from on every call (the witness of vsp_groth16_prove) then
 * travel by asynchronous DMA instead of the runtime's staged pageable path.  The reference keeps its witness in a std::vector
 * (common.hpp:1110-1128); registering that storage once costs nothing per proof. */
int vsp_host_register(vsp_ctx *ctx, void *ptr, size_t bytes);
int vsp_host_unregister(vsp_ctx *ctx, void *ptr);

/* ---- multi-scalar multiplication: algebra::multiexp<multiexp_method_BDLO12> (a1), ------------
 *      multiexp_with_mixed_addition (a2: zero scalars are skipped, equal-to-one scalars are summed
 *      directly -- both happen inside the same bucket pipeline), G2 half of kc_multiexp (a3).
 * result = sum_i scalars[i] * bases[i], returned as an affine point (out_is_inf = 1 for infinity). */
int vsp_msm_g1(vsp_ctx *ctx, const uint64_t *bases /* host n x 12 */, const uint64_t *scalars /* host n x 4 */,
               size_t n, uint64_t out_affine[12], int *out_is_inf);
int vsp_msm_g2(vsp_ctx *ctx, const uint64_t *bases /* host n x 24 */, const uint64_t *scalars /* host n x 4 */,
               size_t n, uint64_t out_affine[24], int *out_is_inf);

/* Resident bases (proving-key slices, a9): uploaded and converted once, reused by every proof. */
vsp_bases *vsp_bases_upload_g1(vsp_ctx *ctx, const uint64_t *bases /* host n x 12 */, size_t n);
vsp_bases *vsp_bases_upload_g2(vsp_ctx *ctx, const uint64_t *bases /* host n x 24 */, size_t n);
/* bases already in device memory (same canonical layout), e.g. produced by vsp_fixed_base_mul_* */
vsp_bases *vsp_bases_from_device_g1(vsp_ctx *ctx, const void *d_bases, size_t n);
vsp_bases *vsp_bases_from_device_g2(vsp_ctx *ctx, const void *d_bases, size_t n);
/* Optional preprocessing of resident bases (once per proving key): store 2^(c*w) * P for every c-bit window w (c = window_bits,
 * 0 = chosen from the number of bases: 16 from 2^19 bases up), 255/c + 1 slices = 16x the memory at c = 16.  Every multi-exponentiation over these bases then uses ONE shared set of
 * 2^(c-1) buckets for all windows: the bucket reduction shrinks by the number of windows and the work per thread is uniform.
 * Results are identical; sub-range calls (first, n) keep working. */
int vsp_bases_precompute(vsp_ctx *ctx, vsp_bases *b, unsigned window_bits);
/* The same table for bases whose scalars are DENSE (the H query; not witness vectors, whose scalars are mostly 0 / 1): beside every window
 * multiple its image under the curve's endomorphism, for the ceil(128 / c) windows of a split scalar k = k1 + k2 lambda -- the
 * endomorphism split of "msm_glv" over ONE bucket set.  Same memory as the plain table at c = 16 (8 windows x 2 rows instead of 16).
 * Needs the order-r subgroup: bases not yet checked are checked here ("bases_check_subgroup"); bases outside it get the plain table. */
int vsp_bases_precompute_split(vsp_ctx *ctx, vsp_bases *b, unsigned window_bits);
size_t vsp_bases_count(const vsp_bases *b);
/* device memory the handle holds: the Montgomery-form points (or the table of window multiples) plus the 28-bit-limb copy */
size_t vsp_bases_device_bytes(const vsp_bases *b);
void vsp_bases_free(vsp_ctx *ctx, vsp_bases *b);

/* MSM over resident bases [first, first+n) with scalars in DEVICE memory (n x 4 uint64, canonical).
 * out_affine is a host buffer (12 or 24 uint64 according to the group of `bases`). */
int vsp_msm_resident(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n,
                     const void *d_scalars, uint64_t *out_affine, int *out_is_inf);
/* Same, but the result is left as a Jacobian partial sum (X, Y, Z canonical: 18 / 36 uint64) in the host
 * buffer -- the fixed-size record ranks exchange in the sharded multi-GPU MSM. */
/* A BATCH of multi-exponentiations over the same resident bases: `batch` (1..64) scalar vectors of n canonical scalars each, vector k at
 * d_scalars + 32 * k * stride bytes (stride >= n, in scalars), out_affine[k] / out_is_inf[k] = sum_i scalars_k[i] * bases[first + i].
 * One digit sort, one bucket accumulation and one bucket reduction serve all vectors (separate buckets per vector, the same base rows):
 * what a prover of MANY small statements over one key needs -- small multi-exponentiations are bound by the latency of their dependent
 * chains, not by work, and a batch is as wide as its vectors together at the latency of one.  Plain bases: a bucket set per (vector, window);
 * bases with a table of window multiples (windows of at most 16 bits): ONE bucket set per vector -- fewer, larger windows, worth it where
 * the table is small (VSP_ERR_UNSUPPORTED for wider windows, or with option "msm_batch_tables" = 0). */
int vsp_msm_resident_batch(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars, size_t batch, size_t stride,
                           uint64_t *out_affine /* batch x 12 or 24 */, int *out_is_inf /* batch, may be NULL */);
int vsp_msm_resident_jacobian(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n,
                              const void *d_scalars, uint64_t *out_jacobian);
/* Pipelined form: vsp_msm_launch enqueues the whole multi-exponentiation on work slot `slot` (0..5; slot 0 runs on the
 * context's stream, the others on streams of their own) and returns once the GPU work is queued; vsp_msm_finish_jacobian
 * waits for that slot and returns the Jacobian record.  Several slots may be in flight, so the latency-bound tail of one
 * multi-exponentiation overlaps the bulk of the next (the prover runs its five this way).  The scalars must be complete in
 * device memory before the launch and must not change until the finish. */
int vsp_msm_launch(vsp_ctx *ctx, unsigned slot, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars);
int vsp_msm_finish_jacobian(vsp_ctx *ctx, unsigned slot, uint64_t *out_jacobian);
/* Same, but the record is left in DEVICE memory at d_out_jacobian (18 / 36 uint64) -- where the RCCL all-gather of the sharded
 * multi-exponentiation reads it.  The record is completed on the host (the last c * W doublings of a multi-exponentiation
 * are one dependent chain, ~50x faster on a CPU core than on a GPU lane), written to a pinned ring entry of the slot and copied by an
 * asynchronous DMA queued on hip_stream (a hipStream_t; NULL = the context's stream): the call returns without waiting for the copy, and
 * anything queued on hip_stream afterwards sees the record. */
int vsp_msm_finish_jacobian_device(vsp_ctx *ctx, unsigned slot, void *d_out_jacobian, void *hip_stream);

/* Fold `count` Jacobian records (host, canonical) into one affine point; group: 1 = G1, 2 = G2. */
int vsp_fold_jacobian(vsp_ctx *ctx, int group, const uint64_t *records, size_t count,
                      uint64_t *out_affine, int *out_is_inf);
/* Same over records in DEVICE memory (the all-gather's output): copied to a pinned buffer behind whatever hip_stream (NULL = the
 * context's stream) already holds, that stream is waited for, the fold runs on the host.  count <= 4096. */
int vsp_fold_jacobian_device(vsp_ctx *ctx, int group, const void *d_records, size_t count, void *hip_stream,
                             uint64_t *out_affine, int *out_is_inf);

/* ---- evaluation_domain<Fr> (a6): basic radix-2 domain of size m = 2^log_m ------------------
 * In-place on n = 2^log_m canonical Fr values.
 *   inverse = 0, coset_g = NULL : fft          a[k] <- sum_j a[j] w^(jk),  w = 7^((r-1)/2^32)^(2^(32-log_m))
 *   inverse = 1, coset_g = NULL : inverse_fft  (w^-1, then scale by m^-1)
 *   inverse = 0, coset_g = g    : coset fft    (a[j] *= g^j first)
 *   inverse = 1, coset_g = g    : inverse coset fft (inverse_fft, then a[j] *= g^-j) */
int vsp_ntt_fr(vsp_ctx *ctx, uint64_t *a /* host m x 4 */, unsigned log_m, int inverse, const uint64_t coset_g[4]);
int vsp_ntt_fr_device(vsp_ctx *ctx, void *d_a /* device m x 4 */, unsigned log_m, int inverse, const uint64_t coset_g[4]);

/* ---- r1cs_to_qap::witness_map (a7) -----------------------------------------------------------
 * From the three evaluation vectors Az, Bz, Cz over the domain (each m x 4, canonical, zero padded; the
 * caller has already placed the "input_i * 0 = 0" rows in Az) compute the m coefficients of
 * H = (A*B - C)/Z  (d1 = d2 = d3 = 0, as the r1cs_gg_ppzksnark prover calls it).  Inputs are overwritten. */
int vsp_witness_map_h(vsp_ctx *ctx, uint64_t *Az, uint64_t *Bz, uint64_t *Cz /* host */, unsigned log_m,
                      uint64_t *H /* host m x 4 */);
int vsp_witness_map_h_device(vsp_ctx *ctx, void *d_Az, void *d_Bz, void *d_Cz, unsigned log_m, void *d_H);

/* ---- evaluation_domain<Fr> handles (a6): make_evaluation_domain, basic_radix2_domain, step_radix2_domain -----------------
 * Replaces crypto3-math math/domains/evaluation_domain.hpp (abstract m, fft, inverse_fft, evaluate_all_lagrange_polynomials,
 * get_domain_element, compute_vanishing_polynomial, add_poly_z, divide_by_z_on_coset), basic_radix2_domain.hpp,
 * step_radix2_domain.hpp and math/algorithms/make_evaluation_domain.hpp (absent submodule, /root/reference/.gitmodules:47-48),
 * which r1cs_to_qap reaches from bin/cli/include/nil/vote_saver/common.hpp:916-917 and :1132-1135.
 * vsp_domain_create(min_size) makes the choice make_evaluation_domain makes: the basic radix-2 domain when min_size is a power of
 * two, else the step radix-2 domain of size big + small (big = 2^(ceil_log2(min_size)-1), small = the next power of two of
 * min_size - big), which is again basic when small == big.  extended_radix2 (m = 2^33 for this field) and the
 * arithmetic/geometric sequence domains (Fr defines no such generators) cannot be selected for any size up to 2^28.
 * Element order of a step domain: the big-th roots of unity w^(2i), then w * (small-th roots), w of order 2 big.
 * NULL is returned (vsp_last_error tells why) for min_size <= 1 or > 2^28.  A domain belongs to the context's device. */
typedef struct vsp_domain vsp_domain;
vsp_domain *vsp_domain_create(vsp_ctx *ctx, size_t min_size);
void vsp_domain_free(vsp_ctx *ctx, vsp_domain *dom);
size_t vsp_domain_size(const vsp_domain *dom);                 /* m */
int vsp_domain_kind(const vsp_domain *dom);                    /* 0 basic_radix2, 1 step_radix2 */
/* fft / inverse_fft / coset variants, in place on m canonical values (same flags as vsp_ntt_fr) */
int vsp_domain_fft(vsp_ctx *ctx, const vsp_domain *dom, uint64_t *a /* host m x 4 */, int inverse, const uint64_t coset_g[4]);
int vsp_domain_fft_device(vsp_ctx *ctx, const vsp_domain *dom, void *d_a /* device m x 4 */, int inverse, const uint64_t coset_g[4]);
/* evaluate_all_lagrange_polynomials(t): out[i] = L_i(t), m values (the indicator vector when t lies in the domain) */
int vsp_domain_lagrange(vsp_ctx *ctx, const vsp_domain *dom, const uint64_t t[4], uint64_t *out /* host m x 4 */);
int vsp_domain_element(vsp_ctx *ctx, const vsp_domain *dom, size_t idx, uint64_t out[4]);            /* get_domain_element */
int vsp_domain_vanishing(vsp_ctx *ctx, const vsp_domain *dom, const uint64_t t[4], uint64_t out[4]);  /* compute_vanishing_polynomial */
int vsp_domain_add_poly_z(vsp_ctx *ctx, const vsp_domain *dom, const uint64_t coeff[4], uint64_t *H /* host (m+1) x 4 */);
/* divide_by_z_on_coset: P[i] /= Z(g x_i) with g the field's multiplicative generator 7 */
int vsp_domain_divide_by_z_on_coset(vsp_ctx *ctx, const vsp_domain *dom, uint64_t *P /* host m x 4 */);
/* witness_map over a domain handle (vsp_witness_map_h is the basic radix-2 case) */
int vsp_domain_witness_map_h(vsp_ctx *ctx, const vsp_domain *dom, uint64_t *Az, uint64_t *Bz, uint64_t *Cz, uint64_t *H /* host m x 4 each */);

/* ---- constraint system + proving key + prover (a8, a9) -------------------------------------- */
/* Three CSR matrices over columns 0..num_vars (column 0 is the constant 1); coefficients canonical Fr. */
vsp_r1cs *vsp_r1cs_upload(vsp_ctx *ctx, size_t num_constraints, size_t num_inputs, size_t num_vars,
                          const uint32_t *row_ptr_a, const uint32_t *col_a, const uint64_t *coef_a,
                          const uint32_t *row_ptr_b, const uint32_t *col_b, const uint64_t *coef_b,
                          const uint32_t *row_ptr_c, const uint32_t *col_c, const uint64_t *coef_c);
void vsp_r1cs_free(vsp_ctx *ctx, vsp_r1cs *cs);
/* the domain r1cs_to_qap uses for this system: make_evaluation_domain(num_constraints + num_inputs + 1); H_query has size - 1 bases */
size_t vsp_r1cs_domain_size(const vsp_r1cs *cs);
int vsp_r1cs_domain_kind(const vsp_r1cs *cs);                  /* 0 basic_radix2, 1 step_radix2 */

/* ---- witness check: bp.is_satisfied(), the gate in front of the prover (common.hpp:1109-1128) ---------------------------------
 * Does z = (1, witness) satisfy (A z)[i] (B z)[i] = (C z)[i] in Fr for every row i < num_constraints?  vsp_r1cs_check_batch answers for
 * `count` witnesses (num_vars x 4 words each, one after the other) with one status byte per witness:
 *     0      satisfied
 *     bit 0  the witness holds a value that is not canonical (>= r), in a wire of a constraint or in one that no constraint names
 *     bit 1  some constraint does not hold
 * first_bad_row_out[k] (may be NULL) is the lowest failing row of witness k, or num_constraints when none fails; bad_rows_out[k] (may be
 * NULL) the number of failing rows.  Both are deterministic.  For a witness with bit 0 the rows are judged on the value reduced mod r:
 * bit 1, first_bad_row and bad_rows are then unspecified beyond first_bad_row <= num_constraints and bad_rows <= num_constraints.  Rows
 * num_constraints .. m - 1 of the domain (the "input_i * 0 = 0" rows, the padding) are not part of the system and are not checked; a
 * system with num_constraints = 0 is satisfied by every canonical witness.
 * The return value is VSP_OK whatever the verdicts are: VSP_ERR_ARG is for a null pointer (also with count = 0) and for a context with a
 * proof in flight (the check uses the prover's workspace), VSP_ERR_HIP as elsewhere.  vsp_r1cs_is_satisfied is the same path with count = 1:
 * *satisfied_out = 1 exactly when the status byte is 0.
 * The check runs the prover's own front half -- the same upload, the same three sparse mat-vecs -- and then one pass over A z, B z, C z
 * (k_r1cs_verdict: one field product per row), so what it approves is word for word what the prover consumes.  Any count: the witnesses
 * go through the device in pieces of at most 64, the batch prover's limit.  Workspace bound per piece: 64 x (num_vars + 1) x 32 bytes of
 * z and 64 x 3 m x 32 bytes of A z, B z, C z (m = vsp_r1cs_domain_size) -- the workspaces of vsp_groth16_prove_batch, nothing beyond them
 * whatever count is -- plus 768 bytes of verdict records.  The call's copy of the witnesses is zeroed before it returns.  Stage times (HIP
 * events, summed since vsp_stats_reset): vsp_get_stat "r1cs_check_ms" (the verdict kernels), "r1cs_check_front_ms" (upload and mat-vecs).
 *
 * Inside the prover: option "prove_check_witness" = 1 queues the same pass between the mat-vecs and witness_map in vsp_groth16_prove,
 * vsp_groth16_prove_launch, vsp_groth16_prove_launch_packed, vsp_saver_encrypt and vsp_groth16_prove_batch(_launch).  The verdict
 * travels to page-locked memory by an asynchronous copy and is read by the finish after its existing waits: no wait is added.
 *   single proof  an unsatisfied witness makes the finish (and the blocking call) return VSP_ERR_UNSATISFIED; A_out, B_out, C_out, proof_out
 *                 (and vsp_saver_encrypt's ct_out) are all zero, vsp_last_error names the first failing row and vsp_get_stat
 *                 ("prove_first_bad_row") reports it (num_constraints after a satisfied witness).  The context is ready for the next proof.
 *   batch         every satisfied member's outputs are byte-identical to the ones without the option, every unsatisfied member's are all
 *                 zero, and the finish returns VSP_ERR_UNSATISFIED if any member failed.  vsp_groth16_prove_batch_verdicts then tells
 *                 which: status_out[k] (count bytes) is 0 or bit 1 as above, first_bad_row_out[k] (may be NULL) the member's first failing
 *                 row or num_constraints.  It speaks of the last batch that FINISHED on this context with the option set (the verdicts
 *                 survive from the launch to the finish and until the next batch finishes); VSP_ERR_ARG if there is none.
 * The GPU work of an unsatisfied witness is NOT skipped: the verdict is known only when the finish reads it, by which time every kernel
 * is queued.  A value >= r keeps returning VSP_ERR_ARG from the finish, as without the option (the multi-exponentiations' census finds
 * it; for a batch, for the whole batch), and takes precedence over VSP_ERR_UNSATISFIED.  With the option 0 nothing is checked: an
 * unsatisfying witness yields VSP_OK and a well-formed proof that no verifier accepts. */
int vsp_r1cs_check_batch(vsp_ctx *ctx, const vsp_r1cs *cs, const uint64_t *witnesses /* host count x num_vars x 4 */, size_t count,
                         uint8_t *status_out /* count */, uint64_t *first_bad_row_out /* count, may be NULL */,
                         uint64_t *bad_rows_out /* count, may be NULL */);
int vsp_r1cs_is_satisfied(vsp_ctx *ctx, const vsp_r1cs *cs, const uint64_t *witness, int *satisfied_out, uint64_t *first_bad_row_out /* may be NULL */);
int vsp_groth16_prove_batch_verdicts(vsp_ctx *ctx, uint8_t *status_out /* count */, uint64_t *first_bad_row_out /* count, may be NULL */);

/* Proving key = { alpha_g1, beta_g1, beta_g2, delta_g1, delta_g2, A_query[num_vars+1],
 * B_query (G2 and G1 halves, num_vars+1 each), H_query[m-1], L_query[num_vars-num_inputs] }
 * (proof_system::proving_key_type, common.hpp:173,749-754).  Query handles stay owned by the caller. */
vsp_pk *vsp_pk_create(vsp_ctx *ctx, const uint64_t alpha_g1[12], const uint64_t beta_g1[12], const uint64_t beta_g2[24],
                      const uint64_t delta_g1[12], const uint64_t delta_g2[24],
                      const vsp_bases *A_query, const vsp_bases *B_query_g1, const vsp_bases *B_query_g2,
                      const vsp_bases *H_query, const vsp_bases *L_query);
void vsp_pk_free(vsp_ctx *ctx, vsp_pk *pk);

/* r1cs_gg_ppzksnark_prover::process with explicit randomness r, s (upstream draws them from a
 * non-seedable device, common.hpp:1131).  witness = primary || auxiliary, num_vars x 4 canonical (host).
 * If saver_P1 != NULL, r_enc * P1 is added to C (encrypted-input / SAVER mode).
 * Outputs: affine A (G1), B (G2), C (G1) canonical, and the 192-byte ZCash-compressed proof A||B||C
 * (the format of the reference's bin/cli/src/data.bin[0:192]); any output pointer may be NULL. */
int vsp_groth16_prove(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness,
                      const uint64_t r[4], const uint64_t s[4],
                      const uint64_t *saver_P1 /* 12 or NULL */, const uint64_t *saver_r_enc /* 4 or NULL */,
                      uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192]);

/* A BATCH of proofs over one key: `count` (1..64) witnesses of num_vars canonical values each, one after the other; r, s: count x 4 words;
 * outputs count x 12 / 24 / 12 words and count x 192 bytes (any may be NULL).  Proof k is byte-identical to vsp_groth16_prove(witness_k,
 * r_k, s_k).  Proofs of a small circuit (2^15..2^16 constraints) are bound by the latency of their dependent kernel chains, not by work:
 * proved together, the same launches run `count` times as wide -- one witness_map over 3 x count transforms, every multi-exponentiation
 * once over `count` scalar vectors.  Over a PLAIN key (vsp_groth16_generate with precompute = 0) every (witness, window) pair has its own
 * bucket set; over a key with tables of window multiples (windows of at most 16 bits) every witness has ONE per query, which is ~12 %
 * faster where the tables are small -- 2^16 constraints, precompute = 17 (all five queries), option "generate_precompute_window" = 14:
 * 1.7 GB -- and no use at 2^20 (19 GB).  Option "msm_batch_tables" = 0 refuses table keys (VSP_ERR_UNSUPPORTED), as the first version did.
 * Ballots in batches -- these proofs with the SAVER addend, beside their ciphertexts -- are vsp_saver_encrypt_batch ("SAVER ballots in batches"). */
int vsp_groth16_prove_batch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witnesses, size_t count,
                            const uint64_t *r, const uint64_t *s, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out);
/* The batch in two halves, as vsp_groth16_prove_launch / _finish below: launch copies the witnesses, r and s, queues every kernel of the
 * `count` proofs and returns; finish does the host-side scalar multiplications, waits and assembles.  One host thread with two contexts
 * over one key keeps the card busy while it assembles the other context's batch.  One batch (or one proof) in flight per context. */
int vsp_groth16_prove_batch_launch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witnesses, size_t count,
                                   const uint64_t *r, const uint64_t *s);
int vsp_groth16_prove_batch_finish(vsp_ctx *ctx, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out);
/* WITNESSES IN DEVICE MEMORY.  A witness generator that runs on the GPU -- vsp_cast_witness_batch_device is one -- hands its witnesses to
 * the batch prover, the witness check and the ballot batch where they lie.  The source is four arguments:
 *     d_witnesses  device memory of the context's device, 16-byte aligned: `rows` rows of `stride` values of 4 canonical words each; a row's
 *                  first num_vars values are a witness (primary || auxiliary), so stride >= num_vars
 *     members      host memory, `count` row indices, each < rows, in any order and with repeats; NULL means rows 0 .. count - 1
 * One kernel (csrc/prover.hip k_witness_gather, 16-byte loads and stores along a row, the map passed by value) writes z_k = (1, row
 * members[k]) into the prover's workspace; everything behind it is the code of the host form, and proof k is byte-identical to the
 * host form's over the same witness.  Nothing is waited for.  STREAM ORDER: the source must be complete on the context's stream when the
 * call is made, as for every other device pointer of this header; every read of it is queued on the context's stream before the call
 * returns, so work queued on that stream afterwards may overwrite or zero the buffer.  `members` is read before the call returns.
 * VSP_ERR_ARG, each with its message, before anything is queued: a null pointer, a pointer that is not 16-byte aligned, stride < num_vars,
 * members[k] >= rows (members NULL: count > rows), count outside 1..64 for the provers, a proof in flight.  Whether d_witnesses IS device
 * memory of the context's device is not checked: no entry point of this header checks its device pointers.
 * _launch_device / _device finish through vsp_groth16_prove_batch_finish like the host form.  vsp_r1cs_check_batch_device: any count, in
 * pieces of 64 members; the same status bytes, first_bad_row and bad_rows as vsp_r1cs_check_batch over the same witnesses.
 * Statistic "prove_witness_h2d_bytes": the witness bytes the prover's front half copied from the host (every host form; a device source adds none). */
int vsp_groth16_prove_batch_launch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows,
                                          const uint32_t *members /* host count, or NULL */, size_t count /* 1..64 */, const uint64_t *r, const uint64_t *s);
int vsp_groth16_prove_batch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows,
                                   const uint32_t *members /* host count, or NULL */, size_t count /* 1..64 */, const uint64_t *r, const uint64_t *s,
                                   uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out);
int vsp_r1cs_check_batch_device(vsp_ctx *ctx, const vsp_r1cs *cs, const void *d_witnesses, size_t stride, size_t rows, const uint32_t *members /* host count, or NULL */,
                                size_t count, uint8_t *status_out /* count */, uint64_t *first_bad_row_out /* count, may be NULL */,
                                uint64_t *bad_rows_out /* count, may be NULL */);
/* The same proof in two halves, so that ONE host thread keeps several proofs in flight over one resident key -- one per context:
 *     vsp_groth16_prove_launch(ctxA, ...); vsp_groth16_prove_launch(ctxB, ...); vsp_groth16_prove_finish(ctxA, ...); launch(ctxA, next) ...
 * launch queues every kernel of the proof on the context's streams and returns (it copies r, s and the SAVER term; a witness in
 * page-locked memory, vsp_host_register, must stay unchanged until the finish -- pageable memory is copied before launch returns);
 * finish does the host-side scalar multiplications, waits for the GPU and assembles the proof.  One proof in flight per context. */
int vsp_groth16_prove_launch(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *witness, const uint64_t r[4], const uint64_t s[4],
                             const uint64_t *saver_P1 /* 12 or NULL */, const uint64_t *saver_r_enc /* 4 or NULL */);
int vsp_groth16_prove_finish(vsp_ctx *ctx, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192]);
/* Packed witness: a Groth16 witness is mostly wires equal to 0 or 1, and its 32 bytes per wire cross PCIe in front of every proof with the
 * GPU idle (0.8 ms at 2^20 constraints).  Packed form: class_words = two bits per wire (0 = zero, 1 = one, 2 = a dense value; 3 reserved),
 * 32 wires per uint64, (num_vars + 31) / 32 words; word_offsets[w] = the index, among the dense values, of word w's first one; dense = the
 * dense values in wire order, 4 canonical words each.  A witness generator can emit this form directly (the reference builds its witness
 * wire by wire, common.hpp:1110-1128); vsp_witness_pack converts a plain witness in one host pass.  The launch validates the map
 * against n_dense and expands it on the GPU; everything else is vsp_groth16_prove_launch. */
size_t vsp_witness_pack_words(size_t num_vars);
int vsp_witness_pack(const uint64_t *witness, size_t num_vars, uint64_t *class_words, uint32_t *word_offsets, uint64_t *dense_out /* or NULL: count only */,
                     size_t dense_capacity, size_t *n_dense_out);
int vsp_groth16_prove_launch_packed(vsp_ctx *ctx, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *class_words, const uint32_t *word_offsets,
                                    const uint64_t *dense, size_t n_dense, const uint64_t r[4], const uint64_t s[4],
                                    const uint64_t *saver_P1, const uint64_t *saver_r_enc);

/* ---- Groth16 generator: zk::generate<proof_system>(constraint_system), bin/cli/.../common.hpp:916-917 ----
 * r1cs_gg_ppzksnark_generator with explicit toxic waste toxic[20] = (t, alpha, beta, gamma, delta), 4 limbs each, canonical
 * (upstream draws them from algebraic_random_device).  Builds the whole key on the GPU: Lagrange coefficients at t, the
 * per-variable QAP evaluations, the exponent vectors and the six batch exponentiations.  precompute additionally stores the window
 * multiples (vsp_bases_precompute) of proving-key queries: bit 0 = the recommended set (A, both halves of B, L; H stays plain: dense scalars
 * gain nothing from it and its 2 GB table would miss the cache); bits 1..5 select A_query, B_query (G1), B_query (G2), H_query, L_query one by one.  The key owns its queries.
 * WHICH TO CHOOSE (measured, 2^20 constraints, 90 % boolean witness, MI355X): precompute = 0, the PLAIN key, holds 1.95 GB and proves in
 * 6.65 ms (194 proofs/s from one thread with two proofs in flight); precompute = 1 holds 19.2 GB and proves in 6.26 ms (203 proofs/s).  The
 * tables buy ~5 % for ten times the memory: keep the key plain unless single-proof latency at that size is what matters.
 * vsp_groth16_prove_batch, the way to prove many statements of one circuit, takes plain keys and keys whose tables have windows of at
 * most 16 bits (not with option "msm_batch_tables" = 0); other keys are refused with VSP_ERR_UNSUPPORTED. */
typedef struct vsp_keypair vsp_keypair;
vsp_keypair *vsp_groth16_generate(vsp_ctx *ctx, const vsp_r1cs *cs, const uint64_t toxic[20], int precompute);
const vsp_pk *vsp_keypair_pk(const vsp_keypair *kp);
/* Key components as canonical affine points (host).  which: 0 A_query, 1 B_query (G1 half), 2 B_query (G2 half), 3 H_query,
 * 4 L_query, 5 gamma_ABC_g1 (verification key), 6 alpha_g1, 7 beta_g1, 8 delta_g1, 9 beta_g2, 10 delta_g2, 11 gamma_g2,
 * 12 gamma_g1 (extended verification key: the SAVER key generation needs it). */
size_t vsp_keypair_count(const vsp_keypair *kp, int which);
size_t vsp_keypair_device_bytes(const vsp_keypair *kp);     /* device memory of the whole key (the six queries) */
int vsp_keypair_export(vsp_ctx *ctx, const vsp_keypair *kp, int which, uint64_t *out);
void vsp_keypair_free(vsp_ctx *ctx, vsp_keypair *kp);

/* ---- SAVER wrapper around the prover: elgamal_verifiable<bls12_381> as the vote phase calls it ----------------
 *     generate_keypair<elgamal_verifiable>(rnd[3 n + 2], {gg_keypair, n})                common.hpp:921-931      n = msg_size = 25 (:163)
 *     encrypt<...>(m_field, {d(), pk_eid, gg_keypair, primary_input, auxiliary_input})   common.hpp:1131-1135    <- proves
 *     rerandomize<...>(rnd[3], ct, {pk_eid, gg_keypair, proof})                          common.hpp:1138-1145
 * (crypto3-pubkey, absent submodule: the SAVER scheme; member names below are upstream's.)  G_i = gamma_ABC_g1[i], H = G2 generator.
 *   rnd (3n + 2 scalars)   s_1..s_n | v_1..v_n | t_0..t_n | rho
 *   public key, flat       delta_g1 (12) | delta_s_g1[i] = s_i delta_g1 (n x 12) | t_g1[i] = t_i G_i (n x 12) | t_g2[j] = t_j H ((n+1) x 24) |
 *                          delta_sum_s_g1 = (t_0 + sum t_j s_j) delta_g1 (12) | gamma_inverse_sum_s_g1 = -(1 + sum s_j) gamma_g1 (12)
 *   secret key             rho (4)
 *   verification key, flat rho_g2 = rho H (24) | rho_sv_g2[i] = s_i v_i H (n x 24) | rho_rhov_g2[i] = rho v_i H (n x 24)
 *   ciphertext             c_0 = r delta_g1 | c_i = r delta_s_g1[i] + m_i G_i | psi = r delta_sum_s_g1 + sum m_i t_g1[i]     ((n + 2) x 12)
 * The random values upstream draws from algebraic_random_device (common.hpp:923, 1131, 1139) are explicit inputs here.
 * gamma_abc_g1 points at the first n + 1 entries of the verification key's accumulation vector (constant term, then the n
 * message inputs).  verify_encryption is vsp_saver_verify_batch below ("SAVER ballot verdicts"); decryption and its verification,
 * pairing work and a discrete logarithm on the one aggregated ciphertext, are vsp_saver_decrypt_batch and
 * vsp_saver_verify_decryption_batch ("SAVER decryption").
 * vsp_saver_keygen, vsp_saver_pk_load and vsp_saver_rerandomize are host-only and accept ctx = NULL; vsp_saver_rerandomize takes one
 * ballot a call, and the ballot box's bulk form of it on the GPU is vsp_saver_rerandomize_batch ("SAVER ballots in batches"). */
typedef struct vsp_saver_pk vsp_saver_pk;
size_t vsp_saver_pk_words(size_t msg_size);     /* uint64 words of the flat public key */
size_t vsp_saver_vk_words(size_t msg_size);
int vsp_saver_keygen(vsp_ctx *ctx, size_t msg_size, const uint64_t delta_g1[12], const uint64_t gamma_g1[12], const uint64_t *gamma_abc_g1,
                     const uint64_t *rnd, uint64_t *pk_out, uint64_t sk_out[4], uint64_t *vk_out);
/* public key resident for many votes: validates the G1 elements and builds the fixed-base tables of its msg_size + 3 bases */
vsp_saver_pk *vsp_saver_pk_load(vsp_ctx *ctx, size_t msg_size, const uint64_t *pk_words, const uint64_t *gamma_abc_g1);
void vsp_saver_pk_free(vsp_ctx *ctx, vsp_saver_pk *spk);
size_t vsp_saver_pk_msg_size(const vsp_saver_pk *spk);
/* encrypt: ciphertext of msg (n x 4, must equal the first n entries of witness = primary || auxiliary) under randomness r_enc, and
 * the Groth16 proof of the statement with C += r_enc * gamma_inverse_sum_s_g1 (vsp_groth16_prove with explicit r, s).  The
 * ciphertext is computed on the host while the GPU proves.  ct_out: (n + 2) x 12. */
int vsp_saver_encrypt(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *msg, const uint64_t *witness,
                      const uint64_t r_enc[4], const uint64_t r[4], const uint64_t s[4],
                      uint64_t *ct_out, uint64_t A_out[12], uint64_t B_out[24], uint64_t C_out[12], uint8_t proof_out[192]);
/* rerandomize in place with rnd = (r', z1, z2):  ct_i += r' X_i,  A' = z1 A,  B' = z1^-1 B + z2 delta_g2,
 * C' = C + (z1 z2) A + r' gamma_inverse_sum_s_g1;  proof_out (may be NULL) receives the 192 compressed bytes of the new proof */
int vsp_saver_rerandomize(vsp_ctx *ctx, const vsp_saver_pk *spk, const uint64_t delta_g2[24], const uint64_t rnd[12],
                          uint64_t *ct, uint64_t A[12], uint64_t B[24], uint64_t C[12], uint8_t proof_out[192]);

/* ---- SAVER ballots in batches: the ciphertexts on the GPU beside vsp_groth16_prove_batch's proofs --------------------
 * THE TABLES.  Every element of a ciphertext is a sum of scalar multiples of FIXED points of the election key, 3 msg_size + 3 of them:
 * X_0 .. X_{n+1} = delta_g1 | delta_s_g1[i] | delta_sum_s_g1, P2 = gamma_inverse_sum_s_g1, the message bases G_1 .. G_n and
 * Y_1 .. Y_n = t_g1[i].  vsp_saver_pk_upload builds the table of each (64 four-bit windows x 15 affine entries d 16^w P in Montgomery
 * form: 92 160 bytes a base, 7.2 MB at msg_size 25) on the host -- those of G and Y exist nowhere else -- and uploads them to the
 * context's device; it does nothing the second time, and the batch calls below make it themselves.  The tables belong to the KEY:
 * contexts of one device share them (another device: VSP_ERR_UNSUPPORTED), vsp_saver_pk_device_bytes is their device size (0 before the
 * upload) and vsp_saver_pk_free releases them.  A base at infinity is legal: its table is flagged and its terms are skipped.
 * vsp_saver_pk_load stays host-only and accepts ctx = NULL.  PRECONDITION, as for the tables vsp_saver_pk_load builds: the key's points
 * are in the order-r subgroup.  The load checks curve membership only, and a curve point of small order has multiples at infinity
 * among its table entries, which the tables' shared inversion does not survive: such a key gives wrong ciphertexts without a message.
 *
 * vsp_saver_ciphertext_batch: `count` ciphertexts and nothing else.  msgs: count x msg_size x 4 words, r_enc: count x 4, all
 * canonical (< r).  ct_out[k] = c_0 | c_1 .. c_n | psi of ballot k as canonical affine words (infinity: all zero) -- bit for bit
 * oracle/saver.py encrypt_ct --, addend_out[k] = r_enc_k gamma_inverse_sum_s_g1 (the term the proof's C carries), ct_blobs_out = each
 * ciphertext as vsp_g1_vector_to_blob writes it (8 + 48 (msg_size + 2) bytes a ballot), ready for vsp_tally_add_blobs.  Any count:
 * pieces of at most "saver_ct_chunk" ballots (option, default and maximum 1024) bound the workspace, the context's own and grow-only, at
 * 320 msg_size + 896 device bytes and 128 msg_size + 320 pinned bytes per ballot of a piece (9.1 MB + 3.6 MB at msg_size 25).
 * VSP_ERR_ARG before any GPU work for a null pointer or a scalar >= r; vsp_last_error names the member.
 * How it is computed (csrc/saver_ct.h, csrc/saver_batch.hip): every output column is a sum of window terms (table of base b, window
 * w, digit w of scalar s) -- 64 for c_0 and for the addend, 128 for c_i, 64 (msg_size + 1) for psi -- described as data; a group of 8 to 64
 * lanes per (ballot, column) adds up a share of the terms each by mixed additions, zero digits skipped, and folds the partial sums
 * through LDS, so no chain of dependent additions is longer than 32 at msg_size 25; a second kernel makes the sums canonical affine
 * points.  Every addition is complete (equal operands double, opposite ones give infinity, infinity on either side).
 *
 * vsp_saver_encrypt_batch: `count` (1..64) ballots of one election, each byte-identical -- ciphertext, A, B, C and the 192 proof
 * bytes -- to vsp_saver_encrypt on the same (msg_k, witness_k, r_enc_k, r_k, s_k).  msgs: count x msg_size x 4, witnesses: count x
 * num_vars x 4, r_enc, r, s: count x 4; outputs count x (msg_size + 2) x 12 | 12 | 24 | 12 words, count x 192 bytes and count blobs as
 * above; any output may be NULL.  _launch makes vsp_saver_encrypt's checks for every member before anything is queued (message
 * canonical and equal to the first msg_size public inputs of the witness, r_enc < r: VSP_ERR_ARG, vsp_last_error names the member),
 * launches the batch prover as vsp_groth16_prove_batch_launch does, and queues the ciphertext kernels on a stream of the context's
 * own, where they fill the gaps between the prover's kernels; the results land in pinned memory behind an event.  _finish waits for that
 * event, hands the members' addends to the batch assembly and finishes the proofs.  One batch (of ballots or of proofs) in flight per
 * context; a finish without a launch is VSP_ERR_ARG.  With option "prove_check_witness" an unsatisfied member's outputs are all zero,
 * ciphertext and blob included, the call returns VSP_ERR_UNSATISFIED, vsp_groth16_prove_batch_verdicts names the members and the other
 * members are as without the check.
 * Option "saver_encrypt_gpu" (default 1): 0 computes the ciphertexts and addends on the host instead -- the same columns over the same
 * tables, a ballot per host thread, in the finish's wait for the proofs -- as the other leg of a measurement and a second
 * implementation for the tests.  Nothing switches to it on its own.
 * Statistics (vsp_get_stat, summed since vsp_stats_reset): "saver_ct_ms" HIP events around the ciphertext kernels, "saver_ct_table_ms"
 * the tables' build and upload (once per key, wall time), "saver_encrypt_batches" batches finished. */
int vsp_saver_pk_upload(vsp_ctx *ctx, vsp_saver_pk *spk);
size_t vsp_saver_pk_device_bytes(const vsp_saver_pk *spk);
int vsp_saver_ciphertext_batch(vsp_ctx *ctx, const vsp_saver_pk *spk, const uint64_t *msgs /* count x msg_size x 4 */, const uint64_t *r_enc /* count x 4 */,
                               size_t count, uint64_t *ct_out /* count x (msg_size + 2) x 12 */, uint64_t *addend_out /* count x 12, may be NULL */,
                               uint8_t *ct_blobs_out /* count x (8 + 48 (msg_size + 2)), may be NULL */);
int vsp_saver_encrypt_batch_launch(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *msgs, const uint64_t *witnesses,
                                   size_t count /* 1..64 */, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s);
int vsp_saver_encrypt_batch_finish(vsp_ctx *ctx, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out);
int vsp_saver_encrypt_batch(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const uint64_t *msgs, const uint64_t *witnesses,
                            size_t count /* 1..64 */, const uint64_t *r_enc, const uint64_t *r, const uint64_t *s, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out,
                            uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out);
/* The ballot batch over witnesses in device memory ("WITNESSES IN DEVICE MEMORY" above: the same four arguments, the same stream order,
 * the same errors).  There is no msgs argument: the message IS the first msg_size values of each member's row.  Behind the gather those
 * values are copied device to device into the ciphertext kernels' scalars, beside r_enc from the host; the ciphertext stream waits for an
 * event behind the gather.  With option "saver_encrypt_gpu" = 0 the count x msg_size message scalars, and nothing else of the witnesses,
 * are copied to the host for the host leg.  The outputs are byte-identical to vsp_saver_encrypt_batch over the same rows, under
 * "prove_check_witness" too.  The host form's launch-time check that every message scalar is canonical has no counterpart here -- the
 * launch never sees the values: a value >= r is found by the multi-exponentiations' census and reported by the finish (VSP_ERR_ARG) for
 * the whole batch, as the batch prover reports it, and every ciphertext output of that batch is then zero.  r_enc, r, s: host, checked at
 * the launch.  Both finish through vsp_saver_encrypt_batch_finish. */
int vsp_saver_encrypt_batch_launch_device(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride,
                                          size_t rows, const uint32_t *members /* host count, or NULL */, size_t count /* 1..64 */, const uint64_t *r_enc,
                                          const uint64_t *r, const uint64_t *s);
int vsp_saver_encrypt_batch_device(vsp_ctx *ctx, const vsp_saver_pk *spk, const vsp_r1cs *cs, const vsp_pk *pk, const void *d_witnesses, size_t stride, size_t rows,
                                   const uint32_t *members /* host count, or NULL */, size_t count /* 1..64 */, const uint64_t *r_enc, const uint64_t *r,
                                   const uint64_t *s, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out);
/* RERANDOMIZATION IN BATCHES: what the ballot box does to every ballot it receives, `count` ballots a call.
 * A vsp_saver_rerandomizer is public data of one election: the key (which must outlive it) with the device tables vsp_saver_pk_upload
 * builds -- _new makes the upload -- and one more table of the same layout in G2, 64 four-bit windows x 15 affine entries d 16^w delta_g2
 * in Montgomery form (184 320 bytes; vsp_saver_rerandomizer_device_bytes counts it and the two column plans, not the key's tables).
 * _new validates delta_g2 on the curve (NULL and vsp_last_error otherwise; infinity is legal, its table is flagged).  PRECONDITION, as for
 * vsp_saver_pk_upload: delta_g2 is in the order-r subgroup -- the table's shared inversion does not survive a multiple at infinity.
 *
 * vsp_saver_rerandomize_batch: for every member k the outputs are, word for word and byte for byte, what vsp_saver_rerandomize writes for
 * (rnd_k, ct_k, A_k, B_k, C_k) under the same key and delta_g2:
 *     ct_i' = ct_i + r' X_i  (i = 0 .. msg_size + 1)     A' = z1 A     B' = z1^-1 B + z2 delta_g2     C' = C + (z1 z2) A + r' P2
 * as canonical affine words, infinity all zero; proofs_out[k] the 192 compressed bytes of (A', B', C'), ct_blobs_out[k] the blob of ct'
 * as vsp_g1_vector_to_blob writes it.  rnd: count x 12 words r' | z1 | z2; ct: count x (msg_size + 2) x 12; A, C: count x 12; B: count x
 * 24.  Any output may be NULL, and an output array may be the input array of the same name.
 * Before any GPU work: a null input, a scalar >= r or z1 = 0 in any member is VSP_ERR_ARG, and vsp_last_error names the member.
 * On the device: every input point has coordinates below p and is on its curve or the all-zero infinity.  A member with a point that
 * is not gets status_out[k] = 1 and all-zero outputs, blob and proof bytes included; the other members are unaffected and the call
 * returns VSP_OK.  With status_out = NULL such a member makes the call return VSP_ERR_ARG after the fact (the outputs are written as
 * described), and vsp_last_error names the first one.  No subgroup check, as in the single call: every addition used is complete for
 * any curve point.
 * Any count: pieces of at most "saver_rerandomize_chunk" ballots (option, default and maximum 2^16) bound the workspace, the context's
 * own and grow-only, at 384 msg_size + 2 276 device bytes and 192 msg_size + 1 316 pinned bytes per ballot of a piece (778 MB + 401 MB
 * for 2^16 ballots at msg_size 25, a quarter of that for pieces of 2^14, which are a third slower; a smaller call takes what its count needs).  While a batch of ballots or of proofs is in flight on the context the call is refused with
 * VSP_ERR_ARG.  Option "saver_rerandomize_w4" (default 1): the variable-base multiplications walk 4-bit windows; 0 walks single bits.
 * How it is computed (csrc/saver_rerand.h, csrc/saver_rerand.hip): the msg_size + 3 sums r' X_i and r' P2 are columns of window terms over
 * the key's tables as in vsp_saver_ciphertext_batch, 8 lanes each, and lane 0 adds the ballot's own ct_i or C; z2 delta_g2 is one
 * such column over the G2 table; z1 A and (z1 z2) A take a lane each and z1^-1 B one, in kernels of their own group; 1 / z1 of a whole
 * piece comes from one inversion on the host.
 * Statistics: "saver_rerandomize_ms" HIP events around the kernels, split into "saver_rerandomize_check_ms", "_columns_ms", "_affine_ms",
 * "_g1_ms" and "_g2_ms"; "saver_rerandomize_ballots" ballots through the kernels. */
typedef struct vsp_saver_rerandomizer vsp_saver_rerandomizer;
vsp_saver_rerandomizer *vsp_saver_rerandomizer_new(vsp_ctx *ctx, vsp_saver_pk *spk, const uint64_t delta_g2[24]);
void   vsp_saver_rerandomizer_free(vsp_ctx *ctx, vsp_saver_rerandomizer *rr);
size_t vsp_saver_rerandomizer_msg_size(const vsp_saver_rerandomizer *rr);
size_t vsp_saver_rerandomizer_device_bytes(const vsp_saver_rerandomizer *rr);
int vsp_saver_rerandomize_batch(vsp_ctx *ctx, const vsp_saver_rerandomizer *rr, const uint64_t *rnd /* count x 12: r' | z1 | z2 */,
                                const uint64_t *ct /* count x (msg_size + 2) x 12 */, const uint64_t *A, const uint64_t *B, const uint64_t *C,
                                size_t count, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out,
                                uint8_t *proofs_out /* count x 192 */, uint8_t *ct_blobs_out, uint8_t *status_out /* count */);

/* ---- generator-side batch exponentiation (section 8(f).1; also builds synthetic benchmark bases) ---
 * out[i] = scalars[i] * generator, written to DEVICE memory as canonical affine points. */
int vsp_fixed_base_mul_g1(vsp_ctx *ctx, const void *d_scalars, size_t n, void *d_out /* n x 12 u64 */);
int vsp_fixed_base_mul_g2(vsp_ctx *ctx, const void *d_scalars, size_t n, void *d_out /* n x 24 u64 */);

/* ---- diagnostics ---------------------------------------------------------------------------------
 * Elementwise field arithmetic on the GPU over n canonical values (host buffers): field 0 = Fp (6 limbs),
 * 1 = Fr (4 limbs); op 0 mul, 1 add, 2 sub, 3 sqr(a), 4 canonical-times-Montgomery product, 5 inverse(a); Fp only: ops 6..12
 * exercise the 14 x 28-bit lazy field of the G1 accumulation (round trip, product, the lazy subtractions and the negation).
 * Fr only: ops 6..9 exercise the 9 x 29-bit lazy field of the NTT butterflies: 6 round trip through the limb form, 7 a b through the
 * product routine and the conditional subtraction, 8 the same through the routine's second register map, 9 a + a b - b^2 through the
 * limb-wise addition, the lazy subtraction, the carry pass and the product that leaves the lazy domain.
 * Lets the tests check the kernels' Montgomery arithmetic directly against known-answer vectors. */
int vsp_selftest_field(vsp_ctx *ctx, int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* The full addition of two bucket sums on its own: out[i] = a[i] + b[i], points as canonical (X, Y, ZZ, ZZZ) records with x = X / ZZ,
 * y = Y / ZZZ, ZZ^3 = ZZZ^2, all-zero = infinity (group 1: 4 x 6 limbs, group 2: 4 x 12 limbs; host buffers).  form 0 = the 12 x 32-bit
 * formulas, 1 = the 14 x 28-bit lazy form the merges and the bucket reduction run.  The result is some representation of the sum
 * (compare X / ZZ, Y / ZZZ).  Covers the exceptional cases -- doubling, cancellation, infinity on either side -- lane by lane. */
int vsp_selftest_xyzz_add(vsp_ctx *ctx, int group, int form, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* One operation of the tower Fp2 / Fp6 / Fp12 (csrc/fp12.h, csrc/gt_dlog.h) as the GPU compiles it, on n values: out[i] = op(a[i], b[i]).
 * Host buffers of canonical little-endian values, an element 6 * level words (level 2, 6 or 12), coefficients in the order of the
 * 576-byte GT encoding (u^i v^j w^k at index (k * 3 + j) * 2 + i); the kernel brings them to Montgomery form and back.  a, b and out
 * have the same element size whatever the operation reads of b.  One lane per value, 64-lane blocks; the level 6 and 12 kernels are part
 * of the pairing kernels' translation unit and call its out-of-line tower functions on values kept in memory.
 *   level 2 (one lane holds the whole value):
 *      0 mul   1 sqr(a)   2 inv(a), the generic power   3 conj(a)   4 f2inv(a), the fixed chain   5 mul_xi(a)   6 f2half(a)   7 add   8 sub
 *      9 mul_fp(a, b.c0)   10 neg(a)   11 dbl(a)   12 fp_half of each component of a   13 fp_inv_chain of each component of a
 *   level 6:
 *      0 mul   1 mul_v(a)   2 inv(a)   3 mul_by_01(a, b.c0, b.c1)   4 mul_by_1(a, b.c1)   7 add   8 sub
 *   level 12:
 *      0 mul   1 sqr(a)   2 inv(a)   3 conj(a)   4 frobenius(a)   5 frobenius2(a)   6 cyclotomic_sqr(a)   7 add   8 sub   9 final_exp(a)
 *      10 mul_by_014(a, l0, l1, l4), the line taken from the Fp2 coefficients 0, 1 and 4 of b, the rest of b ignored
 *      11 is_one(a): 0 or 1 in the first word of out[i], the other words zero
 *      12 gt_pow(a, e), e the first four words of b (256 bits), through the decryption kernels' own power function
 * Inverses map 0 to 0; cyclotomic_sqr and gt_pow are for values of the cyclotomic subgroup only.
 * VSP_ERR_ARG for a null pointer, another level, or an op the level does not have. */
int vsp_selftest_tower(vsp_ctx *ctx, int level, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n);
/* The Fp2 arithmetic of the G2 kernels, where one value lives in a lane pair (even lane c0, odd lane c1) and products exchange halves
 * by DPP, on n sets of canonical Fp2 operands a, b, c, d (12 words each; host buffers); results out_p and, for mul_pair, out_q (12
 * words each; out_q is zero otherwise).  Two lanes per element.
 *   form 0, the 12 x 32-bit Fp2L of csrc/field.h:
 *      0 mul(a, b)   1 sqr(a)   2 mul_pair: p = a b, q = c d   3 prod_diff: a b - c d   4 mul_add2: a b + c d
 *      5 is_zero(a): each lane's answer, 0 or 1, in the first word of its component of out_p
 *      6 add(a, b)   7 sub(a, b)   8 neg(a)   9 dbl(a)
 *   form 1, the 14 x 28-bit pair form of csrc/fp28.h on canonical operands (tight limbs), back through fp28_to_fp:
 *      0 mulF2(a, b, K8_L1)   1 mulF2(a, b, K64_L4)   2 sqrF2(a, K8_L1)   3 sqrF2(a, K32_L1)   4 sqrF2(a, K64_L1)
 *   op -1: element i runs op i mod K (K = 10, form 1: 5), so neighbouring pairs of a wave take different branches around the exchanges.
 * VSP_ERR_ARG for a null pointer, another form, or an op the form does not have. */
int vsp_selftest_fp2_lanes(vsp_ctx *ctx, int form, int op, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d,
                           uint64_t *out_p, uint64_t *out_q, size_t n);

/* ---- wire format helpers (host only, tiny) ---------------------------------------------------
 * compress: VSP_ERR_ARG for a null pointer or a coordinate that is not canonical (>= p). */
int vsp_g1_compress(const uint64_t affine[12], uint8_t out[48]);
int vsp_g2_compress(const uint64_t affine[24], uint8_t out[96]);
/* Inverse: ZCash-compressed bytes -> canonical affine limbs (the 192-byte proof of bin/cli/src/data.bin[0:192] is A (48) | B (96) |
 * C (48)).  VSP_ERR_ARG for an encoding that is not compressed form, not canonical (x >= p, stray bits), not on the curve or --
 * with check_subgroup != 0 -- not in the order-r subgroup. */
int vsp_g1_decompress(const uint8_t in[48], int check_subgroup, uint64_t out_affine[12], int *out_is_inf);
int vsp_g2_decompress(const uint8_t in[96], int check_subgroup, uint64_t out_affine[24], int *out_is_inf);

/* ---- batch decompression of G1 points on the GPU ------------------------------------------------
 * n ZCash-compressed points (48 bytes each, back to back) -> canonical affine limbs and one status byte per point:
 *     0      accepted
 *     bit 0  malformed encoding: the compressed flag (0x80) is missing, an infinity record (0x40) has a payload or a sign bit, or x >= p
 *     bit 1  x^3 + 4 is not a square: no point of the curve has this x
 *     bit 2  not in the order-r subgroup (only with check_subgroup != 0; the endomorphism test of "bases_check_subgroup")
 * A point is accepted exactly when vsp_g1_decompress accepts the same 48 bytes.  A rejected point and infinity (0xC0 00..) are
 * written as all-zero limbs.  The return value is VSP_OK whatever the verdicts are: VSP_ERR_* is for bad arguments (a null pointer,
 * also with n = 0) and HIP failures only.  One lane per point: the square root is a fixed chain of 481 field products (csrc/fp_sqrt.h).
 * Any n: the points go through the device in pieces of at most 2^21 (see the workspace bound below). */
int vsp_g1_decompress_batch(vsp_ctx *ctx, const uint8_t *in /* host n x 48 */, size_t n, int check_subgroup,
                            uint64_t *out_affine /* host n x 12, canonical */, uint8_t *status_out /* host n */);

/* ---- batch decompression of G2 points and of proofs on the GPU -----------------------------------
 * vsp_g2_decompress_batch is the G2 counterpart of the above: n ZCash-compressed G2 points (96 bytes each: x.c1 | x.c0 big-endian, the
 * flag bits in the first byte) -> canonical affine limbs (x.c0 | x.c1 | y.c0 | y.c1) and one status byte per point with the same bits:
 *     bit 0  malformed encoding (flag rules as for G1; a coefficient of x >= p)
 *     bit 1  x^3 + 4 (1 + u) is not a square in Fp2: no point of the twist has this x
 *     bit 2  not in the order-r subgroup (only with check_subgroup != 0; the same endomorphism test over Fp2)
 * A point is accepted exactly when vsp_g2_decompress accepts the same 96 bytes; a rejected point and infinity are all-zero limbs.
 * One lane per point: the root in Fp2 is two fixed chains, 976 field products with the curve equation and the sign rule
 * (csrc/fp2_sqrt.h), where the host function walks four generic square-and-multiply loops.
 * vsp_proof_from_blob_batch decodes n proof blobs lying back to back (A (48) | B (96) | C (48): the layout vsp_proof_to_blob writes and
 * data.bin[0:192) pins).  Proof k's status is the OR of its three points' status bytes in bits 0..2; bits 4, 5, 6 are set when A, B, C
 * respectively was rejected.  A proof is accepted (status 0) exactly when vsp_proof_from_blob accepts the same 192 bytes (infinity
 * members are accepted, as there); all three outputs of a rejected proof are all-zero limbs, its well-formed members included.  Any of
 * A_out, B_out, C_out may be NULL (that member is still decoded and checked); blobs and status_out may not.
 * Both: VSP_OK whatever the verdicts are; VSP_ERR_ARG for a null pointer, also with n = 0; VSP_ERR_HIP as elsewhere.  Any n: the work
 * runs in pieces of at most "tally_chunk_points" points (default 2^21; a proof counts three, at least one proof per piece).
 * Workspace bound per piece: 96 raw + 192 decoded + 1 status byte per G2 point (578 MiB at 2^21 points); 192 raw + 2 x 96 + 192 decoded
 * + 4 status bytes per proof (387 MiB at 2^21 / 3 proofs), of the context's grow-only workspaces whatever n is.  Stage times (HIP
 * events, summed since vsp_stats_reset): vsp_get_stat "g2_decode_ms", "g2_subgroup_ms"; the G1 members of proofs are added to
 * "tally_decode_ms" and "tally_subgroup_ms". */
int vsp_g2_decompress_batch(vsp_ctx *ctx, const uint8_t *in /* host n x 96 */, size_t n, int check_subgroup,
                            uint64_t *out_affine /* host n x 24, canonical */, uint8_t *status_out /* host n */);
int vsp_proof_from_blob_batch(vsp_ctx *ctx, const uint8_t *blobs /* host n x 192, back to back */, size_t n, int check_subgroup,
                              uint64_t *A_out /* n x 12 */, uint64_t *B_out /* n x 24 */, uint64_t *C_out /* n x 12 */,
                              uint8_t *status_out /* n */);

/* ---- tally: the aggregation of common.hpp:1193-1216 (repeated by every verifier at :1257-1279) ----
 * process_encrypted_input_mode_tally_admin_phase deserialises up to 1 << tree_depth ciphertext blobs one after the other and adds
 * them component by component into ct_agg; everything after that is pairing work on the ONE aggregated ciphertext.  A tally handle
 * holds the ct_len = msg_size + 2 running sums (host memory; the device workspaces belong to the context).
 * vsp_tally_add_blobs takes `count` ballots lying back to back, each a G1 vector blob exactly as vsp_g1_vector_to_blob writes it
 * (8-byte big-endian count, then ct_len compressed points: 8 + 48 ct_len bytes), decodes and checks every point on the GPU and adds
 * every ACCEPTED ballot to the running sums.  A ballot's status is the OR of the status bytes of its points (as above), bit 0 also
 * for a count header that differs from ct_len; a rejected ballot contributes none of its components, its well-formed ones included.
 * status_out (count bytes) and accepted_out (ballots this call accepted) may be NULL; t and blobs may not (VSP_ERR_ARG, also with count = 0).  The reference aborts on the first bad blob:
 * a caller who wants that compares *accepted_out with count.  With check_subgroup = 0 curve points outside the subgroup are
 * accepted, and the sums are still the exact curve sums (the additions are generic).
 * vsp_tally_result returns the ct_len sums as canonical affine points (infinity all zero) and the number of ballots accepted since
 * the handle was created or last reset; it may be called at any time and adding may go on afterwards.  No accepted ballot: all
 * infinity and 0.  The result is canonical, so it does not depend on how the ballots were split over calls.
 * Workspace bound: a call with many ballots runs in pieces of at most 2^21 points (2^16 ballots of 27 points take 170 MB decoded),
 * at least one ballot: raw bytes, Montgomery-form points, status bytes and partial sums of one piece stay below 400 MB of the
 * context's grow-only workspaces whatever `count` is.  Stage times (HIP events, summed since vsp_stats_reset): vsp_get_stat
 * "tally_decode_ms", "tally_subgroup_ms", "tally_sum_ms".  Option "tally_chunk_points" (default 2^21) sets the piece size. */
typedef struct vsp_tally vsp_tally;
vsp_tally *vsp_tally_create(vsp_ctx *ctx, size_t ct_len /* msg_size + 2; 1..1024 */);
void vsp_tally_free(vsp_ctx *ctx, vsp_tally *t);
int vsp_tally_add_blobs(vsp_ctx *ctx, vsp_tally *t, const uint8_t *blobs /* host, count x (8 + 48 ct_len), packed */,
                        size_t count, int check_subgroup, uint8_t *status_out /* count, may be NULL */,
                        size_t *accepted_out /* may be NULL */);
int vsp_tally_result(vsp_ctx *ctx, const vsp_tally *t, uint64_t *ct_out /* host ct_len x 12 */, uint64_t *ballots_out /* may be NULL */);
int vsp_tally_reset(vsp_ctx *ctx, vsp_tally *t);

/* ---- pairings and Groth16 verdicts on the GPU ------------------------------------------------------
 * e(P, Q) is the optimal ate pairing of BLS12-381 as oracle/pairing.py defines it: f_{|x|,Q}(P)^((p^12 - 1) / r) with
 * |x| = 0xd201000000010000 and NO conjugation for the negative curve parameter (csrc/pairing.h "CONVENTION": the inverse of the value of
 * libraries that conjugate; products-equal-one tests do not depend on it).  A GT element is 576 bytes: 12 little-endian Fp, the
 * coefficient of u^i v^j w^k at index (k * 3 + j) * 2 + i -- the encoding vsp_vk_to_blob takes and data.bin[196:772) pins.
 * vsp_multi_pairing_batch computes n products of m pairings each: product i is prod_j e(g1[i m + j], g2[i m + j]); m = 1 is a plain
 * batch of pairings.  Points are canonical affine limbs, all zero = infinity (its pairing is one).  gt_out (n x 576) and is_one_out
 * (n bytes: 1 when the product is one) may each be NULL.  One lane per pair for the Miller loop (about 6 700 field products), one lane
 * per product for the final exponentiation (about 9 000, the exact exponent): csrc/pairing.h.
 * SUBGROUP.  The points are ASSUMED to lie in the order-r subgroups: decode with check_subgroup (vsp_proof_from_blob_batch,
 * vsp_g1/g2_decompress_batch).  For other curve points the result is unspecified (the call still terminates without a fault).
 * A coordinate >= p or a point off its curve, found by a check kernel on the device: VSP_ERR_ARG (outputs unspecified; the context
 * stays usable).  VSP_ERR_ARG also for a null g1 / g2 (also with n = 0) and for m = 0 or m > 2^16 (a product is never split over
 * pieces, so its m bounds the workspace); VSP_ERR_HIP as elsewhere.
 * A verification key handle validates its points on the host (canonical, on the curve; VSP_ERR_ARG and NULL otherwise), computes
 * e(alpha_g1, beta_g2) once on the GPU -- vsp_vk_alpha_beta returns its 576 bytes, the gt argument of vsp_vk_to_blob -- and keeps
 * -gamma_g2, -delta_g2 and the multiples 0..15 of every gamma_ABC point (16 entries, the first infinity) resident (n_abc >= 1 points:
 * one more than public inputs).
 * vsp_groth16_verify_batch gives one verdict byte per proof: 1 exactly when
 *     fexp(ml(A, B) ml(acc, -gamma_g2) ml(C, -delta_g2)) = e(alpha_g1, beta_g2),   acc = gamma_ABC[0] + sum_i inputs[i] gamma_ABC[i + 1]
 * which is when oracle/pairing.py groth16_verify accepts; acc is computed on the GPU, one lane per proof.  A coordinate >= p, a point
 * off its curve or a scalar >= r gives verdict 0 for that proof alone.  VSP_OK whatever the verdicts are; VSP_ERR_ARG for a null
 * pointer, also with n = 0 (inputs may be NULL when n_abc = 1); VSP_ERR_HIP as elsewhere.  No random linear combination: every verdict
 * is exact and independent of the other proofs of the batch.
 * Any n: the work runs in pieces of at most "pairing_chunk" products (default and maximum 2^14) and at most 2^16 pairs, at least one
 * product.  Workspace bound per piece: 288 canonical + 288 Montgomery + 576 Miller bytes + 1 status byte per pair and 2 x 576 + 2
 * bytes per product -- below 100 MiB of the context's grow-only workspaces whatever n and m are (m <= 2^16).  Stage times (HIP events,
 * summed since vsp_stats_reset): vsp_get_stat "pairing_miller_ms" (Miller loops and their products), "pairing_finalexp_ms". */
int vsp_multi_pairing_batch(vsp_ctx *ctx, const uint64_t *g1 /* host n*m x 12, canonical affine */, const uint64_t *g2 /* host n*m x 24 */,
                            size_t m /* pairs per product, 1..2^16 */, size_t n /* products */, uint8_t *gt_out /* n x 576, may be NULL */,
                            uint8_t *is_one_out /* n, may be NULL */);
typedef struct vsp_vk vsp_vk;
vsp_vk *vsp_vk_create(vsp_ctx *ctx, const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24],
                      const uint64_t delta_g2[24], const uint64_t *gamma_abc_g1 /* n_abc x 12 */, size_t n_abc);
int vsp_vk_alpha_beta(const vsp_vk *vk, uint8_t gt_out[576]);
void vsp_vk_free(vsp_ctx *ctx, vsp_vk *vk);
int vsp_groth16_verify_batch(vsp_ctx *ctx, const vsp_vk *vk, const uint64_t *inputs /* host n x (n_abc - 1) x 4, canonical Fr */,
                             const uint64_t *A /* n x 12 */, const uint64_t *B /* n x 24 */, const uint64_t *C /* n x 12 */, size_t n,
                             uint8_t *verdict_out /* n: 1 accepted, 0 rejected */);

/* ---- SAVER ballot verdicts on the GPU: verify_encryption<elgamal_verifiable> (common.hpp:1164-1169) ------------------------------
 * The check every ballot passes before it may enter the tally.  A ballot is a ciphertext ct = c_0 | c_1 .. c_n | psi (n = msg_size)
 * with a proof (A, B, C); the ciphertext stands in for the message inputs of the Groth16 statement:
 *     equation 1:  prod_{j=0..n} e(c_j, t_g2[j]) * e(psi, -H) = 1                                   (H the generator of G2)
 *     equation 2:  fexp(ml(A, B) ml(acc, -gamma_g2) ml(C, -delta_g2)) = e(alpha_g1, beta_g2),
 *                  acc = gamma_ABC[0] + c_0 + .. + c_n + sum_k inputs_rest[k] gamma_ABC[n + 1 + k]
 * verdict_out[k] is 1 exactly when oracle/saver.py verify_encryption accepts ballot k.  reason_out[k] (may be NULL) is 0 for an accepted
 * ballot; exactly 1 for a malformed one (a coordinate >= p, a point off its curve, a scalar >= r: no pairing verdict for it, the rest
 * of the batch is unaffected); otherwise bit 1 (value 2) is set when equation 1 fails and bit 2 (value 4) when equation 2 fails.
 * Equal, opposite and infinity ciphertext members are legal (the additions of acc are generic); an infinity member pairs to one.
 * A verifier handle holds a verification key as vsp_vk_create makes it, and the PREPARED LINES of the 29 fixed G2 arguments at
 * msg_size 25 -- t_g2[0..n], -H, -gamma_g2, -delta_g2: the 68 line-coefficient triples of the Miller loop, 19 584 bytes each
 * (csrc/pairing.h) -- so a ballot's Miller loops do no G2 point arithmetic but for B, and the pairs of an equation share their Fp12
 * squarings in groups of "saver_verify_group" pairs (option, default 9; one lane per ballot and group).  saver_pk_words is the flat
 * public key of vsp_saver_keygen (only t_g2 is read).  Creation validates the key points on the host (canonical, on the curve): NULL
 * and the last error otherwise.
 * SUBGROUP.  As for the pairings above, the points of a ballot are ASSUMED to lie in the order-r subgroups: decode with check_subgroup
 * (vsp_tally_add_blobs, vsp_proof_from_blob_batch).
 * vsp_saver_verify_batch returns VSP_OK whatever the verdicts are; VSP_ERR_ARG for a null pointer, also with n = 0 (inputs_rest may be
 * NULL when n_abc = msg_size + 1), and for a verifier made on another device; VSP_ERR_HIP as elsewhere.  No random linear combination:
 * every verdict is exact and independent of the other ballots.
 * Any n: the work runs in pieces of at most "pairing_chunk" ballots (default and maximum 2^14) and at most 2^19 G1 arguments (a ballot
 * has msg_size + 5 and is never split).  Workspace bound per piece: 96 canonical + 96 Montgomery bytes per G1 argument (192 MiB at
 * 2^19), 576 bytes per ballot and group (groups: ceil((msg_size + 2) / saver_verify_group) + 1), 2 x 576 + 384 + 3 bytes and 32 per
 * rest input per ballot -- 149 MiB at msg_size 25 with 2^14 ballots and the default grouping -- of the context's grow-only workspaces
 * whatever n is.  Stage times (HIP events, summed since vsp_stats_reset): vsp_get_stat "saver_verify_prepare_ms",
 * "saver_verify_miller_ms" (Miller loops and their products), "saver_verify_finalexp_ms". */
typedef struct vsp_saver_verifier vsp_saver_verifier;
vsp_saver_verifier *vsp_saver_verifier_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_pk_words /* vsp_saver_pk_words(msg_size) */,
                                              const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24],
                                              const uint64_t delta_g2[24], const uint64_t *gamma_abc_g1 /* n_abc x 12 */,
                                              size_t n_abc /* >= msg_size + 1 */);
void vsp_saver_verifier_free(vsp_ctx *ctx, vsp_saver_verifier *ver);
size_t vsp_saver_verifier_msg_size(const vsp_saver_verifier *ver);
int vsp_saver_verify_batch(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct /* host n x (msg_size + 2) x 12 */,
                           const uint64_t *inputs_rest /* n x (n_abc - 1 - msg_size) x 4; may be NULL when that is 0 */,
                           const uint64_t *A /* n x 12 */, const uint64_t *B /* n x 24 */, const uint64_t *C /* n x 12 */, size_t n,
                           uint8_t *verdict_out /* n: 1 accepted, 0 rejected */, uint8_t *reason_out /* n, may be NULL */);

/* ---- SAVER ballots screened in bulk: one random linear combination per range, exact on failure -------------------------------------
 * vsp_saver_verify_batch confirms every honest ballot on its own.  With caller-supplied coefficients z_i in [1, 2^128) the WELL-FORMED
 * ballots of a range R are accepted together when two pairing-product equations hold (n = msg_size):
 *     S_j = sum_{i in R} z_i c_{i,j} (j = 0..n),  S_psi = sum z_i psi_i,  ACC = sum z_i acc_i,  Csum = sum z_i C_i,  Z = sum z_i mod r
 *     equation 1:  fexp( prod_{j=0..n} ml(S_j, t_g2[j]) * ml(S_psi, -H) ) = 1
 *     equation 2:  fexp( prod_{i in R} ml(z_i A_i, B_i) * ml(ACC, -gamma_g2) * ml(Csum, -delta_g2) * ml(-Z alpha_g1, beta_g2) ) = 1
 * Arguments, layouts, return codes and the SUBGROUP assumption are those of vsp_saver_verify_batch.  coeff (host, n x 2 words, the
 * little-endian 128-bit z_i) must not be NULL, and a zero coefficient is VSP_ERR_ARG before any GPU work; VSP_ERR_ARG as well while a
 * proof is in flight on the context (the call uses the multi-exponentiation work slots: finish the proof first).
 * VERDICTS.  A verdict of 0 and its reason always come from the exact path: they equal what vsp_saver_verify_batch gives for that
 * ballot, reason 1 for a malformed ballot included.  A verdict of 1 means that the exact path accepted the ballot, or that the ballot is
 * well formed and lies in a range whose two equations held.  No valid ballot is ever rejected: if every ballot of a range satisfies an
 * equation, the combined equation holds with certainty.  Malformed ballots are taken out of every sum and product (their coefficient
 * counts as absent, their Miller value as one) and do not make a range fail.
 * SOUNDNESS.  If a ballot of the range fails an equation, the points are in their subgroups, and the z_i are uniform in [1, 2^128) and
 * chosen AFTER the ballots are fixed, the combined equation holds with probability at most 1 / (2^128 - 1).  The coefficients must be
 * fresh for every call, uniform, and drawn after the ballots are fixed: a sender who knows them can make invalid ballots cancel (two
 * ballots whose defects are z_2 and -z_1 pass under (z_1, z_2)).  For points OUTSIDE the order-r subgroups the screened and the exact
 * verdict may differ (a small-order component can vanish under a coefficient): decode with check_subgroup.
 * PROCEDURE.  Pieces of at most "saver_screen_chunk" ballots (option, default and maximum 2^16).  A piece is prepared by the exact
 * path's own kernel, A_i is multiplied by z_i (one lane per ballot), one Miller loop per ballot gives ml(z_i A_i, B_i), a product tree
 * multiplies them, the n + 4 sums are multi-exponentiations over one shared digit sort of the z_i (plain bases, generic additions:
 * exact for equal, opposite and infinity points), and n + 5 Miller loops over prepared lines and two final exponentiations judge the
 * piece.  A piece that fails is cut into "saver_screen_split" equal sub-ranges (option, default 4, at most 1024; 0 or 1: no second
 * level) that are judged the same way in one pass, the per-ballot Miller values reused; the sub-ranges that fail go to
 * vsp_saver_verify_batch's code as contiguous runs.  There is no deeper level.
 * Workspace bound per piece, beside that of the exact path for the runs handed to it: 96 canonical + 96 Montgomery bytes per G1
 * argument (msg_size + 5 per ballot), 576 + 384 + 3 + 48 bytes and 32 per rest input per ballot, 2 x 576 / 16 bytes per ballot for the
 * tree, 672 (msg_size + 5) + 1 154 bytes per sub-range, and the work slots' sort of one 255-bit scalar per ballot -- 438 MiB at msg_size
 * 25 with 2^16 ballots.  Statistics (vsp_get_stat, summed since vsp_stats_reset): "saver_screen_checks" ranges judged,
 * "saver_screen_failed" ranges that failed, "saver_screen_exact_ballots" ballots handed to the exact path; stage times by HIP events
 * "saver_screen_prepare_ms", "saver_screen_scale_ms", "saver_screen_miller_ms" (per-ballot and fixed-argument Miller loops and their
 * products), "saver_screen_msm_ms" (the column sums, their host folds included), "saver_screen_finalexp_ms". */
int vsp_saver_verify_batch_screened(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct /* host n x (msg_size + 2) x 12 */,
                                    const uint64_t *inputs_rest /* n x (n_abc - 1 - msg_size) x 4; may be NULL when that is 0 */,
                                    const uint64_t *A /* n x 12 */, const uint64_t *B /* n x 24 */, const uint64_t *C /* n x 12 */, size_t n,
                                    const uint64_t *coeff /* host n x 2, little-endian 128-bit, not zero */,
                                    uint8_t *verdict_out /* n: 1 accepted, 0 rejected */, uint8_t *reason_out /* n, may be NULL */);

/* ---- ballots received from their blobs: one decode for verdicts and tally --------------------------------------------
 * The ballot box's receiving step as one call: the wire in, verdicts and a running tally out.  A ballot arrives as three blobs -- the
 * ciphertext vector (8 + 48 (msg_size + 2) bytes), the proof (192 bytes) and the remaining public inputs as a scalar vector exactly as
 * vsp_fr_vector_to_blob writes it for n_rest = n_abc - 1 - msg_size scalars (8 + 32 n_rest bytes).  Every point is decoded once, on
 * the device, and stays there for the verifier and the tally; no limb crosses PCIe.  The meaning is that of calls above:
 * WIRE STATUS.  wire_status_out[3k] is the byte vsp_tally_add_blobs gives ciphertext blob k under the same check_subgroup (the count
 * header against msg_size + 2 included); [3k + 1] is the byte vsp_proof_from_blob_batch gives proof k (bits 0..2 and 4..6); [3k + 2]
 * is 0 when vsp_fr_vector_from_blob accepts input blob k with a count of exactly n_rest, else 1 (a wrong header or a scalar >= r).
 * A ballot with any of the three set is WIRE-REJECTED: verdict 0, reason 1; for the screening it is what a malformed ballot is to
 * vsp_saver_verify_batch_screened -- out of every sum and product, and it makes no range fail.
 * VERDICTS.  For every other ballot verdict and reason equal what vsp_saver_verify_batch (coeff NULL: the exact path) or
 * vsp_saver_verify_batch_screened (coeff set) gives on the limbs the decoders produce, every wire-rejected ballot replaced at its own
 * index by a malformed one; options, coefficients and ranges go by the original indices.  All guarantees of the screened call carry
 * over word for word: a verdict of 0 comes from the exact path, no valid ballot is ever rejected, and the SOUNDNESS conditions on the
 * coefficients are unchanged.  SUBGROUP: with check_subgroup = 0 the caller vouches for the subgroups, as for the verify calls.
 * TALLY.  With tally != NULL (its ct_len must be msg_size + 2) every ballot with verdict 1 is added to the handle: afterwards
 * vsp_tally_result is what it would be had vsp_tally_add_blobs been given exactly the ciphertext blobs of those ballots.  Equal
 * ballots, infinity members and a running sum passing through infinity are legal.  A piece is added whole, after its verdicts are
 * known, or not at all: an error leaves the handle as it was after the last complete piece, and *accepted_out says how many ballots
 * (verdict 1, of complete pieces) went in.
 * RETURNS VSP_OK whatever the verdicts are; count = 0 with valid pointers is VSP_OK.  VSP_ERR_ARG before any GPU work for a null ver,
 * ct_blobs, proof_blobs or verdict_out (also with count = 0), a null input_blobs with n_rest > 0, a tally of another ct_len, a
 * verifier of another device, a zero coefficient and, with coeff set, a proof in flight on the context.  VSP_ERR_HIP as elsewhere;
 * after an error nothing stays in flight on the work slots and the context is usable.
 * PIECES of at most min("saver_screen_chunk", "tally_chunk_points" / (msg_size + 2)) ballots when screening; on the exact path
 * "pairing_chunk" and its 2^19-argument bound take the place of "saver_screen_chunk".  A piece is at least one ballot.  Per piece:
 * the ciphertext blobs are decoded and subgroup-checked into a workspace of their own, the proofs behind them, the input blobs by
 * one lane per scalar; the verifier's piece is gathered from the decoded points -- the whole piece first, then the failing
 * sub-ranges for the exact path -- and after the verdicts the accepted ballots' members are summed where they lie.
 * Workspace bound per piece, beside the verifier's own without its canonical upload: per ballot max(8 + 48 (msg_size + 2), 192) raw
 * bytes, 97 (msg_size + 2) bytes of decoded members and their status, 387 bytes of A, B, C and their status, 8 + 64 n_rest bytes of
 * inputs and 5 status bytes; at most 768 KiB of partial sums -- 290 MiB at msg_size 25 with 5 rest inputs and 2^16 ballots.
 * Statistics: the decoding, tally and verify stages feed their existing names ("tally_decode_ms", "tally_subgroup_ms",
 * "g2_decode_ms", "g2_subgroup_ms", "tally_sum_ms", "saver_verify_*", "saver_screen_*"); "saver_receive_prepare_ms" is the time of
 * the two kernels of this section by HIP events, "saver_receive_ballots" the ballots received, "saver_receive_wire_rejected" those
 * wire-rejected. */
int vsp_saver_receive_blobs(vsp_ctx *ctx, const vsp_saver_verifier *ver, vsp_tally *tally /* may be NULL */,
                            const uint8_t *ct_blobs /* host, count x (8 + 48 (msg_size + 2)), back to back */,
                            const uint8_t *proof_blobs /* host, count x 192 */,
                            const uint8_t *input_blobs /* host, count x (8 + 32 n_rest); may be NULL when n_rest = 0 */,
                            size_t count, int check_subgroup,
                            const uint64_t *coeff /* host count x 2, little-endian 128-bit, none zero; NULL = the exact path */,
                            uint8_t *verdict_out /* count */, uint8_t *reason_out /* count, may be NULL */,
                            uint8_t *wire_status_out /* count x 3, may be NULL */, size_t *accepted_out /* may be NULL */);

/* ---- the ballot box: spent serial numbers, eid and rt checked on the GPU -----------------------------------------------
 * vsp_saver_receive_blobs accepts any ballot whose proof verifies against the rest inputs the ballot itself carries.  A ballot box adds
 * the rule that makes the tally mean something (the reference keeps it on chain: voting_admin.sol:112-129): a ballot counts once, and
 * only for this election and this voter list.  The box is a handle over a verifier (which must outlive it, same device) that holds, on
 * the device, the serials of every ballot it has accepted, in ORDINAL order -- a ballot's ordinal is its position among the ballots the
 * box has accepted so far, from 0 -- and an open-addressing table over them (a power of two of slots, at most half full; the first has
 * 2^"ballot_box_table_bits" slots, option read at creation, default 16, 2..30).
 * ROLES.  role[i] says what rest input i is: 0 FREE (ignored), 1 FIXED (must equal expected[4 i ..], a canonical scalar below r), 2 SERIAL.
 * A ballot's serial is its SERIAL inputs, S of them (1..8), concatenated in order.  The reference's rest inputs eid | sn | rt are the roles
 * FIXED, SERIAL, FIXED.  vsp_ballot_box_create: NULL and VSP_ERR_ARG in the last error for a null argument, n_rest = 0 or not the
 * verifier's n_abc - 1 - msg_size, a role above 2, no SERIAL input or more than 8, a FIXED scalar >= r, a verifier of another device.
 * RECEIVING.  vsp_ballot_box_receive_blobs takes the arguments of vsp_saver_receive_blobs (the verifier is the box's) and is the same
 * path.  Walk the ballots in index order, across pieces and across earlier calls on the box: a ballot is ACCEPTED exactly when it is not
 * wire-rejected, its FIXED inputs equal the box's, vsp_saver_verify_batch accepts it (coeff set: the screened call, whose guarantees
 * carry over as for vsp_saver_receive_blobs) and no earlier accepted ballot holds its serial.  Accepted ballots enter the tally and the
 * box, no others do; an invalid ballot never reserves its serial.  verdict_out, the tally, the box's contents, the ordinals and
 * holder_out do not depend on the piece sizes, on how the ballots are split over calls, on coeff being NULL or set, or on how the GPU
 * schedules its lanes.
 * REASONS, the first that applies: 1 wire-rejected; 8 a FIXED input differs; 16 the serial is held by a ballot accepted in an earlier
 * piece or call (such a ballot is not verified: to the verifier it is what a wire-rejected one is -- out of every sum and product, no
 * pairing verdict, no range fails because of it; coefficients and ranges still go by original indices; a piece in which every ballot
 * is turned away before the verifier runs no pairing at all); 2, 4 or 6 the verifier's; 16 the serial is held by an accepted ballot of
 * lower index in the same piece.  holder_out[k] is the holder's ordinal for reason 16 and all-ones otherwise, with one addition.  A
 * ballot that both fails an equation and repeats the serial of an earlier accepted ballot gets 16 when that serial was committed by an
 * earlier piece and the verifier's reason when the holder is in its own piece: reason_out of such ballots is the ONLY output that
 * depends on the piece boundaries.  So that holder_out does not, such a ballot gets the holder's ordinal under either reason (a
 * ballot with reason 2, 4 or 6 whose holder_out is not all-ones is one of them).
 * ATOMICITY.  A piece enters the tally and the box whole or not at all: after an error both are as after the last complete piece (the
 * table is rebuilt from the serials where the piece had claimed slots).  ERRORS as for vsp_saver_receive_blobs, and VSP_ERR_ARG for a
 * null box or input_blobs and a box of another device.  A probe of the table never takes more steps than the table has slots: a full
 * or damaged table is VSP_ERR_HIP with a message that names the ballot box, never a spin.
 * PERSISTENCE.  vsp_ballot_box_serials exports the serials [first, first + count) in ordinal order (count x S x 4 words; VSP_ERR_ARG
 * for a range outside the box).  vsp_ballot_box_add_serials restores them or adds serials in bulk through the same claim: the first
 * occurrence wins and gets the next ordinal, status_out[k] = 1 says serial k was already held (by the box or by a lower index),
 * *added_out how many went in; a scalar >= r is VSP_ERR_ARG before any GPU work.  Exporting box A into a fresh box B gives B the
 * ordinals of A.  vsp_ballot_box_count: accepted ballots; _serial_scalars: S; _device_bytes: device memory the box holds.
 * Statistics: "ballot_box_ms" the box's kernels by HIP events, "ballot_box_mismatched" reason 8, "ballot_box_spent" reason 16,
 * "ballot_box_grown" rebuilds into a larger table. */
typedef struct vsp_ballot_box vsp_ballot_box;
vsp_ballot_box *vsp_ballot_box_create(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *expected /* n_rest x 4 */,
                                      const uint8_t *role /* n_rest */, size_t n_rest);
void vsp_ballot_box_free(vsp_ctx *ctx, vsp_ballot_box *box);
uint64_t vsp_ballot_box_count(const vsp_ballot_box *box);
size_t vsp_ballot_box_serial_scalars(const vsp_ballot_box *box);
size_t vsp_ballot_box_device_bytes(const vsp_ballot_box *box);
int vsp_ballot_box_serials(vsp_ctx *ctx, const vsp_ballot_box *box, uint64_t first, size_t count, uint64_t *out /* count x S x 4 */);
int vsp_ballot_box_add_serials(vsp_ctx *ctx, vsp_ballot_box *box, const uint64_t *serials /* count x S x 4 */, size_t count,
                               uint8_t *status_out /* count: 1 = already held; may be NULL */, size_t *added_out /* may be NULL */);
int vsp_ballot_box_receive_blobs(vsp_ctx *ctx, vsp_ballot_box *box, vsp_tally *tally /* may be NULL */, const uint8_t *ct_blobs,
                                 const uint8_t *proof_blobs, const uint8_t *input_blobs, size_t count, int check_subgroup,
                                 const uint64_t *coeff /* NULL = the exact path */, uint8_t *verdict_out, uint8_t *reason_out /* may be NULL */,
                                 uint8_t *wire_status_out /* may be NULL */, size_t *accepted_out /* may be NULL */,
                                 uint64_t *holder_out /* count, may be NULL */);

/* ---- the voter registry: Pedersen hashes over Jubjub and the Merkle tree of the public keys ----------------------------
 * What the election's set-up and every voter compute outside BLS12-381 (common.hpp:833 pk = hash(sk), :1047 sn = hash(eid | sk),
 * :956-1029 the tree over the public keys, its root rt and a voter's copath): one primitive, the Pedersen hash over Jubjub, the twisted
 * Edwards curve -u^2 + v^2 = 1 + d u^2 v^2 over Fr with d = -10240 / 10241 (order 8 s, s prime; the addition law is complete).
 * THE HASH of a message of n >= 1 bits m_0 .. m_(n-1) under generators G_0 .. G_(g-1): zero bits pad it to whole chunks of 3; chunk c =
 * (m_3c, m_3c+1, m_3c+2) = (s0, s1, s2) encodes (1 - 2 s2)(1 + s0 + 2 s1) and belongs to segment c / 63, window c % 63;
 * P = sum_c enc(c) 2^(4 (c % 63)) G_(c / 63); the digest is the canonical u(P) as 255 bits in four words, bit k of weight 2^k.
 * A message is a row of ceil(n / 64) words, bit k at word k / 64, position k % 64; bits at or above n in the last word are ignored.  A
 * point is 8 words, canonical u | v.  This is the Sapling construction; the reference pins the curve, arity 2, 255-bit digests, the order
 * of the nodes and the blob -- the rest, the generators above all, is the caller's (DESIGN.md 3.6i says which conventions are guesses).
 * vsp_pedersen_create validates the generators on the host (VSP_ERR_ARG and a last error that names the generator for a coordinate >= r,
 * a point off the curve, the identity, a point outside the subgroup of order s; equal or opposite generators are accepted: independence
 * is the caller's business) and builds the window table on the device: per generator 63 windows x {1, 2, 3, 4} 2^(4 j) G as
 * (v + u, v - u, 2 d u v), 24 KiB.  vsp_pedersen_hash_batch: count hashes of nbits bits each; nbits = 0 or above 189 g is VSP_ERR_ARG.
 * A hash is summed by a group of 1, 4, 16 or 64 lanes chosen from the count (option "pedersen_lanes": 0 automatic, 1 / 4 / 16 / 64 forces).
 * THE TREE of depth D over count <= 2^D keys of 255 bits (four words, bit 255 clear; absent keys are zero): level 0 is H(pk_i) over 255
 * bits (hash_leaves = 1, the default of the Python layer) or pk_i itself (0); node i of level l + 1 is H(node(l, 2 i) | node(l, 2 i + 1)),
 * 510 bits, so a registry needs g >= 3.  depth > 24 is VSP_ERR_UNSUPPORTED; count = 0 gives the tree of absent keys.  The levels are built
 * on the device without a host round trip; the top levels run in one single-workgroup launch (option "registry_fused_levels": 0 = the
 * levels of at most four nodes, n > 0 = the top n levels, negative = none).
 * vsp_registry_root: the root and, where asked, rt as the circuit's two public inputs (root mod 2^254 | root >> 254).
 * vsp_registry_nodes: nodes [first, first + count) of a level (0 = leaves).  vsp_registry_paths: for every index x < 2^D the copath
 * node(l, (x >> l) ^ 1), l = 0 .. D - 1 (an index >= 2^D is VSP_ERR_ARG).  THE BLOB: 32 octets a node, leaves first, root last; digest
 * bit b at octet b / 8, bit position 7 - b % 8; the 256th bit is zero.  vsp_registry_from_blob refuses a wrong length and a set 256th
 * bit (VSP_ERR_ARG); with verify = 1 every inner node is compared with the hash of its children and *first_bad_node_out is the lowest
 * index (in blob order) of a node that differs, all-ones when the tree is consistent -- the call returns VSP_OK whatever the verdict.
 * ERRORS as elsewhere: a null pointer is VSP_ERR_ARG also with a count of zero (points_out, rt_scalars_out, first_bad_node_out may be
 * NULL); a count of zero with valid pointers is VSP_OK; a handle made on another device is VSP_ERR_ARG.  Calls on one context run one
 * after the other.  Statistics: "pedersen_ms", "registry_build_ms", "registry_paths_ms", "registry_check_ms": the kernels by HIP events. */
typedef struct vsp_pedersen vsp_pedersen;
int vsp_pedersen_create(vsp_ctx *ctx, const uint64_t *generators /* g x 8 */, size_t g, vsp_pedersen **out);
void vsp_pedersen_free(vsp_ctx *ctx, vsp_pedersen *ped);
size_t vsp_pedersen_generators(const vsp_pedersen *ped);
size_t vsp_pedersen_max_bits(const vsp_pedersen *ped);            /* 189 g */
size_t vsp_pedersen_device_bytes(const vsp_pedersen *ped);
int vsp_pedersen_hash_batch(vsp_ctx *ctx, const vsp_pedersen *ped, const uint64_t *msgs /* count x ceil(nbits / 64) */, size_t nbits, size_t count,
                            uint64_t *digests_out /* count x 4 */, uint64_t *points_out /* count x 8, may be NULL */);
typedef struct vsp_registry vsp_registry;
int vsp_registry_build(vsp_ctx *ctx, const vsp_pedersen *ped, const uint64_t *pks /* count x 4 */, size_t count, unsigned depth, int hash_leaves,
                       vsp_registry **out);
int vsp_registry_from_blob(vsp_ctx *ctx, const vsp_pedersen *ped, const uint8_t *blob, size_t len, unsigned depth, int verify, vsp_registry **out,
                           uint64_t *first_bad_node_out /* ~0 when consistent; may be NULL */);
void vsp_registry_free(vsp_ctx *ctx, vsp_registry *reg);
unsigned vsp_registry_depth(const vsp_registry *reg);
size_t vsp_registry_device_bytes(const vsp_registry *reg);
int vsp_registry_root(vsp_ctx *ctx, const vsp_registry *reg, uint64_t digest_out[4], uint64_t rt_scalars_out[8] /* may be NULL */);
int vsp_registry_nodes(vsp_ctx *ctx, const vsp_registry *reg, unsigned level, uint64_t first, size_t count, uint64_t *out /* count x 4 */);
int vsp_registry_paths(vsp_ctx *ctx, const vsp_registry *reg, const uint64_t *indices, size_t n, uint64_t *siblings_out /* n x depth x 4 */);
size_t vsp_registry_blob_size(unsigned depth);                    /* 32 (2^(depth + 1) - 1) */
int vsp_registry_to_blob(vsp_ctx *ctx, const vsp_registry *reg, uint8_t *out);

/* ---- the voting circuit: the statement of the election's proofs, and its witnesses in batches -------------------------
 * What process_encrypted_input_mode_vote_phase builds (common.hpp:1054-1128): "I know sk and a copath such that H(sk) is a leaf of the
 * tree with root rt, sn = H(eid | sk), and m is my ballot".  PINNED by the reference: the public inputs and their order, m_1 .. m_n |
 * eid_packed (ceil(eid_bits / 254) scalars) | sn_packed (2) | rt_packed (2); the packing in chunks of 254 bits (bit i of a block: scalar
 * i / 254, weight 2^(i % 254)); m = the first n entries of the witness; the rest inputs are what a vsp_ballot_box calls FIXED, SERIAL,
 * FIXED.  The statement's private side and every gadget are this library's (csrc/vote_circuit.h says what each row is): every m_i is 0
 * or 1 and they sum to 1; every private bit is boolean; pk = H(sk) over 255 bits, leaf = H(pk) with hash_leaves (else pk); cur_(l+1) =
 * H(cur_l | sib_l) or H(sib_l | cur_l) by address bit l, cur_depth = rt; sn = H(eid | sk).  H is the hash of `ped`; a digest in the
 * circuit is the canonical 255 bits of u, held below r by a strict comparison.
 * vsp_vote_circuit_create builds the three CSR matrices on the host from the table of `ped` (which must outlive the circuit) and uploads
 * them with vsp_r1cs_upload: vsp_vote_circuit_r1cs is that system, for every prover, generator and checker call.  VSP_ERR_ARG: a null
 * pointer, a handle of another device, fewer than 3 generators, msg_size = 0, eid_bits = 0 or eid_bits + 255 > 189 g; depth > 24 is
 * VSP_ERR_UNSUPPORTED.  vsp_vote_circuit_sizes: rows, public inputs, variables and the entries of A, B, C (any output may be NULL);
 * vsp_vote_circuit_csr copies matrix 0, 1 or 2 out (row_ptr num_constraints + 1, col and coef x 4 words by its entries; columns ascending,
 * column 0 the constant 1).  vsp_vote_circuit_wires: the first index into a witness and the count of a named block.
 * vsp_vote_witness_batch fills the witnesses of `count` ballots (any count, pieces of 64) on the device against a resident registry of
 * the circuit's depth: eid_bits_words ceil(eid_bits / 64) words, sks count x 4 (255 bits), indices the voters' leaves, votes the chosen
 * slot.  status_out[k]: 0 ok; 1 the leaf computed from sk is not the registry's leaf at the index (or a node of the path is not the hash
 * of its children): the witness is all zero; 2 vote >= msg_size, index >= 2^depth or sk >= 2^255: all zero, no GPU work.  VSP_OK whatever
 * the statuses.  The call's device copies of sk, of the chains and of the witnesses are zeroed before it returns.  Statistic
 * "vote_witness_ms": the kernels by HIP events.  vsp_vote_witness_host is the header's one-core host path over the same layout functions
 * from an explicit copath (depth x 4 words), for tests and measurements: nothing switches to it.  leaf_out may be NULL.
 * vsp_vote_cast_batch: count (1..64) ballots = vsp_vote_witness_batch, then vsp_saver_encrypt_batch with m one-hot at the vote over the
 * members of status 0; outputs as vsp_saver_encrypt_batch (any may be NULL) plus status_out; a member of non-zero status gets all-zero
 * outputs.  Option "vote_cast_device" (default 1): the witnesses never leave the device -- in order: the witnesses into the circuit's
 * buffer (vsp_cast_witness_batch_device), the status words to the host, the live members as the `members` map of
 * vsp_saver_encrypt_batch_launch_device, the stream-ordered zeroing of the buffer right behind that launch, the finish, the scatter of
 * the outputs to the members' slots.  With the option 0 the witnesses travel through host memory: to the host, compacted there, and back
 * into the batch prover.  Return codes, statuses and every output byte are the same under both values, under "prove_check_witness" too.
 * Statistics: "vote_witness_d2h_bytes" the witness bytes the vote calls copied to the host, "prove_witness_h2d_bytes" the ones the
 * prover's front half copied back: neither moves across a call with the option 1.
 *
 * The device forms.  (Their names begin vsp_cast_: the vsp_vote_ names above are a closed list.)
 * vsp_cast_witness_batch_device: count (1..64) ballots as vsp_vote_witness_batch, by the same code, but the witnesses stay in the
 * circuit's buffer: *d_witnesses_out is device memory of `count` rows, member k in row k (all zero for a non-zero status), *stride_out =
 * num_vars values a row -- a source for the calls under "WITNESSES IN DEVICE MEMORY", complete on the context's stream.  Only the status
 * words come to the host; the inputs, digests and chains are zeroed before the call returns, as ever.  The rows stay until
 * vsp_cast_witness_release zeroes them (stream-ordered on the context's stream, so it may directly follow a launch that reads them); the
 * next vsp_cast_witness_batch_device, vsp_vote_witness_batch, vsp_vote_cast_batch or vsp_cast_batch_launch on the circuit and
 * vsp_vote_circuit_free release them too.  One context at a time uses a circuit.
 * vsp_cast_batch_launch / _finish: vsp_vote_cast_batch's device path in two halves, so that one thread with two contexts and two circuits
 * builds the witnesses of one batch while the other batch proves.  The launch blocks for the status words alone (status_out is final
 * when it returns) and queues everything else; the finish is vsp_saver_encrypt_batch_finish plus the scatter (outputs as
 * vsp_vote_cast_batch, any may be NULL).  VSP_ERR_ARG: a finish with nothing in flight; a second launch, or any prover, batch or witness
 * check call on that context, while one is in flight -- a batch without a live member included.  The pair takes the device path whatever
 * "vote_cast_device" says. */
typedef struct vsp_vote_circuit vsp_vote_circuit;
enum { VSP_VOTE_M = 0, VSP_VOTE_EID_PACKED = 1, VSP_VOTE_SN_PACKED = 2, VSP_VOTE_RT_PACKED = 3, VSP_VOTE_EID_BITS = 4, VSP_VOTE_SK_BITS = 5,
       VSP_VOTE_ADDRESS_BITS = 6, VSP_VOTE_COPATH_BITS = 7, VSP_VOTE_SN_BITS = 8, VSP_VOTE_RT_BITS = 9 };
int vsp_vote_circuit_create(vsp_ctx *ctx, const vsp_pedersen *ped, size_t msg_size, size_t eid_bits, unsigned depth, int hash_leaves, vsp_vote_circuit **out);
void vsp_vote_circuit_free(vsp_ctx *ctx, vsp_vote_circuit *circ);
const vsp_r1cs *vsp_vote_circuit_r1cs(const vsp_vote_circuit *circ);
int vsp_vote_circuit_sizes(const vsp_vote_circuit *circ, size_t *num_constraints_out, size_t *num_inputs_out, size_t *num_vars_out, size_t nnz_out[3]);
int vsp_vote_circuit_csr(const vsp_vote_circuit *circ, int matrix, uint32_t *row_ptr_out, uint32_t *col_out, uint64_t *coef_out);
int vsp_vote_circuit_wires(const vsp_vote_circuit *circ, int block, size_t *first_out, size_t *count_out);
int vsp_vote_witness_host(const vsp_vote_circuit *circ, const uint64_t *eid_bits_words, const uint64_t sk[4], uint64_t index, uint32_t vote,
                          const uint64_t *copath /* depth x 4 */, uint64_t *witness_out /* num_vars x 4 */, uint64_t leaf_out[4] /* may be NULL */);
int vsp_vote_witness_batch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const uint64_t *eid_bits_words, const uint64_t *sks /* count x 4 */,
                           const uint64_t *indices /* count */, const uint32_t *votes /* count */, size_t count,
                           uint64_t *witnesses_out /* host count x num_vars x 4, canonical */, uint8_t *status_out /* count */);
int vsp_vote_cast_batch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const vsp_saver_pk *spk, const vsp_pk *pk, const uint64_t *eid_bits_words,
                        const uint64_t *sks, const uint64_t *indices, const uint32_t *votes, size_t count /* 1..64 */, const uint64_t *r_enc, const uint64_t *r,
                        const uint64_t *s, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out,
                        uint8_t *status_out /* count */);
int vsp_cast_witness_batch_device(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const uint64_t *eid_bits_words, const uint64_t *sks /* count x 4 */,
                                  const uint64_t *indices /* count */, const uint32_t *votes /* count */, size_t count /* 1..64 */,
                                  const void **d_witnesses_out /* device: count rows */, size_t *stride_out, uint8_t *status_out /* count */);
int vsp_cast_witness_release(vsp_ctx *ctx, vsp_vote_circuit *circ);
int vsp_cast_batch_launch(vsp_ctx *ctx, vsp_vote_circuit *circ, const vsp_registry *reg, const vsp_saver_pk *spk, const vsp_pk *pk, const uint64_t *eid_bits_words,
                          const uint64_t *sks, const uint64_t *indices, const uint32_t *votes, size_t count /* 1..64 */, const uint64_t *r_enc, const uint64_t *r,
                          const uint64_t *s, uint8_t *status_out /* count */);
int vsp_cast_batch_finish(vsp_ctx *ctx, uint64_t *ct_out, uint64_t *A_out, uint64_t *B_out, uint64_t *C_out, uint8_t *proofs_out, uint8_t *ct_blobs_out);

/* ---- SAVER decryption on the GPU: decrypt / verify_decryption<elgamal_verifiable> (common.hpp:1220-1223, 1282-1283) -----------------
 * The last step of the election: opening the aggregated ciphertext that vsp_tally_result returns, and checking a published result.
 * With n = msg_size, G_i = gamma_abc_g1[i], H the generator of G2, V_i = rho_sv_g2[i-1], W_i = rho_rhov_g2[i-1] (the verification key of
 * vsp_saver_keygen) and a ciphertext c_0 | c_1 .. c_n | psi:
 *     nu      = rho c_0                                                   (the decryption proof)
 *     value_i = fexp(ml(c_i, W_i) ml(-nu, V_i)),   base_i = e(G_i, W_i)   i = 1..n
 *     m_i     = the m in [0, max_value] with base_i^m = value_i
 *     verify_decryption:   equation 0   e(nu, H) e(c_0, -rho_g2) = 1        equation i   value_i = base_i^(m_i)
 * Equation i is e(c_i, W_i) e(-nu, V_i) e(-m_i G_i, W_i) = 1 of oracle/saver.py verify_decryption by bilinearity.
 * SUBGROUP.  As for the pairings above, key and ciphertext points are ASSUMED to lie in the order-r subgroups (decode with
 * check_subgroup: vsp_tally_add_blobs checks every ballot); that is also what makes equation i the oracle's.  psi takes no part.
 * A decryptor handle is made of PUBLIC data only -- the secret rho is an argument of vsp_saver_decrypt_batch alone, so a voter who
 * only verifies builds the same object.  Creation validates the key points on the host (canonical, on the curve), prepares the
 * Miller-loop lines of the 2 n + 2 fixed G2 arguments V_i, W_i, H, -rho_g2 (19 584 bytes each, csrc/pairing.h), computes every base_i
 * on the GPU (vsp_saver_decryptor_base returns its 576 bytes: those of vsp_multi_pairing_batch for (G_i, W_i)) and builds the baby-step
 * tables of the discrete logarithm (csrc/gt_dlog.h): per slot B = 2^b entries (fingerprint(base_i^j), j), j < B, sorted by fingerprint
 * on the host once, 12 bytes per entry on the device -- 20 MB at msg_size 25 and b = 16.  The fingerprint of a GT value is the low
 * "saver_decrypt_fp_bits" bits (option, 1..64, default 64, read at creation; small values are a test hook for the collision path)
 * of the low 64 bits of its first coefficient in Montgomery form.  b is option "saver_decrypt_baby_bits" (1..20; 0, the default:
 * ceil(log2(max_value + 1) / 2), kept within 1..20), read at creation; the search then takes ceil((max_value + 1) / B) giant steps,
 * at most 2^24.  NULL and VSP_ERR_ARG in the last error for a null pointer, msg_size outside 1..1022, an option outside its range, more
 * than 2^24 giant steps, a point that is not canonical or not on its curve, and a DEGENERATE key: a G_i, V_i or W_i at infinity or a
 * base_i equal to one.
 * vsp_saver_decrypt_batch opens `count` ciphertexts.  msgs_out[k n + i] is slot i + 1 of ciphertext k, status_out[k n + i]:
 *     0  found
 *     1  no m in [0, max_value] (msgs_out is UINT64_MAX); an m that the last giant step reaches beyond max_value is not a result
 *     2  malformed ciphertext: a coordinate >= p or a point off the curve among c_0 .. c_n.  Every slot of that ciphertext gets 2
 *        (msgs_out UINT64_MAX, nu_out all zero); the others of the batch are unaffected
 * nu_out (count x 12, may be NULL) receives rho c_0 as canonical affine limbs, infinity all zero.  Members at infinity are legal and
 * answer by the equations (an empty tally decrypts to zeros).  The search walks x = value g^k, g = base^(-B), one lane per run of 64
 * giant steps, looks every x up by its fingerprint and CONFIRMS every candidate m = k B + j <= max_value by computing base^m in
 * full: no false positive whatever the fingerprint width, no false negative.  The giant range is launched in pieces until every slot
 * has its result, so a small tally in a large range stops early.  VSP_OK whatever the statuses are.
 * vsp_saver_verify_decryption_batch judges `count` stated results (msgs: canonical scalars, the full width of Fr; nu).  verdict_out[k]
 * is 1 exactly when oracle/saver.py verify_decryption accepts.  reason_out[k] (may be NULL) is 0 for an accepted result; exactly 1 for a
 * malformed one (a coordinate >= p or a point off the curve among c_0 .. c_n and nu, an m_i >= r: no pairing verdict, the rest of the
 * batch unaffected); otherwise bit 1 (value 2) is set when equation 0 fails and bit 2 (value 4) when some slot equation fails.
 * first_bad_slot_out[k] (may be NULL) is the lowest failing slot, 0-based, or UINT32_MAX when none fails (also for a malformed result).
 * No random linear combination: every verdict is exact and independent of the rest of the batch.  It needs no baby table, only the
 * lines and the bases.
 * Both: VSP_ERR_ARG for a null pointer, also with count = 0 (nu_out, reason_out, first_bad_slot_out may be NULL), for a decryptor made
 * on another device and for rho >= r; count = 0 with valid pointers is VSP_OK; VSP_ERR_HIP as elsewhere.
 * Any count: the work runs in pieces of at most "pairing_chunk" ciphertexts (default and maximum 2^14) and at most 65 535 (ciphertext,
 * slot) items (msg_size + 1 per ciphertext, never split).  Workspace bound per piece: 96 canonical + 96 Montgomery bytes per ciphertext
 * member, and 576 Miller + 576 GT + 8 result + 2 status bytes per item -- below 100 MiB of the context's grow-only workspaces whatever
 * count is.  Stage times (HIP events, summed since vsp_stats_reset): vsp_get_stat "saver_decrypt_prepare_ms", "saver_decrypt_values_ms"
 * (Miller loops and final exponentiations), "saver_decrypt_dlog_ms" (the giant search, its waits between launches included),
 * "saver_decrypt_power_ms" (verification: the powers), and of creation "saver_decrypt_table_ms" (the baby-step kernel) and
 * "saver_decrypt_sort_ms" (the host sort, wall time); "saver_decrypt_dlog_launches" counts the launches of the giant search.
 * Three names are CONSTANTS of the search (csrc/gt_dlog.h), not statistics -- vsp_stats_reset does not touch them:
 * "saver_decrypt_run_steps" (giant steps of one lane, 64), "saver_decrypt_block_lanes" (64) and "saver_decrypt_launch_lanes" (2^16:
 * a launch gives every item max(64, floor(2^16 / items / 64) 64) lanes, at most what its range takes). */
typedef struct vsp_saver_decryptor vsp_saver_decryptor;
vsp_saver_decryptor *vsp_saver_decryptor_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_vk_words /* vsp_saver_vk_words(msg_size) */,
                                                const uint64_t *gamma_abc_g1 /* (msg_size + 1) x 12 */, uint64_t max_value);
void vsp_saver_decryptor_free(vsp_ctx *ctx, vsp_saver_decryptor *dec);
size_t vsp_saver_decryptor_msg_size(const vsp_saver_decryptor *dec);
uint64_t vsp_saver_decryptor_max_value(const vsp_saver_decryptor *dec);
unsigned vsp_saver_decryptor_baby_bits(const vsp_saver_decryptor *dec);
int vsp_saver_decryptor_base(const vsp_saver_decryptor *dec, size_t slot /* 0 .. msg_size - 1 */, uint8_t gt_out[576]);
int vsp_saver_decrypt_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t rho[4], const uint64_t *ct /* host count x (msg_size + 2) x 12 */,
                            size_t count, uint64_t *msgs_out /* count x msg_size */, uint64_t *nu_out /* count x 12, may be NULL */,
                            uint8_t *status_out /* count x msg_size */);
int vsp_saver_verify_decryption_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t *ct /* count x (msg_size + 2) x 12 */,
                                      const uint64_t *msgs /* count x msg_size x 4, canonical Fr */, const uint64_t *nu /* count x 12 */, size_t count,
                                      uint8_t *verdict_out /* count */, uint8_t *reason_out /* count, may be NULL */,
                                      uint32_t *first_bad_slot_out /* count, may be NULL */);

/* ---- wire formats of the reference's marshaling_policy (common.hpp:168-203 option::big_endian) --------------------
 * PROVISIONAL where marked: the marshalling sources are absent submodules, and only the proof bytes, the scalar vectors and the head of
 * the verification key (4 bytes, the GT element, three points) are pinned by files of the reference.  The tail of the verification key
 * (vsp_vk_*: count + gamma_ABC_g1 + gamma_g1 and the roles of the three points), the ciphertext vector (vsp_g1_vector_*) and the whole
 * "fast" proving-key layout (vsp_pk_to_blob / vsp_pk_from_blob) are this library's stated guesses: they round-trip with themselves, a
 * blob written by the real upstream cli will most likely be refused.  They stay provisional until a reference-produced blob exists.
 * The marshalling sources are absent submodules; csrc/wire.hip lists, field by field, what the reference's own files pin
 * (proof bytes and the head of the extended verification key: bin/cli/src/data.bin; 8-byte counts and 32-byte scalars:
 * protocol_exec.ipynb) and what is a stated guess.  All host-only except the proving-key pair.
 *   scalar vector   8-byte big-endian count | count x 32-byte big-endian Fr          (primary input, eid, sn, rt, voting result)
 *   G1 vector       8-byte big-endian count | count x 48-byte compressed G1          (the ciphertext)
 *   proof           A (48) | B (96) | C (48), ZCash compressed                       (data.bin[0:192))
 *   verification    head (4) | alpha_g1_beta_g2: 12 x 48-byte LITTLE-endian Fp (576, opaque: the pairing lives on the verifier side) |
 *   key, extended   gamma_g2 (96) | delta_g2 (96) | delta_g1 (48) | count (8) | gamma_ABC_g1 (count x 48) | gamma_g1 (48)
 *   proving key     alpha_g1 beta_g1 (96 each) beta_g2 (192) delta_g1 (96) delta_g2 (192), ZCash UNCOMPRESSED big-endian, then counted
 *   ("fast")        vectors A_query (x 96), B_query (x 192 + 96: G2 | G1), H_query (x 96), L_query (x 96)
 * *_from_blob with a NULL output and a count pointer returns the element count (size query).  VSP_ERR_ARG for malformed input. */
size_t vsp_fr_vector_blob_size(size_t count);
int vsp_fr_vector_to_blob(const uint64_t *vals, size_t count, uint8_t *out);
int vsp_fr_vector_from_blob(const uint8_t *blob, size_t len, uint64_t *vals_out, size_t capacity, size_t *count_out);
size_t vsp_g1_vector_blob_size(size_t count);
int vsp_g1_vector_to_blob(const uint64_t *pts, size_t count, uint8_t *out);
int vsp_g1_vector_from_blob(const uint8_t *blob, size_t len, int check_subgroup, uint64_t *pts_out, size_t capacity, size_t *count_out);
int vsp_proof_to_blob(const uint64_t A[12], const uint64_t B[24], const uint64_t C[12], uint8_t out[192]);
int vsp_proof_from_blob(const uint8_t blob[192], int check_subgroup, uint64_t A[12], uint64_t B[24], uint64_t C[12]);
size_t vsp_vk_blob_size(size_t n_abc);
int vsp_vk_to_blob(uint32_t head, const uint8_t gt[576], const uint64_t gamma_g2[24], const uint64_t delta_g2[24], const uint64_t delta_g1[12],
                   const uint64_t *gamma_abc_g1, size_t n_abc, const uint64_t gamma_g1[12], uint8_t *out);
int vsp_vk_from_blob(const uint8_t *blob, size_t len, int check_subgroup, uint32_t *head, uint8_t gt[576], uint64_t gamma_g2[24], uint64_t delta_g2[24],
                     uint64_t delta_g1[12], uint64_t *gamma_abc_g1, size_t capacity, size_t *n_abc, uint64_t gamma_g1[12]);
/* Proving key: the reference deserialises it inside its timed vote phase (common.hpp:1002-1004; main.cpp:446-456).  vsp_pk_from_blob copies
 * the raw bytes to the GPU once and converts them there (byte order, infinity flags, curve check, Montgomery form, 28-bit-limb table,
 * optionally the window multiples); the result is a resident key (vsp_keypair_pk) without gamma_ABC_g1.  precompute is the bit mask of
 * vsp_groth16_generate (bit 0 = A, both halves of B, L; H stays plain; bits 1..5 one query each).  Records must be well-formed ZCash
 * uncompressed records (no compression or sign flag, an infinity record all zero otherwise), on the curve; queries that keep the plain
 * layout go through the subgroup policy of "bases_check_subgroup".  PROVISIONAL layout (see above). */
size_t vsp_pk_blob_size(const vsp_keypair *kp);
int vsp_pk_to_blob(vsp_ctx *ctx, const vsp_keypair *kp, uint8_t *out);
vsp_keypair *vsp_pk_from_blob(vsp_ctx *ctx, const uint8_t *blob, size_t len, int precompute);

#ifdef __cplusplus
}
#endif
#endif /* VSP_H */
