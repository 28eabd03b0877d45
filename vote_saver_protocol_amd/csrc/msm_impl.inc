// Pippenger (bucket-method) multi-scalar multiplication over BLS12-381 G1 / G2 for gfx950: the half that depends on the field.
//
// Replaces algebra::multiexp<policies::multiexp_method_BDLO12>, multiexp_with_mixed_addition and the
// G2 half of kc_multiexp_with_mixed_addition (crypto3-algebra / crypto3-zk, absent submodules,
// the reference's .gitmodules:8-12; parameter table included at
// bin/cli/include/nil/vote_saver/common.hpp:38, reached from common.hpp:1132-1135).
// The reference algorithm is serial: for each c-bit window, add every base into bucket[digit], then a
// running sum over the buckets, then c doublings between windows.  The value sum_i k_i * P_i is unique
// as an affine point, so any bucket schedule gives bit-identical output after normalisation.
//
// MI355X pipeline (all on one stream, no host round trip until the last few hundred bytes).  Steps 0-2 see scalars, digits and
// 32-bit entries, never a field element: their kernels and the stages that launch them are msm_sort.hip, compiled once for both
// groups (the stages' prototypes and MsmLaunch: common.h).  Steps 3-7 are this include, compiled once per group by msm_g1.hip /
// msm_g2.hip (VSP_MSM_GROUP), so that the two build in parallel; msm_launch<F> below runs the stages of both files in order.
//   0. k_glv_split [msm_sort.hip] (plain resident bases up to 2^20 G1 / 2^18 G2 points) k = k1 + k2 lambda: 2n points (P, phi(P)), signed 127-bit halves
//   1. k_digits    [msm_sort.hip] signed c-bit digits of every scalar (halves the buckets)
//   2. k_count_lds / k_chunk_prefix / scan / k_scatter_lds   [msm_sort.hip] counting sort of point indices (+ sign bit) into bucket order, the
//                  counters of one (chunk, window) in 128 KiB of LDS; k_plan splits buckets larger than T into parts,
//                  k_partsort orders the parts by size
//   3. k_accum28   [here] ONE THREAD (G2: lane pair) PER BUCKET PART: gathers its affine points from the 14 x 28-bit-limb copy of the bases
//                  (128 B / 256 B rows) and folds them with mixed XYZZ additions -- this is where ~80 % of the time goes; it is VALU
//                  integer-multiply bound, not HBM bound.  (k_accum: the same on the 12 x 32-bit form, the fallback and the redo path)
//   4. k_merge_a / k_merge2   [here] buckets that were split (skewed scalars: the 0/1-heavy witnesses of
//                  multiexp_with_mixed_addition) are folded by lane groups or by workgroups, LDS trees
//   5. k_dimsum    [here] the weighted bucket sum  sum_b (b+1) B_b  is decomposed over the 2 (or 3) digits of the bucket
//                  index b = (v1, v0):  plain sums along each digit (lane group + LDS tree per sum),
//   6. k_dimweight [here] then a <=256-term weighted sum per (window, digit) by suffix scan in LDS
//                  (steps 4-6 on the 28-bit form: XYZZ<Fp28> / XYZZ<Fp2x28>, fp28.h)
//   7. host        [here: msm_fold] Horner over W*4 points (c*W doublings) in 64-bit limbs and the affine normalisation
//
// Zero scalars produce no digit and are skipped; scalars equal to one land in one bucket of window 0
// and are summed by steps 3-4 -- the two special cases of multiexp_with_mixed_addition need no
// separate pre-pass.
#include "common.h"
#include "lane_view.h"
#include "fp28.h"
#if VSP_MSM_GROUP == 1
#include "accum28_asm_gfx950.h"
#endif


namespace vsp {
namespace {

// beta of the endomorphism phi(x, y) = (beta x, y) = lambda P (msm_sort.hip k_glv_split), Montgomery form: the cube root of unity in Fp whose
// eigenvalue on this group is that lambda
#if VSP_MSM_GROUP == 1
static constexpr uint32_t GLV_BETA_MONT[12] = {0x8671f071u, 0xcd03c9e4u, 0x1fcda5d2u, 0x5dab2246u, 0xd3851b95u, 0x587042afu, 0x01bacb9eu, 0x8eb60ebeu, 0x83d050d2u, 0x03f97d6eu, 0x54638741u, 0x18f02065u};
#else
static constexpr uint32_t GLV_BETA_MONT[12] = {0x798a64e8u, 0x30f1361bu, 0x7ece5a2au, 0xf3b8ddabu, 0xc61577f7u, 0x16a8ca3au, 0x74fd029bu, 0xc26a2ff8u, 0x60701c6eu, 0x3636b766u, 0x241b6160u, 0x051ba4abu};
#endif
__device__ __forceinline__ Fp glv_beta() { Fp b; for (int i = 0; i < 12; i++) b.l[i] = GLV_BETA_MONT[i]; return b; }
__device__ __forceinline__ void glv_apply(Fp &x) { x = mul(x, glv_beta()); }
__device__ __forceinline__ void glv_apply(Fp2 &x) { Fp b = glv_beta(); x.c0 = mul(x.c0, b); x.c1 = mul(x.c1, b); }
__device__ __forceinline__ void glv_apply(Fp2L &x) { x.v = mul(x.v, glv_beta()); }        // lane pair: each lane scales its own component

// ------------------------------------------------------------------------------------------------
// accumulate: one thread per bucket part, parts taken in descending size order
// waves per SIMD the kernel is compiled for (measured: 2 and 3 waves perform alike -- the kernel is issue bound)
template <class F> struct AccumWaves { static constexpr unsigned W = 2; };
template <class F>
__device__ __forceinline__ XYZZ<typename LaneView<F>::E> accumulate_part(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ off,
                                                const uint32_t *__restrict__ suboff, const uint32_t *__restrict__ part_bucket, uint32_t q,
                                                XYZZ<F> *buckets, XYZZ<F> *partials, bool glv = false) {
    using LV = LaneView<F>; using E = typename LV::E;
    // endomorphism split: entry 2i is P_i, entry 2i + 1 is phi(P_i) = (beta x, y) -- this generic kernel reads the n-row table and scales x
    auto load_entry = [&](uint32_t e) {
        const uint32_t idx = e & 0x7fffffffu;
        Affine<E> p = LV::load(&bases[glv ? (idx >> 1) : idx]);
        if (glv && (idx & 1u)) glv_apply(p.x);                 // infinity stays infinity: beta * 0 = 0
        return p;
    };
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ<E> acc = XYZZ<E>::inf();
    if (start < end) {
        // software pipeline: the next point (and the index after it) is in flight while the current addition runs -- a gather
        // misses L2 (and, with precomputed tables, the Infinity Cache too) and one addition is ~10 us of ALU work
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        Affine<E> p_cur = load_entry(e_cur);
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            Affine<E> p_nxt = p_cur;
            if (more) p_nxt = load_entry(e_nxt);
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            xyzz_madd(acc, p_cur, (e_cur >> 31) != 0);
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    LV::store(parts == 1 ? &buckets[g] : &partials[q], acc);
    return acc;
}
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_accum(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                       const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                       const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                       size_t G, unsigned T, XYZZ<F> *buckets, XYZZ<F> *partials) {
    size_t t = gid<F>();
    if (t >= suboff[G]) return;
    accumulate_part<F>(bases, sorted, off, suboff, part_bucket, perm[t], buckets, partials);
}
// the bucket parts another kernel handed back (k_accum28: equal-x pairs), a small grid striding over the list.  With the 28-bit bucket
// arrays (b28 / p28 not null) the redone part is converted and stored there as well -- one kernel, one wait for a wave slot on a full GPU
#if VSP_MSM_GROUP == 1
using Bucket28 = XYZZ<Fp28>;
__device__ __forceinline__ void store_part28(Bucket28 *dst, const XYZZ<Fp> &a) {
#if defined(__HIP_DEVICE_COMPILE__)
    *dst = xyzz28_from_fp(a);
#endif
}
#else
using Bucket28 = XYZZ<Fp2x28>;
__device__ __forceinline__ void store_part28(Bucket28 *dst, const XYZZ<Fp2L> &a) {      // each lane of the pair converts its own component
#if defined(__HIP_DEVICE_COMPILE__)
    Fp28 *row = reinterpret_cast<Fp28 *>(dst);
    const unsigned comp = threadIdx.x & 1;
    const bool inf = is_inf(a);
    row[comp] = inf ? Fp28::zero() : fp_to_fp28(a.X.v); row[2 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.Y.v);
    row[4 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.ZZ.v); row[6 + comp] = inf ? Fp28::zero() : fp_to_fp28(a.ZZZ.v);
#endif
}
#endif
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_accum_redo(const Affine<F> *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                            const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                            const uint32_t *__restrict__ part_bucket, XYZZ<F> *buckets, XYZZ<F> *partials,
                                                            const uint32_t *redo_list, const uint32_t *redo_count, bool glv, Bucket28 *b28, Bucket28 *p28) {
    const uint32_t count = *redo_count;
    for (size_t t = gid<F>(); t < count; t += (size_t)gridDim.x * blockDim.x / LaneView<F>::LANES) {
        const uint32_t q = redo_list[t];
        auto acc = accumulate_part<F>(bases, sorted, off, suboff, part_bucket, q, buckets, partials, glv);
        if (b28) {
            const uint32_t g = part_bucket[q];
            store_part28(suboff[g + 1] - suboff[g] == 1 ? &b28[g] : &p28[q], acc);
        }
    }
}

#ifndef VSP_ACCUM28_WAVES
#define VSP_ACCUM28_WAVES 2
#endif
#if VSP_MSM_GROUP == 1
// G1: the same accumulation on 14 x 28-bit limbs with lazy reduction (fp28.h) -- a product is 1.38x faster there.  The table is read
// in that form and the bucket parts stay in it: the merges and the bucket reduction are instantiated over XYZZ<Fp28> (fp28.h gives
// it the full addition), and only the four results per window return to the 12 x 32-bit form (k_dimweight's store).
__global__ __launch_bounds__(MSM_THREADS, VSP_ACCUM28_WAVES) void k_accum28_cxx(const Affine28 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp28> *buckets, XYZZ<Fp28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t S = suboff[G];
    if (t >= S) return;
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ28 acc = xyzz28_inf();
    if (start < end) {
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        Affine28 p_cur = bases[e_cur & 0x7fffffffu];
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            Affine28 p_nxt = p_cur;
            if (more) p_nxt = bases[e_nxt & 0x7fffffffu];
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            if (!madd28(acc, p_cur, (e_cur >> 31) != 0)) {      // equal x (doubling / cancellation): the generic kernel redoes this part
                redo_list[atomicAdd(redo_count, 1u)] = q;
                return;
            }
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    XYZZ<Fp28> out; out.X = acc.X; out.Y = acc.Y; out.ZZ = acc.ZZ; out.ZZZ = acc.ZZZ;      // stays in the 28-bit form (infinity: all zero)
    if (parts == 1) buckets[g] = out; else partials[q] = out;
#endif
}
#ifdef VSP_DIAG_CLOCK
__device__ unsigned long long vsp_diag_clock_sums[4];          // shader cycles, 100 MHz ticks, waves (diagnostic build only)
#endif
// The same accumulation through the generated, hand-allocated routine (accum28_asm_gfx950.h, tools/gen_accum28_asm.py): the whole loop of a
// bucket part -- gather of the next point under the current addition, digit sign, points at infinity, the equal-x exit -- in 167 VGPRs, so
// THREE waves share a SIMD.  Measured in shader cycles (tools/ubench_madd28.hip, profiles/r3_ubench_madd28.txt): a wave sharing its SIMD
// with one other takes 1.8 x as long per product as a wave alone, and with two others still 1.8 x -- the third wave is free, which the
// compiler's allocation around the fixed-register product routines (227-238 VGPRs) could not use.  Option "msm_accum28_asm" = 0 runs
// k_accum28_cxx instead; results are identical (same formulas, same column schedule).
__global__ __launch_bounds__(MSM_THREADS, 3) void k_accum28(const Affine28 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp28> *buckets, XYZZ<Fp28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t S = suboff[G];
    if (t >= S) return;
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    const uint32_t end = start + len < b1 ? start + len : b1;
    XYZZ<Fp28> out;
    uint32_t flag;
#ifdef VSP_DIAG_CLOCK
    // DIAGNOSTIC BUILD ONLY (libvsp_hip_diag.so, `make diag`): the clock the chip holds inside this loop = delta s_memtime / delta
    // s_memrealtime x 100 MHz (MI355X_MICROARCH.md, DVFS item 6), stamped once around the loop, summed over waves into a buffer of its own
    unsigned long long dc_t0, dc_r0, dc_t1, dc_r1;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t0), "=s"(dc_r0) :: "memory");
#endif
    accum28_asm(out.X.l, flag, bases, sorted, start, end);           // X | Y | ZZ | ZZZ: 56 consecutive words
#ifdef VSP_DIAG_CLOCK
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t1), "=s"(dc_r1) :: "memory");
    if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {      // first active lane of the wave
        atomicAdd(&vsp_diag_clock_sums[0], dc_t1 - dc_t0); atomicAdd(&vsp_diag_clock_sums[1], dc_r1 - dc_r0); atomicAdd(&vsp_diag_clock_sums[2], 1ull);
    }
#endif
    if (flag) { redo_list[atomicAdd(redo_count, 1u)] = q; return; }  // equal x (doubling / cancellation): the generic kernel redoes this part
    if (parts == 1) buckets[g] = out; else partials[q] = out;
#endif
}
__global__ __launch_bounds__(256) void k_table28(const Affine<Fp> *in, size_t n, Affine28 *out, bool glv) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp> p = in[i];
    Affine28 r;
    r.x = fp_to_fp28(p.x); r.y = fp_to_fp28(p.y);       // infinity (0, 0) stays (0, 0)
    out[glv ? 2 * i : i] = r;
    if (glv) { glv_apply(p.x); r.x = fp_to_fp28(p.x); out[2 * i + 1] = r; }      // phi(P) = (beta x, y); infinity stays infinity (beta * 0 = 0)
#endif
}
#endif

#if VSP_MSM_GROUP == 2
// G2: the accumulation over lane pairs on the 28-bit form (fp28.h: one dual product per Fp2 product and lane); rows of 224 bytes.
// The bucket parts stay in that form (XYZZ<Fp2x28>) through the merges and the bucket reduction, as on G1.
__global__ __launch_bounds__(MSM_THREADS, VSP_ACCUM28_WAVES) void k_accum28(const Affine28x2 *__restrict__ bases, const uint32_t *__restrict__ sorted,
                                                           const uint32_t *__restrict__ off, const uint32_t *__restrict__ suboff,
                                                           const uint32_t *__restrict__ perm, const uint32_t *__restrict__ part_bucket,
                                                           size_t G, unsigned T, XYZZ<Fp2x28> *buckets, XYZZ<Fp2x28> *partials,
                                                           uint32_t *redo_list, uint32_t *redo_count) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t t = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 1;
    const unsigned comp = threadIdx.x & 1;
    uint32_t S = suboff[G];
    if (t >= S) return;                                 // both lanes of a pair leave together
    const uint32_t q = perm[t];
    const uint32_t g = part_bucket[q];
    const uint32_t part = q - suboff[g];
    const uint32_t parts = suboff[g + 1] - suboff[g];
    const uint32_t b0 = off[g], b1 = off[g + 1];
    const uint32_t len = parts == 1 ? b1 - b0 : part_len(b1 - b0, parts);
    uint32_t start = b0 + part * len;
    if (start > b1) start = b1;
    uint32_t end = start + len < b1 ? start + len : b1;
    auto load = [&](uint32_t e) {
        const Fp28 *row = reinterpret_cast<const Fp28 *>(&bases[e & 0x7fffffffu]);      // x.c0, x.c1, y.c0, y.c1
        AffineHalf28 p; p.x = row[comp]; p.y = row[2 + comp]; return p;
    };
    XYZZHalf28 acc = xyzz_half28_inf();
    if (start < end) {
        uint32_t e_cur = sorted[start];
        uint32_t e_nxt = start + 1 < end ? sorted[start + 1] : 0u;
        AffineHalf28 p_cur = load(e_cur);
        for (uint32_t i = start; i < end; i++) {
            const bool more = i + 1 < end;
            AffineHalf28 p_nxt = p_cur;
            if (more) p_nxt = load(e_nxt);
            const uint32_t e_nn = i + 2 < end ? sorted[i + 2] : 0u;
            if (!madd28_g2(acc, p_cur, (e_cur >> 31) != 0)) {        // equal x: the generic kernel redoes this part (one entry per pair)
                if (comp == 0) redo_list[atomicAdd(redo_count, 1u)] = q;
                return;
            }
            p_cur = p_nxt; e_cur = e_nxt; e_nxt = e_nn;
        }
    }
    Fp28 *dst = reinterpret_cast<Fp28 *>(parts == 1 ? &buckets[g] : &partials[q]);      // X.c0, X.c1, Y.c0, Y.c1, ZZ.c0, ...: stays in the 28-bit form
    dst[comp] = acc.X; dst[2 + comp] = acc.Y; dst[4 + comp] = acc.ZZ; dst[6 + comp] = acc.ZZZ;      // infinity: ZZ zero on both lanes
#endif
}
__global__ __launch_bounds__(256) void k_table28(const Affine<Fp2> *in, size_t n, Affine28x2 *out, bool glv) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<Fp2> p = in[i];
    Affine28x2 r;
    r.xc0 = fp_to_fp28(p.x.c0); r.xc1 = fp_to_fp28(p.x.c1); r.yc0 = fp_to_fp28(p.y.c0); r.yc1 = fp_to_fp28(p.y.c1);
    out[glv ? 2 * i : i] = r;
    if (glv) { glv_apply(p.x); r.xc0 = fp_to_fp28(p.x.c0); r.xc1 = fp_to_fp28(p.x.c1); out[2 * i + 1] = r; }
#endif
}
#endif

// workgroup tree reduction of one XYZZ per logical thread; sh: NT entries.
// NT physical threads; with LANES lanes per value the result is valid in the first LANES threads (logical thread 0)
template <class F, unsigned NT>
__device__ __forceinline__ XYZZ<typename LaneView<F>::E> block_sum(XYZZ<typename LaneView<F>::E> acc, XYZZ<typename LaneView<F>::E> *sh) {
    unsigned t = threadIdx.x;
    sh[t] = acc;
    __syncthreads();
    for (unsigned s = NT / 2; s >= LaneView<F>::LANES; s >>= 1) {      // physical stride; lanes of a value keep their parity
        if (t < s) { xyzz_add(acc, sh[t + s]); sh[t] = acc; }
        __syncthreads();
    }
    return acc;
}

// NT physical threads per workgroup (48 KiB of LDS: 192 B per lane either way), NTL logical threads = values per tree
template <class F> struct MsmBlock { static constexpr unsigned NT = 256; static constexpr unsigned NTL = NT / LaneView<F>::LANES; };
// the merges' workgroups (k_merge_a, k_merge2): experiment knob -DVSP_MERGE_NT=64 -- one wave and 14 KiB of LDS per workgroup instead of four and 56 KiB
#ifndef VSP_MERGE_NT
#define VSP_MERGE_NT 256
#endif
template <class F> struct MergeBlock { static constexpr unsigned NT = VSP_MERGE_NT; static constexpr unsigned NTL = NT / LaneView<F>::LANES; };

// merge of split ("heavy") buckets in two stages so that a bucket with thousands of parts (the all-ones bucket of a
// boolean witness) is folded by many workgroups, not one:
//   stage 1: grid (chunks, heavy buckets): each workgroup tree-reduces NT consecutive partials into the chunk's first slot
//   stage 2: one workgroup per heavy bucket tree-reduces the chunk results (stride NT) into the bucket
// (stage 1 shares its launch with the fold of the buckets in few parts, k_merge_a below: disjoint buckets, one wait for wave slots)
// Stage 1's work items are (chunk, heavy bucket) pairs, chunk-major, dealt round-robin to MERGE1_BLOCKS workgroups: one bucket of 10^5
// parts (all the scalars equal to one) and 116 buckets of 550 parts each (the top window of a 19-bit split at 2^23 points: 8 bits of
// digit) both spread over the whole grid.  (A fixed grid of 256 chunks x 4 buckets walked the second case's buckets 29 deep with
// 3 of 256 workgroups busy: 3.8 ms.)
static constexpr unsigned MERGE1_BLOCKS = 1024;
template <class F>
__device__ __forceinline__ void merge1_block(unsigned b, const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                             XYZZ<F> *partials, XYZZ<typename LaneView<F>::E> *sh) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL;
    const uint32_t nh = counters[0], maxparts = counters[4];
    if (!nh || maxparts <= NTL) return;                       // small enough for stage 2 alone
    const uint64_t items = (uint64_t)nh * ((maxparts + NTL - 1) / NTL);
    for (uint64_t i = b; i < items; i += MERGE1_BLOCKS) {
        const uint32_t h = (uint32_t)(i % nh), k = (uint32_t)(i / nh);
        const uint32_t g = heavy[h];
        const uint32_t q0 = suboff[g], q1 = suboff[g + 1];
        if (q1 - q0 <= NTL) continue;
        const uint64_t c0 = (uint64_t)q0 + (uint64_t)k * NTL;
        if (c0 >= q1) continue;
        const uint32_t q = (uint32_t)c0 + lid<F>();
        XYZZ<E> acc = q < q1 ? LV::load(&partials[q]) : XYZZ<E>::inf();
        acc = block_sum<F, NT>(acc, sh);
        if (lid<F>() == 0) LV::store(&partials[c0], acc);
        __syncthreads();
    }
}
template <class F>
__global__ __launch_bounds__(MergeBlock<F>::NT, 2) void k_merge2(const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                                             const XYZZ<F> *partials, XYZZ<F> *buckets) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL;
    __shared__ XYZZ<E> sh[NT];
    uint32_t nh = counters[0];
    for (uint32_t h = blockIdx.x; h < nh; h += gridDim.x) {
        uint32_t g = heavy[h];
        uint32_t q0 = suboff[g], q1 = suboff[g + 1];
        const uint32_t stride = (q1 - q0 <= NTL) ? 1u : NTL;  // after stage 1 only every NTL-th slot is live
        XYZZ<E> acc = XYZZ<E>::inf();
        for (uint32_t q = q0 + lid<F>() * stride; q < q1; q += NTL * stride) xyzz_add(acc, LV::load(&partials[q]));
        acc = block_sum<F, NT>(acc, sh);
        if (lid<F>() == 0) LV::store(&buckets[g], acc);
        __syncthreads();
    }
}

// buckets split in a few parts (2..MERGE_SMALL): LPB logical lanes fold one bucket -- a serial prefix of parts / LPB additions, then a
// log2(LPB)-level tree through LDS.  (One lane per bucket, the earlier form, is a chain of up to 15 additions: a SINGLE such bucket
// in a plain multi-exponentiation held the stream for 0.55 ms on G2.)  launch_tail picks LPB from the expected parts per bucket:
// 16 where only outliers are split, 1 (no tree, no LDS) where every bucket is cut in two or three, 4 in between and in the shared-set mode.
// One launch: the first `small_blocks` workgroups fold the buckets in few parts, the last MERGE1_BLOCKS run stage 1 of the heavy ones.
template <class F, unsigned LPB>
__global__ __launch_bounds__(MergeBlock<F>::NT, 2) void k_merge_a(const uint32_t *medium, const uint32_t *heavy, const uint32_t *counters, const uint32_t *suboff,
                                                                XYZZ<F> *partials, XYZZ<F> *buckets, unsigned small_blocks) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MergeBlock<F>::NT, NTL = MergeBlock<F>::NTL, PER_BLOCK = NTL / LPB;
    __shared__ XYZZ<E> sh[NT];
    if (blockIdx.x >= small_blocks) {                        // uniform over the workgroup
        const unsigned b = blockIdx.x - small_blocks;
        merge1_block<F>(b, heavy, counters, suboff, partials, sh);
        return;
    }
    const uint32_t nm = counters[2];
    const unsigned lt = lid<F>(), lane = lt % LPB, slot = lt / LPB;
    for (size_t base = (size_t)blockIdx.x * PER_BLOCK; base < nm; base += (size_t)small_blocks * PER_BLOCK) {      // uniform over the block
        const size_t t = base + slot;
        const bool live = t < nm;
        const uint32_t g = live ? medium[t] : 0u;
        const uint32_t q0 = live ? suboff[g] : 0u, q1 = live ? suboff[g + 1] : 0u;
        XYZZ<E> acc = XYZZ<E>::inf();
        for (uint32_t q = q0 + lane; q < q1; q += LPB) xyzz_add(acc, LV::load(&partials[q]));
        if constexpr (LPB > 1) {
            sh[threadIdx.x] = acc;
            __syncthreads();
            for (unsigned s = LPB / 2; s >= 1; s >>= 1) {       // lanes of a value keep their parity: physical stride s * LANES
                if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LV::LANES]); sh[threadIdx.x] = acc; }
                __syncthreads();
            }
        }
        if (live && lane == 0) LV::store(&buckets[g], acc);
    }
}

// ---- precomputation of the window multiples of resident bases: out = 2^c * in (XYZZ), then batch-normalised to affine
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_shift_window(const Affine<F> *in, size_t n, unsigned c, XYZZ<F> *out) {
    using LV = LaneView<F>; using E = typename LV::E;
    size_t i = gid<F>();
    if (i >= n) return;
    XYZZ<E> acc = xyzz_from_affine(LV::load(&in[i]));
    for (unsigned k = 0; k < c; k++) acc = xyzz_dbl(acc);
    LV::store(&out[i], acc);
}
static constexpr unsigned PRE_CHUNK = 32;
template <class F>
__global__ __launch_bounds__(64) void k_batch_affine_mont(const XYZZ<F> *in, size_t n, F *pre, Affine<F> *out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = t * PRE_CHUNK, e = b + PRE_CHUNK < n ? b + PRE_CHUNK : n;
    if (b >= n) return;
    F acc = F::one();
    for (size_t i = b; i < e; i++) {
        pre[i] = acc;
        F z = in[i].ZZZ;
        if (!is_zero(z)) acc = mul(acc, z);
    }
    F ai = inv(acc);
    for (size_t i = e; i-- > b;) {
        XYZZ<F> p = in[i];
        Affine<F> r;
        if (is_zero(p.ZZ)) { r.x = F::zero(); r.y = F::zero(); }
        else {
            F zi3 = mul(ai, pre[i]);
            ai = mul(ai, p.ZZZ);
            F zi = mul(zi3, p.ZZ);
            F zi2 = sqr(zi);
            r.x = mul(p.X, zi2);
            r.y = mul(p.Y, zi3);
        }
        out[i] = r;
    }
}

// ---- bucket reduction.  sum_b (b + 1) B_b over the 2^(c-1) buckets of a window is decomposed over the DIGITS of the bucket index
// b = (v2, v1, v0) (q2 + q1 + q0 = c - 1 bits; q2 = 0: two digits): with A_d[v] = the plain sum of the buckets whose digit d is v,
//     sum_b (b + 1) B_b = 2^(q1+q0) sum_v v A_2[v] + 2^q0 sum_v v A_1[v] + sum_v v A_0[v] + sum_b B_b.
// Every bucket goes into one plain sum per digit, so TWO digits cost two additions per bucket instead of three; the digits then
// have up to 2^8 values, which k_dimweight's 256-term trees still take (G1; the lane-pair G2 kernels have 128 slots and keep three
// digits at c = 16).  Why not the reference's running sum: that is one serial chain of 2^c additions per window.
__host__ __device__ __forceinline__ unsigned dims_n2(const MsmGeom &g) { return g.q2 ? (1u << g.q2) : 0u; }
__host__ __device__ __forceinline__ unsigned dims_per_w(const MsmGeom &g) { return (1u << g.q0) + (1u << g.q1) + dims_n2(g); }
// dimbits: the last step is k_dimbits (one wave per digit bit, any number of digit values), not k_dimweight (a tree of at most NTL values):
// two digits of up to 12 bits then serve windows of up to 25 bits with TWO additions per bucket
template <class F> static void split_digits(MsmGeom &g, bool dimbits) {
    const unsigned qb = g.c - 1;
    unsigned maxq = 0; while ((2u << maxq) <= MsmBlock<F>::NTL) maxq++;          // log2 of the slots of a k_dimweight tree
    if (qb <= 2 * maxq || (dimbits && qb <= 24)) { g.q0 = (qb + 1) / 2; g.q1 = qb - g.q0; g.q2 = 0; }
    else { g.q0 = qb / 3; g.q1 = (qb - g.q0) / 2; g.q2 = qb - g.q0 - g.q1; }
    g.bd = (g.q2 == 0 && g.q0 > 8) ? 12u : 8u;
}

// dimension sums A_d[v], dims[w][slot], slot = d-offset + v.  One sum = `items` = B >> q_d buckets.  A sum is folded by LPS lanes
// (logical lanes: a G2 value takes a lane pair): each lane adds items / LPS buckets serially, then a log2(LPS)-level tree through
// LDS.  Several sums share a wave (64 / LANES / LPS of them), one wave per workgroup.  Measured on the plain-bases 2^20 MSM
// (16 windows x 32768 buckets): the earlier form -- one 256-thread workgroup per sum, 4 serial additions and an 8-level tree in
// which half of the remaining lanes idle at every level -- spent 1.17 ms here, 43 % of the accumulation kernel's time, for 1 / 7 of
// its additions; serial prefixes of 8-16 additions per lane keep the lanes busy.
// LPS is chosen at launch (launch_tail): e.g. the whole wave for the single bucket set of the window-multiple mode (384 sums: 96 waves
// at 16 lanes per sum was a 20-addition serial chain on a tenth of the GPU, 280 us; 64 us with 64 lanes).
// (measured, dense 8-window case, 12 x 32-bit field: 32 lanes per sum = 1536 waves took 548 us against 404 us at 16 lanes = 768 waves --
// a second wave on a SIMD halves the speed of both; the 28-bit routines leave a lone wave at half the issue rate, so two per SIMD are free)
template <class F> struct DimSumWaves { static constexpr unsigned MAX = 1024; };
template <> struct DimSumWaves<Fp28> { static constexpr unsigned MAX = 2048; };
template <> struct DimSumWaves<Fp2x28> { static constexpr unsigned MAX = 2048; };
template <class F, unsigned LPS>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimsum(const XYZZ<F> *buckets, MsmGeom g, XYZZ<F> *dims) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LANES = LV::LANES, SPW = 64 / LANES / LPS;
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1;
    const unsigned per_w = dims_per_w(g);
    const unsigned lt = threadIdx.x / LANES;                  // logical lane of the wave
    const unsigned lane = lt % LPS;
    const unsigned sum_id = blockIdx.x * SPW + lt / LPS;
    const bool live = sum_id < g.Wr * per_w;
    const unsigned w = live ? sum_id / per_w : 0;
    const unsigned slot = live ? sum_id % per_w : 0;
    unsigned d, v;
    if (slot < n0) { d = 0; v = slot; } else if (slot < n0 + n1) { d = 1; v = slot - n0; } else { d = 2; v = slot - n0 - n1; }
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const unsigned items = live ? g.B >> qd : 0;
    const XYZZ<F> *bw = buckets + (size_t)w * g.B;
    XYZZ<E> acc = XYZZ<E>::inf();
    for (unsigned i = lane; i < items; i += LPS) {
        unsigned idx;
        if (d == 0) idx = (i << g.q0) | v;
        else if (d == 1) idx = ((i >> g.q0) << (g.q1 + g.q0)) | (v << g.q0) | (i & (n0 - 1));
        else idx = (v << (g.q1 + g.q0)) | i;
        xyzz_add(acc, LV::load(&bw[idx]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = LPS / 2; s >= 1; s >>= 1) {               // lanes of a value keep their parity: physical stride s * LANES
        if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (live && lane == 0) LV::store(&dims[(size_t)w * per_w + slot], acc);
}

// The same sums with a lane count PER DIGIT (round 3).  The sums of one digit run over 2^(other digits' bits) buckets each, so with two
// digits of 7 and 8 bits half of the sums are twice as long as the others; one lane count for all either leaves the short sums' lanes
// idle in the tree or puts 1.5 waves on every SIMD -- and a second wave on a SIMD nearly halves the speed of both (a lone wave takes
// 84 % of the multiplier's issue slots, DESIGN.md 3.1e).  Measured on the dense 8-window case: 32 lanes for every sum (1536 waves)
// 321 us, 16 lanes (768 waves) 284 us, 64 lanes 385 us, 8 lanes 478 us.  Here every digit gets items / 8 lanes (7 serial additions, then
// the tree): 32 lanes for the 256-bucket sums, 16 for the 128-bucket ones = 1024 waves, one per SIMD, 12-13 dependent additions.
// Block b serves digit d when wave0[d] <= b < wave0[d + 1]; one wave per block.
struct DimSumPlan { unsigned lps[3]; unsigned wave0[4]; };
template <class F, bool PREFETCH>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimsum_mixed(const XYZZ<F> *buckets, MsmGeom g, XYZZ<F> *dims, DimSumPlan pl) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LANES = LV::LANES, LL = 64 / LANES;
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1, n2 = dims_n2(g);
    const unsigned per_w = dims_per_w(g);
    const unsigned d = blockIdx.x < pl.wave0[1] ? 0u : (blockIdx.x < pl.wave0[2] ? 1u : 2u);      // uniform over the block
    const unsigned LPS = pl.lps[d], SPW = LL / LPS;
    const unsigned nd = d == 0 ? n0 : (d == 1 ? n1 : n2), base = d == 0 ? 0u : (d == 1 ? n0 : n0 + n1);
    const unsigned lt = threadIdx.x / LANES;                  // logical lane of the wave
    const unsigned lane = lt % LPS;
    const unsigned id = (blockIdx.x - pl.wave0[d]) * SPW + lt / LPS;      // sum of this digit: (window, value)
    const bool live = id < g.Wr * nd;
    const unsigned w = live ? id / nd : 0, v = live ? id % nd : 0;
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const unsigned items = live ? g.B >> qd : 0;
    const XYZZ<F> *bw = buckets + (size_t)w * g.B;
    auto index_of = [&](unsigned i) {
        if (d == 0) return (i << g.q0) | v;
        if (d == 1) return ((i >> g.q0) << (g.q1 + g.q0)) | (v << g.q0) | (i & (n0 - 1));
        return (v << (g.q1 + g.q0)) | i;
    };
    // PREFETCH (G1, option "msm_dimsum_prefetch" = 1; default 0): the next bucket is requested before the current addition starts -- two
    // records live across the field routines.  Round 3 measured this loop 297 -> 250 us and WRONG on doubling-heavy inputs; the cause was the
    // toolchain's machine scheduler (csrc/Makefile SOUND, DESIGN.md 3.7), not the loop: built without that scheduler it passes the probe, the
    // fuzzer and the suite -- and spills 42 registers, which makes it 5 % SLOWER than the plain loop (336 against 319 us, same box,
    // tools/gpu_r4k.sh).  Both are compiled; the plain loop runs.  Lane pairs (G2) have the plain loop only.
    XYZZ<E> acc = XYZZ<E>::inf();
    if constexpr (LANES == 1 && PREFETCH) {
        XYZZ<E> nxt = lane < items ? LV::load(&bw[index_of(lane)]) : XYZZ<E>::inf();
        for (unsigned i = lane; i < items; i += LPS) {
            const XYZZ<E> cur = nxt;
            if (i + LPS < items) nxt = LV::load(&bw[index_of(i + LPS)]);
            xyzz_add(acc, cur);
        }
    } else {
        for (unsigned i = lane; i < items; i += LPS) xyzz_add(acc, LV::load(&bw[index_of(i)]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s = LPS / 2; s >= 1; s >>= 1) {               // lanes of a value keep their parity: physical stride s * LANES
        if (lane < s) { xyzz_add(acc, sh[threadIdx.x + s * LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (live && lane == 0) LV::store(&dims[(size_t)w * per_w + base + v], acc);
}
// The same sums, the same lane count per digit, the same additions -- with the TREE packed onto as few waves as it has live additions
// (one-lane fields; option "msm_dimsum_dense", default 1).  In k_dimsum_mixed a tree level leaves 1/2, 1/4, ... of a wave's lanes live, and
// an EXEC-masked full addition takes the issue slots of a dense one: at 32 lanes per sum a wave issues 7 serial + 5 tree additions.  Here a
// workgroup is four such waves (256 threads, the partial sums in LDS: 256 x 224 B, the footprint of k_merge_a) and a tree level is
// renumbered: its A = (sums of the block) x s live additions sit on threads 0 .. A - 1 -- thread j folds lanes l = j % s and l + s of sum
// j / s -- and a wave without a live addition only reaches the barrier.  4 x 7 + (2 + 1 + 1 + 1 + 1) = 34 wave-additions per block against
// 4 x 12 at 32 lanes per sum, 4 x 7 + (2 + 1 + 1 + 1) = 33 against 4 x 11 at 16: 27 % fewer at c = 16.  The dependent chain is as long as
// before (the serial prefix, then log2(LPS) levels, one barrier each).  Within a level the slot (sum, l) is read and written by its own
// thread only and the slot (sum, l + s) is read only: no hazard inside a level.
// Block b serves digit d when blk0[d] <= b < blk0[d + 1]; the sums of a digit are dealt to whole blocks (a ragged last block per digit).
struct DimSumDensePlan { unsigned lps[3]; unsigned blk0[4]; };
static constexpr unsigned DIMSUM_DENSE_NT = 256;
template <class F>
__global__ __launch_bounds__(DIMSUM_DENSE_NT, AccumWaves<F>::W) void k_dimsum_dense(const XYZZ<F> *buckets, MsmGeom g, XYZZ<F> *dims, DimSumDensePlan pl) {
    using LV = LaneView<F>; using E = typename LV::E;
    static_assert(LV::LANES == 1, "the lane-pair form keeps k_dimsum_mixed");
    constexpr unsigned NT = DIMSUM_DENSE_NT;
    __shared__ XYZZ<E> sh[NT];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1, n2 = dims_n2(g);
    const unsigned per_w = dims_per_w(g);
    const unsigned d = blockIdx.x < pl.blk0[1] ? 0u : (blockIdx.x < pl.blk0[2] ? 1u : 2u);        // uniform over the block
    const unsigned LPS = pl.lps[d], SPB = NT / LPS;                                               // sums per block
    const unsigned nd = d == 0 ? n0 : (d == 1 ? n1 : n2), base = d == 0 ? 0u : (d == 1 ? n0 : n0 + n1);
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const unsigned id0 = (blockIdx.x - pl.blk0[d]) * SPB;                                         // first sum of this block: (window, value)
    const unsigned lane = threadIdx.x % LPS;
    {
        const unsigned id = id0 + threadIdx.x / LPS;
        const bool live = id < g.Wr * nd;
        const unsigned w = live ? id / nd : 0, v = live ? id % nd : 0;
        const unsigned items = live ? g.B >> qd : 0;
        const XYZZ<F> *bw = buckets + (size_t)w * g.B;
        auto index_of = [&](unsigned i) {
            if (d == 0) return (i << g.q0) | v;
            if (d == 1) return ((i >> g.q0) << (g.q1 + g.q0)) | (v << g.q0) | (i & (n0 - 1));
            return (v << (g.q1 + g.q0)) | i;
        };
        XYZZ<E> acc = XYZZ<E>::inf();
        for (unsigned i = lane; i < items; i += LPS) xyzz_add(acc, LV::load(&bw[index_of(i)]));
        sh[threadIdx.x] = acc;
    }
    __syncthreads();
    const unsigned wave_first = threadIdx.x & ~63u;                                              // uniform over the wave
    for (unsigned s = LPS / 2; s >= 1; s >>= 1) {
        const unsigned A = SPB * s;                                                               // live additions of this level
        if (wave_first < A) {                                                                     // a wave above them only reaches the barrier
            const unsigned j = threadIdx.x;
            if (j < A) {
                const unsigned slot = (j / s) * LPS + j % s;
                XYZZ<E> acc = sh[slot];
                xyzz_add(acc, sh[slot + s]);
                if (s > 1) sh[slot] = acc;
                else {                                                                            // thread j holds sum id0 + j
                    const unsigned id = id0 + j;
                    if (id < g.Wr * nd) LV::store(&dims[(size_t)(id / nd) * per_w + base + id % nd], acc);
                }
            }
        }
        __syncthreads();
    }
}
template <class F> static DimSumPlan dimsum_plan(const MsmGeom &g, unsigned MAXW = 1024) {      // wave0[3] == 0: no plan; MAXW 1024 = one wave per SIMD of an MI355X
    constexpr unsigned LL = 64 / LaneView<F>::LANES;
    const unsigned nd[3] = {1u << g.q0, 1u << g.q1, dims_n2(g)};
    const unsigned qd[3] = {g.q0, g.q1, g.q2};
    DimSumPlan pl;
    auto lg2 = [](unsigned x) { unsigned l = 0; while ((1u << l) < x) l++; return l; };
    auto waves_of = [&](unsigned d, unsigned lps) { return nd[d] ? (unsigned)(((size_t)g.Wr * nd[d] * lps + LL - 1) / LL) : 0u; };
    auto steps_of = [&](unsigned d, unsigned lps) { const unsigned items = g.B >> qd[d]; return nd[d] ? (items + lps - 1) / lps + lg2(lps) : 0u; };
    for (unsigned d = 0; d < 3; d++) {
        unsigned l = (g.B >> qd[d]) / 8; if (l < 8) l = 8; if (l > LL) l = LL;
        unsigned p = 8; while (p * 2 <= l) p *= 2;
        pl.lps[d] = nd[d] ? p : 8;
    }
    auto total = [&]() { return waves_of(0, pl.lps[0]) + waves_of(1, pl.lps[1]) + waves_of(2, pl.lps[2]); };
    // more sums than one wave per SIMD serves at 8 items per lane (wide windows, many bucket sets): several rounds are unavoidable and
    // the one-count-for-all choice of launch_tail, which prices the rounds, stays in charge
    if (total() > MAXW) { pl.wave0[3] = 0; return pl; }
    for (int guard = 0; guard < 16; guard++) {                       // room left: more lanes where the chain is longest, while that shortens it
        int pick = -1;
        for (unsigned d = 0; d < 3; d++) {
            if (!nd[d] || pl.lps[d] >= LL || steps_of(d, pl.lps[d] * 2) >= steps_of(d, pl.lps[d])) continue;
            if (total() - waves_of(d, pl.lps[d]) + waves_of(d, pl.lps[d] * 2) > MAXW) continue;
            if (pick < 0 || steps_of(d, pl.lps[d]) > steps_of((unsigned)pick, pl.lps[pick])) pick = (int)d;
        }
        if (pick < 0) break;
        pl.lps[pick] *= 2;
    }
    pl.wave0[0] = 0;
    for (unsigned d = 0; d < 3; d++) pl.wave0[d + 1] = pl.wave0[d] + waves_of(d, pl.lps[d]);
    return pl;
}

// per (window, digit): D = sum_v v * A[v]  and  Tot = sum_v A[v]  by suffix scan + tree sum in LDS.
// winres[w][d] = D_d (d = 0,1,2; with two digits D_2 stays the all-zero record = infinity), winres[w][3] = Tot
// the window results leave in the 12 x 32-bit form the host folds (from the 28-bit form: one conversion per result)
template <class F> struct WinOut { using type = F; };
template <> struct WinOut<Fp28> { using type = Fp; };
template <> struct WinOut<Fp2x28> { using type = Fp2; };
template <class F> __device__ __forceinline__ void store_win(XYZZ<F> *p, const XYZZ<typename LaneView<F>::E> &v) { LaneView<F>::store(p, v); }
__device__ __forceinline__ void store_win(XYZZ<Fp> *p, const XYZZ<Fp28> &v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *p = xyzz28_to_fp(v);
#endif
}
__device__ __forceinline__ void store_win(XYZZ<Fp2> *p, const XYZZ<Fp28L> &v) {      // each lane of the pair converts and writes its component
#if defined(__HIP_DEVICE_COMPILE__)
    Fp *row = reinterpret_cast<Fp *>(p);
    const unsigned comp = threadIdx.x & 1;
    const bool inf = pair_all28(fp28_all_zero(v.ZZ.v));
    row[comp] = inf ? Fp::zero() : fp28_to_fp(v.X.v); row[2 + comp] = inf ? Fp::zero() : fp28_to_fp(v.Y.v);
    row[4 + comp] = inf ? Fp::zero() : fp28_to_fp(v.ZZ.v); row[6 + comp] = inf ? Fp::zero() : fp28_to_fp(v.ZZZ.v);
#endif
}
template <class F>
__global__ __launch_bounds__(MsmBlock<F>::NT, 2) void k_dimweight(const XYZZ<F> *dims, MsmGeom g, XYZZ<typename WinOut<F>::type> *winres) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned NT = MsmBlock<F>::NT, NTL = MsmBlock<F>::NTL;
    __shared__ XYZZ<E> sh[NT];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1, n2 = dims_n2(g);
    const unsigned per_w = dims_per_w(g);
    const unsigned w = blockIdx.x / 3u, d = blockIdx.x % 3u;
    if (d == 2 && !g.q2) {                                   // two digits: D_2 = infinity (uniform over the workgroup)
        if (lid<F>() == 0) store_win(&winres[(size_t)w * 4 + 2], XYZZ<E>::inf());
        return;
    }
    const unsigned cntv = d == 0 ? n0 : (d == 1 ? n1 : n2);
    const unsigned doff = d == 0 ? 0 : (d == 1 ? n0 : n0 + n1);
    const unsigned t = lid<F>();                          // logical thread = digit value
    XYZZ<E> x = t < cntv ? LV::load(&dims[(size_t)w * per_w + doff + t]) : XYZZ<E>::inf();
    sh[at<F>(t)] = x;
    __syncthreads();
    for (unsigned s = 1; s < cntv; s <<= 1) {            // inclusive suffix scan: x[t] = sum_{u >= t} A[u]
        XYZZ<E> y = (t + s < NTL) ? sh[at<F>(t + s)] : XYZZ<E>::inf();
        __syncthreads();
        xyzz_add(x, y);
        sh[at<F>(t)] = x;
        __syncthreads();
    }
    XYZZ<E> tot = sh[at<F>(0)];
    __syncthreads();
    XYZZ<E> acc = (t >= 1 && t < cntv) ? x : XYZZ<E>::inf();   // sum_{v>=1} suffix[v] = sum_v v*A[v]
    acc = block_sum<F, NT>(acc, sh);
    if (t == 0) {
        store_win(&winres[(size_t)w * 4 + d], acc);
        if (d == 0) store_win(&winres[(size_t)w * 4 + 3], tot);
    }
}

// The same weighted sums WITHOUT the weights: sum_v v A[v] = sum_j 2^j S_j with S_j = the plain sum of the A[v] whose digit value v has
// bit j set.  One wave per (window, digit, bit) folds its <= 128 values in ONE tree (7-9 dependent additions where k_dimweight's
// suffix scan + tree is 16), and the powers of two cost nothing: the host's Horner chain doubles once per bit position anyway and
// takes S_j at position (shift of the digit) + j.  The host pays c - 4 more additions per window, so launch_tail uses this form
// where that is cheap: G1 always (0.56 us per host addition), G2 when all windows share one bucket set.
// winres[w][DIMBITS_STRIDE]: [bd d + j] = S_{d,j} (bd = 8 slots per digit, or 12 with two wide digits: MsmGeom.bd), [24] = Tot (the plain sum of every bucket of the window).
static constexpr unsigned DIMBITS_STRIDE = 25;
// One WAVE per sum (a 256-thread workgroup per sum holds four 250-register wave slots and 57 KiB of LDS for a 7-level tree of 128
// values: with 25 sums per window that took a fifth of the throughput of concurrent proofs): a lane adds its 2 (Tot: 4) values, then
// a log2(lanes)-level tree through 14 KiB of LDS.
template <class F>
__global__ __launch_bounds__(64, AccumWaves<F>::W) void k_dimbits(const XYZZ<F> *dims, MsmGeom g, XYZZ<typename WinOut<F>::type> *winres) {
    using LV = LaneView<F>; using E = typename LV::E;
    constexpr unsigned LL = 64 / LV::LANES;                      // logical lanes of the wave
    __shared__ XYZZ<E> sh[64];
    const unsigned n0 = 1u << g.q0, n1 = 1u << g.q1;
    const unsigned per_w = dims_per_w(g);
    const unsigned w = blockIdx.x / DIMBITS_STRIDE, slot = blockIdx.x % DIMBITS_STRIDE;
    // Tot = the plain sum of the values of ANY one digit (each digit's values partition the buckets): the digit with the fewest values
    // (two digits: q1 <= q0; three: q0 <= q1 <= q2, split_digits) keeps this sum as deep as the bit sums -- 128 values at c = 16, not digit 0's 256
    const unsigned dtot = g.q2 ? 0u : 1u;
    const unsigned d = slot == 24 ? dtot : slot / g.bd, j = slot % g.bd;
    const unsigned qd = d == 0 ? g.q0 : (d == 1 ? g.q1 : g.q2);
    const bool live = slot == 24 || (d < 3 && j < qd);           // uniform over the workgroup
    const unsigned doff = d == 0 ? 0 : (d == 1 ? n0 : n0 + n1);
    const unsigned count = !live ? 0u : (slot == 24 ? (1u << qd) : (1u << (qd - 1)));      // values in this sum
    const unsigned t = threadIdx.x / LV::LANES;
    XYZZ<E> acc = XYZZ<E>::inf();
    for (unsigned u = t; u < count; u += LL) {
        // Tot: every value of digit 0.  Bit j: the u-th value with bit j set
        const unsigned v = slot == 24 ? u : (((u >> j) << (j + 1)) | (1u << j) | (u & ((1u << j) - 1u)));
        xyzz_add(acc, LV::load(&dims[(size_t)w * per_w + doff + v]));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (unsigned s2 = LL / 2; s2 >= 1; s2 >>= 1) {               // lanes of a value keep their parity: physical stride s2 * LANES
        if (t < s2) { xyzz_add(acc, sh[threadIdx.x + s2 * LV::LANES]); sh[threadIdx.x] = acc; }
        __syncthreads();
    }
    if (t == 0) store_win(&winres[(size_t)w * DIMBITS_STRIDE + slot], acc);      // dead slots: infinity
}

// canonical affine (host layout) -> Montgomery affine, with the boundary checks include/vsp.h promises:
//   flag bit 0: a coordinate is not canonical (>= p);  bit 1 (check_curve): a point is not on y^2 = x^3 + b
// (b = 4 for G1, 4 (1 + u) for G2; all-zero = infinity is accepted).  Subgroup membership is NOT checked here -- a scalar
// multiplication by r per point; vsp_g1_decompress / vsp_g2_decompress offer it for points that arrive as wire bytes.
__device__ __forceinline__ Fp curve_b_mont(const Fp &) { Fp four = Fp::one(); four = dbl(dbl(four)); return four; }
__device__ __forceinline__ Fp2 curve_b_mont(const Fp2 &) { Fp2 b; b.c0 = dbl(dbl(Fp::one())); b.c1 = b.c0; return b; }
template <class F> __global__ __launch_bounds__(256) void k_bases_to_mont(const Affine<F> *in, Affine<F> *out, size_t n, int check_curve, uint32_t *flag) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<F> p = in[i];
    uint32_t bad = (canon_below_p(p.x) && canon_below_p(p.y)) ? 0u : 1u;
    const bool inf = is_zero(p.x) && is_zero(p.y);
    p.x = to_mont(p.x); p.y = to_mont(p.y);
    if (check_curve && !inf && !bad) {
        F rhs = add(mul(sqr(p.x), p.x), curve_b_mont(p.x));
        if (!eq(sqr(p.y), rhs)) bad |= 2u;
    }
    if (bad) atomicOr(flag, bad);
    out[i] = p;
}

// ---- the precondition of the endomorphism split, checked: phi(P) = lambda P for every base.
// phi(x, y) = (beta x, y) acts as the scalar lambda = z^2 - 1 only on the order-r subgroup; the curve equation alone (checked at upload)
// also admits points with a cofactor component, for which sum k_i P_i computed through the split would be a DIFFERENT point than the
// plain pipeline's (and the reference's generic multiexp's).  The condition below is exactly what the split relies on: with it,
// (k1 + k2 lambda) P = k1 P + k2 phi(P), and the fold-back by lambda^2 + lambda + 1 = r is sound because (phi^2 + phi + 1) P = O holds on the
// whole curve, hence r P = O.  (It is also the known fast membership test of this curve family: phi(P) = -z^2 P for the other cube root.)
// lambda P = |z| (|z| P) - P with |z| = 0xd201000000010000 (Hamming weight 6): 126 doublings and 11 additions per point -- about 45 us of
// one lane's time, 20-30 ms for 2^20 G1 points, once per uploaded key.  flag bit 2 is raised for any point that fails; with `status`
// (one byte per point, non-null) bit 2 of the failing point's byte is raised instead.
static constexpr uint64_t BLS_ABS_Z = 0xd201000000010000ULL;
// the three group operations as REAL calls on memory temporaries: inlined side by side, the generic formulas crash this toolchain's
// machine scheduler next to the fixed-register product routine (as fp28.h notes for its cold branch); a one-off check can afford the calls
template <class E> __device__ __noinline__ void sgc_dbl(XYZZ<E> *a) { *a = xyzz_dbl(*a); }
template <class E> __device__ __noinline__ void sgc_madd(XYZZ<E> *a, const Affine<E> *p, bool negate) { XYZZ<E> t = *a; xyzz_madd(t, *p, negate); *a = t; }
template <class E> __device__ __noinline__ void sgc_add(XYZZ<E> *a, const XYZZ<E> *q) { XYZZ<E> t = *a; xyzz_add(t, *q); *a = t; }
template <class F>
__global__ __launch_bounds__(MSM_THREADS, AccumWaves<F>::W) void k_subgroup_check(const Affine<F> *__restrict__ bases, size_t n, uint32_t *flag, uint8_t *status) {
    using LV = LaneView<F>; using E = typename LV::E;
    const size_t i = gid<F>();
    if (i >= n) return;                                     // both lanes of a pair leave together
    Affine<E> p = LV::load(&bases[i]);
    if (is_inf(p)) return;                                  // infinity is in every subgroup
    XYZZ<E> t1 = xyzz_from_affine(p);
#pragma unroll 1
    for (int b = 62; b >= 0; b--) { sgc_dbl(&t1); if ((BLS_ABS_Z >> b) & 1ull) sgc_madd(&t1, &p, false); }
    XYZZ<E> t2 = t1;
#pragma unroll 1
    for (int b = 62; b >= 0; b--) { sgc_dbl(&t2); if ((BLS_ABS_Z >> b) & 1ull) sgc_add(&t2, &t1); }
    sgc_madd(&t2, &p, true);                                // z^2 P - P = lambda P
    Affine<E> q = p;
    glv_apply(q.x);                                         // phi(P) = (beta x, y)
    E lx, ly;
    mul_pair(q.x, t2.ZZ, q.y, t2.ZZZ, lx, ly);              // equal to t2 iff X = beta x ZZ and Y = y ZZZ (t2 finite)
    const bool inf2 = is_inf(t2);
    const bool ex = is_zero(sub(lx, t2.X));
    const bool ey = is_zero(sub(ly, t2.Y));
    if (inf2 || !ex || !ey) {
        if (status) status[i] |= 4u;                        // a verdict per point (decode.hip); the lanes of a pair write the same byte
        else atomicOr(flag, 4u);
    }
}

// the bit-decomposed last step (k_dimbits) or the weighted one (k_dimweight): `forced` (MsmTuning.dimbits) 1 / 0 forces either, -1 by group
template <class FT> static bool use_dimbits(long forced, const MsmGeom &g) {
    // room for 25 records per window in the slot's pinned buffer: the initial buffer for one vector (52 windows of 5 bits: no), the grown one
    // for a batch (msm_buffers grows it up to 64 MiB: K x Wk windows; k_dimweight's 16-addition chains took a fifth of a batch prover's kernel time)
    const size_t cap = g.K > 1 ? ((size_t)64 << 20) : MsmWork::PINNED_BYTES;
    const bool want = forced >= 0 ? forced != 0 : (LaneView<FT>::LANES == 1 || g.Wr <= 2 || g.c > 16);      // wide windows: digits of 2^10 values and more only k_dimbits takes
    return want && (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<typename WinOut<FT>::type>) <= cap;
}
// merges + bucket reduction over the bucket sums of field FT (F, or Fp28 on the G1 28-bit path); winres in the host's form; dimbits: the
// last step (use_dimbits)
template <class FT>
static int launch_tail(vsp_ctx *ctx, hipStream_t st, const MsmWork *pl, const MsmGeom &g, bool dimbits, XYZZ<FT> *buckets, XYZZ<FT> *partials, XYZZ<FT> *dims,
                       XYZZ<typename WinOut<FT>::type> *winres, XYZZ<typename WinOut<FT>::type> *winres_host) {
    using F = FT;
    constexpr unsigned NT = MsmBlock<F>::NT;
    const unsigned per_w = dims_per_w(g);
    // buckets split in 2..16 parts: up to every bucket (shared-set mode, or a small plain problem whose buckets alone would not fill the
    // GPU), a handful of outliers otherwise.  Expected parts per bucket = mean bucket size / part length.
    {
        const double est = (double)g.n * g.W / (double)g.G / (double)(g.T ? g.T : 1);
        const unsigned lpb = g.single ? 4u : (est < 0.6 ? 16u : (est <= 3.0 ? 1u : 4u));    // est ~ 1: half of the buckets are cut in two
        const unsigned per_block = MergeBlock<F>::NTL / lpb;
        const size_t want = (g.G + per_block - 1) / per_block;
        const dim3 grid((unsigned)(want < 4096 ? want : 4096));
        const uint32_t *medium = (const uint32_t *)pl->medium.p, *counters = (const uint32_t *)pl->counters.p, *suboff = (const uint32_t *)pl->suboff.p;
        const unsigned sb = lpb == 16 ? (grid.x < 1024 ? grid.x : 1024) : grid.x, all = sb + MERGE1_BLOCKS;
        const uint32_t *heavy = (const uint32_t *)pl->heavy.p;
        if (lpb == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 16>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
        else if (lpb == 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 4>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge_a<F, 1>), dim3(all), dim3(MergeBlock<F>::NT), 0, st, medium, heavy, counters, suboff, partials, buckets, sb);
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_merge2<F>), dim3(256), dim3(MergeBlock<F>::NT), 0, st, (const uint32_t *)pl->heavy.p, (const uint32_t *)pl->counters.p,
                       (const uint32_t *)pl->suboff.p, (const XYZZ<F> *)partials, buckets);
    VSP_LAUNCH_CHECK();
    {
        constexpr unsigned LL = 64 / LaneView<F>::LANES;                    // logical lanes of a wave
        const unsigned sums = g.Wr * per_w;
        // lanes per sum: the serial prefix (items / lanes) plus the tree (log2 lanes) additions, times the rounds the grid needs on
        // the 1024 SIMDs -- a wave more than the SIMDs hold at full speed costs a whole extra round
        unsigned minq = g.q0 < g.q1 ? g.q0 : g.q1; if (g.q2 && g.q2 < minq) minq = g.q2;
        const unsigned items = g.B >> minq;
        unsigned lps = 16; size_t best = ~(size_t)0;
        for (unsigned cand = 8, lg = 3; cand <= LL; cand *= 2, lg++) {
            const size_t waves = ((size_t)sums * cand + LL - 1) / LL;
            const size_t rounds = (waves + DimSumWaves<F>::MAX - 1) / DimSumWaves<F>::MAX;
            const size_t cost = ((items + cand - 1) / cand + lg) * rounds;
            if (cost < best) { best = cost; lps = cand; }
        }
        long forced_lanes = 0;
        { const long t = opt(ctx, "msm_dimsum_lanes", 0); if (t == 8 || t == 16 || t == 32 || (t == 64 && LL == 64)) { lps = (unsigned)t; forced_lanes = t; } }
        const unsigned spw = LL / lps;
        const dim3 grid((sums + spw - 1) / spw);
        DimSumPlan pl; pl.wave0[3] = 0;
        const long mw = opt(ctx, "msm_dimsum_maxw", 1024); const unsigned maxw = mw >= 256 && mw <= 4096 ? (unsigned)mw : 1024u;
        if (!forced_lanes) pl = dimsum_plan<F>(g, maxw);      // a lane count per digit (k_dimsum_mixed); "msm_dimsum_lanes" keeps one count for all
        ctx->stats["msm_dimsum_waves"] = pl.wave0[3];
        const long pf = opt(ctx, "msm_dimsum_prefetch", 0);
        bool dense = false;
        if constexpr (LaneView<F>::LANES == 1) {
            // the plan's lane counts, its sums dealt to whole 256-thread blocks per digit ("msm_dimsum_dense" = 0: one wave per block, k_dimsum_mixed)
            if (pl.wave0[3] && !pf && opt(ctx, "msm_dimsum_dense", 1)) {
                const unsigned nd[3] = {1u << g.q0, 1u << g.q1, dims_n2(g)};
                DimSumDensePlan dp; dp.blk0[0] = 0;
                for (unsigned d = 0; d < 3; d++) {
                    dp.lps[d] = pl.lps[d];
                    dp.blk0[d + 1] = dp.blk0[d] + (unsigned)(((size_t)g.Wr * nd[d] * pl.lps[d] + DIMSUM_DENSE_NT - 1) / DIMSUM_DENSE_NT);
                }
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum_dense<F>), dim3(dp.blk0[3]), dim3(DIMSUM_DENSE_NT), 0, st, (const XYZZ<F> *)buckets, g, dims, dp);
                ctx->stats["msm_dimsum_dense_launches"] += 1;
                dense = true;
            }
        }
        if (dense) {}
        else if (pl.wave0[3] && pf && LaneView<F>::LANES == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum_mixed<F, true>), dim3(pl.wave0[3]), dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims, pl);
        else if (pl.wave0[3]) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum_mixed<F, false>), dim3(pl.wave0[3]), dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims, pl);
        else
        if (lps == 8) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 8>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else if (lps == 16) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 16>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else if (lps == 32) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, 32>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimsum<F, (LL == 64 ? 64u : 32u)>), grid, dim3(64), 0, st, (const XYZZ<F> *)buckets, g, dims);
    }
    VSP_LAUNCH_CHECK();
    if (dimbits) {
        // the results go straight into the slot's pinned host buffer (device-visible): no copy operation behind the kernel.  (A 29 KB
        // device-to-host copy per multi-exponentiation rides the DMA engines, behind the 32 MB witness upload of whichever proof another
        // context has just started: two contexts proved no faster than one.)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimbits<F>), dim3(g.Wr * DIMBITS_STRIDE), dim3(64), 0, st, (const XYZZ<F> *)dims, g, winres_host);
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dimweight<F>), dim3(g.Wr * 3u), dim3(NT), 0, st, (const XYZZ<F> *)dims, g, winres_host);
    }
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// ------------------------------------------------------------------------------------------------
// n: scalars that are neither 0 nor 1 (twice that with the endomorphism split: half-length scalars); windows: how many windows c bits need;
// forced: MsmTuning.window_bits
static unsigned pick_window_bits(vsp_ctx *ctx, long forced, size_t n, bool glv) {
    if (forced >= 2 && forced <= 23) return (unsigned)forced;
    unsigned L = ceil_log2(n ? n : 1);
    // mean bucket load n / 2^(c-1) of about 32 points balances the accumulation against the
    // bucket reduction, whose cost grows with 2^c
    int c = (int)L - 4;
    if (c < 4) c = 4;
    if (c > 16) c = 16;
    // From 2^23 points on the window may grow past 16 bits (staged sort, k_ms_*).  Cost in units of one sorted-and-accumulated point of
    // the 16-bit pipeline (0.18 ns at 2^25 points): n W for the accumulation -- x 0.87 behind the staged sort, which is cheaper per entry
    // than the LDS counting sort at these sizes -- plus 4.1 per bucket for the bucket reduction (0.74 ns; fitted to 2^24 .. 2^26 points at
    // c = 20 and 22, profiles/r3_window_sweep.txt).  Measured, ms per multi-exponentiation, c = 16 against the model's choice:
    // 2^23: 22.95 / 22.0 (c = 19; 17 .. 20 are within 3 %), 2^24: 45.7 / 38.95 (20), 2^25: 96.7 / 73.3 (20), 2^26: 218 / 139.6 (20);
    // G2 2^23: 66.4 / 61.9 (19), 2^24: 130.3 / 113.6 (20).  Below 2^23 points the 16-bit pipeline wins (2^22: 11.4 against 12.3 at c = 17).
    // Split scalars (magnitudes below 2^127): 16-bit windows cover them in exactly 8 windows; 15 bits need 9 and 14 bits 10, whose last
    // window holds 8 / 2 bits of digit -- a few hundred (or four) buckets with thousands of points each, cut into parts and merged by
    // workgroups.  Measured (three in flight / one in flight, ms), default against 16 bits: G1 2^17 points 0.83 / 1.29 -> 0.74 / 1.14,
    // 2^18 1.30 / 1.86 -> 1.13 / 1.50 (2^16: a tie); G2 2^18 3.05 / 4.21 -> 3.04 / 3.67 (2^17 and below: 16 bits lose when pipelined).
    // n is the doubled count here.
    if (glv && c < 16 && n >= ((size_t)1 << (VSP_MSM_GROUP == 1 ? 18 : 19))) c = 16;
    const long wide = opt(ctx, "msm_wide_windows", 1);
    // 255-bit scalars (no endomorphism split), 2^20 points and more: 17 bits.  255 = 15 x 17, and with the scalars folded to below 2^254
    // (load_scalar) 15 windows carry everything, against 16 windows of 16 bits: G1 2^21 5.84 against 6.01 ms, 2^22 10.57 against 10.91;
    // G2 2^20 9.15 against 9.44, 2^21 16.8 against 17.3, 2^22 31.4 against 32.8 (profiles/r3_window_sweep.txt)
    if (c == 16 && wide && !glv && n >= ((size_t)1 << 20)) c = 17;
    if (c >= 16 && wide && n >= ((size_t)1 << 23)) {
        double best = 0; int bc = 16;
        for (int k = 16; k <= 23; k++) {
            const double W = glv ? (double)((128 + k - 1) / k) : (double)((255 % k == 0 ? 254 : 255) / k + 1);      // (g.fold)
            const double cost = (double)n * W * (k > 16 ? 0.87 : 1.0) + W * (double)((size_t)1 << (k - 1)) * 4.1;
            if (k == 16 || cost < best) { best = cost; bc = k; }
        }
        c = bc;
    }
    return (unsigned)c;
}

// ------------------------------------------------------------------------------------------------
// Host side.  An MSM is split into launch (everything up to the asynchronous copy of W*4 window results into a pinned
// buffer, all on the work slot's own stream) and finish (wait + Horner on the host), so that several MSMs can be in
// flight at once: the prover runs its five on separate streams, and back-to-back MSMs pipeline.
#if VSP_MSM_GROUP == 1
using F28 = Fp28; using Row28 = Affine28;                   // this group's field and base rows on 28-bit limbs
#else
using F28 = Fp2x28; using Row28 = Affine28x2;
#endif

// geometry: the window size and the part length from the effective problem size (or from the shared plan), then the digit split
template <class F> static int msm_geometry(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, MsmGeom &g, size_t &n_eff) {
    const MsmPre *pre = L.rq.pre; const bool glv = L.rq.glv; const size_t n = L.rq.n; const unsigned batch = L.rq.batch;
    const uint32_t imul = glv ? 2u : 1u;                    // rows per point in the interleaved table
    n_eff = n;
    if (L.plan_from) {
        g = L.plan_from->g; n_eff = L.plan_from->n_eff;
        if (L.plan_from->n != n) return set_error(ctx, VSP_ERR_ARG, "msm: shared plan of a different size");
        if ((g.single != 0) != (pre != nullptr) || (pre && (g.idx_stride != pre->stride * imul || g.idx_first != pre->first * imul || g.c != pre->c)))
            return set_error(ctx, VSP_ERR_ARG, "msm: shared plan needs bases precomputed alike");
    } else {
        VSP_TRY(ensure(ctx, wk.counters, 64, L.st));
        // effective problem size: scalars other than 0 and 1 (one small kernel + a read-back); the census may have been queued
        // earlier by msm_census (the prover queues all of them before any heavy kernel).  The same kernel flags scalars >= r.
        // The count only steers the window size / part length, never the result, so a slot that has seen a vector of this
        // length before plans from that earlier count and reads the fresh one at finish: no host wait on the launch path.
        wk.check_pending = false;
        if (!L.rq.dense) {
            if (!(wk.census_pending && wk.census_n == n && wk.census_scalars == (const void *)L.rq.scalars)) VSP_TRY(msm_census(ctx, wk, L.rq.scalars, n, nullptr, batch, L.rq.stride));
            wk.check_pending = true;
            if (n >= 4096) {
                if (wk.neff_cache_n == n && !opt(ctx, "msm_census_sync", 0)) n_eff = wk.neff_cache;
                else {
                    VSP_HIP(hipEventSynchronize(wk.census_done));
                    uint32_t h_cnt = *wk.h_census.template as<volatile uint32_t>() / batch;      // (a batch is counted together: the mean per vector)
                    n_eff = h_cnt < 256 ? 256 : h_cnt;
                }
            }
        }
        wk.census_pending = false;
        if (glv) n_eff *= 2;                                  // two half-length scalars per counted scalar
        g.c = pre ? pre->c : pick_window_bits(ctx, L.tune.window_bits, n_eff, glv);
        g.sbits = glv ? 128u : 255u;
        // 255-bit scalars: 255 / c + 1 windows cover the bits plus the carry of the signed recoding; split halves are magnitudes below
        // 2^127: ceil(128 / c) windows, and the top window's spare bit absorbs the carry
        g.fold = (!glv && opt(ctx, "msm_fold", 1) && 255u % g.c == 0u) ? 1u : 0u;
        if (batch > 1 && g.c > 16) g.c = 16;
        if (batch > 1 && g.c < 7) g.c = 7;                      // (a batch of tiny vectors: not hundreds of 4-bit windows per vector)
        g.Wk = glv ? (128u + g.c - 1) / g.c : (g.fold ? 254u / g.c + 1 : g.sbits / g.c + 1);
        g.K = batch; g.kstride = batch > 1 ? L.rq.stride : 0;
        g.W = g.Wk * g.K;                                      // what the sort, the accumulation and the reduction see: one bucket set per (vector, window)
        g.B = 1u << (g.c - 1);
        g.lb = g.c > 16 ? g.c - 16 : 0u;
        g.n = glv ? 2 * n : n;
        g.single = pre ? 1u : 0u; g.idx_stride = pre ? (uint32_t)(pre->stride * imul) : 0u; g.idx_first = pre ? (uint32_t)(pre->first * imul) : 0u;
        g.Wr = pre ? g.K : g.W;                                // bucket sets: one per vector over a table of window multiples, else one per window
        g.G = (size_t)g.Wr * g.B;
        const long t = L.tune.split;
        if (pre) {
            // one bucket set: ~n_eff*W/B points per bucket; parts of T points, about 2^18 of them to fill the GPU evenly
            size_t est = n_eff * g.W / ((size_t)1 << 18);
            unsigned T = 16; while (T < est && T < (1u << 20)) T <<= 1;      // ~n_eff*W/B points per bucket -> <= ~8 parts per bucket
            // ... but not a length that fills the GPU a whole number of times: 2^18 equal parts of 64 points are exactly two rounds of the
            // 2048 resident waves, every wave slot has to run exactly two parts, and nothing evens out the stagger of the second round
            // (accumulation 2.87 ms, one multi-exponentiation 4.0 ms); 7/8 of the length makes it 2.5 rounds (2.54 ms, 3.7 ms)
            if (T >= 64) T = T / 8 * 7;
            g.T = t > 0 ? (unsigned)t : T;
            if ((size_t)g.Wk * pre->stride * imul >= ((size_t)1 << 31)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: precomputed table too large to index");
        } else {
            // parts of at most T points; buckets alone may not give the ~2^18 lanes that fill the GPU (few windows, narrow windows,
            // or two lanes per part): then T shrinks until bucket parts do
            size_t mean = n_eff / g.B + 1;
            size_t T = mean * 4 < 128 ? 128 : mean * 4;
            const size_t target = ((size_t)1 << 18) / LaneView<F>::LANES;
            if (g.G < target) {
                size_t t2 = n_eff * g.W / (target - g.G) + 1, p2 = 16;
                while (p2 < t2) p2 <<= 1;
                if (p2 < T) T = p2;
            }
            g.T = t > 0 ? (unsigned)t : (unsigned)T;
        }
    }
    g.bd = 8;
    // per group: a shared plan carries the window size, not the digit split.  Which last step the bucket reduction takes decides how wide a digit may be
    L.dimbits = L.table28 ? use_dimbits<F28>(L.tune.dimbits, g) : use_dimbits<F>(L.tune.dimbits, g);
    split_digits<F>(g, L.dimbits);
    return VSP_OK;
}

// buffer sizing: the pinned landing buffer of the window results, the bucket arrays, and the plan's arrays when this launch makes a plan
template <class F> static int msm_buffers(vsp_ctx *ctx, MsmWork &wk, MsmLaunch &L, const MsmGeom &g) {
    const hipStream_t st = L.st;
    if (!L.dimbits && ((1u << g.q0) > MsmBlock<F>::NTL || (1u << g.q2) > MsmBlock<F>::NTL)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: window too wide");
    if (g.c > 23) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: windows wider than 23 bits are not built");
    L.M = L.n * g.W;
    if (L.M >= ((size_t)1 << 32)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: n * windows >= 2^32 (sorted positions are 32-bit); use wider windows or shard the points");
    L.Smax = g.G + L.M / g.T + 1;
    L.per_w = dims_per_w(g);
    { const size_t need = (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<F>);      // room for either layout of the window results
      if (need > wk.h_pinned.cap) {                                              // (a batch: K times the windows; the slot is idle here, nothing writes the old buffer)
          if (need > ((size_t)64 << 20)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: too many windows (a batch: fewer vectors per call)");
          VSP_HIP(hipStreamSynchronize(st));
          VSP_TRY(ensure_pinned(ctx, wk.h_pinned, need));
      } }
    VSP_TRY(ensure(ctx, wk.buckets, g.G * sizeof(XYZZ<F>), st));
    VSP_TRY(ensure(ctx, wk.partials, L.Smax * sizeof(XYZZ<F>), st));
    VSP_TRY(ensure(ctx, wk.dims, (size_t)g.Wr * L.per_w * sizeof(XYZZ<F>), st));
    VSP_TRY(ensure(ctx, wk.winres, (size_t)g.Wr * DIMBITS_STRIDE * sizeof(XYZZ<F>), st));      // room for either layout (4 or 25 records per window)
    L.nblk = (unsigned)((L.n + MSM_THREADS - 1) / MSM_THREADS);
    L.gblk = (unsigned)((g.G + MSM_THREADS - 1) / MSM_THREADS);
    L.ablk = (unsigned)((L.Smax + MSM_THREADS - 1) / MSM_THREADS);
    if (L.plan_from) return VSP_OK;
    for (DevBuf *b : {&wk.cnt, &wk.off, &wk.cursor, &wk.nsub, &wk.suboff, &wk.heavy, &wk.medium}) VSP_TRY(ensure(ctx, *b, (g.G + 1) * 4, st));
    VSP_TRY(ensure(ctx, wk.sorted, L.M * 4, st));
    VSP_TRY(ensure(ctx, wk.partbucket, L.Smax * 4, st));
    VSP_TRY(ensure(ctx, wk.perm, L.Smax * 4, st));
    VSP_TRY(ensure(ctx, wk.sizehist, 2 * SZ_BINS * 4, st));
    return VSP_OK;
}

// accumulation over the plan (this slot's own or the shared one), then the bucket reduction (launch_tail)
template <class F> static int msm_accumulate(vsp_ctx *ctx, MsmWork &wk, const MsmLaunch &L, const MsmGeom &g) {
    const Affine<F> *bases = (const Affine<F> *)L.rq.bases;
    const hipStream_t st = L.st;
    const MsmWork *pl = L.plan_from ? L.plan_from : &wk;
    XYZZ<F> *buckets = (XYZZ<F> *)wk.buckets.p, *partials = (XYZZ<F> *)wk.partials.p, *winres = (XYZZ<F> *)wk.winres.p;
    wk.dimbits = L.dimbits;
    // (the diagnostic build without hand-laid-out routines runs the multi-exponentiation on the generic 12 x 32-bit kernels only: the
    // 28-bit reduction kernels over portable products crash this toolchain's backend -- Machine Copy Propagation / post-RA pseudo
    // expansion segfault in k_dimsum<Fp28> / k_dimsum<Fp2x28>; the FIELD forms stay covered there: the 28-bit one by vsp_selftest_field
    // (Fp, ops 6..12) and vsp_selftest_xyzz_add, the 29-bit one by vsp_selftest_field (Fr, ops 6..9) and the transforms)
#if defined(VSP_PORTABLE_MUL)
    constexpr bool have28 = sizeof(F) == 0;
#else
    constexpr bool have28 = sizeof(F) != 0;
#endif
    if constexpr (have28) if (L.table28) {
        // 14 x 28-bit accumulation; bucket parts that meet an equal-x pair are listed and redone by the generic kernel
        VSP_TRY(ensure(ctx, wk.redo, (L.Smax + 1) * sizeof(uint32_t), st));
        uint32_t *redo = (uint32_t *)wk.redo.p;               // [0] = count, list from [1]
        if (L.plan_from) VSP_HIP(hipMemsetAsync(redo, 0, sizeof(uint32_t), st));      // (k_plan cleared it when it ran in this launch)
        // the bucket sums stay in the 28-bit form from here to the results per window; the parts the generic kernel redoes (equal-x
        // pairs) are written to the 12 x 32-bit arrays of the same indexing and, converted, to the 28-bit ones
        VSP_TRY(ensure(ctx, wk.buckets28, g.G * sizeof(XYZZ<F28>), st));
        VSP_TRY(ensure(ctx, wk.partials28, L.Smax * sizeof(XYZZ<F28>), st));
        VSP_TRY(ensure(ctx, wk.dims, (size_t)g.Wr * L.per_w * sizeof(XYZZ<F28>), st));
        XYZZ<F28> *buckets28 = (XYZZ<F28> *)wk.buckets28.p, *partials28 = (XYZZ<F28> *)wk.partials28.p;
        VSP_HIP(hipEventRecord(wk.ev0, st));                  // ev0 .. ev1 bracket the accumulation kernel alone
#if VSP_MSM_GROUP == 1
        long use_asm = opt(ctx, "msm_accum28_asm", 1);
#if defined(VSP_PORTABLE_MUL)
        use_asm = 0;                                        // the diagnostic build without hand-laid-out routines: the C++ twin of the generated loop
#endif
        if (!use_asm) {
            hipLaunchKernelGGL(k_accum28_cxx, dim3(L.ablk), dim3(MSM_THREADS), 0, st, (const Row28 *)L.table28, (const uint32_t *)pl->sorted.p,
                               (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                               g.G, g.T, buckets28, partials28, redo + 1, redo);
            ctx->stats["msm_accum28_cxx_launches"] += 1;
        } else
#endif
        hipLaunchKernelGGL(k_accum28, dim3(L.ablk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, (const Row28 *)L.table28, (const uint32_t *)pl->sorted.p,
                           (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                           g.G, g.T, buckets28, partials28, redo + 1, redo);
        VSP_HIP(hipEventRecord(wk.ev1, st));
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_accum_redo<F>), dim3(L.ablk < 64 ? L.ablk : 64), dim3(MSM_THREADS), 0, st, bases, (const uint32_t *)pl->sorted.p,
                           (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->partbucket.p, buckets, partials,
                           (const uint32_t *)(redo + 1), (const uint32_t *)redo, L.rq.glv, buckets28, partials28);
        VSP_LAUNCH_CHECK();
        return launch_tail<F28>(ctx, st, pl, g, L.dimbits, buckets28, partials28, (XYZZ<F28> *)wk.dims.p, winres, wk.h_pinned.template as<XYZZ<F>>());
    }
    VSP_HIP(hipEventRecord(wk.ev0, st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_accum<F>), dim3(L.ablk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, bases, (const uint32_t *)pl->sorted.p,
                       (const uint32_t *)pl->off.p, (const uint32_t *)pl->suboff.p, (const uint32_t *)pl->perm.p, (const uint32_t *)pl->partbucket.p,
                       g.G, g.T, buckets, partials);
    VSP_HIP(hipEventRecord(wk.ev1, st));
    VSP_LAUNCH_CHECK();
    return launch_tail<F>(ctx, st, pl, g, L.dimbits, buckets, partials, (XYZZ<F> *)wk.dims.p, winres, wk.h_pinned.template as<XYZZ<F>>());
}

// one multi-exponentiation (common.h MsmRequest); plan_from: the work slot rq.plan_from names, or null
template <class F>
static int msm_launch(vsp_ctx *ctx, MsmWork &wk, const MsmRequest &rq, const MsmWork *plan_from) {
    const size_t n = rq.n;
    wk.active = false; wk.n = n;
    if (n == 0) { wk.active = true; wk.empty = true; wk.g.K = rq.batch ? rq.batch : 1; return VSP_OK; }
    wk.empty = false;
    const unsigned batch = rq.batch ? rq.batch : 1;
    // a batch (MsmGeom.K): plain bases, its own digit sort through the LDS counting sort, 16-bit windows at most
    // (a shared plan must be a batch of the same vectors: the prover's A, B1 and B2 multiply by the same K witness vectors)
    if (batch > 1 && rq.plan_only) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: a batch plans and accumulates in one launch");
    if (batch > 1 && plan_from && (plan_from->g.K != batch || plan_from->g.kstride != rq.stride || !plan_from->active || plan_from->empty))
        return set_error(ctx, VSP_ERR_ARG, "msm: shared plan of another batch");
    MsmLaunch L{};
    L.rq = rq; L.rq.batch = batch; L.st = wk.stream; L.scalars = rq.scalars; L.n = n;
    L.table28 = rq.pre ? rq.pre->table28 : rq.table28;
    L.rq.glv = rq.glv && (rq.pre ? rq.pre->glv && rq.pre->table28 : rq.table28 != nullptr);      // the split needs the interleaved table
    if (n >= ((size_t)1 << (L.rq.glv ? 30 : 31))) return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: n >= 2^31");
    L.plan_from = plan_from && plan_from->glv == L.rq.glv ? plan_from : nullptr;      // a plan over split scalars serves only launches that split alike
    wk.glv = L.rq.glv;
    L.sort_mode = opt(ctx, "msm_sort", 0);
    L.tune = rq.tuning ? *rq.tuning : MsmTuning{opt(ctx, "msm_window_bits", 0), opt(ctx, "msm_split", 0), opt(ctx, "msm_dimbits", -1)};
    MsmGeom g; size_t n_eff = n;
    VSP_TRY(msm_geometry<F>(ctx, wk, L, g, n_eff));
    wk.g = g; wk.n_eff = n_eff;
    VSP_TRY(msm_split_scalars(ctx, wk, L, g));
    VSP_TRY(msm_buffers<F>(ctx, wk, L, g));
    if (L.plan_from) VSP_HIP(hipStreamWaitEvent(L.st, L.plan_from->plan_ready, 0));
    else { VSP_TRY(msm_digit_sort(ctx, wk, L, g)); VSP_TRY(msm_bucket_plan(ctx, wk, L, g)); }
    if (rq.plan_only) return VSP_OK;                        // the accumulation follows in a later launch over this slot's own plan
    VSP_TRY(msm_accumulate<F>(ctx, wk, L, g));
    VSP_HIP(hipEventRecord(wk.done, L.st));
    wk.active = true;
    return VSP_OK;
}

// A finish in two halves: msm_finish_wait (the wait for the slot's kernels, the census verdict, the statistics -- touches the context, so on
// the caller's thread) and msm_fold (the Horner chains over the window results in the slot's pinned buffer -- pure host arithmetic that reads
// only the slot, so the prover runs the folds of its five multi-exponentiations on host threads while it waits for the next slot).
// out: one result per vector of the batch the launch ran over (MsmGeom.K; one for an ordinary launch)
template <class F, class HF> static void msm_fold(const MsmWork &wk, XYZZ<HF> *out);
template <class F, class HF>
static int msm_finish_wait(vsp_ctx *ctx, MsmWork &wk, unsigned out_count, bool *empty);
template <class F, class HF>
static int msm_finish(vsp_ctx *ctx, MsmWork &wk, XYZZ<HF> *out, unsigned out_count = 1) {
    for (unsigned k = 0; k < out_count; k++) out[k] = XYZZ<HF>::inf();
    bool empty = false;
    VSP_TRY((msm_finish_wait<F, HF>(ctx, wk, out_count, &empty)));
    if (!empty) msm_fold<F, HF>(wk, out);
    return VSP_OK;
}
template <class F, class HF>
static int msm_finish_wait(vsp_ctx *ctx, MsmWork &wk, unsigned out_count, bool *empty) {
    static_assert(sizeof(F) == sizeof(HF), "host/device field layouts must match");
    *empty = true;
    if (!wk.active) return set_error(ctx, VSP_ERR_ARG, "msm: finish without launch");
    wk.active = false;
    if (wk.empty) return VSP_OK;
    *empty = false;
    if (wk.g.K != out_count) return set_error(ctx, VSP_ERR_ARG, "msm: finish asks for another number of results than the launch's batch");
    VSP_HIP(hipEventSynchronize(wk.done));
    const MsmGeom &g = wk.g;
#ifdef VSP_DEBUG_DUMP
    // experiment builds only (tools/dimsum_prefetch_probe.py): the bucket sums and the digit sums of the multi-exponentiation just finished,
    // generic 12 x 32-bit form ("msm_fp28" = 0), for an off-line comparison against big-integer sums
    if (const char *dir = getenv("VSP_DEBUG_DUMP_DIR")) {
        if (FILE *f = fopen((std::string(dir) + "/winres.bin").c_str(), "wb")) { fwrite(wk.h_pinned.p, 1, (size_t)g.Wr * (wk.dimbits ? DIMBITS_STRIDE : 4) * sizeof(XYZZ<HF>), f); fclose(f); }
        const unsigned per_w = dims_per_w(g);
        std::vector<char> hb(g.G * sizeof(XYZZ<F>)), hd((size_t)g.Wr * per_w * sizeof(XYZZ<F>));
        if (wk.buckets.p && wk.dims.p && hipMemcpy(hb.data(), wk.buckets.p, hb.size(), hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(hd.data(), wk.dims.p, hd.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            std::string d(dir);
            if (FILE *f = fopen((d + "/buckets.bin").c_str(), "wb")) { fwrite(hb.data(), 1, hb.size(), f); fclose(f); }
            if (FILE *f = fopen((d + "/dims.bin").c_str(), "wb")) { fwrite(hd.data(), 1, hd.size(), f); fclose(f); }
            if (FILE *f = fopen((d + "/geom.txt").c_str(), "w")) { fprintf(f, "%u %u %u %u %u %u %u %zu\n", g.c, g.W, g.Wr, g.B, g.q0, g.q1, g.q2, sizeof(XYZZ<F>)); fclose(f); }
        }
    }
#endif
    if (wk.check_pending) {
        // the census of this launch (queued before the kernels `done` follows): remember the count for the next plan of this
        // length, refuse the result when a scalar was not canonical
        wk.check_pending = false;
        VSP_HIP(hipEventSynchronize(wk.census_done));
        const volatile uint32_t *hc = wk.h_census.template as<const volatile uint32_t>();
        if (wk.n >= 4096) { const uint32_t c0 = hc[0] / (wk.g.K ? wk.g.K : 1u); wk.neff_cache_n = wk.n; wk.neff_cache = c0 < 256 ? 256 : c0; }
        if (hc[2]) return set_error(ctx, VSP_ERR_ARG, "msm: a scalar is not canonical (>= r)");
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, wk.ev0, wk.ev1) == hipSuccess) {
        ctx->stats["msm_accum_ms"] += ms;
        ctx->stats["msm_accum_launches"] += 1;
    }
    ctx->stats["msm_calls"] += 1;
    ctx->stats["msm_n_eff"] = (double)wk.n_eff;
    ctx->stats["msm_window_bits"] = g.c;
    ctx->stats["msm_windows"] = g.W;
    ctx->stats["msm_bucket_sets"] = g.Wr;
    ctx->stats["msm_split"] = g.T;
    ctx->stats["msm_endomorphism_split"] = wk.glv ? 1 : 0;
    if (opt(ctx, "msm_debug_counts", 0) && wk.counters.p && wk.suboff.p) {      // diagnostic: the plan's counts (a blocking read-back), only when asked for
        uint32_t c4[4] = {0, 0, 0, 0}, parts = 0;
        if (hipMemcpy(c4, wk.counters.p, sizeof c4, hipMemcpyDeviceToHost) == hipSuccess &&
            hipMemcpy(&parts, (const uint32_t *)wk.suboff.p + g.G, 4, hipMemcpyDeviceToHost) == hipSuccess) {
            ctx->stats["msm_heavy_buckets"] = c4[0]; ctx->stats["msm_medium_buckets"] = c4[2]; ctx->stats["msm_parts"] = parts;
            ctx->stats["msm_buckets"] = (double)g.G;
        }
    }
    return VSP_OK;
}
template <class F, class HF> static void msm_fold(const MsmWork &wk, XYZZ<HF> *out) {
    const MsmGeom &g = wk.g;
    const XYZZ<HF> *wr = wk.h_pinned.template as<const XYZZ<HF>>();
    // Horner over bit positions: window w contributes D2 at c*w + q1 + q0, D1 at c*w + q0, D0 + Tot at c*w.  A batch: one chain per vector over
    // its own windows [k Wk, (k + 1) Wk) (one bucket set per window), or over its one bucket set in the shared-set mode
    const unsigned per = g.single ? 1u : (g.K > 1 ? g.Wk : g.Wr);      // window results per vector (shared-set mode: its one bucket set)
    const bool dimbits_layout = wk.dimbits;
    host_parallel_for(g.K, [&, per, dimbits_layout](size_t kb) {
        XYZZ<HF> acc = XYZZ<HF>::inf();
        const int w_lo = (int)(kb * per), w_hi = (int)(kb * per + per);
        if (dimbits_layout) {
            // k_dimbits layout: S_{d,j} enters at bit position (shift of digit d) + j of the window, Tot at position 0 -- one doubling per
            // position, c per window, exactly as below
            const unsigned q[3] = {g.q0, g.q1, g.q2};
            for (int w = w_hi - 1; w >= w_lo; w--) {
                const XYZZ<HF> *rec = wr + (size_t)w * DIMBITS_STRIDE;
                acc = xyzz_dbl(acc);                                    // position c - 1: bucket indices have c - 1 bits
                for (int d = 2; d >= 0; d--)
                    for (int j = (int)q[d] - 1; j >= 0; j--) { acc = xyzz_dbl(acc); xyzz_add(acc, rec[g.bd * d + j]); }
                xyzz_add(acc, rec[24]);
            }
        } else {
            for (int w = w_hi - 1; w >= w_lo; w--) {
                for (unsigned i = 0; i < g.q2 + 1; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 2]);
                for (unsigned i = 0; i < g.q1; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 1]);
                for (unsigned i = 0; i < g.q0; i++) acc = xyzz_dbl(acc);
                xyzz_add(acc, wr[(size_t)w * 4 + 0]);
                xyzz_add(acc, wr[(size_t)w * 4 + 3]);
            }
        }
        out[kb] = acc;
    });
}

// A batch reuses the plan of ANOTHER slot only.  A single launch may name its own slot: that is how the accumulation follows a plan-only launch.
template <class F> static int launch_slot(vsp_ctx *ctx, unsigned slot_id, const MsmRequest &rq) {
    if (slot_id >= VSP_MSM_SLOTS || rq.plan_from >= (int)VSP_MSM_SLOTS || (rq.batch && rq.plan_from == (int)slot_id)) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot");
    VSP_TRY(work_init(ctx, slot(ctx, slot_id), slot_id == 0 ? ctx->stream : nullptr));
    return msm_launch<F>(ctx, slot(ctx, slot_id), rq, rq.plan_from >= 0 ? &slot(ctx, (unsigned)rq.plan_from) : nullptr);
}

}  // anonymous namespace

// the entry points of common.h, defined once for both groups; msm_g1.hip / msm_g2.hip instantiate them for their group (VSP_MSM_GROUP)
// table[w][i] = 2^(c*w) * table[0][i] for w = 1..W-1 (slice 0 already holds the bases); affine, Montgomery
template <class G> int msm_precompute(vsp_ctx *ctx, typename G::Point *table, size_t n, unsigned c) {
    using F = typename G::F;
    const unsigned W = 255 / c + 1;
    hipStream_t st = ctx->stream;
    DevBuf tmp, pre;
    VSP_TRY(ensure(ctx, tmp, n * sizeof(XYZZ<F>), st));
    VSP_TRY(ensure(ctx, pre, n * sizeof(F), st));
    const unsigned blk = (unsigned)((n + MSM_THREADS - 1) / MSM_THREADS);
    const size_t chunks = (n + PRE_CHUNK - 1) / PRE_CHUNK;
    for (unsigned w = 1; w < W; w++) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_shift_window<F>), dim3(blk * LaneView<F>::LANES), dim3(MSM_THREADS), 0, st, (const Affine<F> *)(table + (size_t)(w - 1) * n), n, c, (XYZZ<F> *)tmp.p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_affine_mont<F>), dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, st, (const XYZZ<F> *)tmp.p, n, (F *)pre.p,
                           table + (size_t)w * n);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return set_error(ctx, VSP_ERR_HIP, "precompute: kernel failed");
    return VSP_OK;                                          // behind the wait: tmp and pre go here
}

template <class G> int msm_table28(vsp_ctx *ctx, const typename G::Point *table, size_t count, void *d_out, bool glv) {
    if (!count) return VSP_OK;
#if defined(VSP_PORTABLE_MUL)
    return VSP_ERR_UNSUPPORTED;                              // the diagnostic build without hand-laid-out routines: generic kernels (no 28-bit table, no split)
#endif
    hipLaunchKernelGGL(k_table28, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, table, count, (Row28 *)d_out, glv);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
template <class G> int msm_slot_launch(vsp_ctx *ctx, unsigned slot_id, const MsmRequest &rq) { return launch_slot<typename G::F>(ctx, slot_id, rq); }
template <class G> int msm_slot_finish(vsp_ctx *ctx, unsigned slot_id, XYZZ<typename G::HF> *out, unsigned count) {
    return msm_finish<typename G::F, typename G::HF>(ctx, slot(ctx, slot_id), out, count);
}
template <class G> int msm_slot_finish_wait(vsp_ctx *ctx, unsigned slot_id, unsigned count, bool *empty) {
    return msm_finish_wait<typename G::F, typename G::HF>(ctx, slot(ctx, slot_id), count, empty);
}
template <class G> void msm_slot_fold(vsp_ctx *ctx, unsigned slot_id, XYZZ<typename G::HF> *out) { msm_fold<typename G::F, typename G::HF>(slot(ctx, slot_id), out); }
template <class G> int subgroup_check(vsp_ctx *ctx, const typename G::Point *d_mont, size_t n, uint32_t *d_flag, uint8_t *d_status) {
    using F = typename G::F;
    if (!n) return VSP_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_subgroup_check<F>), dim3((unsigned)((LaneView<F>::LANES * n + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, ctx->stream,
                       d_mont, n, d_flag, d_status);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
template <class G> int bases_to_mont(vsp_ctx *ctx, const void *d_canon, typename G::Point *d_out, size_t n, int check_curve, uint32_t *d_flag) {
    using F = typename G::F;
    if (!n) return VSP_OK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bases_to_mont<F>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const Affine<F> *)d_canon, d_out, n, check_curve, d_flag);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

#if VSP_MSM_GROUP == 1
// diagnostic build: clock held inside the G1 accumulation loop since the last reset (0: no data / production build)
int msm_diag_clock(vsp_ctx *ctx, int reset, double *ghz, double *waves) {
#ifdef VSP_DIAG_CLOCK
    unsigned long long h[4] = {0, 0, 0, 0};
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    VSP_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(vsp_diag_clock_sums), sizeof h));
    if (ghz) *ghz = h[1] ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
    if (waves) *waves = (double)h[2];
    if (reset) { unsigned long long z[4] = {0, 0, 0, 0}; VSP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(vsp_diag_clock_sums), z, sizeof z)); }
    return VSP_OK;
#else
    (void)reset; if (ghz) *ghz = 0.0; if (waves) *waves = 0.0;
    return set_error(ctx, VSP_ERR_UNSUPPORTED, "diag_clock: this is not the diagnostic build (make diag -> libvsp_hip_diag.so)");
#endif
}
#endif

}  // namespace vsp
