// Radix-2 NTT over BLS12-381 Fr for gfx950 (the step radix-2 domain and witness_map built on it are in domain.hip).
//
// Replaces math::evaluation_domain<Fr> / basic_radix2_domain (fft, inverse_fft, coset variants,
// divide_by_z_on_coset) of crypto3-math -- absent submodule, /root/reference/.gitmodules:47-48;
// reached from bin/cli/include/nil/vote_saver/common.hpp:1132-1135 via the prover's witness_map.
// The serial reference algorithm is bit-reverse + log2(m) butterfly stages over one array
// (libfqfft _basic_serial_radix2_FFT); the output is the DFT, unique given omega.
//
// MI355X design:
//  * The log2(m) stages are grouped into passes of <= 8 stages.  One workgroup (512 threads) owns a
//    tile of 2048 elements (64 KiB of LDS, two workgroups per CU), runs all of the pass's stages out
//    of LDS and touches HBM exactly once for read and once for write: traffic per pass = 64 B/element,
//    2-4 passes per transform (m = 2^22: 3 passes, 8+8+6 stages).  Inside a pass the stages run as radix-4 steps: two stages per
//    LDS round trip and barrier.
//  * A tile is [2^K butterfly rows] x [C = 2048/2^K contiguous columns]; every global access is a run
//    of C*32 bytes >= 256 B.  The first pass reads through the bit-reversal permutation (runs of C
//    inputs) and writes natural order, so no separate permutation pass exists.
//  * Values stay CANONICAL in HBM and LDS: a Montgomery product of a canonical value with a
//    Montgomery-form twiddle is already the canonical product, so no domain conversion is ever done.
//  * LDS holds each 32-byte element as two 16-byte halves in separate planes: a wave's ds_read_b128 /
//    ds_write_b128 then covers 64 x 16 contiguous bytes (conflict-free), instead of a 32-byte stride.
//  * Twiddles come from one table omega^j, j < m/2 (64 MiB at m = 2^22, Infinity-Cache resident);
//    the table of the largest domain seen serves every smaller one by striding.
//  * Coset shift (a[j] *= g^j), inverse scaling (m^-1) and inverse coset shift are fused into the
//    first pass's load / the last pass's store.
//  * The path is integer-ALU bound (one 8-limb Montgomery product per butterfly), not HBM bound.
#include <algorithm>
#include "common.h"
#include <type_traits>
#include "fr29.h"

namespace vsp {

#ifndef VSP_NTT_TILE_LOG
#define VSP_NTT_TILE_LOG 11
#define VSP_NTT_THREADS 512
#define VSP_NTT_MAX_STAGES 8
#endif
static constexpr unsigned NTT_TILE_LOG = VSP_NTT_TILE_LOG;      // 2048 elements per workgroup
static constexpr unsigned NTT_THREADS = VSP_NTT_THREADS;     // 2 workgroups per CU (64 KiB tiles) -> 4 waves per SIMD (256: 0.81 ms, 512: 0.74 ms, 1024: 0.84 ms at 2^22)
static constexpr unsigned NTT_MAX_STAGES = VSP_NTT_MAX_STAGES;     // per pass (keeps C >= 8 columns = 256 B runs)
static constexpr unsigned PW_LOG = 11;            // two-level power tables: g^i = lo[i & 2047] * hi[i >> 11]

struct NttPassArgs {
    unsigned log_n, s0, s1, clog, tlog;
    int first, last;
    int premul;     // multiply input i by g^i (forward coset), first pass only
    int postmul;    // last pass only: 0 none, 1 constant `scale`, 2 scale * ginv^pos
    const Fr *tw;
    const Fr *pw_lo, *pw_hi;
    Fr scale;       // Montgomery form
};

__device__ __forceinline__ unsigned brev(unsigned v, unsigned bits) { return bits ? (__brev(v) >> (32 - bits)) : 0u; }

__device__ __forceinline__ Fr lds_load(const uint4 *pl0, const uint4 *pl1, unsigned e) {
    Fr v; uint4 a = pl0[e], b = pl1[e];
    v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w; v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w;
    return v;
}
__device__ __forceinline__ void lds_store(uint4 *pl0, uint4 *pl1, unsigned e, const Fr &v) {
    pl0[e] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    pl1[e] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

__global__ __launch_bounds__(NTT_THREADS) void k_ntt_pass(const Fr *__restrict__ in, Fr *__restrict__ out, NttPassArgs p) {
    __shared__ uint4 lds[2u << NTT_TILE_LOG];
    const unsigned K = p.s1 - p.s0;
    const unsigned C = 1u << p.clog;
    const unsigned tile = 1u << (K + p.clog);
    uint4 *pl0 = lds, *pl1 = lds + tile;
    const unsigned tid = threadIdx.x;
    const unsigned wg = blockIdx.x;
    // position pieces for passes after the first: pos = hi<<s1 | mid<<s0 | lo_hi<<clog | c
    const unsigned lo_bits = p.s0 - p.clog;                   // only meaningful when !first
    const unsigned lo_hi = p.first ? 0u : (wg & ((1u << lo_bits) - 1u));
    const unsigned hi = p.first ? 0u : (wg >> lo_bits);
    const size_t base_pos = p.first ? 0 : (((size_t)hi << p.s1) | ((size_t)lo_hi << p.clog));

    // ---- load tile (LDS index e = mid*C + c; consecutive threads -> consecutive c -> contiguous HBM)
    for (unsigned e = tid; e < tile; e += NTT_THREADS) {
        unsigned mid = e >> p.clog, c = e & (C - 1);
        size_t src;
        if (p.first) src = ((size_t)brev(mid, p.s1) << (p.log_n - p.s1)) + (size_t)wg * C + c;
        else src = base_pos | ((size_t)mid << p.s0) | c;
        Fr v = in[src];
        if (p.premul) {
            Fr g = mul(p.pw_lo[src & ((1u << PW_LOG) - 1u)], p.pw_hi[src >> PW_LOG]);
            v = mul(v, g);
        }
        lds_store(pl0, pl1, e, v);
    }
    __syncthreads();

    // ---- K butterfly stages out of LDS: an odd K starts with one radix-2 stage, the rest run as radix-4 steps (two stages per
    //      LDS round trip and per barrier; a thread owns the four elements mid0 + {0, h, 2h, 3h} of one column)
    const unsigned lo_part = p.first ? 0u : ((lo_hi << p.clog));
    unsigned t = 0;
    if (K & 1) {
        const unsigned s = p.s0;              // global stage: half-size 2^s, twiddle omega_{2^(s+1)}^j
        for (unsigned bf = tid; bf < (tile >> 1); bf += NTT_THREADS) {
            unsigned c = bf & (C - 1), q = bf >> p.clog;
            unsigned e0 = (q << (1 + p.clog)) | c, e1 = e0 + C;
            Fr u = lds_load(pl0, pl1, e0), v = lds_load(pl0, pl1, e1);
            if (s > 0) v = mul(v, p.tw[(size_t)(p.first ? 0u : (lo_part | c)) << (p.tlog - 1 - s)]);
            lds_store(pl0, pl1, e0, add(u, v));
            lds_store(pl0, pl1, e1, sub(u, v));
        }
        __syncthreads();
        t = 1;
    }
    for (; t < K; t += 2) {
        const unsigned s = p.s0 + t;          // stages s and s + 1
        const unsigned h = 1u << t;
        for (unsigned g = tid; g < (tile >> 2); g += NTT_THREADS) {
            unsigned c = g & (C - 1), q = g >> p.clog;
            unsigned mid_lo = q & (h - 1);
            unsigned mid0 = ((q >> t) << (t + 2)) | mid_lo;
            unsigned e0 = (mid0 << p.clog) | c, e1 = e0 + (h << p.clog), e2 = e1 + (h << p.clog), e3 = e2 + (h << p.clog);
            const size_t off = p.first ? 0u : (lo_part | c);
            Fr x0 = lds_load(pl0, pl1, e0), x1 = lds_load(pl0, pl1, e1), x2 = lds_load(pl0, pl1, e2), x3 = lds_load(pl0, pl1, e3);
            if (s > 0) {
                const Fr w1 = p.tw[(((size_t)mid_lo << p.s0) | off) << (p.tlog - 1 - s)];
                x1 = mul(x1, w1); x3 = mul(x3, w1);
            }
            Fr a0 = add(x0, x1), a1 = sub(x0, x1), a2 = add(x2, x3), a3 = sub(x2, x3);
            a2 = mul(a2, p.tw[(((size_t)mid_lo << p.s0) | off) << (p.tlog - 2 - s)]);
            a3 = mul(a3, p.tw[(((size_t)(mid_lo + h) << p.s0) | off) << (p.tlog - 2 - s)]);
            lds_store(pl0, pl1, e0, add(a0, a2));
            lds_store(pl0, pl1, e1, add(a1, a3));
            lds_store(pl0, pl1, e2, sub(a0, a2));
            lds_store(pl0, pl1, e3, sub(a1, a3));
        }
        __syncthreads();
    }

    // ---- store tile
    for (unsigned i = tid; i < tile; i += NTT_THREADS) {
        unsigned mid, c; size_t pos;
        if (p.first) {              // natural-order output: runs of 2^K contiguous elements per column
            mid = i & ((1u << K) - 1u); c = i >> K;
            pos = ((size_t)brev(wg * C + c, p.log_n - p.s1) << p.s1) | mid;
        } else {
            mid = i >> p.clog; c = i & (C - 1);
            pos = base_pos | ((size_t)mid << p.s0) | c;
        }
        Fr v = lds_load(pl0, pl1, (mid << p.clog) | c);
        if (p.last && p.postmul) {
            Fr m = p.scale;
            if (p.postmul == 2) m = mul(m, mul(p.pw_lo[pos & ((1u << PW_LOG) - 1u)], p.pw_hi[pos >> PW_LOG]));
            v = mul(v, m);
        }
        out[pos] = v;
    }
}

// ================================================================================================
// The same pass on 9 x 29-bit limbs with lazy reduction (fr29.h): ~1.4 x fewer instructions per butterfly.  Data enters canonical
// (8 x 32-bit words), stays "lazy" (congruent, tight limbs, value below 48 r) in LDS and -- between passes -- in the scratch buffer
// (three planes: limbs 0-3, limbs 4-7, limb 8: 36 bytes per element), and leaves canonical from the last pass, where the product
// with the scale (1/m, the extra scale, the inverse coset power -- or the Montgomery one when there is none) brings it below 2r.
// Twiddles and coset powers come from tables in Montgomery form for R' = 2^261, canonical, in the same three planes.
struct Planes29 { const uint4 *p0, *p1; const uint32_t *p2; };
struct PlanesOut29 { uint4 *p0, *p1; uint32_t *p2; };
struct NttPass29Args {
    unsigned log_n, s0, s1, clog, tlog;
    int first, last, premul, postmul;
    Planes29 tw, pw_lo, pw_hi;
    Fr29 scale;             // Montgomery (R') form, canonical; the Montgomery one when no scaling is asked for
    // a BATCH of up to three transforms of one size in one launch (grid.y; r1cs_to_qap::witness_map runs three at every step): transform b
    // reads the canonical words of in[b] in its first pass, writes those of out[b] in its last, and keeps its lazy values between passes
    // in the slice [b 2^log_n, (b + 1) 2^log_n) of every scratch plane
    const Fr *in[3];
    Fr *out[3];
    size_t in_stride, out_stride;      // != 0: transform b reads in[0] + b in_stride and writes out[0] + b out_stride (any number of transforms: a batch of proofs)
    // fused load of the first pass (witness_map's last transform): the value transformed is in[0][i] * fuse_b[i] - fuse_c[i], left with the
    // factor 2^-261 of the two products (the caller folds 2^261 into the scale); nullptr: plain load
    const Fr *fuse_b, *fuse_c;
};
__device__ __forceinline__ Fr29 ld29(const Planes29 &t, size_t j) {
    Fr29 v; uint4 a = t.p0[j], b = t.p1[j];
    v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w; v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w; v.l[8] = t.p2[j];
    return v;
}
__device__ __forceinline__ Fr29 lds_load29(const uint4 *pl0, const uint4 *pl1, const uint32_t *pl2, unsigned e) {
    Fr29 v; uint4 a = pl0[e], b = pl1[e];
    v.l[0] = a.x; v.l[1] = a.y; v.l[2] = a.z; v.l[3] = a.w; v.l[4] = b.x; v.l[5] = b.y; v.l[6] = b.z; v.l[7] = b.w; v.l[8] = pl2[e];
    return v;
}
__device__ __forceinline__ void lds_store29(uint4 *pl0, uint4 *pl1, uint32_t *pl2, unsigned e, const Fr29 &v) {
    pl0[e] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
    pl1[e] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
    pl2[e] = v.l[8];
}

#ifdef VSP_DIAG_CLOCK
__device__ unsigned long long vsp_diag_ntt_sums[4096][4];    // per workgroup slot: shader cycles, 100 MHz ticks, waves (diagnostic build only; ONE address for all waves cost 390 us per pass)
#endif
__global__ __launch_bounds__(NTT_THREADS) void k_ntt29_pass(Planes29 in_lazy, PlanesOut29 out_lazy, NttPass29Args p) {
#if defined(__HIP_DEVICE_COMPILE__)
    __shared__ uint4 lds[2u << NTT_TILE_LOG];
    __shared__ uint32_t lds8[1u << NTT_TILE_LOG];
    const Fr *__restrict__ in_words = p.in_stride ? p.in[0] + (size_t)blockIdx.y * p.in_stride : p.in[blockIdx.y];
    Fr *__restrict__ out_words = p.out_stride ? p.out[0] + (size_t)blockIdx.y * p.out_stride : p.out[blockIdx.y];
    const size_t fuse_off = (size_t)blockIdx.y * p.in_stride;      // the fused load's other two operands follow their transform
    { const size_t boff = (size_t)blockIdx.y << p.log_n;          // this transform's slice of the scratch planes
      in_lazy.p0 += boff; in_lazy.p1 += boff; in_lazy.p2 += boff; out_lazy.p0 += boff; out_lazy.p1 += boff; out_lazy.p2 += boff; }
#ifdef VSP_DIAG_CLOCK
    // DIAGNOSTIC BUILD ONLY (libvsp_hip_diag.so): the clock the chip holds inside a pass, stamped once per wave around the whole pass
    unsigned long long dc_t0, dc_r0, dc_t1, dc_r1;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t0), "=s"(dc_r0) :: "memory");
#endif
    const unsigned K = p.s1 - p.s0;
    const unsigned C = 1u << p.clog;
    const unsigned tile = 1u << (K + p.clog);
    uint4 *pl0 = lds, *pl1 = lds + tile;
    uint32_t *pl2 = lds8;
    const unsigned tid = threadIdx.x;
    const unsigned wg = blockIdx.x;
    const unsigned lo_bits = p.s0 - p.clog;                   // only meaningful when !first
    const unsigned lo_hi = p.first ? 0u : (wg & ((1u << lo_bits) - 1u));
    const unsigned hi = p.first ? 0u : (wg >> lo_bits);
    const size_t base_pos = p.first ? 0 : (((size_t)hi << p.s1) | ((size_t)lo_hi << p.clog));

    // ---- load tile
    for (unsigned e = tid; e < tile; e += NTT_THREADS) {
        unsigned mid = e >> p.clog, c = e & (C - 1);
        size_t src;
        if (p.first) src = ((size_t)brev(mid, p.s1) << (p.log_n - p.s1)) + (size_t)wg * C + c;
        else src = base_pos | ((size_t)mid << p.s0) | c;
        Fr29 v;
        if (p.first) {
            v = fr29_from_words(in_words[src]);
            if (p.fuse_b) {                                       // (a b - c) / 2^261: two products of canonical operands, one lazy subtraction, one carry pass
                Fr29 one; for (int k = 0; k < 9; k++) one.l[k] = k == 0 ? 1u : 0u;
                v = norm29(sub29(mul29(v, fr29_from_words(p.fuse_b[fuse_off + src])), mul29(fr29_from_words(p.fuse_c[fuse_off + src]), one)));
            }
            if (p.premul) v = mul29(v, mul29(ld29(p.pw_lo, src & ((1u << PW_LOG) - 1u)), ld29(p.pw_hi, src >> PW_LOG)));
        } else v = ld29(in_lazy, src);
        lds_store29(pl0, pl1, pl2, e, v);
    }
    __syncthreads();

    const unsigned lo_part = p.first ? 0u : ((lo_hi << p.clog));
    unsigned t = 0;
    // the transform's first stage (s == 0) has the twiddle one and no product: the values as LOADED are its subtrahends.  A plain load is
    // canonical and a premultiplied one a product output -- sub29's 2r covers them; the fused load leaves a lazy value up to 3.03 r, which
    // needs the redundant 4r (sub29k4; fr29.h).  A per-pass constant picks a copy of the stage, as for the first pair of products below.
    const bool fused_first = p.first && p.fuse_b != nullptr;
    if (K & 1) {
        const unsigned s = p.s0;
        auto stage = [&](auto fused_load) {
            constexpr bool FUSED = decltype(fused_load)::value;
            for (unsigned bf = tid; bf < (tile >> 1); bf += NTT_THREADS) {
                unsigned c = bf & (C - 1), q = bf >> p.clog;
                unsigned e0 = (q << (1 + p.clog)) | c, e1 = e0 + C;
                Fr29 u = lds_load29(pl0, pl1, pl2, e0), v = lds_load29(pl0, pl1, pl2, e1);
                if (!FUSED && s > 0) v = mul29(v, ld29(p.tw, (size_t)(p.first ? 0u : (lo_part | c)) << (p.tlog - 1 - s)));
                lds_store29(pl0, pl1, pl2, e0, norm29(add29(u, v)));
                lds_store29(pl0, pl1, pl2, e1, norm29(FUSED ? sub29k4(u, v) : sub29(u, v)));       // s == 0 only in the first pass: v is a loaded input there
            }
        };
        if (s == 0 && fused_first) stage(std::true_type{}); else stage(std::false_type{});
        __syncthreads();
        t = 1;
    }
    for (; t < K; t += 2) {
        const unsigned s = p.s0 + t;
        const unsigned h = 1u << t;
        // the first pair of products exists from stage 1 on (stage 0's twiddle is one).  Copies of the loop, not a branch inside it:
        // a value that is "the loaded x1 or the product" is ONE register set for the compiler, which then loads x1 into the routine's
        // result registers and copies it to the operand registers before every call (nine copies per product, section 3.2 of DESIGN.md)
        auto group = [&](unsigned g, auto with_first_pair, auto fused_load) {
            constexpr bool TW1 = decltype(with_first_pair)::value;
            constexpr bool FUSED = decltype(fused_load)::value;           // stage 0 of a fused load: raw subtrahends up to 3.03 r
            static_assert(!(TW1 && FUSED), "a product output never needs the 4r subtraction");
            unsigned c = g & (C - 1), q = g >> p.clog;
            unsigned mid_lo = q & (h - 1);
            unsigned mid0 = ((q >> t) << (t + 2)) | mid_lo;
            unsigned e0 = (mid0 << p.clog) | c, e1 = e0 + (h << p.clog), e2 = e1 + (h << p.clog), e3 = e2 + (h << p.clog);
            const size_t off = p.first ? 0u : (lo_part | c);
            Fr29 x1 = lds_load29(pl0, pl1, pl2, e1), x3 = lds_load29(pl0, pl1, pl2, e3);
            if constexpr (TW1) {
                const Fr29 w1 = ld29(p.tw, (((size_t)mid_lo << p.s0) | off) << (p.tlog - 1 - s));
                x1 = mul29(x1, w1); x3 = mul29q(x3, w1);
            }
            Fr29 x0 = lds_load29(pl0, pl1, pl2, e0), x2 = lds_load29(pl0, pl1, pl2, e2);
            Fr29 a0 = add29(x0, x1), a1 = FUSED ? sub29k4(x0, x1) : sub29(x0, x1), a2 = add29(x2, x3), a3 = FUSED ? sub29k4(x2, x3) : sub29(x2, x3);
            a2 = mul29(a2, ld29(p.tw, (((size_t)mid_lo << p.s0) | off) << (p.tlog - 2 - s)));
            a3 = mul29q(a3, ld29(p.tw, (((size_t)(mid_lo + h) << p.s0) | off) << (p.tlog - 2 - s)));
            lds_store29(pl0, pl1, pl2, e0, norm29(add29(a0, a2)));
            lds_store29(pl0, pl1, pl2, e1, norm29(add29(a1, a3)));
            lds_store29(pl0, pl1, pl2, e2, norm29(sub29(a0, a2)));
            lds_store29(pl0, pl1, pl2, e3, norm29(sub29(a1, a3)));
        };
        if (s > 0) for (unsigned g = tid; g < (tile >> 2); g += NTT_THREADS) group(g, std::true_type{}, std::false_type{});
        else if (fused_first) for (unsigned g = tid; g < (tile >> 2); g += NTT_THREADS) group(g, std::false_type{}, std::true_type{});
        else for (unsigned g = tid; g < (tile >> 2); g += NTT_THREADS) group(g, std::false_type{}, std::false_type{});
        __syncthreads();
    }

    // ---- store tile
    for (unsigned i = tid; i < tile; i += NTT_THREADS) {
        unsigned mid, c; size_t pos;
        if (p.first) { mid = i & ((1u << K) - 1u); c = i >> K; pos = ((size_t)brev(wg * C + c, p.log_n - p.s1) << p.s1) | mid; }
        else { mid = i >> p.clog; c = i & (C - 1); pos = base_pos | ((size_t)mid << p.s0) | c; }
        Fr29 v = lds_load29(pl0, pl1, pl2, (mid << p.clog) | c);
        if (p.last) {
            Fr29 m = p.scale;
            if (p.postmul == 2) m = mul29(m, mul29(ld29(p.pw_lo, pos & ((1u << PW_LOG) - 1u)), ld29(p.pw_hi, pos >> PW_LOG)));
            out_words[pos] = fr29_to_words(csub29(mul29(v, m)));
        } else {
            out_lazy.p0[pos] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
            out_lazy.p1[pos] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
            out_lazy.p2[pos] = v.l[8];
        }
    }
#ifdef VSP_DIAG_CLOCK
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dc_t1), "=s"(dc_r1) :: "memory");
    if ((threadIdx.x & 63u) == 0) {
        unsigned long long *slot = vsp_diag_ntt_sums[(blockIdx.x + 2048u * blockIdx.y) & 4095u];
        atomicAdd(&slot[0], dc_t1 - dc_t0); atomicAdd(&slot[1], dc_r1 - dc_r0); atomicAdd(&slot[2], 1ull);
    }
#endif
#endif
}

// 8 x 32-bit Montgomery table -> three planes in the R' = 2^261 form
__global__ __launch_bounds__(256) void k_table29(const Fr *in, size_t count, uint4 *p0, uint4 *p1, uint32_t *p2) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    Fr29 v = fr29_from_mont256(in[j]);
    p0[j] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]); p1[j] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]); p2[j] = v.l[8];
#endif
}

// T[j] = A[j & 2047] * B[j >> 11]  (all Montgomery)
__global__ __launch_bounds__(256) void k_fill_twiddles(Fr *T, const Fr *A, const Fr *B, size_t count) {
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < count) T[j] = mul(A[j & ((1u << PW_LOG) - 1u)], B[j >> PW_LOG]);
}

// ---- host side ----------------------------------------------------------------------------------
// diagnostic build: clock held inside the passes of the 29-bit transform since the last reset
int ntt_diag_clock(vsp_ctx *ctx, int reset, double *ghz, double *waves) {
#ifdef VSP_DIAG_CLOCK
    std::vector<unsigned long long> all(4096 * 4, 0);
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    VSP_HIP(hipMemcpyFromSymbol(all.data(), HIP_SYMBOL(vsp_diag_ntt_sums), all.size() * sizeof(unsigned long long)));
    unsigned long long h[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < 4096; i++) for (int j = 0; j < 3; j++) h[j] += all[4 * i + j];
    if (ghz) *ghz = h[1] ? (double)h[0] / (double)h[1] * 0.1 : 0.0;
    if (waves) *waves = (double)h[2];
    if (reset) { std::fill(all.begin(), all.end(), 0ull); VSP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(vsp_diag_ntt_sums), all.data(), all.size() * sizeof(unsigned long long))); }
    return VSP_OK;
#else
    (void)reset; if (ghz) *ghz = 0.0; if (waves) *waves = 0.0;
    return set_error(ctx, VSP_ERR_UNSUPPORTED, "diag_clock: this is not the diagnostic build (make diag -> libvsp_hip_diag.so)");
#endif
}
static const uint64_t FR_ROOT_2_32[4] = {0x3829971f439f0d2bULL, 0xb63683508c2280b9ULL, 0xd09b681922c813b4ULL, 0x16a2a19edfe81f20ULL};

HFr host_omega(unsigned log_m) {
    HFr w = host_load_canon<HFr>(FR_ROOT_2_32);
    for (unsigned i = log_m; i < 32; i++) w = sqr(w);
    return w;
}


// lo[k] = base^k (k < 2^PW_LOG), hi[k] = base^(k << PW_LOG) (k < hi_count), Montgomery form
int upload_power_tables(vsp_ctx *ctx, const HFr &base, size_t hi_count, DevBuf &lo, DevBuf &hi) {
    const size_t L = (size_t)1 << PW_LOG;
    std::vector<HFr> a(L), b(hi_count);
    HFr acc = HFr::one();
    for (size_t k = 0; k < L; k++) { a[k] = acc; acc = mul(acc, base); }
    HFr step = acc;                      // base^(2^PW_LOG)
    acc = HFr::one();
    for (size_t k = 0; k < hi_count; k++) { b[k] = acc; acc = mul(acc, step); }
    VSP_TRY(ensure(ctx, lo, L * sizeof(Fr)));
    VSP_TRY(ensure(ctx, hi, hi_count * sizeof(Fr)));
    VSP_HIP(hipMemcpyAsync(lo.p, a.data(), L * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    VSP_HIP(hipMemcpyAsync(hi.p, b.data(), hi_count * sizeof(Fr), hipMemcpyHostToDevice, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));     // a, b go out of scope
    return VSP_OK;
}

int ntt_ensure_twiddles(vsp_ctx *ctx, unsigned log_m) {
    NttTables &t = ctx->ntt;
    if (t.log >= log_m && t.fwd.p) return VSP_OK;
    unsigned lg = log_m < 1 ? 1 : log_m;
    size_t count = (size_t)1 << (lg - 1);
    size_t hi_count = count > ((size_t)1 << PW_LOG) ? (count >> PW_LOG) : 1;
    DevBuf lo, hi;                // gone at every return
    for (int dir = 0; dir < 2; dir++) {
        HFr w = host_omega(lg);
        if (dir) w = inv(w);
        VSP_TRY(upload_power_tables(ctx, w, hi_count, lo, hi));
        DevBuf &dst = dir ? t.inv : t.fwd;
        VSP_TRY(ensure(ctx, dst, count * sizeof(Fr)));
        unsigned blocks = (unsigned)((count + 255) / 256);
        hipLaunchKernelGGL(k_fill_twiddles, dim3(blocks), dim3(256), 0, ctx->stream, (Fr *)dst.p, (const Fr *)lo.p, (const Fr *)hi.p, count);
        VSP_LAUNCH_CHECK();
    }
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    t.log = lg;
    t.log29 = 0;                 // the 29-bit copies follow on demand (ntt29_ensure_tables)
    return VSP_OK;
}

int ntt_ensure_coset_tables(vsp_ctx *ctx, unsigned log_m, const uint64_t *g4) {
    NttTables &t = ctx->ntt;
    if (t.pw_valid && t.pw_log >= log_m && memcmp(t.pw_g, g4, 32) == 0) return VSP_OK;
    size_t n = (size_t)1 << log_m;
    size_t hi_count = n > ((size_t)1 << PW_LOG) ? (n >> PW_LOG) : 1;
    HFr g = host_load_canon<HFr>(g4);
    VSP_TRY(upload_power_tables(ctx, g, hi_count, t.pw_lo_f, t.pw_hi_f));
    VSP_TRY(upload_power_tables(ctx, inv(g), hi_count, t.pw_lo_i, t.pw_hi_i));
    memcpy(t.pw_g, g4, 32); t.pw_log = log_m; t.pw_valid = true;
    t.pw29_valid = false;
    return VSP_OK;
}

// the three planes of a 29-bit table of `count` entries stored at `base`
static Planes29 planes_of(const DevBuf &b, size_t count) {
    Planes29 pl; pl.p0 = (const uint4 *)b.p; pl.p1 = (const uint4 *)((const char *)b.p + 16 * count); pl.p2 = (const uint32_t *)((const char *)b.p + 32 * count);
    return pl;
}
static int convert_table29(vsp_ctx *ctx, const DevBuf &src, size_t count, DevBuf &dst) {
    VSP_TRY(ensure(ctx, dst, 36 * count));
    hipLaunchKernelGGL(k_table29, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, (const Fr *)src.p, count,
                       (uint4 *)dst.p, (uint4 *)((char *)dst.p + 16 * count), (uint32_t *)((char *)dst.p + 32 * count));
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}
// 29-bit copies of the twiddle tables (and of the coset power tables when a coset generator is in use), converted on the GPU
static int ntt29_ensure_tables(vsp_ctx *ctx, bool coset) {
    NttTables &t = ctx->ntt;
    if (t.log29 != t.log) {
        const size_t count = (size_t)1 << (t.log - 1);
        VSP_TRY(convert_table29(ctx, t.fwd, count, t.fwd29));
        VSP_TRY(convert_table29(ctx, t.inv, count, t.inv29));
        t.log29 = t.log;
    }
    if (coset && !(t.pw29_valid && t.pw29_log == t.pw_log && memcmp(t.pw29_g, t.pw_g, 32) == 0)) {
        const size_t L = (size_t)1 << PW_LOG, n = (size_t)1 << t.pw_log, H = n > L ? (n >> PW_LOG) : 1;
        VSP_TRY(convert_table29(ctx, t.pw_lo_f, L, t.pw29[0])); VSP_TRY(convert_table29(ctx, t.pw_hi_f, H, t.pw29[1]));
        VSP_TRY(convert_table29(ctx, t.pw_lo_i, L, t.pw29[2])); VSP_TRY(convert_table29(ctx, t.pw_hi_i, H, t.pw29[3]));
        memcpy(t.pw29_g, t.pw_g, 32); t.pw29_log = t.pw_log; t.pw29_valid = true;
    }
    return VSP_OK;
}
// host value (Montgomery, R = 2^256) -> canonical x * 2^261 mod r as 9 x 29-bit limbs: the Montgomery form of the 29-bit kernels
static Fr29 host_to_fr29_mont(const HFr &x) {
    uint64_t c[4]; host_store_canon(c, x);
    HFr acc = host_load_canon<HFr>(c);                  // x again, through its canonical form
    for (int i = 0; i < 261; i++) acc = add(acc, acc);
    host_store_canon(c, acc);
    Fr29 r;
    for (int i = 0; i < 9; i++) {
        const int bit = 29 * i, w = bit >> 6, s2 = bit & 63;
        unsigned __int128 v = c[w];
        if (w + 1 < 4) v |= (unsigned __int128)c[w + 1] << 64;
        r.l[i] = (uint32_t)(v >> s2) & (i < 8 ? 0x1FFFFFFFu : 0xFFFFFFFFu);
    }
    return r;
}

// Known-answer check of the 29-bit-limb butterflies THROUGH k_ntt29_pass (its product, vsp_mm29, is a hand-laid-out routine with a private
// calling convention: see the note at bases.hip fp28_known_answer_check).  Once per context, before the first transform on that path: a
// 2^13-point vector (two passes: the lazy planes between passes, the first and the last pass) goes through a forward coset transform
// and an inverse coset transform on k_ntt29_pass and on the 8 x 32-bit k_ntt_pass, each path forced by its request; the outputs must
// agree word for word.  On a mismatch the context falls back to the 8 x 32-bit kernel ("ntt_fr29" = 0) for its lifetime.  A check that
// could not run leaves no verdict (ntt29_checked stays 0): the 8 x 32-bit kernel this time, the check again next time.
static void ntt29_known_answer_check(vsp_ctx *ctx) {
    const unsigned lg = 13; const size_t n = (size_t)1 << lg, bytes = n * sizeof(Fr);
    std::vector<uint64_t> h(n * 4), o29(n * 4), o32(n * 4);
    SplitMix64 next{0x243F6A8885A308D3ULL};
    for (size_t i = 0; i < n; i++) { h[4 * i] = next(); h[4 * i + 1] = next(); h[4 * i + 2] = next(); h[4 * i + 3] = next() >> 2; }
    h[0] = h[1] = h[2] = h[3] = 0;                            // a zero and r - 1 among them
    h[4] = 0xffffffff00000000ULL; h[5] = 0x53bda402fffe5bfeULL; h[6] = 0x3339d80809a1d805ULL; h[7] = 0x73eda753299d7d48ULL;
    const uint64_t g7[4] = {7, 0, 0, 0};
    DevBuf buf;
    bool ran = false, same = true;
    if (buf.alloc(bytes) == hipSuccess) {
        void *d = buf.p;
        ran = true;
        for (int inverse = 0; inverse < 2 && ran; inverse++) {
            for (int path = 0; path < 2 && ran; path++) {
                NttRequest rq((Fr *)d, lg, inverse, g7);
                rq.path = path == 0 ? NTT_FR29 : NTT_FR32;
                std::vector<uint64_t> &out = path == 0 ? o29 : o32;
                ran = hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
                      ntt_launch(ctx, rq) == VSP_OK &&
                      hipMemcpyAsync(out.data(), d, bytes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
                      hipStreamSynchronize(ctx->stream) == hipSuccess;
            }
            if (ran && memcmp(o29.data(), o32.data(), bytes) != 0) same = false;
        }
    }
    hipGetLastError();
    if (!ran) { ctx->stats["ntt_fr29_selfcheck"] = 0.0; return; }
    record_verdict(ctx, ctx->ntt29_checked, same, "ntt_fr29_selfcheck_fault", "ntt_fr29_selfcheck", "ntt_fr29",
                   "ntt: the 29-bit-limb butterfly kernel failed its known-answer check; 8 x 32-bit kernel in use");
}

// whether the 29-bit butterflies are in use on this context; runs their known-answer check when it has not run yet.  Callers that set
// tables up (ntt_launch, the step-domain glue) ask this first: the check's own transforms may rebuild the twiddle and coset tables.
bool ntt29_in_use(vsp_ctx *ctx) {
    if (!opt(ctx, "ntt_fr29", 1)) return false;
    if (ctx->ntt29_checked == 0) ntt29_known_answer_check(ctx);
    return ctx->ntt29_checked == 1;
}

// passes of at most NTT_MAX_STAGES stages each, as even as the stage count allows; returns their number
static unsigned ntt_plan(unsigned log_m, unsigned stages[8]) {
    const unsigned npass = log_m <= NTT_TILE_LOG ? 1 : (log_m + NTT_MAX_STAGES - 1) / NTT_MAX_STAGES;
    for (unsigned i = 0; i < npass; i++) stages[i] = log_m / npass + (i < log_m % npass ? 1 : 0);
    // radix-4 steps take stages two at a time: trade a stage between two odd passes (7 + 7 -> 8 + 6), earlier pass the larger
    for (unsigned i = 0; i + 1 < npass; i++)
        if (stages[i] & 1)
            for (unsigned k = i + 1; k < npass; k++)
                if ((stages[k] & 1) && stages[i] < NTT_MAX_STAGES && stages[k] > 1) { stages[i]++; stages[k]--; break; }
    return npass;
}

int ntt_launch(vsp_ctx *ctx, const NttRequest &rq) {
    const bool strided = rq.in_stride || rq.out_stride;
    if (strided && (rq.count < 1 || rq.count > 65535)) return set_error(ctx, VSP_ERR_ARG, "ntt: batch size");
    if (!strided && (rq.count < 1 || rq.count > 3)) return set_error(ctx, VSP_ERR_ARG, "ntt: batch of 1..3 transforms");
    if (rq.log_m > 28) return set_error(ctx, VSP_ERR_UNSUPPORTED, "ntt: log_m > 28");
    if (rq.coset_g && !(rq.coset_g[0] | rq.coset_g[1] | rq.coset_g[2] | rq.coset_g[3])) return set_error(ctx, VSP_ERR_ARG, "ntt: coset generator is zero");
    const bool use29 = rq.path == NTT_AUTO ? ntt29_in_use(ctx) : rq.path == NTT_FR29;
    if (!use29 && (rq.count > 1 || rq.fuse_b || rq.in[0] != rq.out[0])) return set_error(ctx, VSP_ERR_UNSUPPORTED, "ntt: batched / fused transforms need the 29-bit butterflies");
    VSP_TRY(ntt_ensure_twiddles(ctx, rq.log_m));
    if (rq.coset_g) VSP_TRY(ntt_ensure_coset_tables(ctx, rq.log_m, rq.coset_g));
    if (use29) VSP_TRY(ntt29_ensure_tables(ctx, rq.coset_g != nullptr));
    const NttTables &t = ctx->ntt;
    const size_t n = (size_t)1 << rq.log_m;
    unsigned stages[8];
    const unsigned npass = ntt_plan(rq.log_m, stages);
    // between passes: lazy values in three planes, a slice per transform (29-bit), or canonical words (8 x 32-bit)
    if (npass > 1) VSP_TRY(ensure(ctx, ctx->ntt_scratch, (size_t)rq.count * n * (use29 ? 36 : sizeof(Fr))));

    HFr scale = HFr::one();
    if (rq.inverse) scale = inv(host_from_u64((uint64_t)n));
    if (rq.extra_scale) scale = mul(scale, *rq.extra_scale);
    const bool have_scale = rq.inverse || rq.extra_scale;
    const bool coset_in = rq.coset_g && !rq.inverse, coset_out = rq.coset_g && rq.inverse;      // g^i at the first load, ginv^i at the last store
    Fr29 scale29;
    if (use29) scale29 = host_to_fr29_mont(scale);
    const size_t tcount = (size_t)1 << (t.log - 1), L = (size_t)1 << PW_LOG, pn = (size_t)1 << t.pw_log, H = pn > L ? (pn >> PW_LOG) : 1;
    const Planes29 lazy_in = planes_of(ctx->ntt_scratch, (size_t)rq.count * n);
    const PlanesOut29 lazy_out = {(uint4 *)lazy_in.p0, (uint4 *)lazy_in.p1, (uint32_t *)lazy_in.p2};
    Fr *scratch = (Fr *)ctx->ntt_scratch.p;

    for (unsigned i = 0, s0 = 0; i < npass; s0 += stages[i], i++) {
        const bool first = i == 0, last = i + 1 == npass;
        const unsigned clog = npass == 1 ? 0 : NTT_TILE_LOG - stages[i];
        if (!first && s0 < clog) return set_error(ctx, VSP_ERR_UNSUPPORTED, "ntt: pass plan");
        auto common = [&](auto &p) {          // the fields both pass kernels read alike
            memset(&p, 0, sizeof p);
            p.log_n = rq.log_m; p.s0 = s0; p.s1 = s0 + stages[i]; p.clog = clog; p.tlog = t.log;
            p.first = first; p.last = last; p.premul = first && coset_in;
        };
        const dim3 grid((unsigned)(n >> (stages[i] + clog)), rq.count);
        if (use29) {
            NttPass29Args p; common(p);
            p.postmul = last && coset_out ? 2 : 1;                  // the last pass always multiplies: by the scale or by one
            p.tw = planes_of(rq.inverse ? t.inv29 : t.fwd29, tcount);
            if (p.premul) { p.pw_lo = planes_of(t.pw29[0], L); p.pw_hi = planes_of(t.pw29[1], H); }
            if (p.postmul == 2) { p.pw_lo = planes_of(t.pw29[2], L); p.pw_hi = planes_of(t.pw29[3], H); }
            p.scale = scale29;
            for (int b = 0; b < 3; b++) { p.in[b] = rq.in[b]; p.out[b] = rq.out[b]; }
            p.in_stride = rq.in_stride; p.out_stride = rq.out_stride;
            if (first) { p.fuse_b = rq.fuse_b; p.fuse_c = rq.fuse_c; }
            hipLaunchKernelGGL(k_ntt29_pass, grid, dim3(NTT_THREADS), 0, ctx->stream, lazy_in, lazy_out, p);
        } else {
            NttPassArgs p; common(p);
            p.postmul = !last ? 0 : coset_out ? 2 : have_scale ? 1 : 0;      // without a scale the last pass stores as it is
            p.tw = (const Fr *)(rq.inverse ? t.inv.p : t.fwd.p);
            if (p.premul) { p.pw_lo = (const Fr *)t.pw_lo_f.p; p.pw_hi = (const Fr *)t.pw_hi_f.p; }
            if (p.postmul == 2) { p.pw_lo = (const Fr *)t.pw_lo_i.p; p.pw_hi = (const Fr *)t.pw_hi_i.p; }
            p.scale = to_dev(scale);
            hipLaunchKernelGGL(k_ntt_pass, grid, dim3(NTT_THREADS), 0, ctx->stream, first ? rq.in[0] : scratch, last ? rq.out[0] : scratch, p);
        }
        VSP_LAUNCH_CHECK();
    }
    ctx->stats["ntt_passes"] = (double)npass;
    ctx->stats["ntt_fr29"] = use29 ? 1 : 0;
    ctx->stats["ntt_fused_load"] = rq.fuse_b ? 1 : 0;      // the first pass computed its own input (witness_map's last transform)
    return VSP_OK;
}

}  // namespace vsp
