// extern "C" surface of libvsp_hip.so (declared in include/vsp.h): context, device memory, MSM / NTT / witness_map entry points and
// Jacobian record folding (resident bases live in bases.hip, the point compression with the other wire formats in wire.hip).
#include "common.h"
#include "fp28.h"
#include "fr29.h"
#include "gt_dlog.h"
#include "lane_view.h"

namespace vsp {

int set_hip_error(vsp_ctx *ctx, hipError_t e, const char *what, const char *file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    if (ctx) ctx->err = buf;
    return VSP_ERR_HIP;
}
int set_error(vsp_ctx *ctx, int code, const char *msg) {
    if (ctx) ctx->err = msg;
    return code;
}
int ensure(vsp_ctx *ctx, DevBuf &b, size_t bytes, hipStream_t wait) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes && b.p) return VSP_OK;
    if (b.p) { VSP_HIP(hipStreamSynchronize(wait)); b.reset(); }
    const size_t want = bytes + bytes / 8;
    const hipError_t e = b.alloc(want);
    if (e != hipSuccess) { char m[128]; snprintf(m, sizeof m, "device allocation of %zu bytes failed: %s", want, hipGetErrorString(e)); return set_error(ctx, VSP_ERR_NOMEM, m); }
    return VSP_OK;
}
int ensure_pinned(vsp_ctx *ctx, PinnedBuf &b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes && b.p) return VSP_OK;
    VSP_HIP(b.alloc(bytes + bytes / 8));
    return VSP_OK;
}

template <class HF> static int finish_affine(const XYZZ<HF> &acc, uint64_t *out_affine, int *out_is_inf) {
    if (out_affine) host_store_affine(out_affine, xyzz_to_affine(acc));
    if (out_is_inf) *out_is_inf = is_inf(acc) ? 1 : 0;
    return VSP_OK;
}

// elementwise field operations on canonical values (diagnostic entry point vsp_selftest_field)
template <class F> __global__ __launch_bounds__(64) void k_selftest_field(int op, const F *a, const F *b, F *out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    F x = a[i], y = b[i], r;
    switch (op) {
        case 0: r = from_mont(mul(to_mont(x), to_mont(y))); break;
        case 1: r = add(x, y); break;
        case 2: r = sub(x, y); break;
        case 3: r = from_mont(sqr(to_mont(x))); break;
        case 4: r = mul(x, to_mont(y)); break;          // canonical x Montgomery -> canonical (the NTT butterfly product)
        default: r = from_mont(inv(to_mont(x))); break;
    }
    out[i] = r;
}

// the 14 x 28-bit lazy field of the G1 accumulation (fp28.h) against the 12 x 32-bit one, on canonical inputs:
//   op 6 round trip, 7 product, 8 (x - y)^2 through the K32 subtraction and a carry pass, 9 x - 3y through the K8 subtraction of a
//   lazy sum, 10 x (y - x) with a loose operand, 11 -y x through the negation used for signed digits, 12 x (y - x) - y x as one dual product
__global__ __launch_bounds__(64) void k_selftest_fp28(int op, const Fp *a, const Fp *b, Fp *out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp28 x = fp_to_fp28(to_mont(a[i])), y = fp_to_fp28(to_mont(b[i])), r;
    switch (op) {
        case 6: r = x; break;
        case 7: r = mul28(x, y); break;
        case 8: { Fp28 d = norm28(sub28(x, FP28_K32_L1, y)); r = sqr28(d); } break;          // through the dedicated squaring routine
        case 9: { Fp28 s3; for (int k = 0; k < 14; k++) s3.l[k] = y.l[k] + 2u * y.l[k]; r = norm28(sub28(x, FP28_K8_L4, s3)); } break;
        case 10: r = mul28(x, sub28(y, FP28_K32_L1, x)); break;
        case 11: r = mul28(neg28(FP28_K8_L1, y), x); break;
        default: r = mul28x2(x, sub28(y, FP28_K32_L1, x), neg28(FP28_K32_L1, y), x); break;    // op 12: x (y - x) - y x through the dual product
    }
    out[i] = from_mont(fp28_to_fp(r));
#endif
}

// the 9 x 29-bit lazy field of the NTT butterflies (fr29.h), on canonical inputs, canonical out:
//   op 6 round trip through the limb form, 7 x y through vsp_mm29 (y brought to the R' = 2^261 Montgomery form the way fr29_from_mont256
//   makes the tables) and the conditional subtraction, 8 the same through vsp_mm29q (the routine's second register map), 9 x + x y - y^2
//   through add29, sub29, norm29 and the product with the Montgomery one that leaves the lazy domain: the butterfly's own chain
__global__ __launch_bounds__(64) void k_selftest_fr29(int op, const Fr *a, const Fr *b, Fr *out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fr29 x = fr29_from_words(a[i]), y = fr29_from_words(b[i]), r;
    const Fr29 ym = csub29(mul29(y, fr29_const(FR29_R2)));                  // y R'^2 / R' = y R', below 2r -> canonical
    switch (op) {
        case 6: r = x; break;
        case 7: r = csub29(mul29(x, ym)); break;
        case 8: r = csub29(mul29q(x, ym)); break;
        default: {                                                          // op 9
            Fr29 xy = mul29(x, ym), yy = mul29q(y, ym);                     // product outputs below 1.02 r
            Fr29 s = norm29(sub29(add29(x, xy), yy));                       // x + x y + 2r - y^2, below 4.03 r
            r = csub29(mul29(s, fr29_const(FR29_ONE)));
        } break;
    }
    out[i] = fr29_to_words(r);
#endif
}

// The full addition of two bucket sums (curve.h / fp28.h xyzz_add) on its own, in each of the four forms the merges and the bucket
// reduction run it in (diagnostic entry point vsp_selftest_xyzz_add): canonical X, Y, ZZ, ZZZ in, canonical out.  Lanes of one wave take
// different paths (ordinary sum, doubling, cancellation, infinity on either side) as the test orders its cases -- the divergence the
// kernels meet.  form 0: 12 x 32-bit limbs; 1: 14 x 28-bit lazy limbs.  G2 runs on lane pairs (two lanes per point).
__device__ __forceinline__ Fp &fp_of(Fp &x) { return x; }
__device__ __forceinline__ Fp &fp_of(Fp2L &x) { return x.v; }
__device__ __forceinline__ Fp28 &fp28_of(Fp28 &x) { return x; }
__device__ __forceinline__ Fp28 &fp28_of(Fp28L &x) { return x.v; }
template <class M, class F28> __global__ __launch_bounds__(64) void k_selftest_xyzz_add(int form, const XYZZ<M> *a, const XYZZ<M> *b, XYZZ<M> *out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    using LV = LaneView<M>; using E = typename LV::E; using E28 = typename LaneView<F28>::E;
    const size_t i = gid<M>();
    if (i >= n) return;                                           // both lanes of a pair leave together
    XYZZ<E> x = LV::load(&a[i]), y = LV::load(&b[i]);
    for (XYZZ<E> *v : {&x, &y}) { fp_of(v->X) = to_mont(fp_of(v->X)); fp_of(v->Y) = to_mont(fp_of(v->Y)); fp_of(v->ZZ) = to_mont(fp_of(v->ZZ)); fp_of(v->ZZZ) = to_mont(fp_of(v->ZZZ)); }
    if (form == 0) xyzz_add(x, y);
    else {
        XYZZ<E28> x28, y28;                                       // zero stays zero: infinity is all-zero in both forms
        fp28_of(x28.X) = fp_to_fp28(fp_of(x.X)); fp28_of(x28.Y) = fp_to_fp28(fp_of(x.Y)); fp28_of(x28.ZZ) = fp_to_fp28(fp_of(x.ZZ)); fp28_of(x28.ZZZ) = fp_to_fp28(fp_of(x.ZZZ));
        fp28_of(y28.X) = fp_to_fp28(fp_of(y.X)); fp28_of(y28.Y) = fp_to_fp28(fp_of(y.Y)); fp28_of(y28.ZZ) = fp_to_fp28(fp_of(y.ZZ)); fp28_of(y28.ZZZ) = fp_to_fp28(fp_of(y.ZZZ));
        xyzz_add(x28, y28);
        fp_of(x.X) = fp28_to_fp(fp28_of(x28.X)); fp_of(x.Y) = fp28_to_fp(fp28_of(x28.Y)); fp_of(x.ZZ) = fp28_to_fp(fp28_of(x28.ZZ)); fp_of(x.ZZZ) = fp28_to_fp(fp28_of(x28.ZZZ));
    }
    fp_of(x.X) = from_mont(fp_of(x.X)); fp_of(x.Y) = from_mont(fp_of(x.Y)); fp_of(x.ZZ) = from_mont(fp_of(x.ZZ)); fp_of(x.ZZZ) = from_mont(fp_of(x.ZZZ));
    LV::store(&out[i], x);
#endif
}

// The Fp2 arithmetic of the lane pairs on its own (diagnostic entry point vsp_selftest_fp2_lanes; the op tables are in include/vsp.h): a
// record of `in` holds the canonical operands a, b, c, d where a point has X, Y, ZZ, ZZZ, a record of `out` the results p, q, 0, 0, so
// both travel through LaneView as the points of k_selftest_xyzz_add do.  op < 0: element i runs op i mod K -- neighbouring pairs of a
// wave branch apart around the DPP exchanges, as the cases of xyzz_add make them.  form 0: Fp2L (field.h); 1: the 28-bit pair form
// (fp28.h) on tight canonical operands.
__global__ __launch_bounds__(64) void k_selftest_fp2_lanes(int form, int op, const XYZZ<Fp2> *in, XYZZ<Fp2> *out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    using LV = LaneView<Fp2>;
    const size_t i = gid<Fp2>();
    if (i >= n) return;                                           // both lanes of a pair leave together
    const XYZZ<Fp2L> v = LV::load(&in[i]);
    Fp2L a, b, c, d, p = Fp2L::zero(), q = Fp2L::zero();
    a.v = to_mont(v.X.v); b.v = to_mont(v.Y.v); c.v = to_mont(v.ZZ.v); d.v = to_mont(v.ZZZ.v);
    bool flag = false, answer = false;
    if (form == 0) {
        switch (op < 0 ? (int)(i % 10) : op) {
            case 0: p = mul(a, b); break;
            case 1: p = sqr(a); break;
            case 2: mul_pair(a, b, c, d, p, q); break;
            case 3: p = prod_diff(a, b, c, d); break;
            case 4: p = mul_add2(a, b, c, d); break;
            case 5: flag = true; answer = is_zero(a); break;
            case 6: p = add(a, b); break;
            case 7: p = sub(a, b); break;
            case 8: p = neg(a); break;
            default: p = dbl(a); break;                           // op 9
        }
    } else {
        const Fp28 x = fp_to_fp28(a.v), y = fp_to_fp28(b.v);
        Fp28 r;
        switch (op < 0 ? (int)(i % 5) : op) {
            case 0: r = mulF2(x, y, FP28_K8_L1); break;
            case 1: r = mulF2(x, y, FP28_K64_L4); break;
            case 2: r = sqrF2(x, FP28_K8_L1); break;
            case 3: r = sqrF2(x, FP28_K32_L1); break;
            default: r = sqrF2(x, FP28_K64_L1); break;             // op 4
        }
        p.v = fp28_to_fp(r);
    }
    XYZZ<Fp2L> res;
    res.X.v = from_mont(p.v); res.Y.v = from_mont(q.v); res.ZZ = Fp2L::zero(); res.ZZZ = Fp2L::zero();
    if (flag) { res.X.v = Fp::zero(); res.X.v.l[0] = answer ? 1u : 0u; }      // each lane's own answer, not a field value
    LV::store(&out[i], res);
#endif
}

}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_selftest_tower(vsp_ctx *ctx, int level, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    if (!ctx) return VSP_ERR_ARG;
    const bool known = level == 2 ? (op >= 0 && op <= 13) : level == 6 ? ((op >= 0 && op <= 4) || op == 7 || op == 8) : level == 12 ? (op >= 0 && op <= 12) : false;
    if (!a || !b || !out || !known) return set_error(ctx, VSP_ERR_ARG, "selftest: bad argument");
    if (n == 0) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t esz = (size_t)level * sizeof(Fp);
    DevBuf da, db, dc;
    int rc = ensure(ctx, da, n * esz); if (rc == VSP_OK) rc = ensure(ctx, db, n * esz); if (rc == VSP_OK) rc = ensure(ctx, dc, n * esz);
    if (rc == VSP_OK) {
        hipMemcpyAsync(da.p, a, n * esz, hipMemcpyHostToDevice, ctx->stream);
        hipMemcpyAsync(db.p, b, n * esz, hipMemcpyHostToDevice, ctx->stream);
        rc = level == 12 && op == 12 ? decrypt_selftest_gt_pow(ctx, da.p, db.p, dc.p, n) : pairing_selftest_tower(ctx, level, op, da.p, db.p, dc.p, n);
        hipMemcpyAsync(out, dc.p, n * esz, hipMemcpyDeviceToHost, ctx->stream);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "selftest: kernel failed");
    }
    return rc;
}

int vsp_selftest_fp2_lanes(vsp_ctx *ctx, int form, int op, const uint64_t *a, const uint64_t *b, const uint64_t *c, const uint64_t *d, uint64_t *out_p, uint64_t *out_q,
                           size_t n) {
    if (!ctx) return VSP_ERR_ARG;
    if (!a || !b || !c || !d || !out_p || !out_q || (form != 0 && form != 1) || op < -1 || op > (form == 0 ? 9 : 4)) return set_error(ctx, VSP_ERR_ARG, "selftest: bad argument");
    if (n == 0) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    using P = XYZZ<Fp2>;
    constexpr size_t W = sizeof(Fp2) / sizeof(uint64_t);          // words of an operand: 12; a record is four of them
    std::vector<uint64_t> rec(n * 4 * W);
    for (size_t i = 0; i < n; i++) {
        const uint64_t *src[4] = {a + i * W, b + i * W, c + i * W, d + i * W};
        for (int k = 0; k < 4; k++) memcpy(&rec[(i * 4 + k) * W], src[k], W * sizeof(uint64_t));
    }
    DevBuf din, dout;
    int rc = ensure(ctx, din, n * sizeof(P)); if (rc == VSP_OK) rc = ensure(ctx, dout, n * sizeof(P));
    if (rc == VSP_OK) {
        hipMemcpyAsync(din.p, rec.data(), n * sizeof(P), hipMemcpyHostToDevice, ctx->stream);
        hipLaunchKernelGGL(k_selftest_fp2_lanes, dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, ctx->stream, form, op, (const P *)din.p, (P *)dout.p, n);
        hipMemcpyAsync(rec.data(), dout.p, n * sizeof(P), hipMemcpyDeviceToHost, ctx->stream);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "selftest: kernel failed");
    }
    if (rc == VSP_OK)
        for (size_t i = 0; i < n; i++) {
            memcpy(out_p + i * W, &rec[(i * 4) * W], W * sizeof(uint64_t));
            memcpy(out_q + i * W, &rec[(i * 4 + 1) * W], W * sizeof(uint64_t));
        }
    return rc;
}

int vsp_selftest_field(vsp_ctx *ctx, int field, int op, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    if (!ctx) return VSP_ERR_ARG;
    if (!a || !b || !out || (field != 0 && field != 1) || op < 0 || op > (field == 0 ? 12 : 9)) return set_error(ctx, VSP_ERR_ARG, "selftest: bad argument");
    VSP_HIP(hipSetDevice(ctx->device));
    size_t esz = field == 0 ? sizeof(Fp) : sizeof(Fr);
    DevBuf da, db, dc;
    int rc = ensure(ctx, da, n * esz); if (rc == VSP_OK) rc = ensure(ctx, db, n * esz); if (rc == VSP_OK) rc = ensure(ctx, dc, n * esz);
    if (rc == VSP_OK) {
        hipMemcpyAsync(da.p, a, n * esz, hipMemcpyHostToDevice, ctx->stream);
        hipMemcpyAsync(db.p, b, n * esz, hipMemcpyHostToDevice, ctx->stream);
        unsigned blocks = (unsigned)((n + 63) / 64);
        if (field == 0 && op > 5) hipLaunchKernelGGL(k_selftest_fp28, dim3(blocks), dim3(64), 0, ctx->stream, op, (const Fp *)da.p, (const Fp *)db.p, (Fp *)dc.p, n);
        else if (op > 5) hipLaunchKernelGGL(k_selftest_fr29, dim3(blocks), dim3(64), 0, ctx->stream, op, (const Fr *)da.p, (const Fr *)db.p, (Fr *)dc.p, n);
        else if (field == 0) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_selftest_field<Fp>), dim3(blocks), dim3(64), 0, ctx->stream, op, (const Fp *)da.p, (const Fp *)db.p, (Fp *)dc.p, n);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_selftest_field<Fr>), dim3(blocks), dim3(64), 0, ctx->stream, op, (const Fr *)da.p, (const Fr *)db.p, (Fr *)dc.p, n);
        hipMemcpyAsync(out, dc.p, n * esz, hipMemcpyDeviceToHost, ctx->stream);
        if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "selftest: kernel failed");
    }
    return rc;
}

int vsp_selftest_xyzz_add(vsp_ctx *ctx, int group, int form, const uint64_t *a, const uint64_t *b, uint64_t *out, size_t n) {
    if (!ctx) return VSP_ERR_ARG;
    if (!a || !b || !out || (group != 1 && group != 2) || (form != 0 && form != 1)) return set_error(ctx, VSP_ERR_ARG, "selftest: bad argument");
    VSP_HIP(hipSetDevice(ctx->device));
    return with_group(group, [&](auto g) {
        using G = decltype(g); using P = XYZZ<typename G::F>;
        const size_t esz = sizeof(P);
        DevBuf da, db, dc;
        int rc = ensure(ctx, da, n * esz); if (rc == VSP_OK) rc = ensure(ctx, db, n * esz); if (rc == VSP_OK) rc = ensure(ctx, dc, n * esz);
        if (rc == VSP_OK) {
            hipMemcpyAsync(da.p, a, n * esz, hipMemcpyHostToDevice, ctx->stream);
            hipMemcpyAsync(db.p, b, n * esz, hipMemcpyHostToDevice, ctx->stream);
            if constexpr (G::ID == 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_selftest_xyzz_add<Fp, Fp28>), dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, form, (const P *)da.p, (const P *)db.p, (P *)dc.p, n);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_selftest_xyzz_add<Fp2, Fp2x28>), dim3((unsigned)((2 * n + 63) / 64)), dim3(64), 0, ctx->stream, form, (const P *)da.p, (const P *)db.p, (P *)dc.p, n);
            hipMemcpyAsync(out, dc.p, n * esz, hipMemcpyDeviceToHost, ctx->stream);
            if (hipStreamSynchronize(ctx->stream) != hipSuccess || hipGetLastError() != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "selftest: kernel failed");
        }
        return rc;
    });
}

vsp_ctx *vsp_create(int device_ordinal) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device_ordinal < 0 || device_ordinal >= count) return nullptr;
    if (hipSetDevice(device_ordinal) != hipSuccess) return nullptr;
    vsp_ctx *ctx = new vsp_ctx();
    ctx->device = device_ordinal;
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return nullptr; }
    ctx->stream = ctx->own_stream;
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_aux, hipEventDisableTiming) != hipSuccess) { hipStreamDestroy(ctx->own_stream); delete ctx; return nullptr; }
    // The prover's two witness chains get their streams NOW, ahead of every work slot's: the runtime deals its hardware queues (4 per
    // priority unless GPU_MAX_HW_QUEUES says otherwise) to streams in creation order, and two chains that land on one queue run one after
    // the other (7.4 instead of 6.6 ms per proof in a process with a dozen streams).  Created first, they get a queue each whatever else
    // the process creates later -- the library does not depend on that environment variable.
    for (int k = 0; k < 2; k++) if (msm_make_slot_stream(ctx, &ctx->prove_streams[k]) != VSP_OK) ctx->prove_streams[k] = nullptr;
    ctx->err.clear();
    return ctx;
}

void vsp_destroy(vsp_ctx *ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->prove.active) msm_drain_slots(ctx);      // a proof launched and never finished: wait its kernels out before their buffers go
    hipStreamSynchronize(ctx->stream);
    hipDeviceSynchronize();                           // a multi-exponentiation launched and never finished, a record's copy on a caller's stream
    msm_free_slots(ctx);
    saver_ct_release(ctx);
    hipEventDestroy(ctx->ev0); hipEventDestroy(ctx->ev1); hipEventDestroy(ctx->ev_aux);
    for (hipStream_t ps : ctx->prove_streams) if (ps) hipStreamDestroy(ps);
    hipStreamDestroy(ctx->own_stream);
    delete ctx;                 // every buffer and timer goes with its owner
}

const char *vsp_last_error(vsp_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vsp_set_stream(vsp_ctx *ctx, void *hip_stream) {
    if (!ctx) return VSP_ERR_ARG;
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return VSP_OK;
}
int vsp_synchronize(vsp_ctx *ctx) {
    if (!ctx) return VSP_ERR_ARG;
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}
double vsp_get_stat(vsp_ctx *ctx, const char *name) {
    if (!ctx || !name) return 0.0;
    if (!strcmp(name, "saver_decrypt_run_steps")) return (double)DLOG_RUN_STEPS;          // constants of the giant search (csrc/gt_dlog.h)
    if (!strcmp(name, "saver_decrypt_block_lanes")) return (double)DLOG_BLOCK_LANES;
    if (!strcmp(name, "saver_decrypt_launch_lanes")) return (double)DLOG_LAUNCH_LANES;
    if (!strcmp(name, "device_allocations_live")) return (double)DevBuf::live().load();          // process-wide (csrc/common.h OwnedBuf)
    if (!strcmp(name, "pinned_allocations_live")) return (double)PinnedBuf::live().load();
    if (!strcmp(name, "runtime_hw_queues_env")) { const char *q = getenv("GPU_MAX_HW_QUEUES"); return q ? atof(q) : 0.0; }      // include/vsp.h "Runtime environment"
    auto it = ctx->stats.find(name);
    return it == ctx->stats.end() ? 0.0 : it->second;
}
void vsp_stats_reset(vsp_ctx *ctx) { if (ctx) ctx->stats.clear(); }
int vsp_diag_clock(vsp_ctx *ctx, int reset, double *ghz_out, double *waves_out) {
    if (!ctx) return VSP_ERR_ARG;
    VSP_HIP(hipSetDevice(ctx->device));
    return msm_diag_clock(ctx, reset, ghz_out, waves_out);
}
int vsp_diag_clock_ntt(vsp_ctx *ctx, int reset, double *ghz_out, double *waves_out) {
    if (!ctx) return VSP_ERR_ARG;
    VSP_HIP(hipSetDevice(ctx->device));
    return ntt_diag_clock(ctx, reset, ghz_out, waves_out);
}
// Every option the library reads (opt / record_verdict, common.h), documented in include/vsp.h.  vsp_set_option refuses any other name: a
// misspelt option would otherwise be stored, read by nothing, and leave its caller -- a test, most likely -- on the default path without a
// word.  tests/test_option_coverage_cpu.py holds this table against the reads in csrc, the header and the names the suite sets.
static const char *const KNOWN_OPTIONS[] = {
    "ballot_box_table_bits", "bases_check_curve", "bases_check_subgroup", "generate_precompute_window",
    "msm_accum28_asm", "msm_batch_tables", "msm_census_sync", "msm_debug_counts", "msm_dimbits", "msm_dimsum_dense", "msm_dimsum_lanes",
    "msm_dimsum_maxw", "msm_dimsum_prefetch", "msm_fold", "msm_fp28", "msm_fused_scans", "msm_fused_split", "msm_glv", "msm_scatter_rounds",
    "msm_slot_normal_priority", "msm_sort", "msm_split", "msm_wide_windows", "msm_window_bits",
    "ntt_fr29", "pairing_chunk", "pedersen_lanes",
    "prove_batch_share_plan", "prove_check_witness", "prove_fixed_base", "prove_h_first", "prove_host_threads", "prove_plan_first", "prove_witness_streams",
    "registry_fused_levels", "saver_ct_chunk", "saver_decrypt_baby_bits", "saver_decrypt_fp_bits", "saver_encrypt_gpu", "saver_rerandomize_chunk",
    "saver_rerandomize_w4", "saver_screen_chunk", "saver_screen_split", "saver_verify_group", "tally_chunk_points", "vote_cast_device",
    "witness_map_batched",
    // test hooks: the context's self-check of its hand-laid-out routines reports a mismatch it did not find
    "msm_fp28_selfcheck_fault", "ntt_fr29_selfcheck_fault",
};
int vsp_set_option(vsp_ctx *ctx, const char *name, long value) {
    if (!ctx || !name) return VSP_ERR_ARG;
    bool known = false;
    for (const char *k : KNOWN_OPTIONS) known = known || !strcmp(k, name);
    if (!known) return set_error(ctx, VSP_ERR_ARG, (std::string("set_option: unknown option \"") + name + "\"").c_str());
    ctx->opts[name] = value;
    return VSP_OK;
}

// ---- pairings and Groth16 verdicts (pairing.hip)
int vsp_multi_pairing_batch(vsp_ctx *ctx, const uint64_t *g1, const uint64_t *g2, size_t m, size_t n, uint8_t *gt_out, uint8_t *is_one_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!g1 || !g2) return set_error(ctx, VSP_ERR_ARG, "multi_pairing_batch: null argument");
    if (m == 0 || m > ((size_t)1 << 16)) return set_error(ctx, VSP_ERR_ARG, "multi_pairing_batch: m outside 1..2^16");
    return pairing_multi_batch(ctx, g1, g2, m, n, gt_out, is_one_out);
}
vsp_vk *vsp_vk_create(vsp_ctx *ctx, const uint64_t alpha_g1[12], const uint64_t beta_g2[24], const uint64_t gamma_g2[24], const uint64_t delta_g2[24],
                      const uint64_t *gamma_abc_g1, size_t n_abc) {
    if (!ctx) return nullptr;
    if (!alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1 || n_abc == 0) { set_error(ctx, VSP_ERR_ARG, "vk_create: null argument or n_abc = 0"); return nullptr; }
    return pairing_vk_create(ctx, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc);
}
int vsp_vk_alpha_beta(const vsp_vk *vk, uint8_t gt_out[576]) {
    if (!vk || !gt_out) return VSP_ERR_ARG;
    memcpy(gt_out, pairing_vk_alpha_beta(vk), 576);
    return VSP_OK;
}
void vsp_vk_free(vsp_ctx *ctx, vsp_vk *vk) { pairing_vk_free(ctx, vk); }
int vsp_groth16_verify_batch(vsp_ctx *ctx, const vsp_vk *vk, const uint64_t *inputs, const uint64_t *A, const uint64_t *B, const uint64_t *C, size_t n,
                             uint8_t *verdict_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!vk || !A || !B || !C || !verdict_out || (!inputs && pairing_vk_n_abc(vk) > 1)) return set_error(ctx, VSP_ERR_ARG, "groth16_verify_batch: null argument");
    return pairing_verify_batch(ctx, vk, inputs, A, B, C, n, verdict_out);
}

// ---- SAVER ballot verdicts (pairing.hip)
vsp_saver_verifier *vsp_saver_verifier_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_pk_words, const uint64_t alpha_g1[12], const uint64_t beta_g2[24],
                                              const uint64_t gamma_g2[24], const uint64_t delta_g2[24], const uint64_t *gamma_abc_g1, size_t n_abc) {
    if (!ctx) return nullptr;
    if (!saver_pk_words || !alpha_g1 || !beta_g2 || !gamma_g2 || !delta_g2 || !gamma_abc_g1) { set_error(ctx, VSP_ERR_ARG, "saver_verifier_create: null argument"); return nullptr; }
    if (msg_size == 0 || msg_size > 1022 || n_abc < msg_size + 1) { set_error(ctx, VSP_ERR_ARG, "saver_verifier_create: msg_size outside 1..1022 or n_abc < msg_size + 1"); return nullptr; }
    return saver_verifier_create(ctx, msg_size, saver_pk_words, alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1, n_abc);
}
void vsp_saver_verifier_free(vsp_ctx *ctx, vsp_saver_verifier *ver) { saver_verifier_free(ctx, ver); }
size_t vsp_saver_verifier_msg_size(const vsp_saver_verifier *ver) { return ver ? saver_verifier_msg_size(ver) : 0; }
int vsp_saver_verify_batch(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *inputs_rest, const uint64_t *A, const uint64_t *B,
                           const uint64_t *C, size_t n, uint8_t *verdict_out, uint8_t *reason_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ver || !ct || !A || !B || !C || !verdict_out || (!inputs_rest && saver_verifier_n_rest(ver) > 0)) return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch: null argument");
    return saver_verify_batch(ctx, ver, ct, inputs_rest, A, B, C, n, verdict_out, reason_out);
}
// the screened check (screen.hip)
int vsp_saver_verify_batch_screened(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *ct, const uint64_t *inputs_rest, const uint64_t *A, const uint64_t *B,
                                    const uint64_t *C, size_t n, const uint64_t *coeff, uint8_t *verdict_out, uint8_t *reason_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ver || !ct || !A || !B || !C || !coeff || !verdict_out || (!inputs_rest && saver_verifier_n_rest(ver) > 0))
        return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch_screened: null argument");
    for (size_t k = 0; k < n; k++)
        if (!(coeff[2 * k] | coeff[2 * k + 1])) return set_error(ctx, VSP_ERR_ARG, "saver_verify_batch_screened: a coefficient is zero");
    return saver_verify_batch_screened(ctx, ver, ct, inputs_rest, A, B, C, n, coeff, verdict_out, reason_out);
}

// ---- SAVER decryption and its verification (decrypt.hip)
vsp_saver_decryptor *vsp_saver_decryptor_create(vsp_ctx *ctx, size_t msg_size, const uint64_t *saver_vk_words, const uint64_t *gamma_abc_g1, uint64_t max_value) {
    if (!ctx) return nullptr;
    if (!saver_vk_words || !gamma_abc_g1) { set_error(ctx, VSP_ERR_ARG, "saver_decryptor_create: null argument"); return nullptr; }
    if (msg_size == 0 || msg_size > 1022) { set_error(ctx, VSP_ERR_ARG, "saver_decryptor_create: msg_size outside 1..1022"); return nullptr; }
    return saver_decryptor_create(ctx, msg_size, saver_vk_words, gamma_abc_g1, max_value);
}
void vsp_saver_decryptor_free(vsp_ctx *ctx, vsp_saver_decryptor *dec) { saver_decryptor_free(ctx, dec); }
size_t vsp_saver_decryptor_msg_size(const vsp_saver_decryptor *dec) { return dec ? saver_decryptor_msg_size(dec) : 0; }
uint64_t vsp_saver_decryptor_max_value(const vsp_saver_decryptor *dec) { return dec ? saver_decryptor_max_value(dec) : 0; }
unsigned vsp_saver_decryptor_baby_bits(const vsp_saver_decryptor *dec) { return dec ? saver_decryptor_baby_bits(dec) : 0; }
int vsp_saver_decryptor_base(const vsp_saver_decryptor *dec, size_t slot, uint8_t gt_out[576]) {
    const uint8_t *b = dec && gt_out ? saver_decryptor_base(dec, slot) : nullptr;
    if (!b) return VSP_ERR_ARG;
    memcpy(gt_out, b, 576);
    return VSP_OK;
}
int vsp_saver_decrypt_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t rho[4], const uint64_t *ct, size_t count, uint64_t *msgs_out, uint64_t *nu_out,
                            uint8_t *status_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!dec || !rho || !ct || !msgs_out || !status_out) return set_error(ctx, VSP_ERR_ARG, "saver_decrypt_batch: null argument");
    return saver_decrypt_batch(ctx, dec, rho, ct, count, msgs_out, nu_out, status_out);
}
int vsp_saver_verify_decryption_batch(vsp_ctx *ctx, const vsp_saver_decryptor *dec, const uint64_t *ct, const uint64_t *msgs, const uint64_t *nu, size_t count,
                                      uint8_t *verdict_out, uint8_t *reason_out, uint32_t *first_bad_slot_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!dec || !ct || !msgs || !nu || !verdict_out) return set_error(ctx, VSP_ERR_ARG, "saver_verify_decryption_batch: null argument");
    return saver_verify_decryption_batch(ctx, dec, ct, msgs, nu, count, verdict_out, reason_out, first_bad_slot_out);
}

void *vsp_dmalloc(vsp_ctx *ctx, size_t bytes) {
    if (!ctx) return nullptr;
    hipSetDevice(ctx->device);
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { set_error(ctx, VSP_ERR_NOMEM, "vsp_dmalloc: hipMalloc failed"); return nullptr; }
    return p;
}
void vsp_dfree(vsp_ctx *ctx, void *dptr) { if (ctx && dptr) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); hipFree(dptr); } }
int vsp_h2d(vsp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes) {
    if (!ctx || (!dst_dev && bytes) || (!src_host && bytes)) return VSP_ERR_ARG;
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_HIP(hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}
int vsp_d2h(vsp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes) {
    if (!ctx || (!dst_host && bytes) || (!src_dev && bytes)) return VSP_ERR_ARG;
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_HIP(hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}

// page-lock caller memory (a witness vector, say) so that the copies vsp_groth16_prove / vsp_h2d queue from it are asynchronous DMA
// instead of the runtime's staged pageable path
int vsp_host_register(vsp_ctx *ctx, void *ptr, size_t bytes) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ptr || !bytes) return set_error(ctx, VSP_ERR_ARG, "host_register: null pointer or zero size");
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_HIP(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return VSP_OK;
}
int vsp_host_unregister(vsp_ctx *ctx, void *ptr) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ptr) return set_error(ctx, VSP_ERR_ARG, "host_unregister: null pointer");
    VSP_HIP(hipHostUnregister(ptr));
    return VSP_OK;
}

// ---- MSM ----------------------------------------------------------------------------------------
}  // extern "C"
// vsp_msm_launch on slot 0 (its argument checks), its finish, then done(result) with the result in the group's host form
template <class Fn> static int msm_resident_then(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars, Fn &&done) {
    VSP_TRY(vsp_msm_launch(ctx, 0, bases, first, n, d_scalars));
    return with_group(bases->group, [&](auto g) {
        XYZZ<typename decltype(g)::HF> a;
        VSP_TRY(msm_slot_finish<decltype(g)>(ctx, 0, &a));
        return done(a);
    });
}

extern "C" {

int vsp_msm_resident(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars, uint64_t *out_affine, int *out_is_inf) {
    return msm_resident_then(ctx, bases, first, n, d_scalars, [&](const auto &a) { return finish_affine(a, out_affine, out_is_inf); });
}

int vsp_msm_resident_batch(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars, size_t batch, size_t stride,
                           uint64_t *out_affine, int *out_is_inf) {
    if (!ctx) return VSP_ERR_ARG;
    if (!bases || (!d_scalars && n) || !out_affine || batch < 1 || batch > 64 || (batch > 1 && stride < n)) return set_error(ctx, VSP_ERR_ARG, "msm: bad batch argument");
    if (first > bases->n || n > bases->n - first) return set_error(ctx, VSP_ERR_ARG, "msm: range outside the resident bases");
    VSP_HIP(hipSetDevice(ctx->device));
    MsmRequest rq((const Fr *)d_scalars, n); rq.batch = (unsigned)batch; rq.stride = stride;
    VSP_TRY(launch_on_bases(ctx, 0, bases, first, rq));
    return with_group(bases->group, [&](auto g) -> int {
        using G = decltype(g);
        std::vector<XYZZ<typename G::HF>> r(batch);
        VSP_TRY(msm_slot_finish<G>(ctx, 0, r.data(), (unsigned)batch));
        for (size_t k = 0; k < batch; k++) VSP_TRY(finish_affine(r[k], out_affine + k * G::AFFINE_WORDS, out_is_inf ? out_is_inf + k : nullptr));
        return VSP_OK;
    });
}

int vsp_msm_resident_jacobian(vsp_ctx *ctx, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars, uint64_t *out_jacobian) {
    if (!out_jacobian) return set_error(ctx, VSP_ERR_ARG, "msm: null output");
    return msm_resident_then(ctx, bases, first, n, d_scalars, [&](const auto &a) -> int { host_store_jacobian(out_jacobian, xyzz_to_jacobian(a)); return VSP_OK; });
}

// ---- pipelined form: up to VSP_MSM_SLOTS multi-exponentiations in flight, each on its own stream ----
int vsp_msm_launch(vsp_ctx *ctx, unsigned slot, const vsp_bases *bases, size_t first, size_t n, const void *d_scalars) {
    if (!ctx) return VSP_ERR_ARG;
    if (!bases || (!d_scalars && n)) return set_error(ctx, VSP_ERR_ARG, "msm: null argument");
    if (first > bases->n || n > bases->n - first) return set_error(ctx, VSP_ERR_ARG, "msm: range outside the resident bases");
    VSP_HIP(hipSetDevice(ctx->device));
    return launch_on_bases(ctx, slot, bases, first, MsmRequest((const Fr *)d_scalars, n));
}
// the Jacobian record of a finished slot (18 / 36 canonical words); returns the words written
static int finish_record(vsp_ctx *ctx, unsigned slot, uint64_t *out_jacobian, size_t *words) {
    return with_group(ctx->slot_group[slot], [&](auto g) -> int {
        using G = decltype(g);
        XYZZ<typename G::HF> a; VSP_TRY(msm_slot_finish<G>(ctx, slot, &a));
        host_store_jacobian(out_jacobian, xyzz_to_jacobian(a));
        *words = G::JACOBIAN_WORDS;
        return VSP_OK;
    });
}
int vsp_msm_finish_jacobian(vsp_ctx *ctx, unsigned slot, uint64_t *out_jacobian) {
    if (!ctx) return VSP_ERR_ARG;
    if (slot >= VSP_MSM_SLOTS || !out_jacobian) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot or null output");
    size_t words = 0;
    return finish_record(ctx, slot, out_jacobian, &words);
}
// The exchange step of the sharded multi-exponentiation wants the record in DEVICE memory (the RCCL all-gather reads it there).  The
// last step of a multi-exponentiation is a chain of c * W dependent doublings, which the host runs ~50x faster than a GPU lane
// (DESIGN.md 3.4), so the record is born on the host: it is written into a pinned ring entry of the slot and copied to d_out_jacobian
// by an asynchronous DMA queued on hip_stream (NULL = the context's stream) -- the caller's host thread never waits for the copy, and
// work queued on hip_stream afterwards (the all-gather) sees the record.
int vsp_msm_finish_jacobian_device(vsp_ctx *ctx, unsigned slot, void *d_out_jacobian, void *hip_stream) {
    if (!ctx) return VSP_ERR_ARG;
    if (slot >= VSP_MSM_SLOTS || !d_out_jacobian) return set_error(ctx, VSP_ERR_ARG, "msm: bad slot or null output");
    VSP_HIP(hipSetDevice(ctx->device));
    MsmWork &wk = ctx->msm_work[slot];
    if (!wk.inited || !wk.h_rec.p) return set_error(ctx, VSP_ERR_ARG, "msm: finish without launch");
    const unsigned k = wk.rec_idx++ % MsmWork::REC_RING;
    VSP_HIP(hipEventSynchronize(wk.rec_ev[k]));                 // the copy that last read this ring entry (long done in practice; never-recorded events return at once)
    uint64_t *rec = (uint64_t *)(wk.h_rec.as<char>() + (size_t)k * 288);
    size_t words = 0;
    VSP_TRY(finish_record(ctx, slot, rec, &words));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    VSP_HIP(hipMemcpyAsync(d_out_jacobian, rec, words * 8, hipMemcpyHostToDevice, st));
    VSP_HIP(hipEventRecord(wk.rec_ev[k], st));
    return VSP_OK;
}

int vsp_fold_jacobian(vsp_ctx *ctx, int group, const uint64_t *records, size_t count, uint64_t *out_affine, int *out_is_inf) {
    if (!records && count) return set_error(ctx, VSP_ERR_ARG, "fold: null records");
    if (group != 1 && group != 2) return set_error(ctx, VSP_ERR_ARG, "fold: group must be 1 or 2");
    return with_group(group, [&](auto g) {
        using G = decltype(g); using HF = typename G::HF;
        XYZZ<HF> acc = XYZZ<HF>::inf();
        for (size_t i = 0; i < count; i++) xyzz_add(acc, jacobian_to_xyzz(host_load_jacobian<HF>(records + G::JACOBIAN_WORDS * i)));
        return finish_affine(acc, out_affine, out_is_inf);
    });
}

// Fold records that sit in DEVICE memory (the output of the all-gather): one asynchronous copy of count * 144 / 288 bytes into a pinned
// buffer on hip_stream (NULL = the context's stream) -- behind whatever produced the records on that stream --, a wait for that stream,
// then the host fold.  The result is wanted on the host (the prover's caller assembles the proof there).
int vsp_fold_jacobian_device(vsp_ctx *ctx, int group, const void *d_records, size_t count, void *hip_stream, uint64_t *out_affine, int *out_is_inf) {
    if (!ctx) return VSP_ERR_ARG;
    if (group != 1 && group != 2) return set_error(ctx, VSP_ERR_ARG, "fold: group must be 1 or 2");
    if (!d_records && count) return set_error(ctx, VSP_ERR_ARG, "fold: null records");
    if (count > 4096) return set_error(ctx, VSP_ERR_ARG, "fold: more than 4096 records");
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t bytes = count * 8 * with_group(group, [](auto g) { return decltype(g)::JACOBIAN_WORDS; });
    VSP_TRY(ensure_pinned(ctx, ctx->h_fold, bytes));
    hipStream_t st = hip_stream ? (hipStream_t)hip_stream : ctx->stream;
    if (bytes) {
        VSP_HIP(hipMemcpyAsync(ctx->h_fold.p, d_records, bytes, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
    }
    return vsp_fold_jacobian(ctx, group, ctx->h_fold.as<const uint64_t>(), count, out_affine, out_is_inf);
}

static int msm_host(vsp_ctx *ctx, int group, const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t *out_affine, int *out_is_inf) {
    if (!ctx) return VSP_ERR_ARG;
    if ((!bases || !scalars) && n) return set_error(ctx, VSP_ERR_ARG, "msm: null argument");
    VSP_HIP(hipSetDevice(ctx->device));
    vsp_bases *b = nullptr;
    VSP_TRY(bases_create(ctx, group, bases, false, n, BASES_TRANSIENT, &b));      // one call's bases: no endomorphism split, hence no subgroup check
    int rc = ensure(ctx, ctx->msm_scalars, n * 32);
    if (rc == VSP_OK && n) {
        if (hipMemcpyAsync(ctx->msm_scalars.p, scalars, n * 32, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = set_error(ctx, VSP_ERR_HIP, "msm: H2D of scalars failed");
    }
    if (rc == VSP_OK) rc = vsp_msm_resident(ctx, b, 0, n, ctx->msm_scalars.p, out_affine, out_is_inf);
    vsp_bases_free(ctx, b);
    return rc;
}
int vsp_msm_g1(vsp_ctx *ctx, const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_affine[12], int *out_is_inf) {
    return msm_host(ctx, 1, bases, scalars, n, out_affine, out_is_inf);
}
int vsp_msm_g2(vsp_ctx *ctx, const uint64_t *bases, const uint64_t *scalars, size_t n, uint64_t out_affine[24], int *out_is_inf) {
    return msm_host(ctx, 2, bases, scalars, n, out_affine, out_is_inf);
}

// ---- NTT / witness_map ------------------------------------------------------------------------
}  // extern "C"
// the host-buffer form of a routine on the device: on the context's device, m canonical values in through its workspace pr_h (none when
// `in` is null), run(pr_h), the m values there out to `out`, synchronised
template <class Run> static int through_pr_h(vsp_ctx *ctx, const uint64_t *in, uint64_t *out, size_t m, Run &&run) {
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t bytes = m * 32;
    VSP_TRY(ensure(ctx, ctx->pr_h, bytes));
    if (in) VSP_HIP(hipMemcpyAsync(ctx->pr_h.p, in, bytes, hipMemcpyHostToDevice, ctx->stream));
    VSP_TRY(run((Fr *)ctx->pr_h.p));
    VSP_HIP(hipMemcpyAsync(out, ctx->pr_h.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}
// A z, B z, C z in through the prover's workspace of one witness (pr_abc), H out through pr_h
static int witness_map_host(vsp_ctx *ctx, const vsp_domain *d, const uint64_t *Az, const uint64_t *Bz, const uint64_t *Cz, uint64_t *H) {
    return through_pr_h(ctx, nullptr, H, d->m, [&](Fr *dH) {
        const size_t m = d->m;
        VSP_TRY(ensure(ctx, ctx->pr_abc, 3 * m * 32));
        Fr *dA = (Fr *)ctx->pr_abc.p;
        const uint64_t *src[3] = {Az, Bz, Cz};
        for (int k = 0; k < 3; k++) VSP_HIP(hipMemcpyAsync(dA + k * m, src[k], m * 32, hipMemcpyHostToDevice, ctx->stream));
        return witness_map_device(ctx, d, dA, dA + m, dA + 2 * m, 3 * m, 1, dH, m);
    });
}
extern "C" {
int vsp_ntt_fr_device(vsp_ctx *ctx, void *d_a, unsigned log_m, int inverse, const uint64_t coset_g[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d_a) return set_error(ctx, VSP_ERR_ARG, "ntt: null pointer");
    VSP_HIP(hipSetDevice(ctx->device));
    return ntt_launch(ctx, NttRequest((Fr *)d_a, log_m, inverse, coset_g));
}
int vsp_ntt_fr(vsp_ctx *ctx, uint64_t *a, unsigned log_m, int inverse, const uint64_t coset_g[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!a) return set_error(ctx, VSP_ERR_ARG, "ntt: null pointer");
    if (log_m > 28) return set_error(ctx, VSP_ERR_UNSUPPORTED, "ntt: log_m > 28");
    return through_pr_h(ctx, a, a, (size_t)1 << log_m, [&](Fr *d_a) { return ntt_launch(ctx, NttRequest(d_a, log_m, inverse, coset_g)); });
}
int vsp_witness_map_h_device(vsp_ctx *ctx, void *d_Az, void *d_Bz, void *d_Cz, unsigned log_m, void *d_H) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d_Az || !d_Bz || !d_Cz || !d_H) return set_error(ctx, VSP_ERR_ARG, "witness_map: null pointer");
    if (log_m > 28) return set_error(ctx, VSP_ERR_UNSUPPORTED, "witness_map: log_m > 28");
    VSP_HIP(hipSetDevice(ctx->device));
    vsp_domain d; domain_basic(&d, log_m);
    return witness_map_device(ctx, &d, (Fr *)d_Az, (Fr *)d_Bz, (Fr *)d_Cz, 0, 1, (Fr *)d_H, 0);
}
int vsp_witness_map_h(vsp_ctx *ctx, uint64_t *Az, uint64_t *Bz, uint64_t *Cz, unsigned log_m, uint64_t *H) {
    if (!ctx) return VSP_ERR_ARG;
    if (!Az || !Bz || !Cz || !H) return set_error(ctx, VSP_ERR_ARG, "witness_map: null pointer");
    if (log_m > 28) return set_error(ctx, VSP_ERR_UNSUPPORTED, "witness_map: log_m > 28");
    vsp_domain d; domain_basic(&d, log_m);
    return witness_map_host(ctx, &d, Az, Bz, Cz, H);
}

// ---- evaluation_domain<Fr> handles: make_evaluation_domain, basic and step radix-2 ---------------------------------
vsp_domain *vsp_domain_create(vsp_ctx *ctx, size_t min_size) {
    if (!ctx) return nullptr;
    hipSetDevice(ctx->device);
    vsp_domain *d = new vsp_domain();
    if (domain_init(ctx, d, min_size) != VSP_OK) { delete d; return nullptr; }
    return d;
}
void vsp_domain_free(vsp_ctx *ctx, vsp_domain *d) {
    if (!d) return;
    if (ctx) hipSetDevice(ctx->device);
    delete d;
}
size_t vsp_domain_size(const vsp_domain *d) { return d ? d->m : 0; }
int vsp_domain_kind(const vsp_domain *d) { return d ? d->step : -1; }
int vsp_domain_fft_device(vsp_ctx *ctx, const vsp_domain *d, void *d_a, int inverse, const uint64_t coset_g[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !d_a) return set_error(ctx, VSP_ERR_ARG, "domain_fft: null pointer");
    VSP_HIP(hipSetDevice(ctx->device));
    return domain_fft_device(ctx, d, (Fr *)d_a, inverse, coset_g, nullptr);
}
int vsp_domain_fft(vsp_ctx *ctx, const vsp_domain *d, uint64_t *a, int inverse, const uint64_t coset_g[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !a) return set_error(ctx, VSP_ERR_ARG, "domain_fft: null pointer");
    return through_pr_h(ctx, a, a, d->m, [&](Fr *d_a) { return domain_fft_device(ctx, d, d_a, inverse, coset_g, nullptr); });
}
int vsp_domain_lagrange(vsp_ctx *ctx, const vsp_domain *d, const uint64_t t[4], uint64_t *out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !t || !out) return set_error(ctx, VSP_ERR_ARG, "domain_lagrange: null pointer");
    return through_pr_h(ctx, nullptr, out, d->m, [&](Fr *u) {
        VSP_TRY(domain_lagrange_device(ctx, d, host_load_canon<HFr>(t), u));
        return fr_from_mont_device(ctx, u, d->m);
    });
}
int vsp_domain_element(vsp_ctx *ctx, const vsp_domain *d, size_t idx, uint64_t out[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !out || idx >= d->m) return set_error(ctx, VSP_ERR_ARG, "domain_element: bad argument");
    host_store_canon(out, domain_element(d, idx));
    return VSP_OK;
}
int vsp_domain_vanishing(vsp_ctx *ctx, const vsp_domain *d, const uint64_t t[4], uint64_t out[4]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !t || !out) return set_error(ctx, VSP_ERR_ARG, "domain_vanishing: null pointer");
    host_store_canon(out, domain_vanishing(d, host_load_canon<HFr>(t)));
    return VSP_OK;
}
// H (m + 1 coefficients, host, canonical) += coeff * Z
int vsp_domain_add_poly_z(vsp_ctx *ctx, const vsp_domain *d, const uint64_t coeff[4], uint64_t *H) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !coeff || !H) return set_error(ctx, VSP_ERR_ARG, "domain_add_poly_z: null pointer");
    HFr c = host_load_canon<HFr>(coeff);
    auto upd = [&](size_t i, const HFr &delta) { HFr v = host_load_canon<HFr>(H + 4 * i); host_store_canon(H + 4 * i, add(v, delta)); };
    if (!d->step) { upd(d->m, c); upd(0, neg(c)); return VSP_OK; }
    uint64_t e[1] = {(uint64_t)d->small_m};
    HFr cw = mul(c, pow_limbs(host_omega(d->log_big + 1), e, 1));
    upd(d->m, c); upd(d->big_m, neg(cw)); upd(d->small_m, neg(c)); upd(0, cw);
    return VSP_OK;
}
int vsp_domain_divide_by_z_on_coset(vsp_ctx *ctx, const vsp_domain *d, uint64_t *P) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !P) return set_error(ctx, VSP_ERR_ARG, "domain_divide_by_z_on_coset: null pointer");
    return through_pr_h(ctx, P, P, d->m, [&](Fr *p) { return domain_divide_by_z_device(ctx, d, p); });
}
int vsp_domain_witness_map_h(vsp_ctx *ctx, const vsp_domain *d, uint64_t *Az, uint64_t *Bz, uint64_t *Cz, uint64_t *H) {
    if (!ctx) return VSP_ERR_ARG;
    if (!d || !Az || !Bz || !Cz || !H) return set_error(ctx, VSP_ERR_ARG, "witness_map: null pointer");
    return witness_map_host(ctx, d, Az, Bz, Cz, H);
}
size_t vsp_r1cs_domain_size(const vsp_r1cs *cs) { return cs ? cs->dom.m : 0; }
int vsp_r1cs_domain_kind(const vsp_r1cs *cs) { return cs ? cs->dom.step : -1; }

// ---- generator-side batch exponentiation ---------------------------------------------------------
}  // extern "C"
template <class G> static int fixed_base_mul_sync(vsp_ctx *ctx, const void *d_scalars, size_t n, void *d_out) {
    if (!ctx) return VSP_ERR_ARG;
    if ((!d_scalars || !d_out) && n) return set_error(ctx, VSP_ERR_ARG, "fixed_base_mul: null pointer");
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_TRY(fixed_base_mul<G>(ctx, (const Fr *)d_scalars, n, d_out));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}
extern "C" {
int vsp_fixed_base_mul_g1(vsp_ctx *ctx, const void *d_scalars, size_t n, void *d_out) { return fixed_base_mul_sync<G1>(ctx, d_scalars, n, d_out); }
int vsp_fixed_base_mul_g2(vsp_ctx *ctx, const void *d_scalars, size_t n, void *d_out) { return fixed_base_mul_sync<G2>(ctx, d_scalars, n, d_out); }

}  // extern "C"
