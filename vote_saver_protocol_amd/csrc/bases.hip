// Resident bases (vsp_bases, include/vsp.h): upload and validation, the subgroup check, tables of window multiples, the same points on
// 28-bit limbs with the known-answer check that guards them, and the launch of a multi-exponentiation over resident bases.
#include <memory>

#include "common.h"
#include "fp28.h"

namespace vsp {

// bytes of one row of a group's 28-bit-limb table
static size_t row28_bytes(int group) { return with_group(group, [](auto g) { return sizeof(typename decltype(g)::Row28); }); }
// The 28-bit table of b with the endomorphism rows (glv) or without: its row count, and the row at which point `first` starts (in window 0).
// Plain bases: n points, two rows each with glv.  Window multiples: 255 / pre_c + 1 windows of n rows, or -- the split over window
// multiples (pre_split) -- ceil(128 / pre_c) windows of 2n rows.
struct Rows28 { size_t count, first; };
static Rows28 table28_rows(const vsp_bases *b, bool glv, size_t first = 0) {
    const size_t per = glv ? 2 : 1, windows = !b->pre_c ? 1 : glv ? (128 + b->pre_c - 1) / b->pre_c : 255 / b->pre_c + 1;
    return {b->n * windows * per, first * per};
}

// Known-answer check of the hand-laid-out field routines THROUGH the kernels that use them (their products are entered with a private
// calling convention the compiler's hazard recogniser and register allocator cannot see into; field-level selftests run them in another
// code arrangement).  Once per context and group, before the first 28-bit table is used, over points the LIBRARY generates (4096
// multiples of the generator: in the subgroup by construction, independent of whatever the caller uploads): the same multi-exponentiation
//   (a) through k_accum28 over the endomorphism layout, the 28-bit merges (k_merge_a, k_merge2: its scalars hold zeros and ones, so one
//       bucket is split in tens of parts), k_dimsum and k_dimbits / k_dimweight -- the default plan;
//   (b) the same with short bucket parts forced (split 6: every bucket is cut in several parts, the merges' full additions run
//       thousands of times) and the other last step of the bucket reduction;
//   (c) through the generic 12 x 32-bit kernels, no split;
//   (d), (e) the default plan again with 6-bit and with 12-bit windows: other digit splits (q0, q1) of the bucket reduction, other lane counts
//       per sum in k_dimsum_mixed, and -- the last 512 points being ONE point under 512 different scalars -- bucket sums that coincide all
//       over the reduction: the doubling branch of the full addition inside k_dimsum(_mixed), k_dimbits and the merges (round 4).
// All five affine results must be identical.  On a mismatch the 28-bit kernels are switched off for this context ("msm_fp28" = 0:
// every later multi-exponentiation takes the generic kernels).  Returns true when 28-bit tables may be used.
template <class G> static bool fp28_known_answer_check(vsp_ctx *ctx) {
    using HF = typename G::HF;
    const int gi = G::ID - 1;
    if (ctx->fp28_checked[gi] != 0) return ctx->fp28_checked[gi] > 0;
    if (ctx->msm_work[0].active) return true;                 // slot 0 busy (unusual): check at the next table instead
    const size_t n = 4096;
    std::vector<uint64_t> sc(2 * n * 4);                      // [0, n): the multiples that make the points; [n, 2n): the scalars of the check
    SplitMix64 next{0x9E3779B97F4A7C15ULL ^ (uint64_t)G::ID};
    for (size_t i = 0; i < 2 * n; i++) {
        sc[4 * i] = next(); sc[4 * i + 1] = next(); sc[4 * i + 2] = next(); sc[4 * i + 3] = next() >> 2;     // < 2^254 < r
        if (i >= n && i % 7 == 3) { sc[4 * i] &= 1; sc[4 * i + 1] = sc[4 * i + 2] = sc[4 * i + 3] = 0; }     // zeros and ones among the check's scalars
    }
    // equal points and opposite points under equal scalars: the same bucket meets P + P (the doubling path of every addition routine, the
    // equal-x hand-back of the accumulation kernel) and P - P (the infinity paths) in all three pipelines
    for (size_t i = 1; i < n; i++) {
        if (i % 16 == 5) for (int j = 0; j < 4; j++) sc[4 * i + j] = sc[4 * (i - 1) + j];                    // the same point twice
        else if (i % 16 == 9) {                                                                             // a point and its negative: r - k
            unsigned __int128 borrow = 0;
            for (int j = 0; j < 4; j++) {
                const unsigned __int128 d = (unsigned __int128)FrP64::MOD[j] - sc[4 * (i - 1) + j] - borrow;
                sc[4 * i + j] = (uint64_t)d; borrow = (d >> 64) & 1;
            }
        } else continue;
        for (int j = 0; j < 4; j++) sc[4 * (n + i) + j] = sc[4 * (n + i - 1) + j];                           // ... under the same scalar
    }
    for (size_t i = n - 511; i < n; i++) for (int j = 0; j < 4; j++) sc[4 * i + j] = sc[4 * (n - 512) + j];  // one point 512 times, scalars as drawn
    const size_t esz = sizeof(typename G::Point), row = sizeof(typename G::Row28);
    const std::string sfx = "_g" + std::to_string(G::ID);        // of the stat names
    DevBuf pts, tab28;
    bool same = false, ran = false;
    if (ensure(ctx, ctx->msm_scalars, 2 * n * 32) == VSP_OK && ensure(ctx, ctx->val_flag, 16) == VSP_OK &&
        hipMemcpyAsync(ctx->msm_scalars.p, sc.data(), 2 * n * 32, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
        hipStreamSynchronize(ctx->stream) == hipSuccess && pts.alloc(n * esz) == hipSuccess && tab28.alloc(2 * n * row) == hipSuccess) {
        void *d_pts = pts.p, *t28 = tab28.p;
        const Fr *dk = (const Fr *)ctx->msm_scalars.p, *ds = dk + n;
        int rc = fixed_base_mul<G>(ctx, dk, n, d_pts);
        if (rc == VSP_OK) rc = bases_to_mont<G>(ctx, d_pts, (typename G::Point *)d_pts, n, 0, (uint32_t *)ctx->val_flag.p);
        if (rc == VSP_OK) rc = msm_table28<G>(ctx, (const typename G::Point *)d_pts, n, t28, true);
        if (rc == VSP_OK && hipStreamSynchronize(ctx->stream) == hipSuccess) {
            ran = true;
            // legs (a) .. (e): the 28-bit table or not, the tuning each pins (no caller's option reaches them), and the detail bit (stat
            // "msm_fp28_selfcheck_detail_g1/2") of a result other than (c)'s -- for (c): infinity where there should be none; 8 = a launch failed
            struct Leg { bool t28; MsmTuning tune; unsigned bit; };
            const Leg legs[5] = {{true, {0, 0, -1}, 1}, {true, {0, 6, G::ID == 1 ? 0 : 1}, 2}, {false, {0, 0, -1}, 4}, {true, {6, 0, -1}, 16}, {true, {12, 0, -1}, 32}};
            const int ref = 2;
            uint64_t aff[5][24] = {}; int inf[5] = {};
            bool okr = true;
            for (int k = 0; k < 5 && okr; k++) {
                MsmRequest rq(ds, n); rq.bases = d_pts; rq.dense = true; rq.table28 = legs[k].t28 ? t28 : nullptr; rq.glv = legs[k].t28; rq.tuning = &legs[k].tune;
                XYZZ<HF> r;
                okr = msm_slot_launch<G>(ctx, 0, rq) == VSP_OK && msm_slot_finish<G>(ctx, 0, &r) == VSP_OK;
                if (okr) { host_store_affine(aff[k], xyzz_to_affine(r)); inf[k] = is_inf(r); }
            }
            unsigned detail = okr ? 0 : 8;
            for (int k = 0; k < 5; k++)
                if (k == ref ? inf[k] != 0 : (inf[k] != inf[ref] || memcmp(aff[k], aff[ref], sizeof aff[k]) != 0)) detail |= legs[k].bit;
            ctx->stats["msm_fp28_selfcheck_detail" + sfx] = detail;
            same = detail == 0;
        }
    }
    hipGetLastError();
    if (!ran) { ctx->stats["msm_fp28_selfcheck" + sfx] = 0.0; return false; }      // could not run (out of memory): no verdict, no 28-bit table this time
    return record_verdict(ctx, ctx->fp28_checked[gi], same, "msm_fp28_selfcheck_fault", "msm_fp28_selfcheck" + sfx, "msm_fp28",
                          "msm: the 28-bit-limb kernels failed their known-answer check; generic kernels in use");
}
// the points once more on 14 x 28-bit limbs for the accumulation kernel (fp28.h); option "msm_fp28" = 0 switches it off.
// Plain bases (no window multiples) whose points are known to satisfy phi(P) = lambda P (vsp_bases.in_subgroup) get the endomorphism
// layout: 2 count rows, (P_i, phi(P_i)) interleaved (option "msm_glv" = 0: off; 2: on for any size and WITHOUT the check -- the caller vouches)
static bool glv_wanted(vsp_ctx *ctx, int group, size_t count, unsigned pre_c) {
    const long want = opt(ctx, "msm_fp28", 1), want_glv = opt(ctx, "msm_glv", 1);
    const size_t row = row28_bytes(group);
    // The split halves the bucket sets (and the host Horner chain) but doubles the table and the sort's input.  Measured
    // (tools/msm_sizes.py, bench.py; one in flight / three in flight, ms): G1 2^16 1.49 / 1.42 -> 1.35 / 0.80, G1 2^18 2.31 / 1.29 ->
    // 2.04 / 1.27, G1 2^20 4.24 / 3.35 -> 3.98 / 3.34, a 2^20-constraint proof 8.71 -> 8.45 ms (plain key: 9.98 -> 8.95);
    // G2 2^16 3.01 / 1.58 -> 2.67 / 1.40, G2 2^18 5.21 / 3.21 -> 5.56 / 2.90, G2 2^19 7.23 / 4.82 -> 8.28 / 5.58 (dense scalars:
    // the lane-pair merges of the split buckets cost more than the windows saved).  So: on while the doubled table is at most
    // 256 MB for G1 (2^20 points) and 128 MB for G2 (2^18 points); "msm_glv" = 2 forces it on, 0 switches it off.
    const size_t glv_limit = ((size_t)256 << 20) / group;      // 256 MB (G1), 128 MB (G2)
    return want && want_glv && pre_c == 0 && count >= 1024 && count < ((size_t)1 << 30) && (want_glv >= 2 || 2 * count * row <= glv_limit);
}
static void build_table28(vsp_ctx *ctx, vsp_bases *b) {
    b->d28.reset();
    b->glv = false;
    const long want = opt(ctx, "msm_fp28", 1), want_glv = opt(ctx, "msm_glv", 1);
    // "msm_fp28" = 2 (diagnostics: bisecting a failed check with tools/fuzz_msm.py): the 28-bit kernels WITHOUT the context-time check
    if (!want || (want < 2 && !with_group(b->group, [&](auto g) { return fp28_known_answer_check<decltype(g)>(ctx); }))) return;   // the check may have just switched "msm_fp28" off
    // window multiples for dense scalars (pre_split): the 128 / c windows of a split scalar, every row with its endomorphism image beside it
    const bool glv = (b->in_subgroup > 0 || want_glv >= 2) && (b->pre_c ? b->pre_split && want_glv : glv_wanted(ctx, b->group, b->n, 0));
    const size_t rows = table28_rows(b, glv).count;
    DevBuf t28;
    if (t28.alloc(rows * row28_bytes(b->group)) != hipSuccess) { hipGetLastError(); return; }
    int rc = with_group(b->group, [&](auto g) { using G = decltype(g); return msm_table28<G>(ctx, b->d.as<const typename G::Point>(), glv ? rows / 2 : rows, t28.p, glv); });
    if (rc == VSP_OK && hipStreamSynchronize(ctx->stream) == hipSuccess) { b->d28 = std::move(t28); b->glv = glv; }
    else hipGetLastError();
}
// the subgroup check of plain resident bases over the context's validation word, which the caller zeroed: queued, the word read back
// into *h_flag, and -- unless its bits 0 / 1 refuse the upload -- the verdict recorded (b->in_subgroup 1 or -1, the two stats)
static int bases_subgroup_check(vsp_ctx *ctx, vsp_bases *b, uint32_t *h_flag) {
    VSP_TRY(with_group(b->group, [&](auto g) { using G = decltype(g); return subgroup_check<G>(ctx, b->d.as<const typename G::Point>(), b->n, ctx->val_flag.as<uint32_t>()); }));
    VSP_HIP(hipMemcpyAsync(h_flag, ctx->val_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    if (*h_flag & 3u) return VSP_OK;
    ctx->stats["bases_subgroup_checks"] += 1;
    b->in_subgroup = (*h_flag & 4u) ? -1 : 1;
    if (b->in_subgroup < 0) ctx->stats["bases_outside_subgroup"] += 1;
    return VSP_OK;
}
int bases_create(vsp_ctx *ctx, int group, const void *src, bool src_on_device, size_t n, int trust, vsp_bases **out) {
    *out = nullptr;
    if (!ctx) return VSP_ERR_ARG;
    if (!src && n) return set_error(ctx, VSP_ERR_ARG, "bases: null pointer");
    hipSetDevice(ctx->device);
    const size_t esz = point_bytes(group);
    std::unique_ptr<vsp_bases> b(new vsp_bases());
    b->group = group; b->n = n;
    if (b->d.alloc(n ? n * esz : 16) != hipSuccess) return set_error(ctx, VSP_ERR_NOMEM, "bases: hipMalloc failed");
    if (n) {
        if (!src_on_device) {
            if (hipMemcpyAsync(b->d.p, src, n * esz, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return set_error(ctx, VSP_ERR_HIP, "bases: H2D failed");
            src = b->d.p;                    // convert in place
        }
        // boundary validation (include/vsp.h): coordinates below p always; the curve equation unless option "bases_check_curve" = 0
        const long check_curve = opt(ctx, "bases_check_curve", 1);
        // the subgroup (option "bases_check_subgroup"): 1 (default) = checked where the endomorphism split would be used -- bases that fail
        // keep the plain layout, whose result is exact for ANY curve point (like the reference's generic multiexp); 2 = always checked, a
        // failing upload is refused; 0 = never checked, and then never split unless "msm_glv" = 2 (the caller vouches for the points)
        const long check_sub = opt(ctx, "bases_check_subgroup", 1);
        VSP_TRY(ensure(ctx, ctx->val_flag, 16));
        if (hipMemsetAsync(ctx->val_flag.p, 0, 16, ctx->stream) != hipSuccess) return set_error(ctx, VSP_ERR_HIP, "bases: memset failed");
        VSP_TRY(with_group(group, [&](auto g) {
            using G = decltype(g);
            return bases_to_mont<G>(ctx, src, b->d.as<typename G::Point>(), n, (int)check_curve, (uint32_t *)ctx->val_flag.p);
        }));
        uint32_t h_flag = 0;
        if (trust == BASES_OWN) b->in_subgroup = 1;
        // policy 2 covers every upload whose points the library did not make itself (caller's handles, one call's host buffers, key blobs),
        // with or without the curve check; policy 1 only the uploads that would get the endomorphism layout
        if (trust != BASES_OWN && (check_sub >= 2 || (trust == BASES_CALLER && check_curve && check_sub == 1 && glv_wanted(ctx, group, n, 0))))
            VSP_TRY(bases_subgroup_check(ctx, b.get(), &h_flag));
        else if (hipMemcpyAsync(&h_flag, ctx->val_flag.p, 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
            return set_error(ctx, VSP_ERR_HIP, "bases: conversion failed");
        if (h_flag & 3u) return set_error(ctx, VSP_ERR_ARG, (h_flag & 1u) ? "bases: a coordinate is not canonical (>= p)" : "bases: a point is not on the curve");
        if (b->in_subgroup < 0 && check_sub >= 2) return set_error(ctx, VSP_ERR_ARG, "bases: a point is not in the order-r subgroup");
        if (n >= 1024) build_table28(ctx, b.get());       // best effort: without it the 12 x 32-bit kernel runs
    }
    *out = b.release();
    return VSP_OK;
}

// queue the multi-exponentiation rq over points [first, first + rq.n) of resident bases on a work slot: plain bases or a table of window
// multiples, one scalar vector or a batch
int launch_on_bases(vsp_ctx *ctx, unsigned slot, const vsp_bases *bases, size_t first, MsmRequest rq) {
    if (slot < VSP_MSM_SLOTS) ctx->slot_group[slot] = bases->group;
    if (bases->pre_c && rq.batch && (!opt(ctx, "msm_batch_tables", 1) || bases->pre_c > 16))      // (a batch over the table: ONE bucket set per vector)
        return set_error(ctx, VSP_ERR_UNSUPPORTED, "msm: a batch over this table of window multiples is not supported (plain bases, or windows of at most 16 bits)");
    MsmPre pre{bases->n, first, bases->pre_c, bases->d28.p, bases->glv};
    rq.glv = bases->glv;
    if (bases->pre_c) { rq.bases = bases->d.p; rq.pre = &pre; }
    else {
        rq.bases = bases->d.as<const char>() + first * point_bytes(bases->group);
        rq.table28 = bases->d28.p ? bases->d28.as<const char>() + table28_rows(bases, bases->glv, first).first * row28_bytes(bases->group) : nullptr;
    }
    return with_group(bases->group, [&](auto g) { return msm_slot_launch<decltype(g)>(ctx, slot, rq); });
}

static int bases_precompute(vsp_ctx *ctx, vsp_bases *b, unsigned window_bits, bool split) {
    if (!ctx) return VSP_ERR_ARG;
    if (!b) return set_error(ctx, VSP_ERR_ARG, "precompute: null bases");
    // the endomorphism rows need the order-r subgroup (include/vsp.h "bases_check_subgroup"): bases that were not checked at upload are checked now
    if (split && b->pre_c == 0 && b->in_subgroup == 0 && opt(ctx, "msm_glv", 1) == 1 && b->n) {
        VSP_HIP(hipSetDevice(ctx->device));
        VSP_TRY(ensure(ctx, ctx->val_flag, 16));
        VSP_HIP(hipMemsetAsync(ctx->val_flag.p, 0, 4, ctx->stream));
        uint32_t h_flag = 0;
        VSP_TRY(bases_subgroup_check(ctx, b, &h_flag));
    }
    if (window_bits == 0) {                     // automatic: about n * W / 2^(c-1) = 256 points per shared bucket
        unsigned lg = ceil_log2(b->n ? b->n : 1);
        window_bits = lg < 11 ? 8 : (lg - 3 > 16 ? 16 : lg - 3);
    }
    if (window_bits < 8 || window_bits > 22) return set_error(ctx, VSP_ERR_ARG, "precompute: window_bits must be 8..22");
    if (b->pre_c == window_bits) return VSP_OK;
    if (b->pre_c) return set_error(ctx, VSP_ERR_ARG, "precompute: bases already precomputed for another window size");
    if (b->n == 0) { b->pre_c = window_bits; b->pre_split = split; return VSP_OK; }
    VSP_HIP(hipSetDevice(ctx->device));
    const unsigned W = 255 / window_bits + 1;
    const size_t esz = point_bytes(b->group);
    if ((size_t)W * b->n >= ((size_t)1 << 31)) return set_error(ctx, VSP_ERR_UNSUPPORTED, "precompute: table too large to index");
    DevBuf table;
    if (table.alloc((size_t)W * b->n * esz) != hipSuccess) return set_error(ctx, VSP_ERR_NOMEM, "precompute: hipMalloc failed");
    VSP_HIP(hipMemcpyAsync(table.p, b->d.p, b->n * esz, hipMemcpyDeviceToDevice, ctx->stream));
    VSP_TRY(with_group(b->group, [&](auto g) { using G = decltype(g); return msm_precompute<G>(ctx, table.as<typename G::Point>(), b->n, window_bits); }));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    b->d = std::move(table);                                 // the points go, the table stays
    b->pre_c = window_bits;
    b->pre_split = split;                                    // only now: a refused or failed call leaves the handle as it was (bases outside the subgroup get the ordinary table: build_table28 decides)
    build_table28(ctx, b);
    return VSP_OK;
}

}  // namespace vsp

using namespace vsp;

// caller's bases as a handle, or null with the reason in the context's error text
static vsp_bases *bases_upload(vsp_ctx *ctx, int group, const void *src, bool src_on_device, size_t n) {
    vsp_bases *b;
    bases_create(ctx, group, src, src_on_device, n, BASES_CALLER, &b);
    return b;
}

extern "C" {

vsp_bases *vsp_bases_upload_g1(vsp_ctx *ctx, const uint64_t *bases, size_t n) { return bases_upload(ctx, 1, bases, false, n); }
vsp_bases *vsp_bases_upload_g2(vsp_ctx *ctx, const uint64_t *bases, size_t n) { return bases_upload(ctx, 2, bases, false, n); }
vsp_bases *vsp_bases_from_device_g1(vsp_ctx *ctx, const void *d_bases, size_t n) { return bases_upload(ctx, 1, d_bases, true, n); }
vsp_bases *vsp_bases_from_device_g2(vsp_ctx *ctx, const void *d_bases, size_t n) { return bases_upload(ctx, 2, d_bases, true, n); }
size_t vsp_bases_count(const vsp_bases *b) { return b ? b->n : 0; }
size_t vsp_bases_device_bytes(const vsp_bases *b) {
    if (!b) return 0;
    const size_t count = b->n * (b->pre_c ? 255 / b->pre_c + 1 : 1);
    return (count ? count * point_bytes(b->group) : 16) + (b->d28.p ? table28_rows(b, b->glv).count * row28_bytes(b->group) : 0);
}
void vsp_bases_free(vsp_ctx *ctx, vsp_bases *b) {
    if (!b) return;
    if (ctx) { hipSetDevice(ctx->device); hipStreamSynchronize(ctx->stream); }
    delete b;
}
int vsp_bases_precompute(vsp_ctx *ctx, vsp_bases *b, unsigned window_bits) { return bases_precompute(ctx, b, window_bits, false); }
int vsp_bases_precompute_split(vsp_ctx *ctx, vsp_bases *b, unsigned window_bits) { return bases_precompute(ctx, b, window_bits, true); }

}  // extern "C"
