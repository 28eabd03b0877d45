// Generator-side fixed-base batch exponentiation (the Groth16 generator's batch_exp, reached from
// bin/cli/include/nil/vote_saver/common.hpp:916-917): out[i] = scalars[i] * generator, as canonical affine points.
// Implementation include: fixedbase_g1.hip / fixedbase_g2.hip each instantiate fixed_base_mul for their group, so the two build in parallel.
#include "common.h"
#include "lane_view.h"

namespace vsp {
namespace {

// ---- fixed-base windowed multiplication: 32 windows of 8 bits, table[w][d-1] = d * 256^w * G (affine, Montgomery)
static constexpr int FB_WINDOWS = 32, FB_ENTRIES = 255;

template <class F>
__global__ __launch_bounds__(256, 2) void k_fixed_base(const Affine<F> *table, const Fr *scalars, size_t n, XYZZ<F> *out) {
    using LV = LaneView<F>; using E = typename LV::E;       // G2: two lanes per scalar (lane_view.h)
    size_t i = gid<F>();
    if (i >= n) return;
    const uint8_t *kb = (const uint8_t *)scalars[i].l;
    XYZZ<E> acc = XYZZ<E>::inf();
    for (int w = 0; w < FB_WINDOWS; w++) {
        unsigned d = kb[w];
        if (d) xyzz_madd(acc, LV::load(&table[w * FB_ENTRIES + d - 1]));
    }
    LV::store(&out[i], acc);
}

// batch normalisation XYZZ -> canonical affine; each thread owns a chunk and does one inversion for it
// (Montgomery's trick, prefix products kept in global scratch `pre`)
static constexpr unsigned BA_CHUNK = 32;
template <class F>
__global__ __launch_bounds__(64) void k_batch_affine(const XYZZ<F> *in, size_t n, F *pre, Affine<F> *out) {
    size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t b = t * BA_CHUNK, e = b + BA_CHUNK < n ? b + BA_CHUNK : n;
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
            F zi3 = mul(ai, pre[i]);          // 1 / ZZZ_i
            ai = mul(ai, p.ZZZ);
            F zi = mul(zi3, p.ZZ);            // 1 / Z
            F zi2 = sqr(zi);
            r.x = from_mont(mul(p.X, zi2));
            r.y = from_mont(mul(p.Y, zi3));
        }
        out[i] = r;
    }
}

template <class F, class HF>
static int build_fixed_table(vsp_ctx *ctx, const Affine<HF> &gen, DevBuf &dst) {
    if (dst.p) return VSP_OK;
    std::vector<XYZZ<HF>> tj((size_t)FB_WINDOWS * FB_ENTRIES);
    XYZZ<HF> wb = xyzz_from_affine(gen);
    for (int w = 0; w < FB_WINDOWS; w++) {
        XYZZ<HF> acc = wb;
        for (int e = 0; e < FB_ENTRIES; e++) { tj[(size_t)w * FB_ENTRIES + e] = acc; xyzz_add(acc, wb); }
        wb = acc;
    }
    // batch to affine on the host
    size_t cnt = tj.size();
    std::vector<HF> pre(cnt);
    HF acc = HF::one();
    for (size_t i = 0; i < cnt; i++) { pre[i] = acc; acc = mul(acc, tj[i].ZZZ); }
    HF ai = inv(acc);
    std::vector<Affine<HF>> ta(cnt);
    for (size_t i = cnt; i-- > 0;) {
        HF zi3 = mul(ai, pre[i]); ai = mul(ai, tj[i].ZZZ);
        HF zi = mul(zi3, tj[i].ZZ), zi2 = sqr(zi);
        ta[i].x = mul(tj[i].X, zi2); ta[i].y = mul(tj[i].Y, zi3);
    }
    VSP_TRY(ensure(ctx, dst, cnt * sizeof(Affine<F>)));
    VSP_HIP(hipMemcpyAsync(dst.p, ta.data(), cnt * sizeof(Affine<F>), hipMemcpyHostToDevice, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}

}  // anonymous namespace

template <class G> int fixed_base_mul(vsp_ctx *ctx, const Fr *d_scalars, size_t n, void *d_out) {
    using F = typename G::F; using HF = typename G::HF;
    if (!n) return VSP_OK;
    VSP_TRY((build_fixed_table<F, HF>(ctx, host_load_affine<HF>(G::GEN), ctx->fb_table[G::ID - 1])));
    VSP_TRY(ensure(ctx, ctx->fb_tmp, n * sizeof(XYZZ<F>)));
    VSP_TRY(ensure(ctx, ctx->fb_pre, n * sizeof(F)));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fixed_base<F>), dim3((unsigned)((n * LaneView<F>::LANES + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const Affine<F> *)ctx->fb_table[G::ID - 1].p, d_scalars, n, (XYZZ<F> *)ctx->fb_tmp.p);
    VSP_LAUNCH_CHECK();
    size_t chunks = (n + BA_CHUNK - 1) / BA_CHUNK;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_batch_affine<F>), dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, ctx->stream,
                       (const XYZZ<F> *)ctx->fb_tmp.p, n, (F *)ctx->fb_pre.p, (Affine<F> *)d_out);
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

}  // namespace vsp
