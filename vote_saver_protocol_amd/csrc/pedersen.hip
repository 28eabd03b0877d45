// The voter registry (include/vsp.h "the voter registry"): Pedersen hashes over Jubjub in batches, and the Merkle tree of
// the voters' public keys built, read and checked on the device.  The rules -- the group law, the table entry, the chunk encoding, the
// schedule, the lane shares and the fold order, the blob bit order -- are jubjub.h, which the CPU test build runs too.  Kernels:
//   k_pedersen_table   a lane per (generator, window): 4 j doublings from the generator, the four multiples, one inversion, four entries
//   k_pedersen<L>      a hash per group of L lanes (1, 4, 16, 64): every lane adds its share of the chunks, the group folds its partial
//                      sums through LDS in log2 L unified additions, lane 0 normalises (one inversion) and writes the digest and, where
//                      asked, the point -- or, for a tree loaded from a blob, compares the digest with the stored node.  The messages are
//                      rows of words (vsp_pedersen_hash_batch, the leaves) or the two children of a node, read in place
//   k_registry_top     ONE workgroup runs the top levels of a tree, groups of 64 lanes, a barrier between levels
//   k_registry_paths   a lane per (index, level): the sibling's digest
//   k_registry_blob    a lane per word: digest words <-> blob octets (the same map both ways), the 256th bit of a node reported
// Every loop's bound is a function of the kernel's arguments: chunks of the message / L, log2 L fold levels, 255 steps of the inversion,
// 4 j <= 248 doublings, levels and nodes per level of the top.  No kernel waits for another workgroup.
#include "common.h"
#include "jubjub.h"

namespace vsp {

static constexpr unsigned PED_THREADS = 256;
static constexpr size_t PED_PIECE = (size_t)1 << 20;               // hashes of one piece of vsp_pedersen_hash_batch
static constexpr size_t PED_MAX_GENERATORS = 1024;
static constexpr unsigned REG_TOP_GROUPS = PED_THREADS / 64;        // hashes the top kernel's workgroup runs at once

namespace {

using JEntry = JjEntry<Fr>;
using JPoint = JjPoint<Fr>;

// what a launch of k_pedersen hashes and where the results go
struct PedJob {
    const uint64_t *rows;           // rows != null: message i is `row_words` words at rows + i row_words; rows at or past `present` are all zero
    size_t row_words, present;
    const uint64_t *children;       // rows == null: message i is the children's digests at children + 8 i (255 + 255 bits)
    uint32_t nbits;
    size_t count;
    uint64_t *digests;              // count x 4, or null
    uint64_t *points;               // count x 8, or null
    const uint64_t *expect;         // not null: digest i is compared with expect + 4 i and a mismatch lowers *first_bad to first_index + i
    uint64_t first_index;
    unsigned long long *first_bad;
};

__device__ __forceinline__ void ped_finish(const PedJob &job, size_t i, const JPoint &sum) {
    const JjAffine<Fr> a = jj_to_affine(sum);
    uint64_t d[4];
    jj_store_canonical(d, a.u);
    if (job.digests) { uint64_t *o = job.digests + 4 * i; o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3]; }
    if (job.points) {
        uint64_t v[4];
        jj_store_canonical(v, a.v);
        uint64_t *o = job.points + 8 * i;
        o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; o[3] = d[3]; o[4] = v[0]; o[5] = v[1]; o[6] = v[2]; o[7] = v[3];
    }
    if (job.expect) {
        const uint64_t *e = job.expect + 4 * i;
        if ((d[0] ^ e[0]) | (d[1] ^ e[1]) | (d[2] ^ e[2]) | (d[3] ^ e[3]))
            __hip_atomic_fetch_min(job.first_bad, (unsigned long long)(job.first_index + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ JjMessage ped_message(const PedJob &job, size_t i, const uint64_t *zero_row) {
    JjMessage m;
    m.nbits = job.nbits;
    if (job.rows) { m.w = i < job.present ? job.rows + i * job.row_words : zero_row; m.gap = 0; }
    else { m.w = job.children + 8 * i; m.gap = 1; }
    return m;
}

// the fold of a group's partial sums through the block's LDS (jubjub.h jj_fold_gives / jj_fold_takes): part has a slot per thread, a group
// lies inside one wave, the barriers are the block's -- EVERY thread of the block calls this, an idle one with active = false.  A lane gives
// once, so no slot is written twice: one barrier a level
template <unsigned L> __device__ __forceinline__ void ped_fold(JPoint &acc, JPoint *part, unsigned lane, bool active) {
    const unsigned lanes = active ? L : 0;
#pragma unroll 1
    for (unsigned s = L / 2; s >= 1; s >>= 1) {
        if (jj_fold_gives(lane, lanes, s)) part[threadIdx.x] = acc;
        __syncthreads();
        if (jj_fold_takes(lane, lanes, s)) acc = jj_add(acc, part[threadIdx.x + s]);
    }
}

template <unsigned L> __global__ __launch_bounds__(PED_THREADS) void k_pedersen(const JEntry *__restrict__ tab, PedJob job, const uint64_t *__restrict__ zero_row) {
    const size_t i = ((size_t)blockIdx.x * PED_THREADS + threadIdx.x) / L;
    const unsigned lane = threadIdx.x % L;
    const bool active = i < job.count;
    JPoint acc = JPoint::identity();
    if (active) acc = jj_lane_sum(tab, ped_message(job, i, zero_row), lane, L);
    if constexpr (L > 1) {
        __shared__ JPoint part[PED_THREADS];
        ped_fold<L>(acc, part, lane, active);
    }
    if (active && lane == 0) ped_finish(job, i, acc);
}

// The top of a tree in one workgroup: levels first_level .. depth of the tree whose nodes lie at `nodes` (leaves first).  Level l has
// 2^(depth - l) nodes; the workgroup hashes REG_TOP_GROUPS of them at a time, 64 lanes each, and passes a barrier (behind a fence: the
// next level reads what this one wrote to global memory) before the next level
__global__ __launch_bounds__(PED_THREADS) void k_registry_top(const JEntry *__restrict__ tab, uint64_t *nodes, unsigned depth, unsigned first_level) {
    __shared__ JPoint part[PED_THREADS];
    const unsigned group = threadIdx.x / 64, lane = threadIdx.x % 64;
#pragma unroll 1
    for (unsigned l = first_level; l <= depth; l++) {
        PedJob job;
        job.rows = nullptr; job.row_words = 0; job.present = 0;
        job.children = nodes + 4 * jj_level_first(depth, l - 1);
        job.nbits = JJ_NODE_BITS;
        job.count = (size_t)jj_level_nodes(depth, l);
        job.digests = nodes + 4 * jj_level_first(depth, l);
        job.points = nullptr; job.expect = nullptr; job.first_index = 0; job.first_bad = nullptr;
#pragma unroll 1
        for (size_t at = 0; at < job.count; at += REG_TOP_GROUPS) {
            const size_t i = at + group;
            const bool active = i < job.count;
            JPoint acc = JPoint::identity();
            if (active) acc = jj_lane_sum(tab, ped_message(job, i, nullptr), lane, 64);
            ped_fold<64>(acc, part, lane, active);
            if (active && lane == 0) ped_finish(job, i, acc);
            __syncthreads();                                        // the slots of `part` are free again
        }
        __threadfence();
        __syncthreads();
    }
}

__global__ __launch_bounds__(PED_THREADS) void k_pedersen_table(const JjAffine<Fr> *__restrict__ gens, size_t g, JEntry *__restrict__ tab) {
    const size_t t = (size_t)blockIdx.x * PED_THREADS + threadIdx.x;
    if (t >= g * JJ_WINDOWS) return;
    const size_t i = t / JJ_WINDOWS;
    const unsigned j = (unsigned)(t % JJ_WINDOWS);
    JEntry e[JJ_ENTRIES];
    jj_window_entries(jj_window_base(gens[i], j), e);
#pragma unroll
    for (unsigned k = 0; k < JJ_ENTRIES; k++) tab[t * JJ_ENTRIES + k] = e[k];
}

__global__ __launch_bounds__(PED_THREADS) void k_registry_paths(const uint64_t *__restrict__ nodes, unsigned depth, const uint64_t *__restrict__ indices, size_t n,
                                                                uint64_t *__restrict__ out) {
    const size_t t = (size_t)blockIdx.x * PED_THREADS + threadIdx.x;
    if (t >= n * depth) return;
    const size_t q = t / depth;
    const unsigned l = (unsigned)(t % depth);
    const uint64_t *src = nodes + 4 * (jj_level_first(depth, l) + jj_sibling(indices[q], l));
    uint64_t *dst = out + 4 * t;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
}

// words of digests <-> words of blob octets; flag (may be null) is raised when a node's 256th bit is set in the digest form
__global__ __launch_bounds__(PED_THREADS) void k_registry_blob(const uint64_t *in, uint64_t *out, size_t words, uint32_t *flag) {
    const size_t t = (size_t)blockIdx.x * PED_THREADS + threadIdx.x;
    if (t >= words) return;
    const uint64_t w = jj_blob_word(in[t]);
    out[t] = w;
    if (flag && (t & 3) == 3 && (w >> 63)) atomicOr(flag, 1u);
}

unsigned ped_blocks(size_t lanes) { return (unsigned)((lanes + PED_THREADS - 1) / PED_THREADS); }

// the group size of a launch of `count` hashes: option "pedersen_lanes" when it names one, else by the count
unsigned ped_lanes(const vsp_ctx *ctx, size_t count) {
    const long forced = opt(ctx, "pedersen_lanes", 0);
    return jj_lanes_valid(forced) ? (unsigned)forced : jj_group_lanes(count);
}

int ped_launch(vsp_ctx *ctx, const vsp_pedersen *ped, const PedJob &job, unsigned lanes) {
    if (!job.count) return VSP_OK;
    const JEntry *tab = (const JEntry *)ped->table.p;
    const dim3 grid(ped_blocks(job.count * lanes)), block(PED_THREADS);
    const uint64_t *zero_row = (const uint64_t *)ctx->ped_zero.p;
    switch (lanes) {
    case 1: hipLaunchKernelGGL(k_pedersen<1>, grid, block, 0, ctx->stream, tab, job, zero_row); break;
    case 4: hipLaunchKernelGGL(k_pedersen<4>, grid, block, 0, ctx->stream, tab, job, zero_row); break;
    case 16: hipLaunchKernelGGL(k_pedersen<16>, grid, block, 0, ctx->stream, tab, job, zero_row); break;
    default: hipLaunchKernelGGL(k_pedersen<64>, grid, block, 0, ctx->stream, tab, job, zero_row); break;
    }
    VSP_LAUNCH_CHECK();
    return VSP_OK;
}

// the all-zero row that absent keys read: as many words as the longest message of `ped`
int ped_ensure_zero(vsp_ctx *ctx, const vsp_pedersen *ped) {
    const size_t bytes = ((jj_max_bits(ped->g) + 63) / 64) * sizeof(uint64_t);
    if (ctx->ped_zero.p && ctx->ped_zero.cap >= bytes) return VSP_OK;
    VSP_TRY(ensure(ctx, ctx->ped_zero, bytes));
    VSP_HIP(hipMemsetAsync(ctx->ped_zero.p, 0, ctx->ped_zero.cap, ctx->stream));
    return VSP_OK;
}

PedJob ped_rows_job(const uint64_t *rows, size_t row_words, size_t present, uint32_t nbits, size_t count, uint64_t *digests, uint64_t *points) {
    PedJob job;
    job.rows = rows; job.row_words = row_words; job.present = present; job.children = nullptr; job.nbits = nbits; job.count = count;
    job.digests = digests; job.points = points; job.expect = nullptr; job.first_index = 0; job.first_bad = nullptr;
    return job;
}
PedJob ped_level_job(uint64_t *nodes, unsigned depth, unsigned level) {
    PedJob job = ped_rows_job(nullptr, 0, 0, JJ_NODE_BITS, (size_t)jj_level_nodes(depth, level), nodes + 4 * jj_level_first(depth, level), nullptr);
    job.children = nodes + 4 * jj_level_first(depth, level - 1);
    return job;
}

// how many of the top levels the single workgroup takes: option "registry_fused_levels" (0: the levels of at most REG_TOP_GROUPS nodes;
// negative: none), never more than the tree has above its leaves
unsigned reg_fused_levels(const vsp_ctx *ctx, unsigned depth) {
    const long v = opt(ctx, "registry_fused_levels", 0);
    if (v < 0) return 0;
    unsigned f = v == 0 ? ceil_log2(REG_TOP_GROUPS) + 1 : (unsigned)(v > (long)JJ_MAX_DEPTH ? (long)JJ_MAX_DEPTH : v);
    return f < depth ? f : depth;
}

// levels 1 .. depth over the leaves already at `nodes`
int reg_build_levels(vsp_ctx *ctx, const vsp_pedersen *ped, uint64_t *nodes, unsigned depth) {
    const unsigned fused = reg_fused_levels(ctx, depth);
    for (unsigned l = 1; l + fused <= depth; l++) {
        const PedJob job = ped_level_job(nodes, depth, l);
        VSP_TRY(ped_launch(ctx, ped, job, ped_lanes(ctx, job.count)));
    }
    if (fused) {
        hipLaunchKernelGGL(k_registry_top, dim3(1), dim3(PED_THREADS), 0, ctx->stream, (const JEntry *)ped->table.p, nodes, depth, depth - fused + 1);
        VSP_LAUNCH_CHECK();
    }
    return VSP_OK;
}

int ped_check_handle(vsp_ctx *ctx, const vsp_pedersen *ped, const char *who) {
    if (ped->device != ctx->device) { std::string m = std::string(who) + ": the hash's tables belong to another device"; return set_error(ctx, VSP_ERR_ARG, m.c_str()); }
    return VSP_OK;
}

}  // anonymous namespace
}  // namespace vsp

using namespace vsp;

extern "C" {

int vsp_pedersen_create(vsp_ctx *ctx, const uint64_t *generators, size_t g, vsp_pedersen **out) {
    if (!ctx) return VSP_ERR_ARG;
    if (out) *out = nullptr;
    if (!generators || !out) return set_error(ctx, VSP_ERR_ARG, "pedersen_create: null argument");
    if (g == 0 || g > PED_MAX_GENERATORS) return set_error(ctx, VSP_ERR_ARG, "pedersen_create: 1 to 1024 generators expected");
    std::vector<JjAffine<Fr>> gens(g);
    for (size_t i = 0; i < g; i++) {
        JjAffine<HFr> a;
        const int fault = jj_generator_fault<HFr>(generators + 8 * i, &a);
        if (fault != JJ_GEN_OK) {
            static const char *const why[] = {"", "has a coordinate that is not below r", "is not on the curve", "is the identity", "is not in the subgroup of prime order"};
            char msg[160];
            snprintf(msg, sizeof msg, "pedersen_create: generator %zu %s", i, why[fault]);
            return set_error(ctx, VSP_ERR_ARG, msg);
        }
        memcpy(&gens[i], &a, sizeof a);                             // the same Montgomery value on 32-bit limbs
    }
    VSP_HIP(hipSetDevice(ctx->device));
    vsp_pedersen *ped = new vsp_pedersen();
    ped->device = ctx->device; ped->g = g;
    auto setup = [&]() -> int {
        VSP_TRY(ensure(ctx, ped->table, g * JJ_GEN_ENTRIES * sizeof(JEntry)));
        VSP_TRY(ensure(ctx, ctx->ped_in, g * sizeof(JjAffine<Fr>)));
        VSP_HIP(hipMemcpyAsync(ctx->ped_in.p, gens.data(), g * sizeof(JjAffine<Fr>), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pedersen_table, dim3(ped_blocks(g * JJ_WINDOWS)), dim3(PED_THREADS), 0, ctx->stream, (const JjAffine<Fr> *)ctx->ped_in.p, g, (JEntry *)ped->table.p);
        VSP_LAUNCH_CHECK();
        VSP_HIP(hipStreamSynchronize(ctx->stream));
        return VSP_OK;
    };
    const int r = setup();
    if (r != VSP_OK) { vsp_pedersen_free(ctx, ped); return r; }
    *out = ped;
    return VSP_OK;
}

void vsp_pedersen_free(vsp_ctx *ctx, vsp_pedersen *ped) {
    if (!ped) return;
    hipSetDevice(ped->device);
    if (ctx) hipStreamSynchronize(ctx->stream);
    delete ped;
}

size_t vsp_pedersen_generators(const vsp_pedersen *ped) { return ped ? ped->g : 0; }
size_t vsp_pedersen_max_bits(const vsp_pedersen *ped) { return ped ? jj_max_bits(ped->g) : 0; }
size_t vsp_pedersen_device_bytes(const vsp_pedersen *ped) { return ped ? ped->table.cap : 0; }

int vsp_pedersen_hash_batch(vsp_ctx *ctx, const vsp_pedersen *ped, const uint64_t *msgs, size_t nbits, size_t count, uint64_t *digests_out, uint64_t *points_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!ped || !msgs || !digests_out) return set_error(ctx, VSP_ERR_ARG, "pedersen_hash_batch: null argument");
    VSP_TRY(ped_check_handle(ctx, ped, "pedersen_hash_batch"));
    if (nbits == 0 || nbits > jj_max_bits(ped->g)) return set_error(ctx, VSP_ERR_ARG, "pedersen_hash_batch: a message has 1 to 189 g bits");
    if (!count) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t row_words = (nbits + 63) / 64, out_words = points_out ? 12 : 4;
    for (size_t at = 0; at < count; at += PED_PIECE) {
        const size_t c = count - at < PED_PIECE ? count - at : PED_PIECE;
        VSP_TRY(ensure(ctx, ctx->ped_in, c * row_words * sizeof(uint64_t)));
        VSP_TRY(ensure(ctx, ctx->ped_out, c * out_words * sizeof(uint64_t)));
        uint64_t *d_digests = (uint64_t *)ctx->ped_out.p, *d_points = points_out ? d_digests + 4 * c : nullptr;
        VSP_HIP(hipMemcpyAsync(ctx->ped_in.p, msgs + at * row_words, c * row_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_TRY(ctx->ped_timer.mark(ctx, 0, st));
        VSP_TRY(ped_launch(ctx, ped, ped_rows_job((const uint64_t *)ctx->ped_in.p, row_words, c, (uint32_t)nbits, c, d_digests, d_points), ped_lanes(ctx, c)));
        VSP_TRY(ctx->ped_timer.mark(ctx, 1, st));
        VSP_HIP(hipMemcpyAsync(digests_out + 4 * at, d_digests, c * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        if (points_out) VSP_HIP(hipMemcpyAsync(points_out + 8 * at, d_points, c * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        ctx->ped_timer.add(ctx, 0, "pedersen_ms");
    }
    return VSP_OK;
}

int vsp_registry_build(vsp_ctx *ctx, const vsp_pedersen *ped, const uint64_t *pks, size_t count, unsigned depth, int hash_leaves, vsp_registry **out) {
    if (!ctx) return VSP_ERR_ARG;
    if (out) *out = nullptr;
    if (!ped || !pks || !out) return set_error(ctx, VSP_ERR_ARG, "registry_build: null argument");
    VSP_TRY(ped_check_handle(ctx, ped, "registry_build"));
    if (ped->g < JJ_NODE_GENERATORS) return set_error(ctx, VSP_ERR_ARG, "registry_build: a node hashes 510 bits: at least 3 generators are needed");
    if (depth > JJ_MAX_DEPTH) return set_error(ctx, VSP_ERR_UNSUPPORTED, "registry_build: depth above 24");
    if (count > ((size_t)1 << depth)) return set_error(ctx, VSP_ERR_ARG, "registry_build: more keys than the tree has leaves");
    for (size_t i = 0; i < count; i++)
        if (pks[4 * i + 3] >> 63) { char m[96]; snprintf(m, sizeof m, "registry_build: key %zu has bit 255 set", i); return set_error(ctx, VSP_ERR_ARG, m); }
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    vsp_registry *reg = new vsp_registry();
    reg->device = ctx->device; reg->depth = depth;
    auto build = [&]() -> int {
        const size_t leaves = (size_t)1 << depth, key_bytes = count * 4 * sizeof(uint64_t);
        VSP_TRY(ensure(ctx, reg->nodes, jj_tree_nodes(depth) * 4 * sizeof(uint64_t)));
        uint64_t *nodes = (uint64_t *)reg->nodes.p;
        VSP_TRY(ped_ensure_zero(ctx, ped));
        if (hash_leaves) {
            VSP_TRY(ensure(ctx, ctx->ped_in, key_bytes));
            if (count) VSP_HIP(hipMemcpyAsync(ctx->ped_in.p, pks, key_bytes, hipMemcpyHostToDevice, st));
        } else {
            if (count) VSP_HIP(hipMemcpyAsync(nodes, pks, key_bytes, hipMemcpyHostToDevice, st));
            if (count < leaves) VSP_HIP(hipMemsetAsync(nodes + 4 * count, 0, (leaves - count) * 4 * sizeof(uint64_t), st));
        }
        VSP_TRY(ctx->ped_timer.mark(ctx, 0, st));
        if (hash_leaves) VSP_TRY(ped_launch(ctx, ped, ped_rows_job((const uint64_t *)ctx->ped_in.p, 4, count, JJ_DIGEST_BITS, leaves, nodes, nullptr), ped_lanes(ctx, leaves)));
        VSP_TRY(reg_build_levels(ctx, ped, nodes, depth));
        VSP_TRY(ctx->ped_timer.mark(ctx, 1, st));
        VSP_HIP(hipStreamSynchronize(st));
        ctx->ped_timer.add(ctx, 0, "registry_build_ms");
        return VSP_OK;
    };
    const int r = build();
    if (r != VSP_OK) { hipStreamSynchronize(st); delete reg; return r; }
    *out = reg;
    return VSP_OK;
}

size_t vsp_registry_blob_size(unsigned depth) { return depth > JJ_MAX_DEPTH ? 0 : (size_t)jj_tree_nodes(depth) * 32; }

int vsp_registry_from_blob(vsp_ctx *ctx, const vsp_pedersen *ped, const uint8_t *blob, size_t len, unsigned depth, int verify, vsp_registry **out, uint64_t *first_bad_node_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (out) *out = nullptr;
    if (first_bad_node_out) *first_bad_node_out = ~(uint64_t)0;
    if (!ped || !blob || !out) return set_error(ctx, VSP_ERR_ARG, "registry_from_blob: null argument");
    VSP_TRY(ped_check_handle(ctx, ped, "registry_from_blob"));
    if (ped->g < JJ_NODE_GENERATORS) return set_error(ctx, VSP_ERR_ARG, "registry_from_blob: a node hashes 510 bits: at least 3 generators are needed");
    if (depth > JJ_MAX_DEPTH) return set_error(ctx, VSP_ERR_UNSUPPORTED, "registry_from_blob: depth above 24");
    if (len != vsp_registry_blob_size(depth)) return set_error(ctx, VSP_ERR_ARG, "registry_from_blob: the blob of a tree of this depth has 32 (2^(depth + 1) - 1) octets");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    vsp_registry *reg = new vsp_registry();
    reg->device = ctx->device; reg->depth = depth;
    uint64_t bad = ~(uint64_t)0;
    auto load = [&]() -> int {
        const size_t words = (size_t)jj_tree_nodes(depth) * 4;
        VSP_TRY(ensure(ctx, reg->nodes, len));
        VSP_TRY(ensure(ctx, ctx->ped_out, 16));
        uint64_t *nodes = (uint64_t *)reg->nodes.p;
        uint32_t *flag = (uint32_t *)ctx->ped_out.p;
        unsigned long long *first_bad = (unsigned long long *)ctx->ped_out.p + 1;
        VSP_HIP(hipMemcpyAsync(nodes, blob, len, hipMemcpyHostToDevice, st));
        VSP_HIP(hipMemsetAsync(flag, 0, 8, st));
        VSP_HIP(hipMemsetAsync(first_bad, 0xff, 8, st));
        hipLaunchKernelGGL(k_registry_blob, dim3(ped_blocks(words)), dim3(PED_THREADS), 0, st, (const uint64_t *)nodes, nodes, words, flag);
        VSP_LAUNCH_CHECK();
        if (verify) {
            VSP_TRY(ctx->ped_timer.mark(ctx, 0, st));
            for (unsigned l = 1; l <= depth; l++) {
                PedJob job = ped_level_job(nodes, depth, l);
                job.expect = job.digests; job.digests = nullptr;
                job.first_index = jj_level_first(depth, l); job.first_bad = first_bad;
                VSP_TRY(ped_launch(ctx, ped, job, ped_lanes(ctx, job.count)));
            }
            VSP_TRY(ctx->ped_timer.mark(ctx, 1, st));
        }
        uint64_t h[2] = {0, 0};
        VSP_HIP(hipMemcpyAsync(h, ctx->ped_out.p, sizeof h, hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        if (verify) ctx->ped_timer.add(ctx, 0, "registry_check_ms");
        if (h[0] & 1) return set_error(ctx, VSP_ERR_ARG, "registry_from_blob: a node has its 256th bit set");
        bad = h[1];
        return VSP_OK;
    };
    const int r = load();
    if (r != VSP_OK) { hipStreamSynchronize(st); delete reg; return r; }
    if (first_bad_node_out) *first_bad_node_out = bad;
    *out = reg;
    return VSP_OK;
}

void vsp_registry_free(vsp_ctx *ctx, vsp_registry *reg) {
    if (!reg) return;
    hipSetDevice(reg->device);
    if (ctx) hipStreamSynchronize(ctx->stream);
    delete reg;
}

unsigned vsp_registry_depth(const vsp_registry *reg) { return reg ? reg->depth : 0; }
size_t vsp_registry_device_bytes(const vsp_registry *reg) { return reg ? reg->nodes.cap : 0; }

int vsp_registry_nodes(vsp_ctx *ctx, const vsp_registry *reg, unsigned level, uint64_t first, size_t count, uint64_t *out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!reg || !out) return set_error(ctx, VSP_ERR_ARG, "registry_nodes: null argument");
    if (reg->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "registry_nodes: the registry belongs to another device");
    if (level > reg->depth) return set_error(ctx, VSP_ERR_ARG, "registry_nodes: a level above the root");
    const uint64_t have = jj_level_nodes(reg->depth, level);
    if (first > have || count > have - first) return set_error(ctx, VSP_ERR_ARG, "registry_nodes: a range outside the level");
    if (!count) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    VSP_HIP(hipMemcpyAsync(out, (const uint64_t *)reg->nodes.p + 4 * (jj_level_first(reg->depth, level) + first), count * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}

int vsp_registry_root(vsp_ctx *ctx, const vsp_registry *reg, uint64_t digest_out[4], uint64_t rt_scalars_out[8]) {
    if (!ctx) return VSP_ERR_ARG;
    if (!reg || !digest_out) return set_error(ctx, VSP_ERR_ARG, "registry_root: null argument");
    VSP_TRY(vsp_registry_nodes(ctx, reg, reg->depth, 0, 1, digest_out));
    if (rt_scalars_out) jj_rt_split(digest_out, rt_scalars_out);
    return VSP_OK;
}

int vsp_registry_paths(vsp_ctx *ctx, const vsp_registry *reg, const uint64_t *indices, size_t n, uint64_t *siblings_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!reg || !indices || !siblings_out) return set_error(ctx, VSP_ERR_ARG, "registry_paths: null argument");
    if (reg->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "registry_paths: the registry belongs to another device");
    for (size_t i = 0; i < n; i++)
        if (indices[i] >> reg->depth) { char m[96]; snprintf(m, sizeof m, "registry_paths: index %zu is not below 2^depth", i); return set_error(ctx, VSP_ERR_ARG, m); }
    if (!n || !reg->depth) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t D = reg->depth;
    for (size_t at = 0; at < n; at += PED_PIECE) {
        const size_t c = n - at < PED_PIECE ? n - at : PED_PIECE;
        VSP_TRY(ensure(ctx, ctx->ped_in, c * sizeof(uint64_t)));
        VSP_TRY(ensure(ctx, ctx->ped_out, c * D * 4 * sizeof(uint64_t)));
        VSP_HIP(hipMemcpyAsync(ctx->ped_in.p, indices + at, c * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        VSP_TRY(ctx->ped_timer.mark(ctx, 0, st));
        hipLaunchKernelGGL(k_registry_paths, dim3(ped_blocks(c * D)), dim3(PED_THREADS), 0, st, (const uint64_t *)reg->nodes.p, reg->depth, (const uint64_t *)ctx->ped_in.p, c,
                           (uint64_t *)ctx->ped_out.p);
        VSP_LAUNCH_CHECK();
        VSP_TRY(ctx->ped_timer.mark(ctx, 1, st));
        VSP_HIP(hipMemcpyAsync(siblings_out + at * D * 4, ctx->ped_out.p, c * D * 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        VSP_HIP(hipStreamSynchronize(st));
        ctx->ped_timer.add(ctx, 0, "registry_paths_ms");
    }
    return VSP_OK;
}

int vsp_registry_to_blob(vsp_ctx *ctx, const vsp_registry *reg, uint8_t *out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!reg || !out) return set_error(ctx, VSP_ERR_ARG, "registry_to_blob: null argument");
    if (reg->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "registry_to_blob: the registry belongs to another device");
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t words = (size_t)jj_tree_nodes(reg->depth) * 4;
    VSP_TRY(ensure(ctx, ctx->ped_out, words * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_registry_blob, dim3(ped_blocks(words)), dim3(PED_THREADS), 0, st, (const uint64_t *)reg->nodes.p, (uint64_t *)ctx->ped_out.p, words, (uint32_t *)nullptr);
    VSP_LAUNCH_CHECK();
    VSP_HIP(hipMemcpyAsync(out, ctx->ped_out.p, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    return VSP_OK;
}

}  // extern "C"
