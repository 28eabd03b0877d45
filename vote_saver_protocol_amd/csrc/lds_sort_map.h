// Which (window, chunk) pair a workgroup of the LDS counting sort owns (msm_sort.hip: k_count_lds, k_scatter_lds), and in how many
// rounds over bucket ranges k_scatter_lds places its entries.  Shared by the gfx950 kernels, the host code that launches them and,
// through g++, by the CPU test build (tests/cpu_build/lds_sort_map_check.cpp).  Plain words, no field arithmetic.
//
// Workgroups are dealt round-robin over the 8 XCDs, so the blocks with equal blockIdx.x % 8 -- a "label" -- share one XCD and its
// 4 MiB L2 (observed, not promised: placement is a matter of speed only, no result depends on it).  Two mappings:
//   even (labelled = false): block = chunk W + w, W nchunks blocks, every XCD gets as many as the next.  W a multiple of 8 (the 8 windows
//     of a split 2^20-point problem, the 16 of an unsplit one): all chunks of a window carry the label w % 8 by themselves.
//   labelled (labelled = true): k_scatter_lds in rounds wants the workgroups that write one window's slice of `sorted` on ONE L2, so that a
//     line of it is completed there and leaves once: window w has label w % 8; on its label it is window j = w / 8 of ceil(W / 8); block
//     8 (chunk ceil(W / 8) + j) + w % 8 owns (w, chunk).  For W a multiple of 8 this IS the even mapping.  Any other W cannot have whole
//     windows on a label AND use every block id -- W = 1 with two chunks: blocks 0 and 1 carry different labels -- so the grid is rounded
//     up to 8 ceil(W / 8) nchunks blocks, the blocks whose window would be >= W own nothing and return at once, and the labels are loaded
//     unevenly (W = 15 with 17 chunks: 34 workgroups on seven XCDs of 32 CUs, 17 on the eighth -- a second wave of workgroups where the
//     even mapping needs one).  Such window counts are everyday ones (folded 17-bit windows: 15; 15-bit windows: 17), so the labelled
//     mapping is used only where rounds were asked for by the option; the automatic rule takes rounds only for a multiple of 8.
// Both kernels of a sort get the same choice, so the histogram a block reads is the one it wrote.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSP_LDSMAP_HD __host__ __device__ __forceinline__
#else
#define VSP_LDSMAP_HD inline
#endif

namespace vsp {

static constexpr unsigned LDS_SORT_LABELS = 8;            // XCDs of an MI355X
static constexpr unsigned LDS_SORT_MAX_ROUNDS = 32;       // what the option may force
// The automatic choice, from the sweep in profiles/scatter_rounds_sweep.txt (16-bit windows: 16 windows of 2^18, 2^20 and 2^22 entries,
// two on a label, and 8 windows of 2^20 entries -- 2, 8, 32 and 4 MiB of `sorted` per label).
// The part of `sorted` that the workgroups on one label write in one round should be no more than half of that XCD's 4 MiB L2; and a
// round is not free -- one pass over 16.7 M digits issues about 26 us of instructions, against 0.19 ms that the stores of a single
// pass cost -- so more than 4 rounds lose more than they save at every size measured: a slice that 4 rounds do not bring under the
// budget (32 MiB) is placed in a single pass, as before.  Only for W a multiple of 8: any other W would need the uneven grid above.
static constexpr size_t LDS_SORT_ROUND_BYTES = (size_t)2 << 20;
static constexpr unsigned LDS_SORT_AUTO_MAX_ROUNDS = 4;

struct LdsSortBlock { unsigned w, chunk; bool valid; };

VSP_LDSMAP_HD unsigned lds_sort_windows_per_label(unsigned W) { return (W + LDS_SORT_LABELS - 1) / LDS_SORT_LABELS; }
// blocks to launch for W windows of nchunks chunks each: W * nchunks in the even mapping, and in the labelled one when W is a multiple of 8
VSP_LDSMAP_HD unsigned lds_sort_grid(unsigned W, unsigned nchunks, bool labelled) {
    return labelled ? LDS_SORT_LABELS * lds_sort_windows_per_label(W) * nchunks : W * nchunks;
}
VSP_LDSMAP_HD LdsSortBlock lds_sort_block(unsigned block, unsigned W, unsigned nchunks, bool labelled) {
    if (!labelled) { LdsSortBlock e; e.w = block % W; e.chunk = block / W; e.valid = e.chunk < nchunks; return e; }
    const unsigned per = lds_sort_windows_per_label(W);
    const unsigned label = block % LDS_SORT_LABELS, slot = block / LDS_SORT_LABELS;
    LdsSortBlock r;
    r.w = label + LDS_SORT_LABELS * (slot % per);
    r.chunk = slot / per;
    r.valid = r.w < W && r.chunk < nchunks;
    return r;
}

// Rounds of k_scatter_lds: the smallest power of two R with (bytes of `sorted` the windows of one label write) / R <= the budget, if
// that is at most 4 (and at most the B buckets of a window) and W is a multiple of 8; 1 otherwise.  `entries`: sorted entries per window (the scalars of the
// problem); `single`: the shared-set mode, where the Wk windows of a vector write ONE set of buckets, so a label's workgroups spread
// over that whole set (K of them in a batch).  forced > 0 (option "msm_scatter_rounds"): that many rounds, rounded down to a power
// of two, 32 at most.
VSP_LDSMAP_HD unsigned lds_sort_rounds(unsigned W, unsigned Wk, unsigned K, bool single, unsigned B, size_t entries, long forced) {
    unsigned cap = LDS_SORT_MAX_ROUNDS < B ? LDS_SORT_MAX_ROUNDS : B;
    if (cap < 1) cap = 1;
    unsigned R = 1;
    if (forced > 0) { while (2 * R <= (unsigned long)forced && 2 * R <= cap) R *= 2; return R; }
    if (W % LDS_SORT_LABELS != 0) return 1;
    if (cap > LDS_SORT_AUTO_MAX_ROUNDS) cap = LDS_SORT_AUTO_MAX_ROUNDS;
    const unsigned per = lds_sort_windows_per_label(W);
    const size_t slices = single ? (size_t)(per < K ? per : K) * Wk : per;
    const size_t bytes = slices * entries * sizeof(uint32_t);
    while (R < cap && bytes / R > LDS_SORT_ROUND_BYTES) R *= 2;
    return bytes / R > LDS_SORT_ROUND_BYTES ? 1u : R;
}

}  // namespace vsp
