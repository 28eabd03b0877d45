// CPU test build of the LDS counting sort's block mapping and round count (vote_saver_protocol_amd/csrc/lds_sort_map.h, compiled by
// g++).  Test infrastructure only.  A program of its own (tests/test_lds_sort_map_cpu.py builds and runs it): for every window count
// W in 1..64 and every chunk count 1..256 -- the host takes 256 / W halved while chunks are shorter than 8192 scalars, so every
// power of two and values such as 28 -- in the LABELLED mapping the blocks 0 .. grid - 1 that own something map one-to-one onto the
// (window, chunk) pairs, all chunks of a window carry one label (block % 8), the windows are dealt over the labels as evenly as W allows,
// and a W that is a multiple of 8 has no idle block and the mapping block = chunk W + w; in the EVEN mapping the blocks 0 .. W chunks - 1
// map one-to-one onto the pairs with no idle block for any W, and for a multiple of 8 it is the labelled mapping.
#include <stdio.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/lds_sort_map.h"
using namespace vsp;

static int fail(const char *what, unsigned W, unsigned chunks, unsigned block) {
    printf("lds_sort_map_check: FAILED: %s (W = %u, chunks = %u, block = %u)\n", what, W, chunks, block);
    return 1;
}

static int check_even_mapping(unsigned W, unsigned chunks) {
    if (lds_sort_grid(W, chunks, false) != W * chunks) return fail("even grid", W, chunks, 0);
    std::vector<int> owner(W * chunks, -1);
    for (unsigned b = 0; b < W * chunks; b++) {
        const LdsSortBlock m = lds_sort_block(b, W, chunks, false);
        if (!m.valid || m.w >= W || m.chunk >= chunks) return fail("even: pair out of range", W, chunks, b);
        if (owner[m.chunk * W + m.w] != -1) return fail("even: pair owned twice", W, chunks, b);
        owner[m.chunk * W + m.w] = (int)b;
        if (b != m.chunk * W + m.w) return fail("even: not chunk W + w", W, chunks, b);
        const LdsSortBlock l = lds_sort_block(b, W, chunks, true);
        if (W % 8 == 0 && (!l.valid || l.w != m.w || l.chunk != m.chunk)) return fail("the two mappings differ for a multiple of 8", W, chunks, b);
    }
    return 0;
}

static int check_mapping(unsigned W, unsigned chunks) {
    const unsigned grid = lds_sort_grid(W, chunks, true);
    if (grid < W * chunks || grid % 8 != 0) return fail("grid", W, chunks, grid);
    if (W % 8 == 0 && grid != W * chunks) return fail("idle blocks though W is a multiple of 8", W, chunks, grid);
    if (grid - W * chunks >= 8 * chunks) return fail("more than seven windows' worth of idle blocks", W, chunks, grid);
    std::vector<int> owner(W * chunks, -1), label(W, -1), per_label(8, 0);
    unsigned owned = 0;
    for (unsigned b = 0; b < grid; b++) {
        const LdsSortBlock m = lds_sort_block(b, W, chunks, true);
        if (!m.valid) continue;
        if (m.w >= W || m.chunk >= chunks) return fail("pair out of range", W, chunks, b);
        if (owner[m.chunk * W + m.w] != -1) return fail("pair owned twice", W, chunks, b);
        owner[m.chunk * W + m.w] = (int)b;
        if (label[m.w] == -1) { label[m.w] = (int)(b % 8); per_label[b % 8]++; }
        if (label[m.w] != (int)(b % 8)) return fail("chunks of one window on two labels", W, chunks, b);
        if (W % 8 == 0 && b != m.chunk * W + m.w) return fail("not chunk W + w", W, chunks, b);
        owned++;
    }
    if (owned != W * chunks) return fail("pairs without a block", W, chunks, owned);
    int lo = per_label[0], hi = per_label[0];
    for (int x = 1; x < 8; x++) { if (per_label[x] < lo) lo = per_label[x]; if (per_label[x] > hi) hi = per_label[x]; }
    if (hi - lo > 1 || hi != (int)lds_sort_windows_per_label(W)) return fail("windows dealt unevenly over the labels", W, chunks, (unsigned)hi);
    return 0;
}

// the round count: forced values, the caps, and the automatic choice as a function of the bytes a label writes
static int check_rounds() {
    int bad = 0;
    const unsigned B = 1u << 15;
    const long forced[] = {1, 2, 3, 4, 8, 16, 31, 32, 33, 1000};
    const unsigned want[] = {1, 2, 2, 4, 8, 16, 16, 32, 32, 32};
    for (int i = 0; i < 10; i++) bad |= lds_sort_rounds(8, 8, 1, false, B, (size_t)1 << 21, forced[i]) != want[i];
    bad |= lds_sort_rounds(8, 8, 1, false, 4, (size_t)1 << 21, 32) != 4;                      // never more rounds than buckets
    // the automatic choice by the bytes of `sorted` per label: 8 windows of 2^19 .. 2^23 entries
    bad |= lds_sort_rounds(8, 8, 1, false, B, (size_t)1 << 19, 0) != 1;                        // 2 MiB per label: fits
    bad |= lds_sort_rounds(8, 8, 1, false, B, (size_t)1 << 20, 0) != 2;
    bad |= lds_sort_rounds(8, 8, 1, false, B, (size_t)1 << 21, 0) != 4;                        // the headline: 8 MiB in four rounds
    bad |= lds_sort_rounds(8, 8, 1, false, B, (size_t)1 << 23, 0) != 1;                        // 32 MiB: four rounds would not do, a single pass
    bad |= lds_sort_rounds(16, 16, 1, false, B, (size_t)1 << 20, 0) != 4;                      // unsplit: two windows per label
    bad |= lds_sort_rounds(8, 8, 1, false, 2, (size_t)1 << 21, 0) != 1;                        // two buckets cannot make four ranges
    bad |= lds_sort_rounds(15, 15, 1, false, B, (size_t)1 << 21, 0) != 1;                      // folded 17-bit windows: 15, no multiple of 8
    bad |= lds_sort_rounds(17, 17, 1, false, B, (size_t)1 << 19, 0) != 1;
    bad |= lds_sort_rounds(10, 10, 1, false, B, (size_t)1 << 21, 4) != 4;                      // (the option still forces them)
    for (unsigned W = 1; W <= 64; W++)
        for (unsigned lg = 10; lg <= 26; lg++) {
            const size_t n = (size_t)1 << lg;
            // one bucket set per window: ceil(W / 8) slices per label; the shared-set mode: the Wk = W windows of the one vector write one set
            const size_t bytes[2] = {(size_t)lds_sort_windows_per_label(W) * n * 4, (size_t)W * n * 4};
            for (int single = 0; single < 2; single++) {
                const unsigned R = lds_sort_rounds(W, W, 1, single != 0, B, n, 0);
                if (R < 1 || R > LDS_SORT_AUTO_MAX_ROUNDS || (R & (R - 1))) bad = 1;
                if (R > 1 && bytes[single] / R > LDS_SORT_ROUND_BYTES) bad = 1;                 // rounds only where they bring the slice within the budget ...
                if (R > 1 && bytes[single] / (R / 2) <= LDS_SORT_ROUND_BYTES) bad = 1;          // ... and half as many would not
                if (R > 1 && W % 8 != 0) bad = 1;                                               // ... and never for a W that would need the uneven grid
                if (R == 1 && W % 8 == 0 && bytes[single] > LDS_SORT_ROUND_BYTES && bytes[single] / LDS_SORT_AUTO_MAX_ROUNDS <= LDS_SORT_ROUND_BYTES) bad = 1;
            }
        }
    if (bad) printf("lds_sort_map_check: FAILED: round count\n");
    return bad;
}

int main() {
    for (unsigned W = 1; W <= 64; W++)
        for (unsigned chunks = 1; chunks <= 256; chunks++)
            if (check_mapping(W, chunks) || check_even_mapping(W, chunks)) return 1;
    if (check_rounds()) return 1;
    printf("lds_sort_map_check: ok\n");
    return 0;
}
