// CPU test build of the ballot box's rules (vote_saver_protocol_amd/csrc/ballot_box.h: roles, hash, probe sequence, slot encoding, claim
// and find), compiled by g++.  The claim is run one slot operation at a time: a scheduler drawn from a seed picks which lane takes its
// next step, so the lanes' compare-and-swaps and minimums interleave as they may on the device.  Test infrastructure only.  With
// -DBALLOT_BOX_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_ballot_box_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/ballot_box.h"
using namespace vsp;

namespace {

// the table on the host: every operation is one indivisible step of the scheduler
struct HostTable {
    uint64_t *slot;
    uint64_t cas(uint64_t pos, uint64_t expected, uint64_t desired) { const uint64_t was = slot[pos]; if (was == expected) slot[pos] = desired; return was; }
    uint64_t fetch_min(uint64_t pos, uint64_t v) { const uint64_t was = slot[pos]; if (v < was) slot[pos] = v; return was; }
    uint64_t load(uint64_t pos) const { return slot[pos]; }
};

struct XorShift {
    uint64_t x;
    uint64_t operator()() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; }
};

}  // namespace

extern "C" {

uint32_t chk_box_hash(const uint32_t *w, size_t words) { return box_hash(w, words); }
uint64_t chk_box_probe(uint32_t hash, uint64_t step, uint64_t slots) { return box_probe(hash, step, slots); }
uint64_t chk_box_slots_for(unsigned bits, uint64_t held) { return box_slots_for(bits, held); }
int chk_box_fixed_match(const uint32_t *rest, const uint32_t *expected, const uint8_t *role, size_t L) { return box_fixed_match(rest, expected, role, L) ? 1 : 0; }
void chk_box_gather_serial(const uint32_t *rest, const uint8_t *role, size_t L, uint32_t *out) { box_gather_serial(rest, role, L, out); }

// One piece over a table of `slots` slots (table[] as the caller filled it: BOX_EMPTY, committed ordinals into store).  The c lanes with
// skip[k] = 0 claim under the interleaving of `seed`, then every such lane resolves.  win[k]: the value of its slot (all-ones: skipped),
// pos[k]: the slot.  steps_out: slot operations of the longest lane.  Returns the OR of the BOX_ERR bits raised
int chk_box_piece(uint64_t *table, uint64_t slots, const uint32_t *store, const uint32_t *pend, size_t words, const uint8_t *skip, size_t c, uint64_t seed, uint64_t *win,
                  uint64_t *pos, uint64_t *steps_out) {
    HostTable mem{table};
    const BoxKeys keys{store, pend, words};
    std::vector<BoxClaim> lane(c);
    std::vector<uint64_t> taken(c, 0);
    std::vector<size_t> going;
    for (size_t k = 0; k < c; k++) {
        lane[k] = box_claim_start(pend + k * words, words);
        if (!skip[k]) going.push_back(k);
    }
    XorShift rnd{seed * 0x9E3779B97F4A7C15ULL + 0x1234567ULL};
    int flag = 0;
    uint64_t longest = 0;
    while (!going.empty()) {
        const size_t i = (size_t)(rnd() % going.size()), k = going[i];
        const int r = box_claim_step(mem, lane[k], slots, keys, pend + k * words, box_pending(k));
        taken[k]++;
        if (taken[k] > longest) longest = taken[k];
        if (taken[k] > slots + 1) { flag |= 4; break; }               // a lane that outlives the bound: the harness's own alarm
        if (r == BOX_GOING) continue;
        if (r == BOX_OVERRUN) flag |= BOX_ERR_OVERRUN;
        going[i] = going.back(); going.pop_back();
    }
    for (size_t k = 0; k < c; k++) {
        win[k] = BOX_NONE; pos[k] = 0;
        if (skip[k]) continue;
        uint64_t v = 0, at = 0;
        const int r = box_find(mem, slots, keys, pend + k * words, &v, &at);
        if (r == BOX_DONE) { win[k] = v; pos[k] = at; }
        else flag |= r == BOX_OVERRUN ? BOX_ERR_OVERRUN : BOX_ERR_LOST;
    }
    if (steps_out) *steps_out = longest;
    return flag;
}

// the lookup of k_box_screen: 1 and *value when the serial is in the table, 0 when absent, -1 on an overrun
int chk_box_find(const uint64_t *table, uint64_t slots, const uint32_t *store, const uint32_t *pend, size_t words, const uint32_t *mine, uint64_t *value) {
    const HostTable mem{const_cast<uint64_t *>(table)};
    const BoxKeys keys{store, pend, words};
    uint64_t at = 0;
    const int r = box_find(mem, slots, keys, mine, value, &at);
    return r == BOX_DONE ? 1 : (r == BOX_ABSENT ? 0 : -1);
}

// the table of k_box_rebuild: the store's `count` serials claimed in the order of `seed`; returns the BOX_ERR bits
int chk_box_rebuild(uint64_t *table, uint64_t slots, const uint32_t *store, size_t words, uint64_t count, uint64_t seed) {
    HostTable mem{table};
    const BoxKeys keys{store, store, words};
    for (uint64_t i = 0; i < slots; i++) table[i] = BOX_EMPTY;
    std::vector<uint64_t> order(count);
    for (uint64_t o = 0; o < count; o++) order[o] = o;
    XorShift rnd{seed + 88172645463325252ULL};
    for (uint64_t o = count; o > 1; o--) { const uint64_t j = rnd() % o; const uint64_t t = order[o - 1]; order[o - 1] = order[j]; order[j] = t; }
    int flag = 0;
    for (uint64_t o : order)
        if (box_claim(mem, slots, keys, store + o * words, o) != BOX_DONE) flag |= BOX_ERR_OVERRUN;
    return flag;
}
}

#ifdef BALLOT_BOX_CHECK_MAIN
#include <stdio.h>
int main() {
    int bad = 0;
    XorShift rnd{2463534242ULL};
    for (size_t S : {(size_t)1, (size_t)2, (size_t)8}) {
        const size_t words = 8 * S;
        for (unsigned bits = 2; bits <= 4; bits++) {
            const uint64_t slots = (uint64_t)1 << bits;
            const size_t c = (size_t)(slots / 2);                   // exactly half load when all are distinct
            for (int shape = 0; shape < 3; shape++) {
                // shape 0: distinct; 1: every lane the same serial; 2: lanes 0 and c - 1 equal
                std::vector<uint32_t> pend(c * words), store(words, 0);
                for (size_t k = 0; k < c; k++)
                    for (size_t i = 0; i < words; i++) pend[k * words + i] = shape == 1 ? (uint32_t)(7 + i) : (uint32_t)rnd();
                if (shape == 2) memcpy(&pend[(c - 1) * words], &pend[0], words * sizeof(uint32_t));
                for (uint64_t seed = 1; seed <= 16; seed++) {
                    std::vector<uint64_t> table(slots, BOX_EMPTY), win(c), pos(c);
                    std::vector<uint8_t> skip(c, 0);
                    uint64_t steps = 0;
                    bad |= chk_box_piece(table.data(), slots, store.data(), pend.data(), words, skip.data(), c, seed, win.data(), pos.data(), &steps) != 0;
                    for (size_t k = 0; k < c; k++) {
                        size_t first = k;
                        for (size_t j = 0; j < k; j++)
                            if (!memcmp(&pend[j * words], &pend[k * words], words * sizeof(uint32_t))) { first = j; break; }
                        bad |= win[k] != box_pending(first);
                    }
                }
            }
        }
    }
    // a full table of other keys: the claim ends at the bound and says so
    {
        const size_t words = 8;
        const uint64_t slots = 4;
        std::vector<uint32_t> store(slots * words), pend(words, 5);
        for (size_t i = 0; i < store.size(); i++) store[i] = (uint32_t)(i + 100);
        std::vector<uint64_t> table(slots);
        for (uint64_t i = 0; i < slots; i++) table[i] = i;
        uint64_t win = 0, pos = 0, steps = 0;
        const uint8_t skip = 0;
        const int flag = chk_box_piece(table.data(), slots, store.data(), pend.data(), words, &skip, 1, 3, &win, &pos, &steps);
        bad |= flag != BOX_ERR_OVERRUN || steps != slots || win != BOX_NONE;
        uint64_t v = 0;
        bad |= chk_box_find(table.data(), slots, store.data(), pend.data(), words, pend.data(), &v) != -1;
    }
    bad |= box_slots_for(2, 2) != 4 || box_slots_for(2, 3) != 8 || box_slots_for(16, 0) != 65536;
    printf(bad ? "ballot_box_check: FAILED\n" : "ballot_box_check: ok\n");
    return bad;
}
#endif
