// The rules of the ballot box (ballot_box.hip; include/vsp.h "the ballot box") that a CPU can check: the roles of the
// rest inputs, the hash of a serial's words, the probe sequence, the slot encoding, and the claim and find steps over the
// open-addressing table.  Shared by the gfx950 kernels and, through g++, by the CPU test build (tests/cpu_build/ballot_box_check.cpp),
// which runs the claim one slot operation at a time under random interleavings of the lanes.  No field arithmetic: plain words.
//
// A SERIAL is the SERIAL rest inputs of a ballot concatenated in order: S scalars of 8 canonical 32-bit words.  The box keeps the
// serials of the accepted ballots in ordinal order (the STORE) and a table of 64-bit slots over them.  During a piece the serials of
// its ballots lie in a second array (the PENDING serials, by index in the piece).  A slot names the serial it holds:
//   BOX_EMPTY              nothing
//   o < 2^63               the committed serial of ordinal o             (store + o words)
//   BOX_PENDING | k        the pending serial of ballot k of the piece   (pend + k words)
// The key of a slot never changes once the slot is not empty; among pending ballots of one key the value only ever falls (lowest
// index wins), and a committed ordinal is below every pending value, so one unsigned minimum serves both.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSP_BOX_HD __host__ __device__ __forceinline__
#else
#define VSP_BOX_HD inline
#endif

namespace vsp {

enum { BOX_FREE = 0, BOX_FIXED = 1, BOX_SERIAL = 2 };               // role bytes
static constexpr size_t BOX_MAX_SERIAL = 8;                         // SERIAL inputs of a ballot, at most
static constexpr unsigned BOX_MIN_BITS = 2, BOX_MAX_BITS = 30, BOX_DEFAULT_BITS = 16;      // option "ballot_box_table_bits"
static constexpr uint64_t BOX_EMPTY = ~(uint64_t)0, BOX_PENDING = (uint64_t)1 << 63, BOX_NONE = ~(uint64_t)0;
enum { BOX_GOING = 0, BOX_DONE = 1, BOX_OVERRUN = 2, BOX_ABSENT = 3 };
// the skip byte of a ballot behind the verdicts: 0 accepted so far (claims its serial), 1 out (wire-rejected, turned away by the box, or
// -- set by the resolve step -- its serial is held by an earlier ballot), 2 refused by the verifier (claims nothing; the resolve step
// still reads whether an accepted ballot of lower index holds its serial, so that the holder it reports does not depend on the pieces).
// The tally's sum leaves out every ballot whose byte is not zero
enum { BOX_SKIP_NONE = 0, BOX_SKIP_OUT = 1, BOX_SKIP_REFUSED = 2 };
// bits of the device-side error word
enum { BOX_ERR_OVERRUN = 1, BOX_ERR_LOST = 2 };

// ---- the roles: FIXED inputs must equal the box's, SERIAL inputs make the serial.  rest: L x 8 words of one ballot
VSP_BOX_HD bool box_fixed_match(const uint32_t *rest, const uint32_t *expected, const uint8_t *role, size_t L) {
    uint32_t diff = 0;
    for (size_t i = 0; i < L; i++) {
        if (role[i] != BOX_FIXED) continue;
        for (int j = 0; j < 8; j++) diff |= rest[8 * i + j] ^ expected[8 * i + j];
    }
    return diff == 0;
}
VSP_BOX_HD void box_gather_serial(const uint32_t *rest, const uint8_t *role, size_t L, uint32_t *out) {
    size_t at = 0;
    for (size_t i = 0; i < L; i++) {
        if (role[i] != BOX_SERIAL) continue;
        for (int j = 0; j < 8; j++) out[at + j] = rest[8 * i + j];
        at += 8;
    }
}

// ---- the hash: a fixed mix of the serial's words (the 32-bit finalizer of MurmurHash3 around a multiply-rotate per word).  Fixed,
// not keyed: only serials of verified ballots are ever inserted
VSP_BOX_HD uint32_t box_hash(const uint32_t *w, size_t words) {
    uint32_t h = 0x9e3779b9u ^ (uint32_t)words;
    for (size_t i = 0; i < words; i++) {
        uint32_t k = w[i] * 0xcc9e2d51u;
        k = (k << 15) | (k >> 17);
        h ^= k * 0x1b873593u;
        h = ((h << 13) | (h >> 19)) * 5u + 0xe6546b64u;
    }
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
// linear probing: step s of a key looks at slot (hash + s) mod slots; slots is a power of two
VSP_BOX_HD uint64_t box_probe(uint32_t hash, uint64_t step, uint64_t slots) { return ((uint64_t)hash + step) & (slots - 1); }
// the smallest table of at least 2^bits slots that `held` serials leave at most half full
VSP_BOX_HD uint64_t box_slots_for(unsigned bits, uint64_t held) {
    uint64_t slots = (uint64_t)1 << bits;
    while (2 * held > slots) slots <<= 1;
    return slots;
}

// ---- slots and keys
VSP_BOX_HD uint64_t box_pending(uint64_t k) { return BOX_PENDING | k; }
VSP_BOX_HD bool box_is_pending(uint64_t v) { return v != BOX_EMPTY && (v & BOX_PENDING) != 0; }
struct BoxKeys {
    const uint32_t *store, *pend;                                   // the committed and the pending serials
    size_t words;                                                   // 8 S
};
VSP_BOX_HD const uint32_t *box_key(const BoxKeys &keys, uint64_t v) {
    return box_is_pending(v) ? keys.pend + (v & ~BOX_PENDING) * keys.words : keys.store + v * keys.words;
}
VSP_BOX_HD bool box_key_equal(const uint32_t *a, const uint32_t *b, size_t words) {
    uint32_t diff = 0;
    for (size_t i = 0; i < words; i++) diff |= a[i] ^ b[i];
    return diff == 0;
}

// ---- the claim of one lane, one slot operation per step.  Mem is the table: cas(pos, expected, desired) and fetch_min(pos, v), both
// atomic and returning the slot's earlier value.  The lane offers the value `me` (a pending index, or when the table is rebuilt a
// committed ordinal) for the key `mine`:
//   step      cas(slot, EMPTY, me): an empty slot is taken; a slot of an equal key goes to the minimum step; another key: next slot
//   minimum   fetch_min(slot, me)
// After `slots` probes without an end the step answers BOX_OVERRUN: no path loops on a full or damaged table.
struct BoxClaim {
    uint32_t hash;
    uint64_t step;                                                  // probes made so far
    int settle;                                                     // 1: the slot at `step` holds an equal key; the minimum is due
};
VSP_BOX_HD BoxClaim box_claim_start(const uint32_t *mine, size_t words) { BoxClaim c; c.hash = box_hash(mine, words); c.step = 0; c.settle = 0; return c; }
template <class Mem> VSP_BOX_HD int box_claim_step(Mem &mem, BoxClaim &c, uint64_t slots, const BoxKeys &keys, const uint32_t *mine, uint64_t me) {
    if (c.step >= slots) return BOX_OVERRUN;
    const uint64_t pos = box_probe(c.hash, c.step, slots);
    if (c.settle) { mem.fetch_min(pos, me); return BOX_DONE; }
    const uint64_t was = mem.cas(pos, BOX_EMPTY, me);
    if (was == BOX_EMPTY) return BOX_DONE;
    if (box_key_equal(box_key(keys, was), mine, keys.words)) { c.settle = 1; return BOX_GOING; }
    c.step++;
    return c.step >= slots ? BOX_OVERRUN : BOX_GOING;
}
// the whole claim of a lane: at most slots + 1 steps
template <class Mem> VSP_BOX_HD int box_claim(Mem &mem, uint64_t slots, const BoxKeys &keys, const uint32_t *mine, uint64_t me) {
    BoxClaim c = box_claim_start(mine, keys.words);
    int r;
    do r = box_claim_step(mem, c, slots, keys, mine, me); while (r == BOX_GOING);
    return r;
}

// ---- find: the slot that holds the key `mine`, over a table nobody writes.  Mem: load(pos).  BOX_DONE with the slot's value and
// position, BOX_ABSENT at the first empty slot of the chain, BOX_OVERRUN after `slots` probes
template <class Mem> VSP_BOX_HD int box_find(const Mem &mem, uint64_t slots, const BoxKeys &keys, const uint32_t *mine, uint64_t *value, uint64_t *at) {
    const uint32_t hash = box_hash(mine, keys.words);
    for (uint64_t step = 0; step < slots; step++) {
        const uint64_t pos = box_probe(hash, step, slots), v = mem.load(pos);
        if (v == BOX_EMPTY) return BOX_ABSENT;
        if (box_key_equal(box_key(keys, v), mine, keys.words)) { *value = v; *at = pos; return BOX_DONE; }
    }
    return BOX_OVERRUN;
}

}  // namespace vsp
