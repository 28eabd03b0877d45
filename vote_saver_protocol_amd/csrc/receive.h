// The rules of receiving ballots from their blobs (receive.hip; include/vsp.h "ballots received from their blobs")
// that a CPU can check: which input blob k_receive_scalars accepts, and where k_receive_prepare finds and puts the points of a
// ballot.  Shared by the gfx950 kernels and, through g++, by the CPU test build (tests/cpu_build/receive_check.cpp).  No field
// arithmetic: plain words.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VSP_RECV_HD __host__ __device__ __forceinline__
#else
#define VSP_RECV_HD inline
#endif

namespace vsp {

// ---- the input blob of a ballot: a scalar vector as vsp_fr_vector_to_blob writes it for n_rest scalars -- an 8-byte big-endian
// count, then 32 big-endian bytes per scalar.  The blob is read as 32-bit words of a little-endian machine (every blob starts at a
// multiple of 8 bytes of a buffer whose stride, 8 + 32 n_rest, is one too).
VSP_RECV_HD size_t recv_input_blob_bytes(size_t n_rest) { return 8 + 32 * n_rest; }
VSP_RECV_HD uint32_t recv_bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// the count header (two words as loaded) names exactly n_rest scalars
VSP_RECV_HD bool recv_header_ok(uint32_t w0, uint32_t w1, size_t n_rest) {
    return (((uint64_t)recv_bswap32(w0) << 32) | recv_bswap32(w1)) == (uint64_t)n_rest;
}
// the 8 words of a scalar as loaded -> its canonical little-endian 32-bit words (the layout k_ballot_prepare reads its `rest` from);
// true when the scalar is below r = 0x73eda753299d7d48 3339d80809a1d805 53bda402fffe5bfe ffffffff00000001
VSP_RECV_HD bool recv_scalar_decode(const uint32_t *be, uint32_t out[8]) {
    const uint32_t r[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    for (int i = 0; i < 8; i++) out[i] = recv_bswap32(be[7 - i]);
    bool lt = false, gt = false;
    for (int i = 7; i >= 0; i--) {
        lt = lt || (!gt && out[i] < r[i]);
        gt = gt || (!lt && out[i] > r[i]);
    }
    return lt;
}
// the whole rule on the host, as the lanes of k_receive_scalars apply it together: 0 accepted, 1 a wrong count or a scalar >= r
// (wire_status_out[3k + 2]).  out: n_rest x 8 words, or null
inline uint8_t recv_input_blob_status(const uint8_t *blob, size_t n_rest, uint32_t *out) {
    const uint32_t *w = (const uint32_t *)blob;
    uint8_t st = recv_header_ok(w[0], w[1], n_rest) ? 0 : 1;
    for (size_t i = 0; i < n_rest; i++) {
        uint32_t s[8];
        if (!recv_scalar_decode(w + 2 + 8 * i, s)) st = 1;
        if (out) for (int j = 0; j < 8; j++) out[8 * i + j] = s[j];
    }
    return st;
}

// ---- the two layouts of a piece.  The decoder leaves the n + 2 ciphertext members of the pc ballots of a piece ballot-major; a
// verifier's piece of c ballots -- the range [lo, lo + c) of the decoded piece -- wants them column by column, argument j of ballot k
// at pts[j c + k], followed by the columns acc (n + 2) and C (n + 3), then the c points A: (n + 5) c points in all.
VSP_RECV_HD size_t recv_member_index(size_t n, size_t ballot, size_t j) { return ballot * (n + 2) + j; }     // ballot: index in the decoded piece
VSP_RECV_HD size_t recv_column_index(size_t c, size_t j, size_t k) { return j * c + k; }                      // k: index in the range
VSP_RECV_HD size_t recv_a_index(size_t pc, size_t ballot) { (void)pc; return ballot; }                        // A and C of the proofs: two sets of pc
VSP_RECV_HD size_t recv_c_index(size_t pc, size_t ballot) { return pc + ballot; }
// lanes of k_receive_scalars for a piece: one per (ballot, scalar), and one per ballot where there are no scalars (the header alone)
VSP_RECV_HD size_t recv_scalar_lanes(size_t n_rest) { return n_rest ? n_rest : 1; }
// the wire status bytes of a piece of pc ballots: three arrays of a stride that keeps each 4-byte aligned (the lanes of a ballot OR
// into its byte through the 32-bit word that holds it)
VSP_RECV_HD size_t recv_wire_stride(size_t pc) { return (pc + 3) & ~(size_t)3; }

}  // namespace vsp
