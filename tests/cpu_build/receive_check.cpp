// CPU test build of the rules of receiving ballots from their blobs (vote_saver_protocol_amd/csrc/receive.h: the input blob's
// acceptance rule and the index maps between the decoder's ballot-major layout and the verifiers' columns), compiled by g++.  Test
// infrastructure only.  With -DRECEIVE_CHECK_MAIN the file is a program of its own (the sanitizer run of tests/test_receive_cpu.py).
#include <string.h>
#include <vector>
#include "../../vote_saver_protocol_amd/csrc/receive.h"
using namespace vsp;

// what k_receive_prepare does with the points of the range [lo, lo + c) of a decoded piece of pc ballots, on point NUMBERS: the
// decoded piece holds the numbers 0 .. pc (n + 2) - 1 in its members, pc (n + 2) + i in the A / C sets (2 pc of them); out gets the
// (n + 5) c entries of the verifier's piece -- columns 0 .. n + 1, acc (entry -1: computed, not gathered), C, then the c points A.
// Returns 0, or 1 when an index left its array or an entry was written twice
static int gather(size_t pc, size_t n, size_t lo, size_t c, int64_t *out) {
    const size_t total = (n + 5) * c;
    std::vector<int> seen(total, 0);
    int bad = 0;
    auto put = [&](size_t at, int64_t v) { if (at >= total || seen[at]++) bad = 1; else out[at] = v; };
    for (size_t k = 0; k < c; k++) {
        const size_t ballot = lo + k;
        if (recv_a_index(pc, ballot) >= 2 * pc || recv_c_index(pc, ballot) >= 2 * pc) bad = 1;
        put((n + 4) * c + k, (int64_t)(pc * (n + 2) + recv_a_index(pc, ballot)));
        put(recv_column_index(c, n + 3, k), (int64_t)(pc * (n + 2) + recv_c_index(pc, ballot)));
        put(recv_column_index(c, n + 2, k), -1);
        for (size_t j = 0; j < n + 2; j++) {
            if (recv_member_index(n, ballot, j) >= pc * (n + 2)) bad = 1;
            put(recv_column_index(c, j, k), (int64_t)recv_member_index(n, ballot, j));
        }
    }
    for (size_t i = 0; i < total; i++) if (!seen[i]) bad = 1;
    return bad;
}

extern "C" {
// the status byte of one input blob and its scalars as 8 little-endian 32-bit words each (out may be null)
int chk_input_blob(const uint8_t *blob, size_t n_rest, uint32_t *out) { return recv_input_blob_status(blob, n_rest, out); }
size_t chk_input_blob_bytes(size_t n_rest) { return recv_input_blob_bytes(n_rest); }
int chk_gather(size_t pc, size_t n, size_t lo, size_t c, int64_t *out) { return gather(pc, n, lo, c, out); }
size_t chk_wire_stride(size_t pc) { return recv_wire_stride(pc); }
size_t chk_scalar_lanes(size_t n_rest) { return recv_scalar_lanes(n_rest); }
}

#ifdef RECEIVE_CHECK_MAIN
#include <stdio.h>
static void be32(uint8_t *o, const uint32_t w[8]) { for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) o[4 * (7 - i) + (3 - b)] = (uint8_t)(w[i] >> (8 * b)); }
int main() {
    const uint32_t r[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};
    uint32_t r1[8], ones[8], out[16];
    memcpy(r1, r, sizeof r); r1[0] = 0;
    for (uint32_t &w : ones) w = 0xffffffffu;
    int bad = 0;
    alignas(8) uint8_t blob[8 + 64] = {0};
    blob[7] = 2;
    be32(blob + 8, r1); be32(blob + 40, r1);
    bad |= recv_input_blob_status(blob, 2, out) != 0 || memcmp(out, r1, sizeof r1) != 0 || memcmp(out + 8, r1, sizeof r1) != 0;
    be32(blob + 40, r);
    bad |= recv_input_blob_status(blob, 2, out) != 1;
    be32(blob + 40, ones);
    bad |= recv_input_blob_status(blob, 2, nullptr) != 1;
    be32(blob + 40, r1);
    blob[7] = 1;
    bad |= recv_input_blob_status(blob, 2, nullptr) != 1;
    blob[7] = 2; blob[0] = 1;
    bad |= recv_input_blob_status(blob, 2, nullptr) != 1;
    blob[0] = 0; blob[7] = 0;
    bad |= recv_input_blob_status(blob, 0, nullptr) != 0;
    const size_t shapes[][4] = {{1, 1, 0, 1}, {63, 2, 0, 63}, {64, 1, 0, 64}, {65, 2, 0, 65}, {130, 2, 33, 64}, {130, 1, 129, 1}, {65, 25, 17, 48}};
    for (auto &s : shapes) {
        std::vector<int64_t> v((s[1] + 5) * s[3]);
        bad |= gather(s[0], s[1], s[2], s[3], v.data());
    }
    bad |= recv_wire_stride(1) != 4 || recv_wire_stride(64) != 64 || recv_wire_stride(65) != 68;
    printf(bad ? "receive_check: FAILED\n" : "receive_check: ok\n");
    return bad;
}
#endif
