// The ballot box (include/vsp.h "the ballot box"): which serial numbers are spent, and whether a ballot belongs to this
// election (eid) and this voter list (rt), decided on the device beside the decoded rest inputs.  The rules -- roles, hash, probe
// sequence, slot encoding, claim and find -- are ballot_box.h, which the CPU test build runs too.  Kernels, one lane per ballot:
//   k_box_screen   before the verifier: the FIXED inputs against the box's, the serial gathered into the piece's pending serials and
//                  looked up among the committed ones; a status byte (0 | 8 | 16) and the holder's ordinal
//   k_box_claim    after the verdicts: every accepted ballot claims the slot of its serial -- a compare-and-swap on the empty slot, an
//                  unsigned minimum on a slot of an equal key: among equal serials of the piece the lowest index wins
//   k_box_resolve  every accepted ballot reads who holds its slot; a loser raises its skip byte for the tally
//   k_box_commit   the winners' serials go to the store at their ordinals (index order: the host's prefix count over the verdict bytes it
//                  already holds) and their slots from the pending index to the ordinal
//   k_box_rebuild  the table from the store: growth, and the way back after an error
// Every probe loop ends after as many steps as the table has slots and raises the error word; the host turns it into VSP_ERR_HIP.
// The slots are touched by atomic read-modify-write operations alone inside k_box_claim and k_box_rebuild (agent scope: the value a lane
// gets back is the slot's, whichever compute die the other lanes run on); the kernels before and after read them with plain loads,
// across a kernel boundary.  The serials a slot's value points to are written by earlier kernels and read-only here.
#include "common.h"
#include "ballot_box.h"

namespace vsp {

static constexpr unsigned BOX_THREADS = 256;
static constexpr size_t BOX_ADD_PIECE = (size_t)1 << 16;            // serials of one piece of vsp_ballot_box_add_serials

namespace {

struct BoxDeviceTable {
    uint64_t *slot;
    __device__ __forceinline__ uint64_t cas(uint64_t pos, uint64_t expected, uint64_t desired) {
        __hip_atomic_compare_exchange_strong(slot + pos, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;
    }
    __device__ __forceinline__ uint64_t fetch_min(uint64_t pos, uint64_t v) { return __hip_atomic_fetch_min(slot + pos, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ uint64_t load(uint64_t pos) const { return slot[pos]; }
};

__device__ __forceinline__ void box_raise(uint32_t *flag, uint32_t bits) { atomicOr(flag, bits); }

__global__ __launch_bounds__(BOX_THREADS) void k_box_screen(const uint32_t *__restrict__ rest, size_t c, size_t L, const uint8_t *__restrict__ role,
                                                            const uint32_t *__restrict__ expected, uint64_t *table, uint64_t slots, const uint32_t *__restrict__ store,
                                                            size_t words, uint32_t *__restrict__ pend, uint8_t *__restrict__ row, uint64_t *__restrict__ hold, uint32_t *flag) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const uint32_t *mine = rest + k * L * 8;
    uint32_t *serial = pend + k * words;
    box_gather_serial(mine, role, L, serial);
    uint8_t st = 0;
    uint64_t holder = BOX_NONE;
    if (!box_fixed_match(mine, expected, role, L)) st = 8;
    else {
        const BoxDeviceTable mem{table};
        const BoxKeys keys{store, pend, words};
        uint64_t v = 0, at = 0;
        const int r = box_find(mem, slots, keys, serial, &v, &at);
        if (r == BOX_DONE) { st = 16; holder = v; }
        else if (r == BOX_OVERRUN) box_raise(flag, BOX_ERR_OVERRUN);
    }
    row[k] = st;
    hold[k] = holder;
}

__global__ __launch_bounds__(BOX_THREADS) void k_box_claim(const uint8_t *__restrict__ skip, size_t c, uint64_t *table, uint64_t slots, const uint32_t *__restrict__ store,
                                                           const uint32_t *__restrict__ pend, size_t words, uint32_t *flag) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c || skip[k]) return;
    BoxDeviceTable mem{table};
    const BoxKeys keys{store, pend, words};
    if (box_claim(mem, slots, keys, pend + k * words, box_pending(k)) != BOX_DONE) box_raise(flag, BOX_ERR_OVERRUN);
}

__global__ __launch_bounds__(BOX_THREADS) void k_box_resolve(uint8_t *__restrict__ skip, size_t c, uint64_t *table, uint64_t slots, const uint32_t *__restrict__ store,
                                                             const uint32_t *__restrict__ pend, size_t words, uint64_t *__restrict__ win, uint64_t *__restrict__ pos,
                                                             uint32_t *flag) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    uint64_t v = BOX_NONE, at = 0;
    const uint8_t s = skip[k];
    if (s == BOX_SKIP_NONE || s == BOX_SKIP_REFUSED) {
        const BoxDeviceTable mem{table};
        const BoxKeys keys{store, pend, words};
        const int r = box_find(mem, slots, keys, pend + k * words, &v, &at);
        if (r == BOX_OVERRUN) { box_raise(flag, BOX_ERR_OVERRUN); v = BOX_NONE; }
        else if (r == BOX_ABSENT) { if (s == BOX_SKIP_NONE) box_raise(flag, BOX_ERR_LOST); v = BOX_NONE; }      // a claimed serial is in the table
        else if (s == BOX_SKIP_NONE) { if (v != box_pending(k)) skip[k] = BOX_SKIP_OUT; }                       // an earlier ballot holds the serial
        else if (box_is_pending(v) && (v & ~BOX_PENDING) > k) v = BOX_NONE;                                      // held by a later ballot only
    }
    win[k] = v;
    pos[k] = at;
}

__global__ __launch_bounds__(BOX_THREADS) void k_box_commit(const uint64_t *__restrict__ ord, const uint64_t *__restrict__ pos, size_t c, uint64_t *__restrict__ table,
                                                            uint64_t slots, uint32_t *__restrict__ store, const uint32_t *__restrict__ pend, size_t words) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= c) return;
    const uint64_t o = ord[k];
    if (o == BOX_NONE || pos[k] >= slots) return;
    for (size_t i = 0; i < words; i++) store[o * words + i] = pend[k * words + i];
    table[pos[k]] = o;
}

__global__ __launch_bounds__(BOX_THREADS) void k_box_rebuild(uint64_t count, uint64_t *table, uint64_t slots, const uint32_t *__restrict__ store, size_t words, uint32_t *flag) {
    const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= count) return;
    BoxDeviceTable mem{table};
    const BoxKeys keys{store, store, words};
    if (box_claim(mem, slots, keys, store + o * words, o) != BOX_DONE) box_raise(flag, BOX_ERR_OVERRUN);
}

unsigned box_blocks(size_t lanes) { return (unsigned)((lanes + BOX_THREADS - 1) / BOX_THREADS); }

// b holds at least `bytes`, its first `keep` bytes as they were
int box_grow_buf(vsp_ctx *ctx, DevBuf &b, size_t bytes, size_t keep) {
    if (b.p && b.cap >= bytes) return VSP_OK;
    size_t want = b.cap * 2 > bytes ? b.cap * 2 : bytes;
    if (want < 4096) want = 4096;
    DevBuf grown;
    if (grown.alloc(want) != hipSuccess) return set_error(ctx, VSP_ERR_NOMEM, "ballot_box: hipMalloc failed");
    if (b.p && keep) {
        hipError_t e = hipMemcpyAsync(grown.p, b.p, keep, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return set_hip_error(ctx, e, "ballot_box: copy of the serial store", __FILE__, __LINE__);
    } else if (b.p) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return set_hip_error(ctx, e, "ballot_box: hipStreamSynchronize", __FILE__, __LINE__);
    }
    b = std::move(grown);                   // behind the wait: the smaller buffer goes
    return VSP_OK;
}

// a table of `slots` slots holding exactly the store's serials; waits for the stream and reads the error word
int box_build_table(vsp_ctx *ctx, vsp_ballot_box *box, uint64_t slots) {
    hipStream_t st = ctx->stream;
    VSP_TRY(box_grow_buf(ctx, box->table, slots * sizeof(uint64_t), 0));
    VSP_HIP(hipMemsetAsync(box->table.p, 0xff, slots * sizeof(uint64_t), st));
    VSP_HIP(hipMemsetAsync(box->flag.p, 0, sizeof(uint32_t), st));
    box->slots = slots;
    if (box->count) {
        hipLaunchKernelGGL(k_box_rebuild, dim3(box_blocks(box->count)), dim3(BOX_THREADS), 0, st, box->count, (uint64_t *)box->table.p, slots, (const uint32_t *)box->store.p,
                           box->words, (uint32_t *)box->flag.p);
        VSP_LAUNCH_CHECK();
    }
    VSP_HIP(hipMemcpyAsync(box->h_flag, box->flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipStreamSynchronize(st));
    if (box->h_flag[0]) return set_error(ctx, VSP_ERR_HIP, "ballot_box: rebuilding the table ran a probe chain through every slot (the box's table or store is damaged)");
    return VSP_OK;
}

int box_flag_error(vsp_ctx *ctx, uint32_t flag) {
    if (flag & BOX_ERR_LOST) return set_error(ctx, VSP_ERR_HIP, "ballot_box: a claimed serial was not found in the table again (the box's table is damaged)");
    return set_error(ctx, VSP_ERR_HIP, "ballot_box: a probe chain ran through every slot of the table (the box's table is full or damaged)");
}

}  // anonymous namespace

int box_restore(vsp_ctx *ctx, vsp_ballot_box *box) {
    VSP_TRY(box_build_table(ctx, box, box->slots));
    box->dirty = false;
    return VSP_OK;
}

int box_piece_screen(vsp_ctx *ctx, vsp_ballot_box *box, const uint32_t *d_rest, size_t c, uint8_t *d_row) {
    hipStream_t st = ctx->stream;
    if (box->dirty) VSP_TRY(box_restore(ctx, box));
    VSP_TRY(ensure(ctx, box->pend, c * box->words * sizeof(uint32_t)));
    VSP_TRY(ensure(ctx, box->hold, c * sizeof(uint64_t)));
    VSP_HIP(hipMemsetAsync(box->flag.p, 0, sizeof(uint32_t), st));
    VSP_TRY(box->timer[0].mark(ctx, 0, st));
    hipLaunchKernelGGL(k_box_screen, dim3(box_blocks(c)), dim3(BOX_THREADS), 0, st, d_rest, c, box->L, (const uint8_t *)box->d_role.p, (const uint32_t *)box->d_expected.p,
                       (uint64_t *)box->table.p, box->slots, (const uint32_t *)box->store.p, box->words, (uint32_t *)box->pend.p, d_row, (uint64_t *)box->hold.p,
                       (uint32_t *)box->flag.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(box->timer[0].mark(ctx, 1, st));
    box->h_hold.resize(c);
    VSP_HIP(hipMemcpyAsync(box->h_hold.data(), box->hold.p, c * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipMemcpyAsync(box->h_flag + 1, box->flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return VSP_OK;
}

int box_piece_settle(vsp_ctx *ctx, vsp_ballot_box *box, size_t c, uint8_t *d_skip) {
    hipStream_t st = ctx->stream;
    if (box->h_flag[1]) return box_flag_error(ctx, box->h_flag[1]);  // the screening's (the caller has waited for it)
    const size_t serial_bytes = box->words * sizeof(uint32_t);
    VSP_TRY(box_grow_buf(ctx, box->store, (box->count + c) * serial_bytes, box->count * serial_bytes));
    VSP_TRY(ensure(ctx, box->win, c * sizeof(uint64_t)));
    VSP_TRY(ensure(ctx, box->pos, c * sizeof(uint64_t)));
    VSP_TRY(ensure(ctx, box->ord, c * sizeof(uint64_t)));
    VSP_TRY(box->timer[1].mark(ctx, 0, st));
    const uint64_t want = box_slots_for(ceil_log2(box->slots), box->count + c);
    if (want > box->slots) {
        VSP_TRY(box_build_table(ctx, box, want));
        ctx->stats["ballot_box_grown"] += 1.0;
    }
    box->dirty = true;
    VSP_HIP(hipMemsetAsync(box->flag.p, 0, sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_box_claim, dim3(box_blocks(c)), dim3(BOX_THREADS), 0, st, (const uint8_t *)d_skip, c, (uint64_t *)box->table.p, box->slots,
                       (const uint32_t *)box->store.p, (const uint32_t *)box->pend.p, box->words, (uint32_t *)box->flag.p);
    VSP_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_box_resolve, dim3(box_blocks(c)), dim3(BOX_THREADS), 0, st, d_skip, c, (uint64_t *)box->table.p, box->slots, (const uint32_t *)box->store.p,
                       (const uint32_t *)box->pend.p, box->words, (uint64_t *)box->win.p, (uint64_t *)box->pos.p, (uint32_t *)box->flag.p);
    VSP_LAUNCH_CHECK();
    VSP_TRY(box->timer[1].mark(ctx, 1, st));
    box->h_win.resize(c);
    VSP_HIP(hipMemcpyAsync(box->h_win.data(), box->win.p, c * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VSP_HIP(hipMemcpyAsync(box->h_flag, box->flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    return VSP_OK;
}

int box_piece_commit(vsp_ctx *ctx, vsp_ballot_box *box, size_t c, uint8_t *verdict, uint8_t *reason, uint64_t *holder, bool as_status, size_t *accepted_out) {
    hipStream_t st = ctx->stream;
    if (box->h_flag[0]) return box_flag_error(ctx, box->h_flag[0]);
    box->h_ord.assign(c, BOX_NONE);
    uint64_t next = box->count;
    size_t lost = 0;
    for (size_t k = 0; k < c; k++) {
        const uint64_t v = box->h_win[k];
        const bool refused = !as_status && verdict[k] == 0;          // by the verifier (or out before it: then v is BOX_NONE)
        if (as_status) verdict[k] = 0;
        if (v == BOX_NONE) continue;
        if (!refused && v == box_pending(k)) { box->h_ord[k] = next++; continue; }
        // held: by a committed ordinal, or by a winner of lower index in this piece
        uint64_t by = v;
        if (box_is_pending(v)) {
            const uint64_t j = v & ~BOX_PENDING;
            if (j >= k || box->h_ord[j] == BOX_NONE) return set_error(ctx, VSP_ERR_HIP, "ballot_box: a slot names a holder that did not win it (the box's table is damaged)");
            by = box->h_ord[j];
        }
        if (refused) { if (holder) holder[k] = by; continue; }      // the verifier's reason stands
        if (as_status) verdict[k] = 1;
        else { verdict[k] = 0; if (reason) reason[k] = 16; }
        if (holder) holder[k] = by;
        lost++;
    }
    VSP_HIP(hipMemcpyAsync(box->ord.p, box->h_ord.data(), c * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    VSP_TRY(box->timer[1].mark(ctx, 2, st));
    hipLaunchKernelGGL(k_box_commit, dim3(box_blocks(c)), dim3(BOX_THREADS), 0, st, (const uint64_t *)box->ord.p, (const uint64_t *)box->pos.p, c, (uint64_t *)box->table.p,
                       box->slots, (uint32_t *)box->store.p, (const uint32_t *)box->pend.p, box->words);
    VSP_LAUNCH_CHECK();
    VSP_TRY(box->timer[1].mark(ctx, 3, st));
    VSP_HIP(hipStreamSynchronize(st));
    // the piece is in the box
    *accepted_out = (size_t)(next - box->count);
    box->count = next;
    box->dirty = false;
    if (!as_status) ctx->stats["ballot_box_spent"] += (double)lost;
    return VSP_OK;
}

void box_add_times(vsp_ctx *ctx, vsp_ballot_box *box, bool screen, bool settle) {
    if (screen) box->timer[0].add(ctx, 0, "ballot_box_ms");
    if (settle) { box->timer[1].add(ctx, 0, "ballot_box_ms"); box->timer[1].add(ctx, 2, "ballot_box_ms"); }
}

}  // namespace vsp

using namespace vsp;

extern "C" {

vsp_ballot_box *vsp_ballot_box_create(vsp_ctx *ctx, const vsp_saver_verifier *ver, const uint64_t *expected, const uint8_t *role, size_t n_rest) {
    if (!ctx) return nullptr;
    auto fail = [&](int code, const char *msg) -> vsp_ballot_box * { set_error(ctx, code, msg); return nullptr; };
    if (!ver || !expected || !role) return fail(VSP_ERR_ARG, "ballot_box_create: null argument");
    if (n_rest == 0 || n_rest != saver_verifier_n_rest(ver)) return fail(VSP_ERR_ARG, "ballot_box_create: n_rest is zero or not the verifier's count of rest inputs");
    if (ver->device != ctx->device) return fail(VSP_ERR_ARG, "ballot_box_create: the verifier belongs to another device");
    size_t S = 0;
    for (size_t i = 0; i < n_rest; i++) {
        if (role[i] > BOX_SERIAL) return fail(VSP_ERR_ARG, "ballot_box_create: a role above 2");
        if (role[i] == BOX_SERIAL) S++;
        if (role[i] == BOX_FIXED && !below_mod<FrP64>(expected + 4 * i)) return fail(VSP_ERR_ARG, "ballot_box_create: a FIXED scalar is not below r");
    }
    if (S < 1 || S > BOX_MAX_SERIAL) return fail(VSP_ERR_ARG, "ballot_box_create: 1 to 8 SERIAL inputs expected");
    const long bv = opt(ctx, "ballot_box_table_bits", (long)BOX_DEFAULT_BITS);
    const unsigned bits = bv < (long)BOX_MIN_BITS ? BOX_MIN_BITS : (bv > (long)BOX_MAX_BITS ? BOX_MAX_BITS : (unsigned)bv);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(VSP_ERR_HIP, "ballot_box_create: hipSetDevice failed");
    vsp_ballot_box *box = new vsp_ballot_box();
    box->device = ctx->device; box->ver = ver; box->L = n_rest; box->S = S; box->words = 8 * S;
    box->role.assign(role, role + n_rest);
    // the FIXED values as the decoded rest inputs lie: 8 x 32-bit words per scalar (the same bytes as 4 little-endian 64-bit words)
    auto setup = [&]() -> int {
        VSP_TRY(ensure(ctx, box->d_role, n_rest));
        VSP_TRY(ensure(ctx, box->d_expected, n_rest * 32));
        VSP_TRY(ensure(ctx, box->flag, 16));
        VSP_TRY(ensure(ctx, box->store, 4096));
        VSP_HIP(hipMemcpyAsync(box->d_role.p, box->role.data(), n_rest, hipMemcpyHostToDevice, ctx->stream));
        VSP_HIP(hipMemcpyAsync(box->d_expected.p, expected, n_rest * 32, hipMemcpyHostToDevice, ctx->stream));
        return box_build_table(ctx, box, (uint64_t)1 << bits);
    };
    if (setup() != VSP_OK) { vsp_ballot_box_free(ctx, box); return nullptr; }
    return box;
}

void vsp_ballot_box_free(vsp_ctx *ctx, vsp_ballot_box *box) {
    if (!box) return;
    hipSetDevice(box->device);
    if (ctx) hipStreamSynchronize(ctx->stream);
    delete box;
}

uint64_t vsp_ballot_box_count(const vsp_ballot_box *box) { return box ? box->count : 0; }
size_t vsp_ballot_box_serial_scalars(const vsp_ballot_box *box) { return box ? box->S : 0; }
size_t vsp_ballot_box_device_bytes(const vsp_ballot_box *box) {
    if (!box) return 0;
    size_t total = 0;
    for (const DevBuf *b : {&box->d_role, &box->d_expected, &box->store, &box->table, &box->pend, &box->hold, &box->win, &box->pos, &box->ord, &box->flag}) total += b->cap;
    return total;
}

int vsp_ballot_box_serials(vsp_ctx *ctx, const vsp_ballot_box *box, uint64_t first, size_t count, uint64_t *out) {
    if (!ctx) return VSP_ERR_ARG;
    if (!box || (!out && count)) return set_error(ctx, VSP_ERR_ARG, "ballot_box_serials: null argument");
    if (box->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "ballot_box_serials: the box belongs to another device");
    if (first > box->count || count > box->count - first) return set_error(ctx, VSP_ERR_ARG, "ballot_box_serials: a range outside the box");
    if (!count) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    const size_t serial_bytes = box->words * sizeof(uint32_t);
    VSP_HIP(hipMemcpyAsync(out, (const uint8_t *)box->store.p + first * serial_bytes, count * serial_bytes, hipMemcpyDeviceToHost, ctx->stream));
    VSP_HIP(hipStreamSynchronize(ctx->stream));
    return VSP_OK;
}

int vsp_ballot_box_add_serials(vsp_ctx *ctx, vsp_ballot_box *box, const uint64_t *serials, size_t count, uint8_t *status_out, size_t *added_out) {
    if (!ctx) return VSP_ERR_ARG;
    if (added_out) *added_out = 0;
    if (!box || (!serials && count)) return set_error(ctx, VSP_ERR_ARG, "ballot_box_add_serials: null argument");
    if (box->device != ctx->device) return set_error(ctx, VSP_ERR_ARG, "ballot_box_add_serials: the box belongs to another device");
    for (size_t i = 0; i < count * box->S; i++)
        if (!below_mod<FrP64>(serials + 4 * i)) return set_error(ctx, VSP_ERR_ARG, "ballot_box_add_serials: a scalar is not below r");
    if (!count) return VSP_OK;
    VSP_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t serial_bytes = box->words * sizeof(uint32_t);
    std::vector<uint8_t> status;
    size_t added = 0;
    auto pieces = [&]() -> int {
        if (box->dirty) VSP_TRY(box_restore(ctx, box));
        for (size_t at = 0; at < count; at += BOX_ADD_PIECE) {
            const size_t c = count - at < BOX_ADD_PIECE ? count - at : BOX_ADD_PIECE;
            size_t in = 0;
            VSP_TRY(ensure(ctx, box->pend, c * serial_bytes));
            VSP_TRY(ensure(ctx, box->hold, c));                      // the skip bytes: every serial takes part
            VSP_HIP(hipMemcpyAsync(box->pend.p, serials + at * box->S * 4, c * serial_bytes, hipMemcpyHostToDevice, st));
            VSP_HIP(hipMemsetAsync(box->hold.p, 0, c, st));
            box->h_flag[1] = 0;
            VSP_TRY(box_piece_settle(ctx, box, c, (uint8_t *)box->hold.p));
            VSP_HIP(hipStreamSynchronize(st));
            status.resize(c);
            VSP_TRY(box_piece_commit(ctx, box, c, status.data(), nullptr, nullptr, true, &in));
            box_add_times(ctx, box, false, true);
            if (status_out) memcpy(status_out + at, status.data(), c);
            added += in;
            if (added_out) *added_out = added;
        }
        return VSP_OK;
    };
    const int r = pieces();
    if (r != VSP_OK && box->dirty) {
        const std::string err = ctx->err;
        if (box_restore(ctx, box) == VSP_OK) ctx->err = err;
    }
    return r;
}

}  // extern "C"
