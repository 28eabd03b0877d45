"""The tally's aggregation (vsp_tally_add_blobs: decode, check and add ciphertext blobs on the GPU) against the only path the library had
before it: vsp_g1_vector_from_blob per ballot on one host thread (decoding alone -- the library exports no point addition).
2^16 ballots of 27 points: multiples of the generator by vsp_fixed_base_mul_g1, compressed on the host by vsp_g1_vector_to_blob.
Reports GPU ballots/s at 2^12 and 2^16 ballots with and without the subgroup check, the HIP-event time per stage, the host figure at
2^10 ballots, and whether the GPU exceeds 16 x the single-thread host figure at 2^16 with the check on (the feature's bar).
The sums are checked: column j must equal (sum of its scalars mod r) * G."""
import os, sys, time, ctypes as C
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vote_saver_protocol_amd as v  # noqa: E402
from vote_saver_protocol_amd.api import _ptr  # noqa: E402

R_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CT_LEN = int(os.environ.get("CT_LEN", "27"))
LOG_MAX = int(os.environ.get("LOG_BALLOTS", "16"))
LOG_HOST = int(os.environ.get("LOG_HOST", "10"))
REPS = int(os.environ.get("R", "3"))
ctx = v.Context(0)
lib = ctx.lib
rng = np.random.default_rng(11)
nb = 1 << LOG_MAX
n = nb * CT_LEN
ks = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
ks[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
t0 = time.perf_counter()
d_k = ctx.to_device(ks)
d_p = v.fixed_base_mul(ctx, d_k, n)
pts = np.zeros((n, 12), np.uint64); ctx.d2h(pts, d_p)
ctx.dfree(d_k); ctx.dfree(d_p)
flat = np.frombuffer(v.g1_vector_to_blob(pts), dtype=np.uint8)[8:].reshape(nb, 48 * CT_LEN)
head = np.frombuffer(int(CT_LEN).to_bytes(8, "big"), dtype=np.uint8)
blobs = np.ascontiguousarray(np.concatenate([np.broadcast_to(head, (nb, 8)), flat], axis=1))      # [ballots, 8 + 48 ct_len]
print("generated %d ballots of %d points in %.1f s" % (nb, CT_LEN, time.perf_counter() - t0))


def column_scalars(count):
    a = ks[:count * CT_LEN].reshape(count, CT_LEN, 4)
    out = np.zeros((CT_LEN, 4), np.uint64)
    for j in range(CT_LEN):
        s = sum(int(a[:, j, w].astype(object).sum()) << (64 * w) for w in range(4)) % R_MOD
        out[j] = [(s >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]
    return out


def expected(count):
    d_s = ctx.to_device(column_scalars(count))
    d_o = v.fixed_base_mul(ctx, d_s, CT_LEN)
    out = np.zeros((CT_LEN, 12), np.uint64); ctx.d2h(out, d_o)
    ctx.dfree(d_s); ctx.dfree(d_o)
    return out


t = v.Tally(ctx, CT_LEN)
t.add_blobs(blobs[:256].tobytes())                                   # warm-up: code objects, workspaces
gpu_rate = {}
for lg in sorted({min(12, LOG_MAX), LOG_MAX}):
    count = 1 << lg
    data = blobs[:count].tobytes()
    want = expected(count)
    for check in (1, 0):
        best = None
        for _ in range(REPS):
            t.reset(); ctx.stats_reset()
            t0 = time.perf_counter()
            status, accepted = t.add_blobs(data, check_subgroup=bool(check))
            dt = time.perf_counter() - t0
            stages = tuple(ctx.stat(s) for s in ("tally_decode_ms", "tally_subgroup_ms", "tally_sum_ms"))
            if best is None or dt < best[0]:
                best = (dt, stages)
        ct, ballots = t.result()
        ok = accepted == count and ballots == count and np.array_equal(ct, want)
        gpu_rate[(lg, check)] = count / best[0]
        print("GPU  2^%-2d ballots, subgroup check %d: %9.1f ms  %10.0f ballots/s   stages: decode %.2f ms, subgroup %.2f ms, sum %.2f ms   sums correct: %s"
              % (lg, check, best[0] * 1e3, count / best[0], best[1][0], best[1][1], best[1][2], ok))
t.free()

# the path before this feature: one ballot at a time through vsp_g1_vector_from_blob, one host thread, decoding only
count = 1 << min(LOG_HOST, LOG_MAX)
size = 8 + 48 * CT_LEN
out = np.zeros((CT_LEN, 12), np.uint64); got = C.c_size_t(0)
host_rate = {}
for check in (1, 0):
    t0 = time.perf_counter()
    for b in range(count):
        rc = lib.vsp_g1_vector_from_blob(_ptr(blobs[b]), size, check, _ptr(out), CT_LEN, C.byref(got))
        assert rc == 0 and got.value == CT_LEN
    dt = time.perf_counter() - t0
    host_rate[check] = count / dt
    print("host 2^%-2d ballots, subgroup check %d: %9.1f ms  %10.1f ballots/s   (vsp_g1_vector_from_blob per ballot, one thread, decoding only)"
          % (min(LOG_HOST, LOG_MAX), check, dt * 1e3, count / dt))
ratio = gpu_rate[(LOG_MAX, 1)] / host_rate[1]
print("GPU at 2^%d with the check / one host thread with the check: %.1f x   bar (16 x): %s" % (LOG_MAX, ratio, "met" if ratio > 16 else "MISSED"))
ctx.close()
