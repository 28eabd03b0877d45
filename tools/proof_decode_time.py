"""Decoding proof blobs on the GPU (vsp_proof_from_blob_batch: A | B | C decompressed and subgroup-checked) against the only path the
library had before it: vsp_proof_from_blob per proof on one host thread.
2^16 proofs: A, C multiples of the G1 generator and B of the G2 generator by vsp_fixed_base_mul_g1/_g2, compressed on the host.
Reports, for 2^12 and 2^16 proofs with the subgroup check on, the wall time of the blocking call (best of R), its HIP-event stage times,
the host loop's time over the same bytes (2^LOG_HOST proofs, scaled), and the ratio.  Every status must be 0 and the first 64 proofs
must equal the host function's output."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vote_saver_protocol_amd as v  # noqa: E402
from vote_saver_protocol_amd.api import _ptr  # noqa: E402

LOG_MAX = int(os.environ.get("LOG_PROOFS", "16"))
LOG_HOST = int(os.environ.get("LOG_HOST", "10"))
REPS = int(os.environ.get("R", "3"))
ctx = v.Context(0)
lib = ctx.lib
rng = np.random.default_rng(12)
n = 1 << LOG_MAX
t0 = time.perf_counter()


def multiples(count, group):
    ks = rng.integers(0, 1 << 64, size=(count, 4), dtype=np.uint64)
    ks[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    d_k = ctx.to_device(ks)
    d_p = v.fixed_base_mul(ctx, d_k, count, group)
    pts = np.zeros((count, 12 * group), np.uint64); ctx.d2h(pts, d_p)
    ctx.dfree(d_k); ctx.dfree(d_p)
    return pts


g1, g2 = multiples(2 * n, 1), multiples(n, 2)
blobs = np.zeros((n, 192), np.uint8)
for k in range(n):
    assert lib.vsp_proof_to_blob(_ptr(g1[k]), _ptr(g2[k]), _ptr(g1[n + k]), _ptr(blobs[k])) == 0
print("generated %d proofs in %.1f s" % (n, time.perf_counter() - t0))

v.proofs_from_blob_batch(ctx, blobs[:256].tobytes())                    # warm-up: code objects, workspaces
gpu_ms = {}
for lg in sorted({min(12, LOG_MAX), LOG_MAX}):
    count = 1 << lg
    data = np.ascontiguousarray(blobs[:count]).reshape(-1)
    A = np.zeros((count, 12), np.uint64); B = np.zeros((count, 24), np.uint64); Cc = np.zeros((count, 12), np.uint64); status = np.ones(count, np.uint8)
    best = None
    for _ in range(REPS):
        ctx.stats_reset()
        t0 = time.perf_counter()
        ctx.check(lib.vsp_proof_from_blob_batch(ctx.h, _ptr(data), count, 1, _ptr(A), _ptr(B), _ptr(Cc), _ptr(status)))
        dt = time.perf_counter() - t0
        stages = tuple(ctx.stat(s) for s in ("tally_decode_ms", "tally_subgroup_ms", "g2_decode_ms", "g2_subgroup_ms"))
        if best is None or dt < best[0]:
            best = (dt, stages)
    ok = not status.any() and np.array_equal(A, g1[:count]) and np.array_equal(B, g2[:count]) and np.array_equal(Cc, g1[n:n + count])
    gpu_ms[lg] = best[0] * 1e3
    print("GPU  2^%-2d proofs, subgroup check 1: %9.2f ms  %10.0f proofs/s   stages: G1 decode %.2f ms, G1 subgroup %.2f ms, G2 decode %.2f ms, G2 subgroup %.2f ms   points correct: %s"
          % (lg, best[0] * 1e3, count / best[0], best[1][0], best[1][1], best[1][2], best[1][3], ok))

# the path before this feature: one proof at a time through vsp_proof_from_blob, one host thread
count = 1 << min(LOG_HOST, LOG_MAX)
hA = np.zeros(12, np.uint64); hB = np.zeros(24, np.uint64); hC = np.zeros(12, np.uint64)
t0 = time.perf_counter()
for k in range(count):
    assert lib.vsp_proof_from_blob(_ptr(blobs[k]), 1, _ptr(hA), _ptr(hB), _ptr(hC)) == 0
    if k < 64:
        assert np.array_equal(hA, g1[k]) and np.array_equal(hB, g2[k]) and np.array_equal(hC, g1[n + k])
host_per = (time.perf_counter() - t0) / count
print("host 2^%-2d proofs, subgroup check 1: %9.1f ms  %10.1f proofs/s   (vsp_proof_from_blob per proof, one thread)" % (min(LOG_HOST, LOG_MAX), host_per * count * 1e3, 1 / host_per))
for lg, ms in gpu_ms.items():
    print("2^%-2d proofs: host loop %.1f ms (scaled from 2^%d) / GPU batch %.2f ms = %.1f x" % (lg, host_per * (1 << lg) * 1e3, min(LOG_HOST, LOG_MAX), ms, host_per * (1 << lg) * 1e3 / ms))
ctx.close()
