"""Rerandomization of SAVER ballots in batches (vsp_saver_rerandomize_batch) beside the single call in a loop, at the reference's msg_size 25.

The inputs are curve points, not valid ballots -- validity does not matter for the cost: 2^10 distinct ballots of random multiples of the
generators (the C oracle makes them), repeated up to the size of the batch, under random scalars that differ for every member.  In one
process, for every size, the batch call alternates with vsp_saver_rerandomize in a loop over the first 2^10 ballots of the same inputs
(its time scaled to the size); wall time of the blocking calls with every output asked for, best of R (default 3) after a warm-up, and
the kernels' share of "saver_rerandomize_ms" in the best run.  The first 2^10 members of every batch are compared with the loop's.

    sizes            SIZES=10,12,14,16 (logs)         ballots/s of both, the ratio, the stages
    pieces           CHUNKS=12,14,16 at 2^CHUNK_AT    option "saver_rerandomize_chunk": which default to keep
    multiplications  W4_AT=14                         option "saver_rerandomize_w4" 1 and 0: 4-bit windows or single bits

    timeout -k 10 900 python3 tools/saver_rerandomize_time.py    prints the report and writes it to profiles/saver_rerandomize_time.txt
                                                                 (OUT=path for another file; an empty SIZES, CHUNKS or W4_AT leaves that part out,
                                                                 so that each part can run under a time limit of its own)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, d))
import vote_saver_protocol_amd as v  # noqa: E402
import cref  # noqa: E402  (the generator of the inputs, not the thing measured)

N = int(os.environ.get("N", "25"))
REPS = int(os.environ.get("R", "3"))
logs = lambda name, dflt: [int(x) for x in os.environ.get(name, dflt).split(",") if x]
SIZES, CHUNKS, CHUNK_AT, W4_AT = logs("SIZES", "10,12,14,16"), logs("CHUNKS", "12,14,16"), int(os.environ.get("CHUNK_AT", "16")), logs("W4_AT", "14")
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "saver_rerandomize_time.txt"))
DISTINCT = 1 << 10
STAGES = ("saver_rerandomize_ms", "saver_rerandomize_check_ms", "saver_rerandomize_columns_ms", "saver_rerandomize_affine_ms", "saver_rerandomize_g1_ms", "saver_rerandomize_g2_ms")
ctx = v.Context(0)
lib, p = ctx.lib, v.api._ptr
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def rand_fr(rng, n):
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)                        # < 2^254 < r
    a[:, 0] |= np.uint64(1)                                         # never zero
    return a


rng = np.random.default_rng(2026)
pts = cref.g1_batch_mul_gen(rand_fr(rng, N + 3))
pk_w, _, _ = v.saver_generate_keypair(ctx, rand_fr(rng, 3 * N + 2), np.ascontiguousarray(pts[:N + 1]), pts[N + 1], pts[N + 2], N)
spk = v.SaverPublicKey(ctx, pk_w, np.ascontiguousarray(pts[:N + 1]), N)
delta_g2 = cref.g2_batch_mul_gen(rand_fr(rng, 1))[0]
rr = v.SaverRerandomizer(ctx, spk, delta_g2)
g1 = cref.g1_batch_mul_gen(rand_fr(rng, DISTINCT * (N + 4))).reshape(DISTINCT, N + 4, 12)
CT0, A0, C0 = (np.ascontiguousarray(x) for x in (g1[:, :N + 2], g1[:, N + 2], g1[:, N + 3]))
B0 = cref.g2_batch_mul_gen(rand_fr(rng, DISTINCT))
BLOB = lib.vsp_g1_vector_blob_size(N + 2)


class Batch:
    def __init__(self, count):
        reps = (count + DISTINCT - 1) // DISTINCT
        tile = lambda x: np.ascontiguousarray(np.concatenate([x] * reps)[:count])
        self.count, self.ct, self.A, self.B, self.C = count, tile(CT0), tile(A0), tile(B0), tile(C0)
        self.rnd = rand_fr(rng, 3 * count).reshape(count, 12)
        self.o_ct, self.o_A, self.o_B, self.o_C = (np.zeros_like(x) for x in (self.ct, self.A, self.B, self.C))
        self.o_pr, self.o_bl, self.o_st = np.zeros((count, 192), np.uint8), np.zeros((count, BLOB), np.uint8), np.zeros(count, np.uint8)
        m = min(count, DISTINCT)
        self.l_ct, self.l_A, self.l_B, self.l_C, self.l_pr = self.ct[:m].copy(), self.A[:m].copy(), self.B[:m].copy(), self.C[:m].copy(), np.zeros((m, 192), np.uint8)

    def batch(self):
        ctx.check(lib.vsp_saver_rerandomize_batch(ctx.h, rr.h, p(self.rnd), p(self.ct), p(self.A), p(self.B), p(self.C), self.count, p(self.o_ct), p(self.o_A), p(self.o_B),
                                                  p(self.o_C), p(self.o_pr), p(self.o_bl), p(self.o_st)))

    def loop(self):
        """the single call over the first 2^10 members, in place on copies of them"""
        m = len(self.l_ct)
        self.l_ct[:], self.l_A[:], self.l_B[:], self.l_C[:] = self.ct[:m], self.A[:m], self.B[:m], self.C[:m]
        d2 = p(delta_g2)
        for k in range(m):
            ctx.check(lib.vsp_saver_rerandomize(ctx.h, spk.h, d2, p(self.rnd[k]), p(self.l_ct[k]), p(self.l_A[k]), p(self.l_B[k]), p(self.l_C[k]), p(self.l_pr[k])))

    def agree(self):
        m = len(self.l_ct)
        return bool(np.array_equal(self.o_ct[:m], self.l_ct) and np.array_equal(self.o_A[:m], self.l_A) and np.array_equal(self.o_B[:m], self.l_B)
                    and np.array_equal(self.o_C[:m], self.l_C) and np.array_equal(self.o_pr[:m], self.l_pr) and not self.o_st.any())


def timed(fn):
    ctx.stats_reset()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, [ctx.stat(s) for s in STAGES]


def best_batch(b):
    return min((timed(b.batch) for _ in range(REPS)), key=lambda x: x[0])


def stages(st):
    return "kernels %.1f ms: check %.1f, columns %.1f, affine %.1f, G1 multiplications %.1f, G2 multiplications %.1f" % tuple(st)


say("msg_size %d, %d distinct ballots of random curve points repeated, random scalars; best of %d after a warm-up; rerandomizer %d bytes on the device beside the key's %d"
    % (N, DISTINCT, REPS, rr.device_bytes, spk.device_bytes))
for lg in SIZES:
    b = Batch(1 << lg)
    b.batch()                                                       # warm-up: code objects, workspaces, pinned memory
    best_b, best_l = None, None
    for _ in range(REPS):                                           # alternate
        tb = timed(b.batch)
        tl = timed(b.loop)
        best_b = tb if best_b is None or tb[0] < best_b[0] else best_b
        best_l = tl if best_l is None or tl[0] < best_l[0] else best_l
    per_b, per_l = best_b[0] / b.count, best_l[0] / len(b.l_ct)
    say("2^%-2d ballots: batch %9.1f ms = %9.0f ballots/s | loop of %d single calls %8.1f ms = %7.0f ballots/s | batch / loop %6.2f x | equal bytes: %s"
        % (lg, best_b[0] * 1e3, 1 / per_b, len(b.l_ct), best_l[0] * 1e3, 1 / per_l, per_l / per_b, b.agree()))
    say("            " + stages(best_b[1]))
if CHUNKS:
    b = Batch(1 << CHUNK_AT)
    say("pieces at 2^%d ballots (option saver_rerandomize_chunk):" % CHUNK_AT)
    for lg in CHUNKS:
        ctx.set_option("saver_rerandomize_chunk", 1 << lg)
        b.batch()
        dt, st = best_batch(b)
        say("  pieces of 2^%-2d: %9.1f ms = %9.0f ballots/s; %s" % (lg, dt * 1e3, b.count / dt, stages(st)))
    ctx.set_option("saver_rerandomize_chunk", 1 << 16)
for lg in W4_AT:
    b = Batch(1 << lg)
    say("variable-base multiplications at 2^%d ballots (option saver_rerandomize_w4):" % lg)
    for w4 in (1, 0):
        ctx.set_option("saver_rerandomize_w4", w4)
        b.batch()
        dt, st = best_batch(b)
        say("  %s: %9.1f ms; %s" % ("4-bit windows" if w4 else "single bits  ", dt * 1e3, stages(st)))
    ctx.set_option("saver_rerandomize_w4", 1)
rr.free(); spk.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
