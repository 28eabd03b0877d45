"""Batched pairings and Groth16 verdicts on the GPU (vsp_multi_pairing_batch, vsp_groth16_verify_batch): pairings/s at 2^10 and 2^14
pairs, proofs/s at 2^12 proofs, wall time of the blocking call and the two stage times, and field products/s from the operation count
of DESIGN.md 3.6c (csrc/pairing.h): 6 700 per Miller loop, 9 196 per final exponentiation -- to set beside k_point_decode<G1>'s 56 G field
products/s, a kernel of the same kind.
The points are multiples of the generators by vsp_fixed_base_mul.  The "proofs" are random subgroup points, not valid proofs: the work of
a verdict does not depend on the data, and every verdict must come out 0.  The pairings are checked on the first 256 pairs:
e(k G1, G2) e(G1, -k G2) = 1.

    python3 tools/pairing_time.py            prints the report and writes it to profiles/pairing_time.txt (OUT=path for another file)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vote_saver_protocol_amd as v  # noqa: E402

P_MOD = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
MILLER_PRODUCTS, FINALEXP_PRODUCTS = 6700, 9196
REPS = int(os.environ.get("R", "3"))
N_INPUTS = int(os.environ.get("INPUTS", "4"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "pairing_time.txt"))
ctx = v.Context(0)
rng = np.random.default_rng(12)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def multiples(n, group):
    ks = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    ks[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    d_k = ctx.to_device(ks)
    d_p = v.fixed_base_mul(ctx, d_k, n, group)
    out = np.zeros((n, 12 * group), np.uint64); ctx.d2h(out, d_p)
    ctx.dfree(d_k); ctx.dfree(d_p)
    return ks, out


def limbs(x, n=6):
    return [(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def value(row):
    return sum(int(w) << (64 * i) for i, w in enumerate(row))


def best_of(fn):
    best = None
    for _ in range(REPS):
        ctx.stats_reset()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        st = (ctx.stat("pairing_miller_ms"), ctx.stat("pairing_finalexp_ms"))
        if best is None or dt < best[0]:
            best = (dt, st, out)
    return best


n_max = 1 << 14
_, g1 = multiples(n_max, 1)
_, g2 = multiples(n_max, 2)
# correctness on 256 products: e(k G1, G2) e(G1, -k G2) = 1
ks = rng.integers(1, 1 << 62, size=(256, 4), dtype=np.uint64); ks[:, 1:] = 0
d_k = ctx.to_device(ks)
a = np.zeros((256, 12), np.uint64); b = np.zeros((256, 24), np.uint64)
d_a = v.fixed_base_mul(ctx, d_k, 256, 1); ctx.d2h(a, d_a); d_b = v.fixed_base_mul(ctx, d_k, 256, 2); ctx.d2h(b, d_b)
one = np.zeros((1, 4), np.uint64); one[0, 0] = 1
d_1 = ctx.to_device(one)
G1 = np.zeros((1, 12), np.uint64); G2 = np.zeros((1, 24), np.uint64)
d_g = v.fixed_base_mul(ctx, d_1, 1, 1); ctx.d2h(G1, d_g); d_h = v.fixed_base_mul(ctx, d_1, 1, 2); ctx.d2h(G2, d_h)
for p in (d_k, d_a, d_b, d_1, d_g, d_h):
    ctx.dfree(p)
for k in range(256):                                                 # -k G2: y -> p - y
    b[k, 12:18] = limbs(P_MOD - value(b[k, 12:18]) if value(b[k, 12:18]) else 0)
    b[k, 18:24] = limbs(P_MOD - value(b[k, 18:24]) if value(b[k, 18:24]) else 0)
p1 = np.stack([x for k in range(256) for x in (a[k], G1[0])]); p2 = np.stack([x for k in range(256) for x in (G2[0], b[k])])
_, is_one = v.multi_pairing_batch(ctx, p1, p2, 2, want_gt=False)
say("256 products e(k G1, G2) e(G1, -k G2): all one: %s" % bool(is_one.all()))

v.multi_pairing_batch(ctx, g1[:256], g2[:256], 1)                    # warm-up: code objects, scratch, workspaces
for lg in (10, 14):
    n = 1 << lg
    dt, st, _ = best_of(lambda: v.multi_pairing_batch(ctx, g1[:n], g2[:n], 1))
    say("2^%-2d pairings: %8.1f ms  %9.0f pairings/s   stages: miller %.2f ms (%.1f G field products/s), final exp %.2f ms (%.1f G field products/s)"
          % (lg, dt * 1e3, n / dt, st[0], n * MILLER_PRODUCTS / st[0] / 1e6, st[1], n * FINALEXP_PRODUCTS / st[1] / 1e6))

n = 1 << 12
_, gabc = multiples(N_INPUTS + 1, 1)
vk = v.VerifyingKey(ctx, g1[0], g2[0], g2[1], g2[2], gabc)
inputs = rng.integers(0, 1 << 64, size=(n, N_INPUTS, 4), dtype=np.uint64); inputs[:, :, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
A, B, Cc = g1[:n], g2[:n], g1[n:2 * n]
v.groth16_verify_batch(ctx, vk, inputs[:64], A[:64], B[:64], Cc[:64])
dt, st, verdict = best_of(lambda: v.groth16_verify_batch(ctx, vk, inputs, A, B, Cc))
say("2^12 proofs, %d public inputs: %8.1f ms  %9.0f proofs/s   stages: miller + product %.2f ms (%.1f G field products/s), final exp %.2f ms (%.1f G field products/s)   "
      "all rejected (random points): %s" % (N_INPUTS, dt * 1e3, n / dt, st[0], n * (3 * MILLER_PRODUCTS + 108) / st[0] / 1e6, st[1], n * FINALEXP_PRODUCTS / st[1] / 1e6,
                                            not verdict.any()))
vk.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
