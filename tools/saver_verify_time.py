"""SAVER ballot verdicts on the GPU (vsp_saver_verify_batch) at the reference's msg_size 25, against the only route the library offered
before it for the same two verdicts: vsp_multi_pairing_batch with m = 27 over the ciphertext pairs plus vsp_multi_pairing_batch with
m = 4 over (-A, B), (alpha, beta), (acc, gamma), (C, delta), acc computed on the host and not timed.

The ballots are real: a few one-hot ballots made by vsp_saver_encrypt over a small synthetic system, each rerandomized by
vsp_saver_rerandomize until there are 2^12.  Both routes must accept every ballot and reject one tampered member.  Wall time of the
blocking calls, best of R (default 3); the three stage times of the new call; a sweep of option "saver_verify_group" at 2^12 ballots.
Field products per ballot from the operation count of DESIGN.md 3.6d.

    python3 tools/saver_verify_time.py       prints the report and writes it to profiles/saver_verify_time.txt (OUT=path for another file)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vote_saver_protocol_amd as v  # noqa: E402
import cref  # noqa: E402  (the generator of the synthetic system and the host sum of acc, not the thing measured)
import bls12_381 as o  # noqa: E402

N, NC, NI = 25, int(os.environ.get("NC", "200")), 30
LOG_MAX = int(os.environ.get("LOG_MAX", "12"))
REPS = int(os.environ.get("R", "3"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "saver_verify_time.txt"))
VOTES = (7, 3, 24, 0)
STATS = ("saver_verify_prepare_ms", "saver_verify_miller_ms", "saver_verify_finalexp_ms")
ctx = v.Context(0)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


def fr(vals):
    return np.array([[(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for x in vals], np.uint64)


def neg_g1(rows):
    out = rows.copy()
    for row in out:
        y = sum(int(w) << (64 * i) for i, w in enumerate(row[6:]))
        if y:
            row[6:] = [((o.P - y) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]
    return out


def best_of(fn, stats=()):
    best = None
    for _ in range(REPS):
        ctx.stats_reset()
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        if best is None or dt < best[0]:
            best = (dt, [ctx.stat(s) for s in stats], out)
    return best


# ---- the election and 2^LOG_MAX ballots
gen = o.splitmix64(2025)
tox = fr([o.rand_fr(gen) for _ in range(5)])
rnd = fr([o.rand_fr(gen) for _ in range(3 * N + 2)])
total = 1 << LOG_MAX
per = total // len(VOTES)
cts, As, Bs, Cs, rests = [], [], [], [], []
dcs = kp = None
t_make = time.perf_counter()
for vote in VOTES:
    cs, wit = cref.R1CS.synth(NC, NI, 5, ballot=(N, vote))
    if dcs is None:
        dcs = v.R1CS(ctx, NC, NI, cs.num_vars, *cs.export())
        kp = v.Keypair(ctx, dcs, tox)
        parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
        gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
        pk_w, _, _ = v.saver_generate_keypair(ctx, rnd, gabc, parts["delta_g1"][0], parts["gamma_g1"][0], N)
        spk = v.SaverPublicKey(ctx, pk_w, gabc[:N + 1], N)
    r_enc, r, s = (fr([o.rand_fr(gen)])[0] for _ in range(3))
    ct, abc, _ = v.saver_encrypt(ctx, spk, dcs, kp.pk, wit[:N], wit, r_enc, r, s)
    for _ in range(per):
        ct, abc, _ = v.saver_rerandomize(ctx, spk, parts["delta_g2"][0], fr([o.rand_fr(gen) for _ in range(3)]), ct, abc)
        cts.append(ct); As.append(abc[0].reshape(12)); Bs.append(abc[1].reshape(24)); Cs.append(abc[2].reshape(12)); rests.append(wit[N:NI].copy())
    cs.free()
ct, rest, A, B, Cc = (np.ascontiguousarray(np.stack(x)) for x in (cts, rests, As, Bs, Cs))
Cc[total // 2] = neg_g1(Cc[total // 2:total // 2 + 1])[0]                # one tampered member: equation 2 fails
want = np.ones(total, np.uint8); want[total // 2] = 0
say("msg_size %d, %d rest inputs, %d ballots (%d real, each rerandomized %d times; member %d has C negated): made in %.1f s"
    % (N, NI - 1 - N + 1, total, len(VOTES), per, total // 2, time.perf_counter() - t_make))

# ---- the parent route's inputs: acc on the host (not timed), the fixed G2 arguments repeated per ballot
t_g2 = pk_w[12 + 24 * N:12 + 24 * N + 24 * (N + 1)].reshape(N + 1, 24)
H = np.array(o.g2_to_limbs(o.G2.gen), np.uint64)
ones = fr([1] * (N + 2))
acc = np.stack([cref.msm_g1(np.concatenate([gabc[:1], ct[k, :N + 1], gabc[N + 1:]]), np.concatenate([ones, rest[k]])) for k in range(total)]).reshape(total, 12)
ct_neg_psi = ct.copy(); ct_neg_psi[:, N + 1] = neg_g1(ct[:, N + 1])
q1 = np.ascontiguousarray(np.broadcast_to(np.concatenate([t_g2, H[None]]), (total, N + 2, 24)))
p2 = np.ascontiguousarray(np.stack([neg_g1(A), np.broadcast_to(parts["alpha_g1"][0], (total, 12)), acc, Cc], axis=1))
q2 = np.ascontiguousarray(np.stack([B] + [np.broadcast_to(parts[k][0], (total, 24)) for k in ("beta_g2", "gamma_g2", "delta_g2")], axis=1))


def parent_route(n):
    _, one1 = v.multi_pairing_batch(ctx, ct_neg_psi[:n].reshape(-1, 12), q1[:n].reshape(-1, 24), N + 2, want_gt=False)
    _, one2 = v.multi_pairing_batch(ctx, p2[:n].reshape(-1, 12), q2[:n].reshape(-1, 24), 4, want_gt=False)
    return one1 & one2


ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], gabc, N)
new_call = lambda n: v.saver_verify_batch(ctx, ver, ct[:n], rest[:n], A[:n], B[:n], Cc[:n])[0]
new_call(64); parent_route(64)                                          # warm-up: code objects, scratch, workspaces
ratio = None
for lg in sorted({min(10, LOG_MAX), LOG_MAX}):
    n = 1 << lg
    dt_new, st, got_new = best_of(lambda: new_call(n), STATS)
    dt_old, _, got_old = best_of(lambda: parent_route(n))
    ok = np.array_equal(got_new, want[:n]) and np.array_equal(got_old, want[:n])
    ratio = dt_old / dt_new
    say("2^%-2d ballots: vsp_saver_verify_batch %8.1f ms (%7.0f ballots/s; prepare %.2f, miller + products %.2f, final exp %.2f ms)   "
        "multi_pairing m=27 + m=4 %8.1f ms   ratio %.2f x   verdicts as expected on both routes: %s"
        % (lg, dt_new * 1e3, n / dt_new, st[0], st[1], st[2], dt_old * 1e3, ratio, ok))
say("operation count per ballot (DESIGN.md 3.6d): parent route 226 000 field products, this call 135 000: predicted 1.6 x, measured %.2f x at 2^%d" % (ratio, LOG_MAX))
n = total
for group in (3, 5, 9, 14, 27):
    ctx.set_option("saver_verify_group", group)
    new_call(64)
    dt, st, got = best_of(lambda: new_call(n), STATS)
    say("saver_verify_group %2d (%2d + 1 groups): %8.1f ms   prepare %.2f, miller + products %.2f, final exp %.2f ms   verdicts as expected: %s"
        % (group, (N + 2 + group - 1) // group, dt * 1e3, st[0], st[1], st[2], np.array_equal(got, want)))
ctx.set_option("saver_verify_group", 9)
ver.free(); spk.free(); kp.free(); dcs.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
