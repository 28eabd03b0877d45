"""ballots per second beside proofs per second: 2^LOG_M constraints, msg_size 25, one-hot ballots, batches of K over a plain key.
Legs, alternated in one run after a warm-up of each, WINDOW seconds each:
  a   vsp_groth16_prove_batch                     proofs/s   (twice: first and last, for the spread)
  b   vsp_saver_encrypt_batch                     ballots/s  one context
  c   the same, two batches in flight from one thread (launch / finish on two contexts)
  d   b with option saver_encrypt_gpu = 0         the ciphertexts on the host
  e   vsp_saver_encrypt in a loop                 one ballot per call
  f   b with full-size message blocks
The *_ms_per_batch figures are the FIRST context's laps over its own batches (in leg c the second context made the other half).
One batch of every ballot leg goes through vsp_saver_verify_batch_screened: every ballot must be accepted.  Prints one JSON line."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import cref, bls12_381 as o
import vote_saver_protocol_amd as v

lg = int(os.environ.get("LOG_M", "16")); K = int(os.environ.get("K", "32")); window = float(os.environ.get("WINDOW", "3")); n = 25
ni = 30; nc = (1 << lg) - ni - 2
ctx, ctx2 = v.Context(0), v.Context(0)
gen = o.splitmix64(16)
fr = lambda count: np.array([o.int_to_limbs(o.rand_fr(gen), 4) for _ in range(count)], np.uint64)
cs, _ = cref.R1CS.synth(nc, ni, 40, ballot=(n, 3))
dcs = v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())
kp = v.Keypair(ctx, dcs, fr(5), precompute=0)
parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1", "alpha_g1", "beta_g2", "gamma_g2", "delta_g2")}
gabc = np.ascontiguousarray(parts["gamma_ABC_g1"][:n + 1])
pk_w, _, _ = v.saver_generate_keypair(ctx, fr(3 * n + 2), gabc, parts["delta_g1"][0], parts["gamma_g1"][0], n)
spk = v.SaverPublicKey(ctx, pk_w, gabc, n)
spk.upload()
ver = v.SaverVerifier(ctx, pk_w, parts["alpha_g1"][0], parts["beta_g2"][0], parts["gamma_g2"][0], parts["delta_g2"][0], parts["gamma_ABC_g1"], n)
# four distinct votes (and four witnesses with full-size public inputs), repeated through the batch under fresh r_enc, r, s
one_hot = [cs.resample_witness(100 + j, ballot=(n, (7 * j) % n)) for j in range(4)]
full = [cs.resample_witness(200 + j) for j in range(4)]
W1 = np.stack([one_hot[k % 4] for k in range(K)]); WF = np.stack([full[k % 4] for k in range(K)])
Renc, R, S = fr(K), fr(K), fr(K)
msgs = lambda W: np.ascontiguousarray(W[:, :n])


def screened(ct, abc, W):
    verdict, _ = v.saver_verify_batch_screened(ctx, ver, ct, np.ascontiguousarray(W[:, n:ni]), *abc)
    return int(verdict.sum())


launched = []                                                          # leg c: the contexts with a batch in flight


def leg_a():
    v.groth16_prove_batch(ctx, dcs, kp.pk, W1, R, S); return K
def leg_b(W=W1):
    leg_b.last = v.saver_encrypt_batch(ctx, spk, dcs, kp.pk, msgs(W), W, Renc, R, S); return K
def leg_c():
    # two batches in flight: launch on the other context before finishing this one's
    for c in (ctx, ctx2):
        if c in launched: leg_c.last = v.saver_encrypt_batch_finish(c); launched.remove(c)
        v.saver_encrypt_batch_launch(c, spk, dcs, kp.pk, msgs(W1), W1, Renc, R, S); launched.append(c)
    return 2 * K
def drain_c():
    while launched: leg_c.last = v.saver_encrypt_batch_finish(launched.pop(0))
def leg_d():
    ctx.set_option("saver_encrypt_gpu", 0)
    try: leg_d.last = v.saver_encrypt_batch(ctx, spk, dcs, kp.pk, msgs(W1), W1, Renc, R, S)
    finally: ctx.set_option("saver_encrypt_gpu", 1)
    return K
def leg_e():
    outs = [v.saver_encrypt(ctx, spk, dcs, kp.pk, W1[k, :n], W1[k], Renc[k], R[k], S[k]) for k in range(K)]
    leg_e.last = (np.stack([x[0] for x in outs]), tuple(np.stack([x[1][j] for x in outs]) for j in range(3)))
    return K
def leg_f():
    return leg_b(WF)


def run(leg):
    """-> (units per second over a window, the context's statistics per call)"""
    leg()                                                              # warm-up: every shape of the window
    drain_c()
    ctx.stats_reset()
    done, calls, t0 = 0, 0, time.perf_counter()
    while time.perf_counter() - t0 < window:
        done += leg(); calls += 1
    drain_c()
    rate = done / (time.perf_counter() - t0)
    names = ("saver_ct_ms", "prove_batch_launch_ms", "prove_batch_delta_ms", "prove_batch_witness_finishes_ms", "prove_batch_sA_rB1_ms", "prove_batch_h_finish_ms", "prove_batch_assembly_ms")
    batches = max(ctx.stat("prove_batches"), 1)
    return rate, {k: round(ctx.stat(k) / batches, 3) for k in names if ctx.stat(k)}


res = {"log_m": lg, "K": K, "msg_size": n, "window_s": window, "saver_pk_device_bytes": spk.device_bytes, "saver_ct_table_ms": round(ctx.stat("saver_ct_table_ms"), 1)}
for name, leg in (("a_prove_batch", leg_a), ("b_ballots", leg_b), ("c_ballots_two_in_flight", leg_c), ("d_ballots_host_ct", leg_d), ("e_single_calls", leg_e),
                  ("f_ballots_full_size", leg_f), ("a_prove_batch_again", leg_a)):
    rate, stats = run(leg)
    res[name + "_per_s"] = round(rate, 1)
    if stats: res[name + "_ms_per_batch"] = stats
    if leg is not leg_a:
        last = leg_b.last if leg is leg_f else leg.last
        res[name + "_screened_accepted"] = "%d/%d" % (screened(last[0], last[1], WF if leg is leg_f else W1), K)
# the ciphertext kernels alone, nothing beside them
ctx.stats_reset()
for _ in range(20): v.saver_ciphertext_batch(ctx, spk, msgs(W1), Renc)
res["ct_alone_one_hot_ms_per_batch"] = round(ctx.stat("saver_ct_ms") / 20, 3)
ctx.stats_reset()
for _ in range(20): v.saver_ciphertext_batch(ctx, spk, msgs(WF), Renc)
res["ct_alone_full_size_ms_per_batch"] = round(ctx.stat("saver_ct_ms") / 20, 3)
print(json.dumps(res))
