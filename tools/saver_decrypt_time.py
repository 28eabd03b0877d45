"""SAVER decryption on the GPU (vsp_saver_decrypt_batch, vsp_saver_verify_decryption_batch) at the reference's msg_size 25.

The key and the ciphertexts have known logs (tests/dlog_decrypt.py), so a ciphertext holds any chosen counts at no pairing's cost; the
counts are uniform in [0, max_value] (fixed seed): the giant search stops once every slot has its result, so its time depends on the
largest count of the piece, and uniform counts put that near the top of the range.  Every result is compared with the chosen counts.
Wall time of the blocking calls, best of R (default 3), and the stage stats of the best run:

    creation for max_value 2^20 and 2^32 - 1: wall time, the baby-step kernel and the host sort apart, table bytes
    decrypt of 1 and of 64 ciphertexts, by stage; verify_decryption of the same
    for comparison the values alone through vsp_multi_pairing_batch (m = 2): the only route to them before this call
    a sweep of option "saver_decrypt_baby_bits" for max_value 2^32 - 1, one ciphertext

    python3 tools/saver_decrypt_time.py       prints the report and writes it to profiles/saver_decrypt_time.txt (OUT=path for another file)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import vote_saver_protocol_amd as v  # noqa: E402
import bls12_381 as o  # noqa: E402
import dlog_decrypt as dd  # noqa: E402  (known-log keys and ciphertexts: the generator of the inputs, not the thing measured)
from dlog_election import g1_points, rng as make_rng  # noqa: E402

N = int(os.environ.get("N", "25"))
REPS = int(os.environ.get("R", "3"))
SWEEP = [int(x) for x in os.environ.get("SWEEP", "12,14,16,18,20").split(",") if x]
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "saver_decrypt_time.txt"))
DEC_STATS = ("saver_decrypt_prepare_ms", "saver_decrypt_values_ms", "saver_decrypt_dlog_ms")
VER_STATS = ("saver_decrypt_prepare_ms", "saver_decrypt_values_ms", "saver_decrypt_power_ms")
ctx = v.Context(0)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


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


def neg_g1(rows):
    out = rows.copy()
    for row in out:
        y = sum(int(w) << (64 * i) for i, w in enumerate(row[6:]))
        if y:
            row[6:] = [((o.P - y) >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(6)]
    return out


rg = make_rng(2026)
key = dd.DecryptKey(rg, N)
V = key.vk_words.reshape(-1, 24)[1:1 + N]
W = key.vk_words.reshape(-1, 24)[1 + N:]


def make(max_value, count):
    rows = [[rg.randrange(max_value + 1) for _ in range(N)] for _ in range(count)]
    return rows, dd.ct_batch(key, [key.ciphertext(row, rg) for row in rows])


def create(max_value, baby_bits=0):
    ctx.stats_reset()
    t0 = time.perf_counter()
    dec = v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, N, max_value, baby_bits=baby_bits)
    dt = time.perf_counter() - t0
    return dec, dt, ctx.stat("saver_decrypt_table_ms"), ctx.stat("saver_decrypt_sort_ms")


def measure(dec, rows, ct, label):
    n = len(rows)
    dt, st, (msgs, nu, status) = best_of(lambda: v.saver_decrypt_batch(ctx, dec, key.rho_limbs, ct), DEC_STATS)
    ok = msgs.tolist() == rows and not status.any()
    say("%s: decrypt of %2d ciphertexts %9.2f ms (prepare %.2f, values %.2f, search %.2f ms)   counts as chosen: %s" % (label, n, dt * 1e3, st[0], st[1], st[2], ok))
    return msgs, nu


with v.SaverDecryptor(ctx, key.vk_words, key.gamma_abc, N, 1000) as warm:                # warm-up: code objects, scratch, workspaces
    rows, ct = make(1000, 2)
    m, nu, _ = v.saver_decrypt_batch(ctx, warm, key.rho_limbs, ct)
    v.saver_verify_decryption_batch(ctx, warm, ct, m, nu)

say("msg_size %d, known-log key, counts uniform in [0, max_value]; best of %d" % (N, REPS))
for name, max_value in (("2^20", 1 << 20), ("2^32 - 1", (1 << 32) - 1)):
    dec, dt, t_tab, t_sort = create(max_value)
    B = 1 << dec.baby_bits
    say("max_value %s: baby bits %d (automatic), %d giant steps; creation %.1f ms (baby-step kernel %.2f, host sort %.2f ms), table %d bytes"
        % (name, dec.baby_bits, (max_value >> dec.baby_bits) + 1, dt * 1e3, t_tab, t_sort, N * B * 12))
    for count in (1, 64):
        rows, ct = make(max_value, count)
        msgs, nu = measure(dec, rows, ct, "  max_value %s" % name)
        dt, st, (verdict, reason, _) = best_of(lambda: v.saver_verify_decryption_batch(ctx, dec, ct, msgs, nu), VER_STATS)
        say("  max_value %s: verify  of %2d results     %9.2f ms (prepare %.2f, values %.2f, powers %.2f ms)   all accepted: %s"
            % (name, count, dt * 1e3, st[0], st[1], st[2], bool(verdict.all()) and not reason.any()))
        # the values alone by the route the library had before: n products of the two pairs (c_i, W_i) (-nu, V_i) per ciphertext
        neg_nu = neg_g1(nu)
        g1 = np.ascontiguousarray(np.stack([np.stack([ct[k, 1:N + 1], np.broadcast_to(neg_nu[k], (N, 12))], axis=1) for k in range(count)])).reshape(-1, 12)
        g2 = np.ascontiguousarray(np.broadcast_to(np.stack([W, V], axis=1), (count, N, 2, 24))).reshape(-1, 24)
        dt, _, _ = best_of(lambda: v.multi_pairing_batch(ctx, g1, g2, 2))
        say("  max_value %s: the %4d values alone through vsp_multi_pairing_batch (m = 2) %9.2f ms" % (name, count * N, dt * 1e3))
    dec.free()

max_value = (1 << 32) - 1
rows, ct = make(max_value, 1)
say("sweep of saver_decrypt_baby_bits at max_value 2^32 - 1, one ciphertext (largest count %d):" % max(rows[0]))
for b in SWEEP:
    dec, dt, t_tab, t_sort = create(max_value, baby_bits=b)
    say("  baby bits %2d: creation %8.1f ms (kernel %.2f, sort %.2f ms), table %10d bytes" % (b, dt * 1e3, t_tab, t_sort, N * (1 << b) * 12))
    measure(dec, rows, ct, "  baby bits %2d" % b)
    dec.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
