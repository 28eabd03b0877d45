"""The ballot box's receiving step as one call (vsp_saver_receive_blobs) against the composition a caller had before it, in the same
process and alternated: msg_size 25 with 5 rest inputs, the pool of 2^10 distinct ballots of known logs (tests/dlog_election.py)
that tools/saver_screen_time.py tiles, as blobs, tiled to 2^12, 2^14 and 2^16 with distinct random coefficients; check_subgroup 1;
all valid and one bad ballot; screened and exact.  The composition, every step through the C interface on arrays that are already
numpy (no Python loop over ballots):
    the records without their count headers (one strided copy)  ->  vsp_g1_decompress_batch  (limbs down to the host)
    vsp_proof_from_blob_batch                                    (limbs down to the host)
    the input blobs decoded on the host (numpy: byte order, scalars below r, the count headers)
    vsp_saver_verify_batch_screened / vsp_saver_verify_batch     (limbs up again)
    vsp_tally_add_blobs of the accepted ballots' blobs           (the second decode of every point)
Wall time of the blocking calls after a warm-up at every size, best of R (default 3) for each of: the receive call, the composition,
and the composition once more (the a/a spread: |a - a'| of two interleaved series of the same code).  The bar: at every size the receive
call is faster than the composition by more than that spread, and verdicts and tallies agree.  The stage split of both and the
composition's second decode ("tally_decode_ms" + "tally_subgroup_ms" of its vsp_tally_add_blobs: the saved stage time) are printed.

    python3 tools/ballot_receive_time.py     prints the report and writes it to profiles/ballot_receive_time.txt (OUT=path for another file)"""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import vote_saver_protocol_amd as v  # noqa: E402
import dlog_election as de  # noqa: E402  (ballots whose verdicts are integer congruences; not the thing measured)

N, N_REST, POOL = 25, 5, int(os.environ.get("POOL", str(1 << 10)))
LOGS = [int(x) for x in os.environ.get("LOGS", "12,14,16").split(",")]
REPS = int(os.environ.get("R", "3"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "ballot_receive_time.txt"))
CT_LEN, CT_BYTES, IN_BYTES = N + 2, 8 + 48 * (N + 2), 8 + 32 * N_REST
DECODE = ("tally_decode_ms", "tally_subgroup_ms", "g2_decode_ms", "g2_subgroup_ms")
STAGES = DECODE + ("tally_sum_ms", "saver_receive_prepare_ms", "saver_screen_prepare_ms", "saver_screen_scale_ms", "saver_screen_miller_ms", "saver_screen_msm_ms",
                   "saver_screen_finalexp_ms", "saver_verify_prepare_ms", "saver_verify_miller_ms", "saver_verify_finalexp_ms")
R_WORDS = np.array([(de.R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], np.uint64)
ctx = v.Context(0)
lib, p = ctx.lib, v.api._ptr
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


# ---- the election, the pool as blobs, and a bad twin of every pool member's proof (C + G: equation 2 fails)
rng = de.rng(2026)
t_make = time.perf_counter()
el = de.Election(rng, N, N_REST)
members = [de.make_ballot(el, [de.nonzero(rng) for _ in range(N + 1)], [rng.randrange(de.R) for _ in range(N_REST)], rng) for _ in range(POOL)]
pool = de.ballot_batch(el, members)
bad_C = de.g1_points([(m["z"] + 1) % de.R for m in members])
as_rows = lambda blobs: np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), -1)
pool_ct = as_rows([v.g1_vector_to_blob(pool["ct"][i]) for i in range(POOL)])
pool_pr = as_rows([v.g1_compress(pool["A"][i]) + v.g2_compress(pool["B"][i]) + v.g1_compress(pool["C"][i]) for i in range(POOL)])
pool_bad = as_rows([v.g1_compress(pool["A"][i]) + v.g2_compress(pool["B"][i]) + v.g1_compress(bad_C[i]) for i in range(POOL)])
pool_in = as_rows([v.fr_vector_to_blob(pool["rest"][i]) for i in range(POOL)])
assert pool_ct.shape[1] == CT_BYTES and pool_pr.shape[1] == 192 and pool_in.shape[1] == IN_BYTES
k = el.key
ver = v.SaverVerifier(ctx, el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, N)
say("msg_size %d, %d rest inputs, a pool of %d distinct ballots of known logs as blobs, tiled; check_subgroup 1: made in %.1f s" % (N, N_REST, POOL, time.perf_counter() - t_make))


def batch(n, bad):
    idx = np.arange(n) % POOL
    b = dict(ct=np.ascontiguousarray(pool_ct[idx]), pr=np.ascontiguousarray(pool_pr[idx]), inp=np.ascontiguousarray(pool_in[idx]))
    want = np.zeros(n, np.uint8)
    for i in bad:
        b["pr"][i] = pool_bad[i % POOL]; want[i] = 4
    z = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    z[:, 0] |= np.uint64(1)                                             # not zero
    return b, z, want


def tally_result(t):
    ct = np.zeros((CT_LEN, 12), np.uint64); ballots = C.c_uint64(0)
    ctx.check(lib.vsp_tally_result(ctx.h, t.h, p(ct), C.byref(ballots)))
    return ct, ballots.value


def receive(b, z, t):
    n = b["ct"].shape[0]
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8); wire = np.zeros((n, 3), np.uint8); accepted = C.c_size_t(0)
    ctx.check(lib.vsp_saver_receive_blobs(ctx.h, ver.h, t.h, p(b["ct"]), p(b["pr"]), p(b["inp"]), n, 1, p(z), p(verdict), p(reason), p(wire), C.byref(accepted)))
    assert not wire.any() and accepted.value == int(verdict.sum())
    return reason, None


def host_inputs(inp):
    """n input blobs -> (rest [n, N_REST, 4] canonical words, accepted [n]): the count header, the byte order, scalars below r"""
    n = inp.shape[0]
    ok = (inp[:, :7] == 0).all(axis=1) & (inp[:, 7] == N_REST)
    rest = np.ascontiguousarray(inp[:, 8:].reshape(n, N_REST, 32)[:, :, ::-1]).view(np.uint64).reshape(n, N_REST, 4)
    below = np.zeros((n, N_REST), bool); decided = np.zeros((n, N_REST), bool)
    for i in (3, 2, 1, 0):
        below |= ~decided & (rest[:, :, i] < R_WORDS[i]); decided |= rest[:, :, i] != R_WORDS[i]
    return rest, ok & below.all(axis=1)


def composition(b, z, t):
    """-> (reasons, stage time of the second decode)"""
    n = b["ct"].shape[0]
    records = np.ascontiguousarray(b["ct"][:, 8:])
    pts = np.zeros((n * CT_LEN, 12), np.uint64); st = np.zeros(n * CT_LEN, np.uint8)
    ctx.check(lib.vsp_g1_decompress_batch(ctx.h, p(records), n * CT_LEN, 1, p(pts), p(st)))
    A = np.zeros((n, 12), np.uint64); B = np.zeros((n, 24), np.uint64); Cc = np.zeros((n, 12), np.uint64); pst = np.zeros(n, np.uint8)
    ctx.check(lib.vsp_proof_from_blob_batch(ctx.h, p(b["pr"]), n, 1, p(A), p(B), p(Cc), p(pst)))
    rest, in_ok = host_inputs(b["inp"])
    assert not st.any() and not pst.any() and in_ok.all()              # (a wire-rejected ballot would be replaced by a malformed one here)
    verdict = np.zeros(n, np.uint8); reason = np.zeros(n, np.uint8)
    if z is not None:
        ctx.check(lib.vsp_saver_verify_batch_screened(ctx.h, ver.h, p(pts), p(rest), p(A), p(B), p(Cc), n, p(z), p(verdict), p(reason)))
    else:
        ctx.check(lib.vsp_saver_verify_batch(ctx.h, ver.h, p(pts), p(rest), p(A), p(B), p(Cc), n, p(verdict), p(reason)))
    first = sum(ctx.stat(s) for s in DECODE[:2])
    blobs = b["ct"] if verdict.all() else np.ascontiguousarray(b["ct"][verdict != 0])
    status = np.zeros(blobs.shape[0], np.uint8); accepted = C.c_size_t(0)
    ctx.check(lib.vsp_tally_add_blobs(ctx.h, t.h, p(blobs), blobs.shape[0], 1, p(status), C.byref(accepted)))
    assert accepted.value == blobs.shape[0]
    return reason, sum(ctx.stat(s) for s in DECODE[:2]) - first


def timed(fn, b, z, want):
    """one blocking call on a fresh tally -> (seconds, stage times, second-decode ms, the tally, verdicts as expected)"""
    t = v.Tally(ctx, CT_LEN)
    try:
        ctx.stats_reset()
        t0 = time.perf_counter(); reason, second = fn(b, z, t); dt = time.perf_counter() - t0
        return dt, {s: ctx.stat(s) for s in STAGES}, second, tally_result(t), bool(np.array_equal(reason, want))
    finally:
        t.free()


def stage_text(st, mode):
    pre = "saver_screen_" if mode == "screened" else "saver_verify_"
    verify = sum(val for key, val in st.items() if key.startswith(pre))
    return ("decode G1 %.1f + G2 %.1f, subgroup G1 %.1f + G2 %.1f, receive kernels %.1f, %s stages %.1f (prepare %.1f), tally sum %.1f ms"
            % (st["tally_decode_ms"], st["g2_decode_ms"], st["tally_subgroup_ms"], st["g2_subgroup_ms"], st["saver_receive_prepare_ms"], mode, verify, st[pre + "prepare_ms"],
               st["tally_sum_ms"]))


CASES = (("all valid", lambda n: []), ("one bad", lambda n: [n // 2 + 1]))
warm, wz, ww = batch(256, [100])
for z in (wz, None):                                                    # warm-up: code objects, scratch, workspaces
    timed(receive, warm, z, ww); timed(composition, warm, z, ww)
bar = True
for lg in LOGS:
    n = 1 << lg
    for name, bad in CASES:
        b, z, want = batch(n, bad(n))
        for mode, zz in (("screened", z), ("exact", None)):
            timed(receive, b, zz, want); timed(composition, b, zz, want)    # workspaces at this size
            best = {}
            agree = True
            for _ in range(REPS):
                for key, fn in (("receive", receive), ("composition", composition), ("composition'", composition)):
                    r = timed(fn, b, zz, want)
                    agree = agree and r[4]
                    if key not in best or r[0] < best[key][0]:
                        best[key] = r
            rc, ca, cb = best["receive"], best["composition"], best["composition'"]
            agree = agree and all(np.array_equal(rc[3][0], x[3][0]) and rc[3][1] == x[3][1] == n - len(bad(n)) for x in (ca, cb))
            comp, spread = min(ca[0], cb[0]), abs(ca[0] - cb[0])
            met = comp - rc[0] > spread and agree
            bar = bar and met
            second = ca[2] if ca[0] <= cb[0] else cb[2]
            saved = (comp - rc[0]) * 1e3
            say("2^%-2d ballots, %-9s, %-8s: receive %8.1f ms (%7.0f ballots/s)   composition %8.1f ms, again %8.1f ms (a/a spread %5.1f ms)   composition / receive %5.2f x   "
                "verdicts and tallies agree: %s   bar: %s" % (lg, name, mode, rc[0] * 1e3, n / rc[0], ca[0] * 1e3, cb[0] * 1e3, spread * 1e3, comp / rc[0], agree, "met" if met else "NOT met"))
            say("      receive:     " + stage_text(rc[1], mode))
            say("      composition: " + stage_text(ca[1] if ca[0] <= cb[0] else cb[1], mode))
            say("      the composition's second decode (tally_decode_ms + tally_subgroup_ms of its vsp_tally_add_blobs): %.1f ms; saved wall time %.1f ms = %.2f x of it"
                % (second, saved, saved / second if second else 0.0))
say("bar (the receive call faster than the composition by more than the a/a spread at every size, verdicts and tallies agree): %s" % ("met" if bar else "NOT met"))
ver.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
