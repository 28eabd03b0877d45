"""The ballot box (vsp_ballot_box_receive_blobs) against the plain receiving call (vsp_saver_receive_blobs), in one process and alternated:
msg_size 25 with 5 rest inputs eid | sn | rt | x | y under the roles FIXED, SERIAL, FIXED, FREE, FREE, 2^14 DISTINCT valid ballots of
known logs (tests/dlog_election.py; a serial is a public input, so every ballot has a proof of its own), as blobs; check_subgroup 1;
exact and screened.  Three things are measured, wall time of the blocking call on a fresh tally, best of R (default 5) after a warm-up:
    plain      vsp_saver_receive_blobs                              (twice, interleaved: |plain - plain'| is the a/a spread)
    distinct   the box call on a fresh box: every ballot is accepted and its serial committed
    replay     the box call on a box that already holds every serial of the batch: every ballot is turned away before the verifier
Reported: the box's overhead over the plain call on distinct ballots (against the spread), the replay batch's rate against the distinct
batch's, "ballot_box_ms" (the box's kernels by HIP events) and the stage split of the replay call -- which stages a replay still pays for.

    python3 tools/ballot_box_time.py     prints the report and writes it to profiles/ballot_box_time.txt (OUT=path for another file)"""
import ctypes as C
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import vote_saver_protocol_amd as v  # noqa: E402
import dlog_election as de  # noqa: E402  (ballots whose verdicts are integer congruences; not the thing measured)

N, N_REST = 25, 5
LOG = int(os.environ.get("LOG", "14"))
REPS = int(os.environ.get("R", "5"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "ballot_box_time.txt"))
CT_LEN = N + 2
ROLES = [v.api.FIXED, v.api.SERIAL, v.api.FIXED, v.api.FREE, v.api.FREE]
STAGES = ("tally_decode_ms", "tally_subgroup_ms", "g2_decode_ms", "g2_subgroup_ms", "saver_receive_prepare_ms", "ballot_box_ms", "tally_sum_ms")
VERIFY = ("saver_screen_prepare_ms", "saver_screen_scale_ms", "saver_screen_miller_ms", "saver_screen_msm_ms", "saver_screen_finalexp_ms", "saver_verify_prepare_ms",
          "saver_verify_miller_ms", "saver_verify_finalexp_ms")
ctx = v.Context(0)
lib, p = ctx.lib, v.api._ptr
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


rng = de.rng(2027)
t_make = time.perf_counter()
n = 1 << LOG
el = de.Election(rng, N, N_REST)
EID, RT = de.nonzero(rng), de.nonzero(rng)
members = [de.make_ballot(el, [de.nonzero(rng) for _ in range(N + 1)], [EID, 1 + i, RT, rng.randrange(de.R), rng.randrange(de.R)], rng) for i in range(n)]
batch = de.ballot_batch(el, members)
assert not any(batch["want"])
as_rows = lambda blobs: np.frombuffer(b"".join(blobs), np.uint8).reshape(len(blobs), -1)
ct = as_rows([v.g1_vector_to_blob(batch["ct"][i]) for i in range(n)])
pr = as_rows([v.g1_compress(batch["A"][i]) + v.g2_compress(batch["B"][i]) + v.g1_compress(batch["C"][i]) for i in range(n)])
inp = as_rows([v.fr_vector_to_blob(batch["rest"][i]) for i in range(n)])
serials = np.ascontiguousarray(batch["rest"][:, 1:2, :])
k = el.key
ver = v.SaverVerifier(ctx, el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, N)
expected = de._fr([EID, 0, RT, 0, 0])
z = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
z[:, 0] |= np.uint64(1)                                                 # not zero
say("msg_size %d, %d rest inputs (roles FIXED, SERIAL, FIXED, FREE, FREE), 2^%d distinct valid ballots of known logs as blobs; check_subgroup 1; best of %d: made in %.1f s"
    % (N, N_REST, LOG, REPS, time.perf_counter() - t_make))


def outputs():
    return np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros((n, 3), np.uint8), C.c_size_t(0), np.zeros(n, np.uint64)


def plain(zz, t, box):
    verdict, reason, wire, accepted, _ = outputs()
    ctx.check(lib.vsp_saver_receive_blobs(ctx.h, ver.h, t.h, p(ct), p(pr), p(inp), n, 1, p(zz) if zz is not None else None, p(verdict), p(reason), p(wire), C.byref(accepted)))
    return accepted.value == n and not reason.any()


def boxed(want_reason):
    def call(zz, t, box):
        verdict, reason, wire, accepted, holder = outputs()
        ctx.check(lib.vsp_ballot_box_receive_blobs(ctx.h, box.h, t.h, p(ct), p(pr), p(inp), n, 1, p(zz) if zz is not None else None, p(verdict), p(reason), p(wire),
                                                   C.byref(accepted), p(holder)))
        if want_reason == 0:
            return accepted.value == n and not reason.any() and box.count() == n
        return accepted.value == 0 and (reason == 16).all() and np.array_equal(holder, np.arange(n, dtype=np.uint64)) and box.count() == n
    return call


def timed(fn, zz, filled):
    """one blocking call on a fresh tally and a fresh box (filled: holding the batch's serials already) -> (seconds, stage times, as expected)"""
    t, box = v.Tally(ctx, CT_LEN), v.BallotBox(ctx, ver, expected, ROLES)
    try:
        if filled:
            status, added = box.add_serials(serials)
            assert added == n and not status.any()
        ctx.synchronize()
        ctx.stats_reset()
        t0 = time.perf_counter(); ok = fn(zz, t, box); dt = time.perf_counter() - t0
        st = {s: ctx.stat(s) for s in STAGES}
        st["verify"] = sum(ctx.stat(s) for s in VERIFY)
        ballots = t.result()[1]
        return dt, st, ok and ballots == (0 if filled else n)
    finally:
        box.free(); t.free()


def stage_text(st):
    return ("decode G1 %.1f + G2 %.1f, subgroup G1 %.1f + G2 %.1f, receive kernels %.1f, box kernels %.2f, verifier stages %.1f, tally sum %.1f ms"
            % (st["tally_decode_ms"], st["g2_decode_ms"], st["tally_subgroup_ms"], st["g2_subgroup_ms"], st["saver_receive_prepare_ms"], st["ballot_box_ms"], st["verify"],
               st["tally_sum_ms"]))


SERIES = (("plain", plain, False), ("distinct", boxed(0), False), ("replay", boxed(16), True), ("plain'", plain, False))
for mode, zz in (("exact", None), ("screened", z)):
    for name, fn, filled in SERIES[:3]:                                 # warm-up: code objects, scratch, workspaces at this size
        timed(fn, zz, filled)
    best, agree = {}, True
    for _ in range(REPS):
        for name, fn, filled in SERIES:
            r = timed(fn, zz, filled)
            agree = agree and r[2]
            if name not in best or r[0] < best[name][0]:
                best[name] = r
    pa, pb, di, re = best["plain"], best["plain'"], best["distinct"], best["replay"]
    base, spread = min(pa[0], pb[0]), abs(pa[0] - pb[0])
    say("2^%d ballots, %-8s: plain %8.1f ms, again %8.1f ms (a/a spread %5.1f ms, %7.0f ballots/s)   box, distinct %8.1f ms (%7.0f ballots/s)   box, replay %8.1f ms (%7.0f ballots/s)   "
        "results as expected: %s" % (LOG, mode, pa[0] * 1e3, pb[0] * 1e3, spread * 1e3, n / base, di[0] * 1e3, n / di[0], re[0] * 1e3, n / re[0], agree))
    say("      the box's overhead on distinct ballots: %+.1f ms = %+.1f %% of the plain call (spread %.1f ms); its kernels by HIP events: %.2f ms"
        % ((di[0] - base) * 1e3, (di[0] - base) / base * 100, spread * 1e3, di[1]["ballot_box_ms"]))
    say("      replay / distinct rate: %.2f x" % (di[0] / re[0]))
    say("      plain:    " + stage_text(pa[1] if pa[0] <= pb[0] else pb[1]))
    say("      distinct: " + stage_text(di[1]))
    say("      replay:   " + stage_text(re[1]))
ver.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
