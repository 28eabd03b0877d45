"""SAVER ballots screened in bulk (vsp_saver_verify_batch_screened) against the exact path (vsp_saver_verify_batch) on the same arrays in
the same process, the two calls alternated: msg_size 25 with 5 rest inputs, a pool of 2^10 distinct ballots of known logs
(tests/dlog_election.py) tiled to 2^12, 2^14 and 2^16 with distinct random coefficients -- duplicates are legal input.  Cases: all valid,
one bad ballot, 1 % bad ballots.  Wall time of the blocking calls after a warm-up, best of R (default 3); the stage timers and the
counters of the screened call; the sweeps of "saver_screen_chunk" over {2^12, 2^14, 2^16} and of "saver_screen_split" over {0, 4, 16, 64}.
Both calls must give the model's verdicts in every line.

    python3 tools/saver_screen_time.py       prints the report and writes it to profiles/saver_screen_time.txt (OUT=path for another file)"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))
import vote_saver_protocol_amd as v  # noqa: E402
import dlog_election as de  # noqa: E402  (ballots whose verdicts are integer congruences; not the thing measured)

N, N_REST, POOL = 25, 5, 1 << 10
LOGS = [int(x) for x in os.environ.get("LOGS", "12,14,16").split(",")]
REPS = int(os.environ.get("R", "3"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "saver_screen_time.txt"))
TIMERS = ("prepare", "scale", "miller", "msm", "finalexp")
COUNTS = ("checks", "failed", "exact_ballots")
DEFAULTS = dict(saver_screen_chunk=1 << 16, saver_screen_split=4)
ctx = v.Context(0)
report = []


def say(line):
    print(line, flush=True)
    report.append(line)


# ---- the election, the pool and one bad twin of every pool member (equation 2 fails)
rng = de.rng(2026)
t_make = time.perf_counter()
el = de.Election(rng, N, N_REST)
members = [de.make_ballot(el, [de.nonzero(rng) for _ in range(N + 1)], [rng.randrange(de.R) for _ in range(N_REST)], rng) for _ in range(POOL)]
pool = de.ballot_batch(el, members)
bad_C = de.g1_points([(m["z"] + 1) % de.R for m in members])
k = el.key
ver = v.SaverVerifier(ctx, el.pk_words, k.alpha, k.beta, k.gamma, k.delta, k.gamma_abc, N)
say("msg_size %d, %d rest inputs, a pool of %d distinct ballots of known logs, tiled: made in %.1f s" % (N, N_REST, POOL, time.perf_counter() - t_make))


def batch(n, bad):
    """n ballots tiled from the pool, the members of `bad` with C + G (reason 4) -> (arrays, expected reasons)"""
    idx = np.arange(n) % POOL
    b = {key: np.ascontiguousarray(pool[key][idx]) for key in ("ct", "rest", "A", "B", "C")}
    want = np.zeros(n, np.uint8)
    for i in bad:
        b["C"][i] = bad_C[i % POOL]; want[i] = 4
    z = np.random.default_rng(n).integers(0, 1 << 64, size=(n, 2), dtype=np.uint64)
    z[:, 0] |= np.uint64(1)                                             # not zero
    return b, z, want


def screened(b, z):
    return v.saver_verify_batch_screened(ctx, ver, b["ct"], b["rest"], b["A"], b["B"], b["C"], z)[1]


def exact(b):
    return v.saver_verify_batch(ctx, ver, b["ct"], b["rest"], b["A"], b["B"], b["C"])[1]


def alternate(b, z, want, with_exact=True):
    """best of REPS of each call, alternated -> (screened s, exact s, timers, counters, verdicts as expected)"""
    best_s = best_e = None
    ok = True
    for _ in range(REPS):
        ctx.stats_reset()
        t0 = time.perf_counter(); got = screened(b, z); dt = time.perf_counter() - t0
        ok = ok and np.array_equal(got, want)
        if best_s is None or dt < best_s[0]:
            best_s = (dt, [ctx.stat("saver_screen_%s_ms" % t) for t in TIMERS], [int(ctx.stat("saver_screen_" + c)) for c in COUNTS])
        if with_exact:
            t0 = time.perf_counter(); got = exact(b); dt = time.perf_counter() - t0
            ok = ok and np.array_equal(got, want)
            best_e = dt if best_e is None or dt < best_e else best_e
    return best_s[0], best_e, best_s[1], best_s[2], ok


def stage_text(tm, cn):
    return ("prepare %.1f, scale %.1f, miller + products %.1f, column sums %.1f, final exp %.1f ms; %d checks, %d failed, %d ballots to the exact path"
            % (tuple(tm) + tuple(cn)))


CASES = (("all valid", lambda n: []), ("one bad", lambda n: [n // 2 + 1]), ("1 % bad", lambda n: list(range(37, n, 100))))
warm, wz, _ = batch(256, [100])
screened(warm, wz); exact(warm)                                         # warm-up: code objects, scratch, workspaces
ratio_valid_14 = None
for lg in LOGS:
    n = 1 << lg
    for name, bad in CASES:
        b, z, want = batch(n, bad(n))
        screened(b, z); exact(b)                                        # workspaces at this size
        ds, dx, tm, cn, ok = alternate(b, z, want)
        say("2^%-2d ballots, %-9s: screened %8.1f ms (%7.0f ballots/s)   exact %8.1f ms (%7.0f ballots/s)   exact / screened %5.2f x%s   verdicts as expected: %s"
            % (lg, name, ds * 1e3, n / ds, dx * 1e3, n / dx, dx / ds, "  SLOWER than the exact path" if ds > dx else "", ok))
        say("      " + stage_text(tm, cn))
        if lg == 14 and name == "all valid":
            ratio_valid_14 = dx / ds
if ratio_valid_14 is not None:
    say("operation count per ballot (DESIGN.md 3.6f): exact 124 000 field products, screened about 20 000: predicted 6 x, measured %.2f x at 2^14, all valid" % ratio_valid_14)

# ---- the sweeps: the piece size on valid ballots (no second level runs), the split on one failing piece of the default size
n = 1 << max(LOGS)
b, z, want = batch(n, [])
for chunk in (1 << 12, 1 << 14, 1 << 16):
    ctx.set_option("saver_screen_chunk", chunk)
    screened(b, z)
    ds, _, tm, cn, ok = alternate(b, z, want, with_exact=False)
    say("saver_screen_chunk 2^%d, 2^%d ballots, all valid: %8.1f ms (%7.0f ballots/s)   %s   verdicts as expected: %s"
        % (chunk.bit_length() - 1, n.bit_length() - 1, ds * 1e3, n / ds, stage_text(tm, cn), ok))
ctx.set_option("saver_screen_chunk", DEFAULTS["saver_screen_chunk"])
for name, bad in CASES[1:]:
    b, z, want = batch(n, bad(n))
    for split in (0, 4, 16, 64):
        ctx.set_option("saver_screen_split", split)
        screened(b, z)
        ds, _, tm, cn, ok = alternate(b, z, want, with_exact=False)
        say("saver_screen_split %2d, 2^%d ballots, %-7s: %8.1f ms (%7.0f ballots/s)   %s   verdicts as expected: %s"
            % (split, n.bit_length() - 1, name, ds * 1e3, n / ds, stage_text(tm, cn), ok))
ctx.set_option("saver_screen_split", DEFAULTS["saver_screen_split"])
ver.free()
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(report) + "\n")
