"""The witness check (vsp_r1cs_check_batch: the prover's front half and k_r1cs_verdict) against the only path there was before it, the
oracle's is_satisfied on one host core, and the cost of option "prove_check_witness" inside the prover.

    python3 tools/r1cs_check_time.py              both parts
    PART=check | prove python3 tools/...          one of them
    PKG_ROOT=<tree> PART=prove python3 tools/...  the prover part over another build of the package (a parent commit: option 0 only)

check: 2^16 constraints x 32 witnesses and 2^20 x 1 -- wall time of the blocking call, "r1cs_check_ms" (the verdict kernels) and
       "r1cs_check_front_ms" (upload, mat-vecs), best of R and the spread; the verdict kernels' time against the 3 x 32 bytes per row and
       member they must read; the oracle on the same witnesses.
prove: vsp_groth16_prove at 2^20 and vsp_groth16_prove_batch (32 members) at 2^16 with the option 0 and 1 on the same build, interleaved
       call by call after a warm-up; best, median and spread of each."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_ROOT = os.environ.get("PKG_ROOT", ROOT)
sys.path.insert(0, PKG_ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import vote_saver_protocol_amd as v  # noqa: E402
import cref  # noqa: E402  (the yardstick and the generator of the synthetic system, not the thing measured)

PART = os.environ.get("PART", "both")
REPS = int(os.environ.get("R", "9"))
LOG_BIG = int(os.environ.get("LOG_BIG", "20"))
LOG_SMALL = int(os.environ.get("LOG_SMALL", "16"))
MEMBERS = int(os.environ.get("MEMBERS", "32"))
HAS_CHECK = hasattr(v.R1CS, "check")
ctx = v.Context(0)
rng = np.random.default_rng(5)


def rand_fr(n):
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return a


def system(log_nc, ni=3):
    nc = (1 << log_nc) - ni - 1                               # the domain is exactly 2^log_nc
    cs, wit = cref.R1CS.synth(nc, ni, 40 + log_nc)
    return cs, wit, v.R1CS(ctx, nc, ni, cs.num_vars, *cs.export())


def spread(xs):
    xs = sorted(xs)
    return "best %8.3f  median %8.3f  worst %8.3f ms" % (xs[0], xs[len(xs) // 2], xs[-1])


def part_check():
    for log_nc, K in ((LOG_SMALL, MEMBERS), (LOG_BIG, 1)):
        cs, wit, dcs = system(log_nc)
        wits = np.ascontiguousarray(np.broadcast_to(wit, (K,) + wit.shape))
        bad = wits.copy(); bad[K - 1, cs.num_vars - 1] = [5, 0, 0, 0]      # the last wire (a boolean one or a product): the last row fails
        dcs.check(ctx, wits)                                               # warm-up: code objects, workspaces
        wall, kern, front = [], [], []
        for _ in range(REPS):
            ctx.stats_reset()
            t0 = time.perf_counter()
            status, first, nbad = dcs.check(ctx, wits)
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(ctx.stat("r1cs_check_ms")); front.append(ctx.stat("r1cs_check_front_ms"))
            assert not status.any() and (first == dcs.num_constraints).all() and not nbad.any()
        sb, fb, nb = dcs.check(ctx, bad)
        assert sb.tolist() == [0] * (K - 1) + [2] and fb[K - 1] == dcs.num_constraints - 1 and nb[K - 1] == 1
        t0 = time.perf_counter()
        n_ref = min(K, 4)
        assert all(cs.is_satisfied(wits[k]) for k in range(n_ref)) and not cs.is_satisfied(bad[K - 1])
        ref_ms = (time.perf_counter() - t0) * 1e3 / (n_ref + 1) * K
        rows_bytes = 3 * 32 * dcs.num_constraints * K
        print("check 2^%d constraints x %d witnesses" % (log_nc, K))
        print("  blocking call      %s" % spread(wall))
        print("  r1cs_check_ms      %s   (verdict kernels; they read %.1f MB: %.0f GB/s at the best time)" % (spread(kern), rows_bytes / 1e6, rows_bytes / min(kern) / 1e6))
        print("  r1cs_check_front_ms %s  (upload of %.1f MB and the three mat-vecs)" % (spread(front), wits.nbytes / 1e6))
        print("  oracle is_satisfied, one core: %.1f ms for the %d witnesses (%.1f ms each) -> %.1f x the blocking call's best" % (ref_ms, K, ref_ms / K, ref_ms / min(wall)))
        dcs.free(); cs.free()


def part_prove():
    tox, rs = rand_fr(5), rand_fr(2 * MEMBERS)
    for log_nc, K in ((LOG_BIG, 1), (LOG_SMALL, MEMBERS)):
        cs, wit, dcs = system(log_nc)
        kp = v.Keypair(ctx, dcs, tox)
        wits = np.ascontiguousarray(np.broadcast_to(wit, (K,) + wit.shape))
        r, s = rs[:K], rs[MEMBERS:MEMBERS + K]

        def once(option):
            if HAS_CHECK:
                ctx.set_option("prove_check_witness", option)
            t0 = time.perf_counter()
            out = v.groth16_prove(ctx, dcs, kp.pk, wit, r[0], s[0]) if K == 1 else v.groth16_prove_batch(ctx, dcs, kp.pk, wits, r, s)
            return (time.perf_counter() - t0) * 1e3, out[3]
        options = (0, 1) if HAS_CHECK else (0,)
        for _ in range(3):
            for op in options:
                once(op)
        times = {op: [] for op in options}
        proofs = {}
        for _ in range(REPS * 3):
            for op in options:                                              # interleaved: 0, 1, 0, 1, ...
                ms, proofs[op] = once(op)
                times[op].append(ms)
        name = "vsp_groth16_prove 2^%d" % log_nc if K == 1 else "vsp_groth16_prove_batch 2^%d x %d" % (log_nc, K)
        for op in options:
            print("%s  prove_check_witness %d  %s  (%d calls)" % (name, op, spread(times[op]), len(times[op])))
        if HAS_CHECK:
            assert proofs[0] == proofs[1]
            med = [sorted(times[op])[len(times[op]) // 2] for op in options]
            print("  option 1 - option 0: best %+.3f ms, median %+.3f ms; spread of option 0 itself (worst - best): %.3f ms"
                  % (min(times[1]) - min(times[0]), med[1] - med[0], max(times[0]) - min(times[0])))
        kp.free(); dcs.free(); cs.free()


print("package: %s   witness check available: %s" % (os.path.dirname(v.__file__), HAS_CHECK))
if PART in ("both", "check") and HAS_CHECK:
    part_check()
if PART in ("both", "prove"):
    part_prove()
ctx.close()
