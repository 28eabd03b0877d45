"""The voting circuit's witness step (vsp_vote_witness_batch, vsp_vote_cast_batch) on one GPU at depth 20, eid_bits 64, n 25, 3 generators,
and the header's host path (csrc/vote_circuit.h compiled by g++ -O2) on one CPU core beside it.  Steps, each in a process of its own
under its own time limit (the parent never opens the GPU and starts nothing more after a step that fails), each after a warm-up call, R
(default 5) repetitions, reported as min / median / max:
    witness   K = 1, 8, 64 ballots of registered voters: the blocking call's wall time (the witnesses land in host memory) and the
              kernels' time by HIP events ("vote_witness_ms"), as witnesses per second of the median
    cast      K = 1, 8, 64: vsp_vote_cast_batch with option vote_cast_device = 0 beside vsp_saver_encrypt_batch on witnesses made
              beforehand, the same key, the same process: what the witness step and its round trip through host memory cost a ballot
    device    K = 1, 8, 64, four legs alternated in one process: vsp_vote_cast_batch with vote_cast_device = 0 (the witnesses through
              host memory: the yardstick), with vote_cast_device = 1 (the witnesses stay on the device), vsp_saver_encrypt_batch on ready
              witnesses, and vsp_cast_batch_launch / _finish from one thread with two contexts and two circuits (two batches of K a
              repetition, reported per batch)
    cpu       tests/cpu_build/vote_circuit_check.cpp: one ballot's witness by the header's host path, one core

    python3 tools/vote_witness_time.py          witness, cast and cpu: prints the report and writes it to profiles/vote_witness_time.txt
    python3 tools/vote_witness_time.py report device    the device step alone, to profiles/vote_cast_device_time.txt
    (OUT=path for another file)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

REPS = int(os.environ.get("R", "5"))
LIMITS = {"witness": 240, "cast": 420, "device": 400, "cpu": 120}   # seconds
DEPTH, EID_BITS, N, KS = 20, 64, 25, (1, 8, 64)


def spread(xs):
    xs = sorted(xs)
    return "min %9.3f  median %9.3f  max %9.3f ms" % (xs[0], xs[len(xs) // 2], xs[-1])


def median(xs):
    return sorted(xs)[len(xs) // 2]


def gpu_step(name):
    import numpy as np
    import jubjub_model as jm
    import vote_saver_protocol_amd as v
    ctx = v.Context(0)
    ped = v.Pedersen(ctx, np.array([jm.point_words(g) for g in jm.generators(3)], np.uint64))
    rng = np.random.default_rng(7)

    def keys(n):
        k = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        k[:, 3] >>= np.uint64(1)
        return k

    def fr(n):
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        return a

    # 64 voters at scattered leaves of a full tree of 2^20 keys
    sks = keys(64)
    idx = np.sort(rng.choice(1 << DEPTH, size=64, replace=False)).astype(np.uint64)
    pks = keys(1 << DEPTH)
    pks[idx] = v.pedersen_hash_batch(ctx, ped, sks, 255)
    reg = v.Registry.build(ctx, ped, pks, DEPTH)
    circ = v.VoteCircuit(ctx, ped, N, EID_BITS, DEPTH)
    eid = np.array([0x0123456789ABCDEF], np.uint64)
    votes = (np.arange(64) % N).astype(np.uint32)
    print("circuit: num_constraints %d  num_inputs %d  num_vars %d  domain %d (%s)" % (circ.num_constraints, circ.num_inputs, circ.num_vars, circ.cs.m, circ.cs.domain_kind))

    if name == "witness":
        for K in KS:
            def call():
                _, status = circ.witness_batch(reg, eid, sks[:K], idx[:K], votes[:K])
                assert not status.any()
            call()
            wall, events = [], []
            for _ in range(REPS):
                ctx.synchronize(); ctx.stats_reset()
                t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
                events.append(ctx.stat("vote_witness_ms"))
            print("witness K = %2d: wall %s = %8.1f witnesses/s   kernels by events %s = %8.1f witnesses/s" %
                  (K, spread(wall), K * 1e3 / median(wall), spread(events), K * 1e3 / median(events)))
    else:
        kp = v.Keypair(ctx, circ.cs, fr(5), precompute=17, precompute_window=14)
        parts = {k: kp.part(k) for k in ("gamma_ABC_g1", "delta_g1", "gamma_g1")}
        gabc = np.ascontiguousarray(parts["gamma_ABC_g1"])
        pk_w, _, _ = v.saver_generate_keypair(ctx, fr(3 * N + 2), gabc, parts["delta_g1"][0], parts["gamma_g1"][0], N)
        spk = v.SaverPublicKey(ctx, pk_w, gabc[:N + 1], N)
        ctx2 = circ2 = None
        if name == "device":                                        # the second context and circuit of the launch / finish leg
            ctx2 = v.Context(0)
            circ2 = v.VoteCircuit(ctx2, ped, N, EID_BITS, DEPTH)

        def cast_with(option, K, rnd):
            ctx.set_option("vote_cast_device", option)
            try:
                return circ.cast_batch(reg, spk, kp.pk, eid, sks[:K], idx[:K], votes[:K], *rnd)
            finally:
                ctx.set_option("vote_cast_device", 1)

        def two_contexts(K, rnd):
            args = (reg, spk, kp.pk, eid, sks[:K], idx[:K], votes[:K]) + tuple(rnd)
            circ.cast_batch_launch(*args); circ2.cast_batch_launch(*args)
            circ.cast_batch_finish(); circ2.cast_batch_finish()

        for K in KS:
            rnd = [fr(K) for _ in range(3)]
            wit, status = circ.witness_batch(reg, eid, sks[:K], idx[:K], votes[:K])
            assert not status.any()
            msgs = np.ascontiguousarray(wit[:, :N])
            legs = {"cast_batch": lambda: cast_with(0, K, rnd),
                    "encrypt_batch on ready witnesses": lambda: v.saver_encrypt_batch(ctx, spk, circ.cs, kp.pk, msgs, wit, *rnd)}
            per_call = {}
            if name == "device":
                legs = {"cast_batch, vote_cast_device 0": legs["cast_batch"], "cast_batch, vote_cast_device 1": lambda: cast_with(1, K, rnd),
                        "encrypt_batch on ready witnesses": legs["encrypt_batch on ready witnesses"],
                        "launch / finish, two contexts (per batch)": lambda: two_contexts(K, rnd)}
                per_call = {"launch / finish, two contexts (per batch)": 2}
            ms = {}
            for leg, call in legs.items():
                call()
                ms[leg] = []
            for _ in range(REPS):                                   # the two legs alternate, so that drift meets both
                for leg, call in legs.items():
                    ctx.synchronize()
                    if ctx2:
                        ctx2.synchronize()
                    t0 = time.perf_counter(); call(); ms[leg].append((time.perf_counter() - t0) * 1e3 / per_call.get(leg, 1))
            for leg in legs:
                print("K = %2d %-42s wall %s = %8.1f ballots/s" % (K, leg + ":", spread(ms[leg]), K * 1e3 / median(ms[leg])))
        if circ2:
            circ2.free(); ctx2.close()
        spk.free(); kp.free()
    circ.free(); reg.free(); ped.free()
    ctx.close()


def cpu_step():
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "vote_circuit_check_time_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DVOTE_CIRCUIT_CHECK_MAIN", "-o", exe, os.path.join(ROOT, "tests", "cpu_build", "vote_circuit_check.cpp")])
    try:
        out = subprocess.run([exe, str(DEPTH), str(EID_BITS), str(N), "8"], capture_output=True, text=True, check=True).stdout.splitlines()
    finally:
        os.unlink(exe)
    ms = [float(l.split()[-1]) for l in out if "witness_ms" in l][1:]      # the first repetition warms the caches
    print("one CPU core, g++ -O2, the same vote_circuit.h on 64-bit limbs, one ballot a call: %s = %.1f witnesses/s" % (spread(ms), 1e3 / median(ms)))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] != "report":
        cpu_step() if sys.argv[1] == "cpu" else gpu_step(sys.argv[1])
        sys.exit(0)
    steps = sys.argv[2:] if len(sys.argv) > 2 and sys.argv[1] == "report" else ("witness", "cast", "cpu")
    OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "vote_cast_device_time.txt" if tuple(steps) == ("device",) else "vote_witness_time.txt"))
    report = ["voting circuit witnesses on one GPU: depth %d, eid_bits %d, n %d, 3 generators; %d repetitions after a warm-up call; every step in its own process" %
              (DEPTH, EID_BITS, N, REPS)]
    print(report[0], flush=True)
    for i, step in enumerate(steps):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            report.append("%s: ended at its time limit of %d s; nothing further was started" % (step, LIMITS[step]))
            print(report[-1], flush=True)
            break
        lines = r.stdout.strip().splitlines()
        if i and step != "cpu" and lines:
            lines = lines[1:]                                       # the circuit's sizes were printed by the first step
        report += lines
        print("\n".join(lines), flush=True)
        if r.returncode != 0:
            report.append("%s: exit status %d; nothing further was started\n%s" % (step, r.returncode, r.stderr.strip()[-2000:]))
            print(report[-1], flush=True)
            break
    with open(OUT, "w") as f:
        f.write("\n".join(report) + "\n")
