"""The voter registry's timings (vsp_registry_build, vsp_pedersen_hash_batch, vsp_registry_paths, vsp_registry_from_blob) on one GPU, and
the same csrc/jubjub.h compiled by g++ -O2 on one CPU core beside them.  Steps, each in a process of its own under its own time limit
(the parent never opens the GPU and starts nothing more after a step that fails), each after a warm-up call, R (default 7) repetitions,
reported as min / median / max of the blocking call's wall time and the minimum of the kernels' time by HIP events:
    build16, build20   Registry.build over 2^16 / 2^20 random 255-bit keys, hash_leaves = 1 (2^17 - 1 / 2^21 - 1 hashes); the wall time
                       includes the upload of the keys
    hash510            2^16 hashes of 510 bits, a lane per hash (option "pedersen_lanes" = 1)
    paths              2^14 copaths of a tree of depth 20
    from_blob          Registry.from_blob of the depth-20 tree's blob (64 MiB) with verify = 1: the upload, the bit order, 2^20 - 1 hashes
    cpu                tests/cpu_build/jubjub_check.cpp (the header's own code, 64-bit limbs, a lane per hash) building a tree of depth 12
                       on one core -- SCALED by the node count to depths 16 and 20, and the report says so
Generators: tests/jubjub_model.py (SHA-256 try-and-increment, cofactor cleared); any generators cost the same.

    python3 tools/registry_time.py        prints the report and writes it to profiles/registry_time.txt (OUT=path for another file)"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))

REPS = int(os.environ.get("R", "7"))
OUT = os.environ.get("OUT", os.path.join(ROOT, "profiles", "registry_time.txt"))
LIMITS = {"build16": 120, "build20": 180, "hash510": 120, "paths": 180, "from_blob": 240, "cpu": 180}      # seconds
CPU_DEPTH = 12


def spread(xs):
    xs = sorted(xs)
    return "min %9.3f  median %9.3f  max %9.3f ms" % (xs[0], xs[len(xs) // 2], xs[-1])


def gpu_step(name):
    import numpy as np
    import jubjub_model as jm
    import vote_saver_protocol_amd as v
    ctx = v.Context(0)
    ped = v.Pedersen(ctx, np.array([jm.point_words(g) for g in jm.generators(3)], np.uint64))
    rng = np.random.default_rng(5)

    def keys(n):
        k = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        k[:, 3] >>= np.uint64(1)
        return k

    def measure(call, stat):
        call()                                                      # warm-up: code objects, workspaces at this size
        wall, events = [], []
        for _ in range(REPS):
            ctx.synchronize(); ctx.stats_reset()
            t0 = time.perf_counter(); call(); wall.append((time.perf_counter() - t0) * 1e3)
            events.append(ctx.stat(stat))
        return "wall %s   kernels by events: min %9.3f ms" % (spread(wall), min(events))

    if name in ("build16", "build20"):
        depth = int(name[5:])
        pks = keys(1 << depth)

        def call():
            v.Registry.build(ctx, ped, pks, depth).free()
        print("build, depth %d (%d hashes): %s" % (depth, (2 << depth) - 1, measure(call, "registry_build_ms")))
    elif name == "hash510":
        msgs = rng.integers(0, 1 << 64, size=(1 << 16, 8), dtype=np.uint64)
        ctx.set_option("pedersen_lanes", 1)
        print("2^16 hashes of 510 bits, a lane per hash: %s" % measure(lambda: v.pedersen_hash_batch(ctx, ped, msgs, 510), "pedersen_ms"))
    else:
        reg = v.Registry.build(ctx, ped, keys(1 << 20), 20)
        if name == "paths":
            idx = rng.integers(0, 1 << 20, size=1 << 14, dtype=np.uint64)
            print("2^14 copaths, depth 20: %s" % measure(lambda: reg.paths(idx), "registry_paths_ms"))
        else:
            blob = reg.to_blob()

            def call():
                r = v.Registry.from_blob(ctx, ped, blob, 20, verify=True)
                assert r.first_bad_node is None
                r.free()
            print("from_blob, depth 20, verify = 1 (%d MiB, %d hashes): %s" % (len(blob) >> 20, (1 << 20) - 1, measure(call, "registry_check_ms")))
        reg.free()
    ped.free()
    ctx.close()


def cpu_step():
    exe = os.path.join(os.environ.get("TMPDIR", "/tmp"), "jubjub_check_time_%d" % os.getpid())
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-DJUBJUB_CHECK_MAIN", "-o", exe, os.path.join(ROOT, "tests", "cpu_build", "jubjub_check.cpp")])
    try:
        ms = []
        for _ in range(3):
            out = subprocess.run([exe, str(CPU_DEPTH)], capture_output=True, text=True, check=True).stdout.split()
            ms.append(float(out[out.index("ms") + 1]))
    finally:
        os.unlink(exe)
    hashes = (2 << CPU_DEPTH) - 1
    best = min(ms)
    print("one CPU core, g++ -O2, the same jubjub.h on 64-bit limbs: depth %d (%d hashes) measured: %s = %.1f us per hash" % (CPU_DEPTH, hashes, spread(ms), best * 1e3 / hashes))
    for depth in (16, 20):
        print("      depth %d: %.1f s  -- NOT measured: the depth-%d time SCALED by the node count (%d / %d)" % (depth, best * ((2 << depth) - 1) / hashes / 1e3, CPU_DEPTH, (2 << depth) - 1, hashes))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        cpu_step() if sys.argv[1] == "cpu" else gpu_step(sys.argv[1])
        sys.exit(0)
    report = ["voter registry on one GPU, %d repetitions after a warm-up call; 3 generators; every step in its own process" % REPS]
    print(report[0], flush=True)
    for step in ("build16", "build20", "hash510", "paths", "from_blob", "cpu"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), step], capture_output=True, text=True, timeout=LIMITS[step])
        except subprocess.TimeoutExpired:
            report.append("%s: ended at its time limit of %d s; nothing further was started" % (step, LIMITS[step]))
            print(report[-1], flush=True)
            break
        lines = r.stdout.strip().splitlines()
        report += lines
        print("\n".join(lines), flush=True)
        if r.returncode != 0:
            report.append("%s: exit status %d; nothing further was started\n%s" % (step, r.returncode, r.stderr.strip()[-2000:]))
            print(report[-1], flush=True)
            break
    with open(OUT, "w") as f:
        f.write("\n".join(report) + "\n")
