"""k_scatter_lds by number of rounds (option "msm_scatter_rounds") and problem size: the workload, and the report from a rocprofv3 run of it.

   rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/scatter_rounds_sweep.py run PLAN.json
   rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d DIR2 -- python3 tools/scatter_rounds_sweep.py run PLAN2.json
   python3 tools/scatter_rounds_sweep.py report PLAN.json DIR [PLAN2.json DIR2 ...]

run: G1 multi-exponentiations over plain bases at 2^LOG_N points (env LOG_N, default 18,20,22), 16-bit windows, one in flight, for
every number of rounds in env ROUNDS (default 1,2,4,8,16; 0 = the automatic choice), REPS (default 5) timed calls after one warm-up
each; every result is compared with the first of its size.  ONE set of 2^max(LOG_N) bases serves every size, and whether scalars are
split by the endomorphism is decided for that set when it is uploaded: above 2^20 points it is not, unless env MSM_GLV=2 forces it (option
"msm_glv").  So LOG_N=18,20,22 runs 16 windows of 2^LOG_N entries, LOG_N=19 alone 8 windows of 2^20: the report prints what ran.
All uploads come first, so the LAST launches of k_scatter_lds and k_count_lds in the trace are the plan's, in its order.  With VSP_LIB_PATH naming a library that does not know the option every row is
a single pass.
report: per (size, rounds) the median time of k_scatter_lds and of k_count_lds (kernel trace) and the mean of every counter found
(counter collection)."""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(plan_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import vote_saver_protocol_amd as v
    logs = [int(x) for x in os.environ.get("LOG_N", "18,20,22").split(",")]
    rounds = [int(x) for x in os.environ.get("ROUNDS", "1,2,4,8,16").split(",")]
    reps = int(os.environ.get("REPS", "5"))
    ctx = v.Context(0)
    ctx.set_option("msm_window_bits", 16)
    if os.environ.get("MSM_GLV"):
        ctx.set_option("msm_glv", int(os.environ["MSM_GLV"]))
    nmax = 1 << max(logs)
    rng = np.random.default_rng(11)

    def rand_fr(n):
        a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        return a

    d_k, d_s = ctx.to_device(rand_fr(nmax)), ctx.to_device(rand_fr(nmax))
    d_b = v.fixed_base_mul(ctx, d_k, nmax, 1)
    B = ctx.bases_from_device(d_b, nmax, 1)
    B.msm(d_s, n=1 << min(logs))                               # the context's self-checks and first-use work, before the plan's launches
    plan = []
    for lg in logs:
        first = None
        for r in rounds:
            ctx.set_option("msm_scatter_rounds", r)
            for _ in range(reps + 1):
                got, _inf = B.msm(d_s, n=1 << lg)
            first = got if first is None else first
            plan.append({"log_n": lg, "rounds": r, "rounds_run": int(ctx.stat("msm_scatter_rounds")), "launches": reps + 1, "windows": int(ctx.stat("msm_windows")),
                         "split": int(ctx.stat("msm_endomorphism_split")), "same_result": bool(np.array_equal(got, first))})
    json.dump({"library": os.environ.get("VSP_LIB_PATH", "shipped"), "plan": plan}, open(plan_path, "w"))
    B.free()
    for p in (d_k, d_s, d_b):
        ctx.dfree(p)
    ctx.close()
    print("ran", len(plan), "configurations; all results equal:", all(p["same_result"] for p in plan))


def _rows(d, suffix):
    f = glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True)
    return list(csv.DictReader(open(f[0]))) if f else []


def _of(rows, kernel):
    return [r for r in rows if kernel in r["Kernel_Name"]]


def report(pairs):
    for plan_path, d in pairs:
        meta = json.load(open(plan_path))
        plan = meta["plan"]
        total = sum(p["launches"] for p in plan)
        print("library:", "this commit" if meta["library"] == "shipped" else "VSP_LIB_PATH " + os.path.basename(meta["library"]), " trace:", os.path.basename(d.rstrip("/")))
        trace = sorted(_rows(d, "kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
        counters = _rows(d, "counter_collection.csv")
        for kernel in ("k_scatter_lds", "k_count_lds"):
            tr = _of(trace, kernel)[-total:]
            by_counter = {}
            for r in _of(counters, kernel):
                by_counter.setdefault(r["Counter_Name"], []).append(r)
            at = 0
            for p in plan:
                line = "  %-14s 2^%d  %2d windows%s  rounds %2d (ran %2d)" % (kernel, p["log_n"], p["windows"], ", split" if p["split"] else "", p["rounds"], p["rounds_run"])
                if len(tr) == total:
                    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in tr[at + 1:at + p["launches"]]]      # (skip the warm-up call)
                    line += "  median %8.1f us  min %8.1f  max %8.1f" % (statistics.median(us), min(us), max(us))
                for name, rows in sorted(by_counter.items()):
                    rows = (sorted(rows, key=lambda r: int(r["Dispatch_Id"])) if "Dispatch_Id" in rows[0] else rows)[-total:]
                    vals = [float(r["Counter_Value"]) for r in rows[at + 1:at + p["launches"]]]
                    if vals:
                        line += "  %s %12.0f" % (name, sum(vals) / len(vals))
                print(line + ("" if p["same_result"] else "  RESULT DIFFERS"))
                at += p["launches"]


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(list(zip(sys.argv[2::2], sys.argv[3::2])))
