"""bench.py end to end on the GPU: a plain run prints the headline line and nothing the headline does not need, its dumped result is
the right point (the plain run no longer checks it itself), and --full still adds the bit-exact check, the one-in-flight leg and the
roofline.  Small step counts: these check what the line carries, not how fast the steps are."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("verified_bit_exact", "latency_ms_one_in_flight", "roofline", "roofline_valu", "cpu_baseline", "cpu_baseline_all_cores",
             "extras", "secondary", "scaling_strong")


def run_bench(*args, timeout=600):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", *args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_right_point(tmp_path, cref):
    j = run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path), timeout=300)
    assert all(k in j for k in HEADLINE)
    assert j["unit"] == "points/s" and j["higher_is_better"] is True and j["dtype"] == "u32" and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0
    assert j["value"] == pytest.approx(j["config"]["points_per_gpu"] * 1e3 / j["ms_per_step"])
    assert not [k for k in FULL_ONLY if k in j]
    # the last timed step's result against the oracle: (sum_i k_i s_i) * G over bench.py's own synthetic inputs (bases k_i * G)
    import bls12_381 as o
    from bench import R_MOD, limbs, rand_fr, to_ints
    n = j["config"]["points_per_gpu"]
    e = int(sum((to_ints(rand_fr(n, seed=1000)) * to_ints(rand_fr(n, seed=2000))).tolist()) % R_MOD)
    want = cref.g1_mul(np.array(o.g1_to_limbs(o.G1.gen), dtype=np.uint64), limbs(e, 4))
    words = np.load(tmp_path / "msm_g1_result.npy")
    assert words.shape == (2, 12)
    got = words.reshape(-1).astype("<u4").view("<u8")
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64).reshape(-1))


@pytest.mark.gpu
def test_full_run_adds_the_checks_and_the_roofline():
    j = run_bench("--steps", "2", "--warmup", "1", "--full", "--no-extras", "--no-prove", "--no-config5", "--no-cpu-baseline", "--no-diag-clock")
    assert all(k in j for k in HEADLINE)
    assert j["verified_bit_exact"] is True
    assert j["latency_ms_one_in_flight"] > 0 and j["roofline"]["avg_launch_ms"] > 0 and j["roofline_valu"]["peak"] > 0
