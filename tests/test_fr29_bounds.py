"""CPU: mechanical check of the bound discipline of the 9 x 29-bit lazy Fr arithmetic the NTT butterflies run on
(vote_saver_protocol_amd/csrc/fr29.h, k_ntt29_pass in ntt.hip), with the constants parsed from the generated header:

 1. an exact limb-level model of vsp_mm29 (the column schedule of tools/gen_mont_asm.py body29) asserting that no column reaches
    2^64, and of the radix-2 / radix-4 butterflies, driven through whole transforms of random and of adversarial data -- every
    intermediate is checked (no 32-bit limb wraps in either direction, every subtrahend is dominated by the 2r constant, every
    product operand stays below 2^261) and the result is the plain big-integer DFT;
 2. a worst-case propagation (value bound and per-limb bound) through the butterfly, showing that 11 radix-4 steps from a canonical
    input (the deepest transform the pass plan allows is 2^28: 14 steps -- checked too) keep every constraint;
 3. the transform's FIRST stage as the kernel runs it -- its twiddle is one, so the loaded values themselves are subtrahends -- for
    each of the three loads (plain, coset-premultiplied, witness_map's fused a b - c), in the propagation and in the exact model at
    the two ends of the fused load's range.
The model itself is oracle/fr29_model.py (tests/test_gpu_ntt_structured.py crafts its inputs with it).  No GPU needed; tests/test_gpu_ntt.py and tests/test_gpu_domain.py compare the kernels with the oracle's transforms bit for bit."""
import random

import pytest

import bls12_381 as o
from fr29_model import (B, K, K2, K4, LOW_TRIPLE, MASK, N, R, RL, RP, W, Bound, add29, b_add, b_mul, b_norm, b_sub, b_transform, brev,
                        csub29, first_stage_sources, fused_load, high_triple, mm29, model_ntt, norm29, radix4, sub29, tight, tw, val)


def test_constants():
    assert val(RL) == R and RL == tight(R) and RL[0] == 1                 # r = 1 mod 2^29: m_k is a negation
    assert (-pow(R, -1, 1 << W)) % (1 << W) == MASK
    assert val(K["FR29_ONE"]) == RP % R and val(K["FR29_R2"]) == RP * RP % R
    assert val(K2) == 2 * R and all(x >= MASK for x in K2[:-1]) and all(x < 1 << 31 for x in K2)
    assert val(K["FR29_K4_L1"]) == 4 * R
    # the top limb of 2r (after lending one unit) dominates the top limb of anything below 1.9 r
    assert K2[-1] >= (19 * R // 10) >> (W * (N - 1))


@pytest.mark.parametrize("log_n", [1, 2, 3, 6, 7])
def test_exact_model_transform_matches_the_dft(log_n):
    rng = random.Random(log_n)
    n = 1 << log_n
    for kind in ("random", "max"):
        vals = [rng.randrange(R) for _ in range(n)] if kind == "random" else [R - 1] * n
        got, worst = model_ntt(vals, log_n)
        assert got == o.dft_naive(vals, o.fr_root_of_unity(log_n))
        assert worst < (1 + 4 * ((log_n + 1) // 2) + 1) * R                 # V + 4r per step (one more for the radix-2 stage)


def test_product_column_bound_at_the_loosest_operands():
    """the largest limbs a data operand reaches inside a butterfly: a3 = x2 + 2r - x3, below 2^29 + 2^30 per limb, against a tight twiddle"""
    a = [(1 << 29) - 1 + K2[i] for i in range(N - 1)] + [(40 * R) >> (W * (N - 1))]
    assert max(a[:-1]) < 1 << 31 and val(a) < RP
    mm29(a, tight(R - 1))
    mm29(a, [MASK] * (N - 1) + [(R - 1) >> (W * (N - 1))])                # every twiddle limb at its maximum
    with pytest.raises(Bound):
        mm29([0xFFFFFFFF] * N, [MASK] * N)


# ------------------------------------------------------------------------------------------------ worst-case propagation
@pytest.mark.parametrize("steps", [11, 14])
def test_bounds_are_inductive_over_a_whole_transform(steps):
    """from a canonical input (or a coset-shifted one: a product output below 1.02 r) through `steps` radix-4 steps -- 11 for 2^22,
    14 for the largest supported transform 2^28 -- every constraint holds and the value stays below 2^261 = 70.4 r"""
    w = B.tight(R)                                                        # twiddles are canonical
    V = B.tight(R + R // 50)
    for step in range(steps):
        x1 = b_mul(V, w); assert x1.v < 1.9 * R
        a0, a1 = b_add(V, x1), b_sub(V, x1)
        p2, p3 = b_mul(a0, w), b_mul(a1, w); assert p3.v < 1.9 * R
        outs = [b_norm(b_add(a0, p2)), b_norm(b_add(a1, p3)), b_norm(b_sub(a0, p2)), b_norm(b_sub(a1, p3))]
        V = B.tight(max(x.v for x in outs))
        assert V.v <= (103 + 400 * (step + 1)) * R // 100                 # + 4r per step
    assert V.v < RP
    # leaving the lazy domain: the product with the scale (or the Montgomery one) is below 2r, one conditional subtraction follows
    assert b_mul(V, w).v < 2 * R


def test_the_model_notices_a_broken_bound():
    with pytest.raises(Bound):
        b_sub(B.tight(R), B.tight(3 * R))                                 # a subtrahend that is not a product output
    with pytest.raises(Bound):
        sub29(tight(5), tight(2 * R + 5))
    with pytest.raises(Bound):
        b_mul(B(RP, [1 << 32] * N), B.tight(R))


def test_fused_pointwise_load_of_witness_map_stays_inside_the_lazy_domain():
    """round 4: the first pass of witness_map's last transform computes its own input, (a b - c) / 2^261, from canonical a, b, c
    (k_ntt29_pass, NttPass29Args.fuse_b / fuse_c): two products of tight operands, the lazy subtraction (its subtrahend IS a product
    output), one carry pass.  Exact model on edge and random values against plain integers; then the worst-case propagation of a whole
    transform starting from that bound (3.03 r instead of a canonical input's 1.02 r) -- 11 steps (2^22) and 14 (2^28) keep every constraint."""
    rng = random.Random(29)
    one = [1] + [0] * (N - 1)
    rinv = pow(RP, -1, R)
    edge = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (1 << 254) - 1, (1 << 29) - 1, 1 << 29]
    cases = [(a, b, c) for a in edge for b in edge for c in edge] + [(rng.randrange(R), rng.randrange(R), rng.randrange(R)) for _ in range(300)]
    worst = 0
    for a, b, c in cases:
        v = norm29(sub29(mm29(tight(a), tight(b)), mm29(tight(c), one)))
        assert val(v) % R == (a * b - c) * rinv % R
        assert all(x <= MASK for x in v[:-1])
        worst = max(worst, val(v))
    assert worst < 3.03 * R
    w = B.tight(R)
    for steps in (11, 14):
        V = B.tight(int(3.03 * R))
        for step in range(steps):
            x1 = b_mul(V, w); assert x1.v < 1.9 * R
            a0, a1 = b_add(V, x1), b_sub(V, x1)
            p2, p3 = b_mul(a0, w), b_mul(a1, w); assert p3.v < 1.9 * R
            outs = [b_norm(b_add(a0, p2)), b_norm(b_add(a1, p3)), b_norm(b_sub(a0, p2)), b_norm(b_sub(a1, p3))]
            V = B.tight(max(x.v for x in outs))
        assert V.v < RP and b_mul(V, w).v < 2 * R


# ------------------------------------------------------------------------------------------------ the first stage, as the kernel runs it
FUSED_BOUND = int(3.03 * R)              # test_fused_pointwise_load_of_witness_map_stays_inside_the_lazy_domain: the fused load stays below


@pytest.mark.parametrize("steps", [11, 14])
@pytest.mark.parametrize("odd", [False, True])
def test_first_stage_of_the_plain_and_the_premultiplied_load(steps, odd):
    """the first stage skips its twiddle product (the twiddle is one), so x1, x3 (radix-4) or v (the radix-2 stage of an odd stage
    count) are subtrahends as loaded.  A plain load is canonical and a coset-premultiplied one is a product output below 1.02 r: 2r
    dominates both, and the growth is no more than the later steps'."""
    w = B.tight(R)
    canonical = B.tight(R)
    premultiplied = b_mul(B.tight(R), b_mul(w, w))                        # v * (pw_lo * pw_hi): both products of canonical operands
    assert premultiplied.v < 1.02 * R
    for V in (canonical, premultiplied):
        trace = b_transform(V, steps, odd=odd)
        assert trace[0] <= 5.02 and trace[-1] <= 1.02 + 4 * len(trace)    # + 4r per stage, the first included


@pytest.mark.parametrize("odd", [False, True])
def test_first_stage_with_2r_rejects_the_fused_load(odd):
    """REGRESSION of the finding: the fused load is a lazy value up to 3.02 r, not a product output; a first stage that subtracts it
    against 2r (the kernel before sub29k4) breaks the bound discipline -- 2r's top limb does not dominate it."""
    with pytest.raises(Bound, match="2r does not dominate"):
        b_transform(B.tight(FUSED_BOUND), 11, odd=odd, k_first=K2)
    lo, hi = fused_load(*LOW_TRIPLE), fused_load(*high_triple())
    with pytest.raises(Bound, match="borrows in limb 8"):
        sub29(lo, hi)
    assert hi[-1] > K2[-1] + lo[-1]


@pytest.mark.parametrize("steps", [11, 14])
@pytest.mark.parametrize("odd", [False, True])
def test_first_stage_with_4r_accepts_the_fused_load(steps, odd):
    """the fixed first stage (k_ntt29_pass with FUSED: sub29k4) subtracts the raw fused values against the redundant 4r.  4r dominates
    3.03 r limb by limb; the stage grows more than a later one (a0 = x0 + x1 has no product on x1: 3.03 r -> 9.03 r instead of + 4r,
    and -> 7.03 r through the radix-2 stage), and the deepest plan -- 14 radix-4 steps, 2^28 -- still ends below 2^261 = 70.4 r with
    its last product below 2r."""
    assert all(k >= l - 1 for k, l in zip(K4, B.tight(FUSED_BOUND).l)) and all(x < 1 << 31 for x in K4)
    trace = b_transform(B.tight(FUSED_BOUND), steps, odd=odd, k_first=K4)
    assert trace[0] <= (7.04 if odd else 9.04)
    assert trace[-1] <= trace[0] + 4 * (len(trace) - 1) + 0.01 and trace[-1] < 64


def _extreme_fused_inputs(log_n, run):
    """canonical (a, b, c) per natural-order position: the low / high triple laid out so that the values the first stage combines take
    every pattern -- group q of run `run` gets pattern (q + run * groups) mod 16, bit j deciding x_j"""
    lo, hi = LOW_TRIPLE, high_triple()
    groups = first_stage_sources(log_n)
    trip = [None] * (1 << log_n)
    for q, src in enumerate(groups):
        pattern = (q + run * len(groups)) % 16
        for j, i in enumerate(src):
            trip[i] = hi if pattern >> j & 1 else lo
    return trip


@pytest.mark.parametrize("log_n", [2, 3, 6, 7])
def test_exact_model_transform_of_extreme_fused_inputs(log_n):
    """witness_map's last transform in the exact model, from the two ends of the fused load's range (r + 1 and above 3.0 r) in every
    low / high pattern over a first-stage butterfly -- all 16 over (x0, x1, x2, x3), which hold the 4 over the radix-2 stage's (u, v):
    no bound is broken with the 4r first stage and the result is the plain inverse DFT of (a b - c) / 2^261; with the 2r first stage
    the model raises."""
    lo, hi = fused_load(*LOW_TRIPLE), fused_load(*high_triple())
    assert val(lo) == R + 1 and val(hi) >= 3 * R and val(hi) < FUSED_BOUND
    n = 1 << log_n
    groups = n // 4
    omega_inv = pow(o.fr_root_of_unity(log_n), -1, R)
    rinv, ninv = pow(RP, -1, R), pow(n, -1, R)
    seen = set()
    for run in range(max(1, 16 // groups)):
        trip = _extreme_fused_inputs(log_n, run)
        for q, src in enumerate(first_stage_sources(log_n)):
            seen.add(tuple(trip[i] is not LOW_TRIPLE for i in src))
        loaded = [fused_load(*t) for t in trip]
        got, worst = model_ntt(loaded, log_n, omega=omega_inv, k_first=K4, scale=ninv, loaded=True)
        plain = [(a * b - c) * rinv % R for a, b, c in trip]
        assert got == [x * ninv % R for x in o.dft_naive(plain, omega_inv)]
        assert worst < ((7.03 + 4 * (log_n // 2)) if log_n & 1 else (9.03 + 4 * (log_n // 2 - 1))) * R   # the first stage, then + 4r per step
        if any(trip[src[1]] is not LOW_TRIPLE and trip[src[0]] is LOW_TRIPLE for src in first_stage_sources(log_n)):
            with pytest.raises(Bound, match="borrows in limb 8"):
                model_ntt(loaded, log_n, omega=omega_inv, k_first=K2, scale=ninv, loaded=True)
    assert len(seen) == 16
