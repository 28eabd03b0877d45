"""Every kernel variant an option selects (include/vsp.h: "results never depend on" the options) on the inputs kernels go wrong on, against
the C oracle: identical affine limbs, identical infinity flag, no tolerance.

THE HARD SET, per (group, n), seeded.  Bases: uniform multiples of the generator; infinity at index 0, n // 2 and n - 1; the generator itself
at 1; one point P 200 times at [48, 248) and -P 200 times at [248, 448) (equal x in the accumulation: the k_accum_redo path, doublings and
cancellations); a second point Q at 64 scattered places.  Scalars: uniform, then one value on [448, 1948) (one crowded bucket per window),
90 % zeros and ones on the last 1500 (at n = 3000 and 2500 the two stretches overlap: 2 x 1500 + 448 > n; the tenth of the second stretch
that is not 0 / 1 keeps what lay there), and on top the edge values -- 0, 1, 2, r - 1, r - 2, (r -+ 1) / 2, 2^254 - 1, 2^254; around the
endomorphism split k = k1 + k2 lambda: lambda, lambda +- 1, r - lambda, r - lambda +- 1, 2^127 - 1, 2^127, 2^128, a value below 2^64 (k2 = 0);
the signed-digit carry chains 0x8000 / 0x7FFF / 0xFFFF in every 16-bit field and 0x1000 / 0x0FFF / 0x1FFF in every 13-bit field, reduced
mod r -- planted on ordinary bases [2, 27), on the P run [48, 73) and on the -P run [248, 273).  A second vector over the same bases sums to
infinity: one scalar on both runs, zero elsewhere.  Each vector runs over the whole range and over the unaligned sub-range [123, 123 + 0.8 n),
on plain bases, on the table of window multiples and (n >= 3000) on the 13-bit table with the endomorphism rows.

Sizes: the smallest that select each path -- G1 3000 (28-bit table, global counting sort, k_glv_split a kernel of its own), G1 33001 (ragged;
LDS counting sort, the split fused into the digit kernel by default), G2 2500 and G2 16500 (2 n >= 2^15: LDS sort under the split).
Inputs and the oracle's answers are computed once per (group, n) and shared by all variants; every variant runs on a context of its own."""
import numpy as np
import pytest

import bls12_381 as o
from conftest import L, fr_array, fr_ints_fast, g1_limbs, g2_limbs, rand_fr_array

import vote_saver_protocol_amd as v

gpu = pytest.mark.gpu                                   # (the oracle's own check below runs on the CPU: no module-wide mark)

LAMBDA = o.BLS_X ** 2 - 1                               # the eigenvalue of k_glv_split (msm_sort.hip): z^2 - 1
FIRST = 123
RUN_P, RUN_N, RUN_END, RUN_LEN = 48, 248, 448, 200
SIZES = ((1, 3000), (1, 33001), (2, 2500), (2, 16500))
_CASES = {}


def edge_scalars():
    r, lam = o.R, LAMBDA
    assert (lam * lam + lam + 1) % r == 0 and lam.bit_length() == 128

    def fields(width, value):                           # `value` in every width-bit field of a 256-bit word, reduced mod r
        x = 0
        for at in range(0, 256, width):
            x |= value << at
        return (x & ((1 << 256) - 1)) % r
    e = [0, 1, 2, r - 1, r - 2, (r - 1) // 2, (r + 1) // 2, (1 << 254) - 1, 1 << 254,
         lam, lam + 1, lam - 1, r - lam, r - lam + 1, r - lam - 1, (1 << 127) - 1, 1 << 127, 1 << 128, 0xDEADBEEFCAFEF00D,
         fields(16, 0x8000), fields(16, 0x7FFF), fields(16, 0xFFFF), fields(13, 0x1000), fields(13, 0x0FFF), fields(13, 0x1FFF)]
    assert all(0 <= x < r for x in e) and len(e) <= RUN_P - 2 - 4
    return fr_array(e)


def hard_set(cref, group, n):
    """-> bases [n, 12 | 24], the hard scalar vector, the cancelling one"""
    seed = 9000 + 10 * n + group
    ks = rand_fr_array(n, seed)
    ks[1] = L(1, 4)                                                          # the generator itself
    mul_gen = cref.g1_batch_mul_gen if group == 1 else cref.g2_batch_mul_gen
    bases = mul_gen(ks)
    if group == 1:
        neg = lambda row: g1_limbs(o.G1.neg(o.g1_from_limbs(row)))
    else:
        neg = lambda row: g2_limbs(o.G2.neg(o.g2_from_limbs(row)))
    P = bases[RUN_P].copy()
    bases[RUN_P:RUN_N] = P; bases[RUN_N:RUN_END] = neg(P)
    Q = mul_gen(rand_fr_array(1, seed + 1))[0]
    step = (n - RUN_END - 22) // 60
    q_at = [28, 29, 30, 31] + [RUN_END + 12 + j * step + (RUN_END + 12 + j * step == n // 2) for j in range(60)]
    assert len(set(q_at)) == 64 and max(q_at) < n - 1 and n // 2 not in q_at
    bases[q_at] = Q
    bases[0] = 0; bases[n // 2] = 0; bases[n - 1] = 0                        # infinity: first, middle, last
    rng = np.random.default_rng(seed + 2)
    ss = rand_fr_array(n, seed + 3)
    ss[RUN_END:RUN_END + 1500] = ss[RUN_END - 1]                             # one crowded bucket per window
    tail = np.arange(n - 1500, n)[rng.random(1500) < 0.9]
    ss[tail] = 0; ss[tail, 0] = rng.integers(0, 2, size=len(tail), dtype=np.uint64)
    e = edge_scalars()
    for at in (2, RUN_P, RUN_N):
        ss[at:at + len(e)] = e
    cancel = np.zeros((n, 4), np.uint64)
    cancel[RUN_P:RUN_END] = rand_fr_array(1, seed + 4)[0]
    return bases, ss, cancel


def hard_cases(cref, group, n):
    """bases and [(name, scalars, first, count, the oracle's point)], once per (group, n)"""
    if (group, n) not in _CASES:
        bases, ss, cancel = hard_set(cref, group, n)
        ref = cref.msm_g1 if group == 1 else cref.msm_g2
        m = int(0.8 * n)
        cases = []
        for name, vec in (("hard", ss), ("cancelling", cancel)):
            for first, cnt in ((0, n), (FIRST, m)):
                cases.append((name, vec, first, cnt, ref(bases[first:first + cnt], vec[first:first + cnt], mixed=True)))
        assert not cases[2][4].any() and cases[0][4].any() and cases[3][4].any()      # P - P over the whole runs; 125 P - 200 P over the sub-range
        for x in (bases, ss, cancel):
            x.setflags(write=False)
        _CASES[(group, n)] = (bases, cases)
    return _CASES[(group, n)]


def test_the_oracle_handles_the_hard_set(cref):
    """the reference first (CPU): the C oracle's multiexp_with_mixed_addition agrees with the plain double-and-add sums of
    oracle/bls12_381.py on the first 300 entries of the hard set -- the infinity, the generator, every edge value on ordinary bases and on
    the P run, 200 P and 52 -P -- and on 100 P + 100 -P under one scalar, where both must say infinity"""
    for group, n in ((1, 3000), (2, 2500)):
        bases, ss, cancel = hard_set(cref, group, n)
        ref, G, pt, limbs = (cref.msm_g1, o.G1, o.g1_from_limbs, g1_limbs) if group == 1 else (cref.msm_g2, o.G2, o.g2_from_limbs, g2_limbs)
        pts = [None if not row.any() else pt(row) for row in bases[:348]]
        assert pts[0] is None and pts[1] == G.gen and pts[RUN_P] == pts[RUN_N - 1] == G.neg(pts[RUN_N]) and pts[28] == pts[31]
        want = G.msm_naive(pts[:300], fr_ints_fast(ss[:300]))
        assert want is not None and np.array_equal(ref(bases[:300], ss[:300], mixed=True), limbs(want)), group
        assert G.msm_naive(pts[148:348], fr_ints_fast(cancel[148:348])) is None
        assert not ref(bases[148:348], cancel[148:348], mixed=True).any()
        assert not ref(bases, cancel, mixed=True).any()


def run_matrix(c, cref, group, n, after=None, forms=("plain", "table", "split table")):
    """every vector and range of the hard set over every form of the bases on context c: the oracle's point and flag; after(form, name,
    first, count) asserts what the variant must have run (the statistics are cleared before each multi-exponentiation)"""
    bases, cases = hard_cases(cref, group, n)
    vecs = {}
    try:
        for name, vec, _, _, _ in cases:
            if name not in vecs:
                vecs[name] = c.to_device(vec)
        for form in forms:
            if form == "split table" and n < 3000:
                continue
            B = c.upload_bases(bases, group)
            try:
                if form == "table":
                    B.precompute(0)
                elif form == "split table":
                    B.precompute(13, split=True)
                for name, vec, first, cnt, want in cases:
                    c.stats_reset()
                    got, inf = B.msm(vecs[name] + 32 * first, n=cnt, first=first)
                    assert np.array_equal(got, want), (group, n, form, name, first)
                    assert inf == (not want.any()), (group, n, form, name, first)
                    if after:
                        after(form, name, first, cnt)
            finally:
                B.free()
    finally:
        for d in vecs.values():
            c.dfree(d)


def variant_checks(c, variant, group, n):
    """what each variant must be seen to have run"""
    split_sizes = ((1, 33001), (2, 16500))

    def default(form, name, first, cnt):
        assert c.stat("msm_accum28_cxx_launches") == 0 and c.stat("msm_scan3_launches") == 0
        if (group, n) in split_sizes and form == "plain" and first == 0:     # the split runs inside the digit kernel
            assert c.stat("msm_endomorphism_split") == 1 and c.stat("msm_glv_split_launches") == 0

    def accum28_cxx(form, name, first, cnt):
        assert group == 1 and c.stat("msm_accum28_cxx_launches") > 0         # every G1 run here has a 28-bit table (n >= 1024)
        if variant == "accum28_cxx_glv0":
            assert c.stat("msm_endomorphism_split") == 0
        if variant == "accum28_cxx_split64":
            assert c.stat("msm_split") == 64

    def fused_split(form, name, first, cnt):
        split = c.stat("msm_endomorphism_split")
        if form in ("plain", "split table"):
            assert split == 1
        assert c.stat("msm_glv_split_launches") == split                     # k_glv_split as a kernel of its own wherever the scalars are split

    def fused_scans(form, name, first, cnt):
        assert c.stat("msm_scan3_launches") > 0

    def dimsum_maxw(form, name, first, cnt):
        assert c.stat("msm_dimsum_waves") <= int(variant.rsplit("_", 1)[1]) and c.stat("msm_calls") == 1

    def debug_counts(form, name, first, cnt):
        assert c.stat("msm_buckets") == c.stat("msm_bucket_sets") * 2 ** (c.stat("msm_window_bits") - 1) > 0
        assert 0 < c.stat("msm_parts")
        assert c.stat("msm_heavy_buckets") + c.stat("msm_medium_buckets") <= c.stat("msm_buckets")

    return {"default": default, "accum28_cxx": accum28_cxx, "accum28_cxx_glv0": accum28_cxx, "accum28_cxx_split64": accum28_cxx, "fused_split_0": fused_split,
            "fused_scans_0": fused_scans, "dimsum_maxw_256": dimsum_maxw, "dimsum_maxw_4096": dimsum_maxw, "debug_counts": debug_counts}[variant]


VARIANTS = {"default": {},
            "accum28_cxx": {"msm_accum28_asm": 0},
            "accum28_cxx_glv0": {"msm_accum28_asm": 0, "msm_glv": 0},
            "accum28_cxx_split64": {"msm_accum28_asm": 0, "msm_split": 64},
            "fused_split_0": {"msm_fused_split": 0},
            "fused_scans_0": {"msm_fused_scans": 0},
            "dimsum_maxw_256": {"msm_dimsum_maxw": 256},
            "dimsum_maxw_4096": {"msm_dimsum_maxw": 4096},
            "debug_counts": {"msm_debug_counts": 1}}
# (the C++ twin of the generated loop is G1 code: the G2 sizes run only for the options that reach G2 code)
MATRIX = [(name, group, n) for name in VARIANTS for group, n in SIZES if group == 1 or not name.startswith("accum28")]


@gpu
@pytest.mark.parametrize("variant,group,n", MATRIX, ids=["%s-g%d-%d" % m for m in MATRIX])
def test_variant_on_the_hard_set(cref, variant, group, n):
    c = v.Context(0)
    try:
        for option, value in VARIANTS[variant].items():
            c.set_option(option, value)
        run_matrix(c, cref, group, n, after=variant_checks(c, variant, group, n))
    finally:
        c.close()


@gpu
def test_dimsum_maxw_changes_the_lane_plan(cref):
    """"msm_dimsum_maxw" bounds the waves of the bucket reduction's per-digit lane plan: at G1 33001 on plain bases (the policy's window for
    these scalars, 12 bits: no width needs forcing) 256 and 4096 must give DIFFERENT plans -- else the two cases of the matrix ran one
    kernel configuration twice -- and both the oracle's point.  (dimsum_plan by hand at 11 bucket sets of 2048 buckets, digits of 6 and 5
    bits: 88 + 88 = 176 waves fit under 256, the next doubling would take 264; under 4096 both digits double once more, 352.)"""
    waves = {}
    for maxw in (256, 4096):
        c = v.Context(0)
        try:
            c.set_option("msm_dimsum_maxw", maxw)
            seen = []
            run_matrix(c, cref, 1, 33001, forms=("plain",), after=lambda form, name, first, cnt: seen.append((c.stat("msm_window_bits"), c.stat("msm_dimsum_waves"))))
            waves[maxw] = seen[0]
        finally:
            c.close()
    print("msm_dimsum_maxw 256 / 4096 at G1 33001: (window bits, waves) =", waves[256], waves[4096])
    assert waves[256][0] == waves[4096][0] and 0 < waves[256][1] <= 256 < waves[4096][1] <= 4096, waves


@gpu
def test_wide_windows_off_keeps_16_bit_windows_at_2p20(cref):
    """"msm_wide_windows" acts from 2^20 points without the endomorphism split: 17-bit windows by default, 16 with the option at 0, and the
    same point -- the discrete-log identity sum s_i (k_i G) = (sum k_i s_i) G of test_msm_full_size_2p20_discrete_log_identity"""
    n = 1 << 20
    ks = rand_fr_array(n, seed=1); ss = rand_fr_array(n, seed=2)
    e = sum(a * b for a, b in zip(fr_ints_fast(ks), fr_ints_fast(ss))) % o.R
    want = cref.g1_mul(g1_limbs(o.G1.gen), L(e, 4))
    c = v.Context(0)
    try:
        c.set_option("msm_glv", 0)
        d_k = c.to_device(ks); d_s = c.to_device(ss)
        d_b = v.fixed_base_mul(c, d_k, n, 1)
        B = c.bases_from_device(d_b, n, 1)
        try:
            for wide, bits in ((1, 17), (0, 16)):
                c.set_option("msm_wide_windows", wide)
                got, inf = B.msm(d_s)
                assert not inf and np.array_equal(got, want), wide
                assert c.stat("msm_window_bits") == bits and c.stat("msm_endomorphism_split") == 0
        finally:
            B.free(); c.dfree(d_b); c.dfree(d_k); c.dfree(d_s)
    finally:
        c.close()
