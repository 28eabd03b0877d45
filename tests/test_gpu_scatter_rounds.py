"""GPU parity of the rounds of k_scatter_lds (msm_sort.hip; option "msm_scatter_rounds"; block mapping: csrc/lds_sort_map.h).

The scatter kernel of the LDS counting sort walks its chunk once per bucket range and places, in round r, exactly the entries whose bucket
lies in range r.  Counts, offsets and the entries of every bucket are those of a single pass, so the affine result of every case must be,
bit for bit, the result of the same call with "msm_scatter_rounds" = 1 and the oracle's point -- for 2, 4, 8 and 32 forced rounds and for
the automatic choice.  2^15 points is the smallest size at which the LDS counting sort takes over.  The stat "msm_scatter_rounds" proves
that the kernel ran, and in how many rounds.

Cases: split G1 (8 windows of 16 bits); scalars that are mostly 1 and 0 (one bucket holds half a window: the lanes that share the
leader's bucket; zero digits); digits on the first and last bucket of each of four ranges, with the digit's sign bit and the half's sign
byte set; unsplit scalars (16 windows: two per label); a batch (W = K Wk); 13-bit windows (10 windows: a grid with idle blocks); bases
with precomputed window multiples (the shared-set mode); 17-bit windows through the two-pass sort (the low-bits byte travels with its
entry); G2."""
import numpy as np
import pytest

import bls12_381 as o
from conftest import fr_array, rand_fr_array

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

N = 1 << 15
ROUNDS = [2, 4, 8, 32, 0]                                   # forced rounds, then the automatic choice
LAMBDA = 0xac45a4010001a40200000000ffffffff                  # the endomorphism's eigenvalue (msm_sort.hip, glv_split_scalar)
DEFAULTS = dict(msm_glv=1, msm_window_bits=0, msm_sort=0, msm_scatter_rounds=0)


@pytest.fixture(scope="module")
def box():
    c = v.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def points(box):
    """{group: (device pointer, host copy)} of N multiples of the generator, made once on the GPU"""
    d_k = box.to_device(rand_fr_array(N, seed=7301))
    out = {}
    for group, words in ((1, 12), (2, 24)):
        d_b = v.fixed_base_mul(box, d_k, N, group)
        host = np.zeros((N, words), np.uint64)
        box.d2h(host, d_b)
        out[group] = (d_b, host)
    box.dfree(d_k)
    yield out
    for d_b, _ in out.values():
        box.dfree(d_b)


def _check(c, cref, points, scalars, *, group=1, glv=2, window_bits=16, sort=0, precompute=False, windows=None):
    """scalars [K, N, 4] (K > 1: the batch entry point).  Every number of rounds gives the single pass's points, which are the oracle's."""
    d_b, host_b = points[group]
    scalars = np.ascontiguousarray(scalars, np.uint64).reshape(-1, N, 4)
    K = scalars.shape[0]
    ref_msm = cref.msm_g1 if group == 1 else cref.msm_g2
    want = np.stack([ref_msm(host_b, s) for s in scalars])
    d_s = c.to_device(scalars)
    B = None
    try:
        c.set_option("msm_glv", glv); c.set_option("msm_window_bits", window_bits); c.set_option("msm_sort", sort)      # (the split is laid out at upload)
        B = c.bases_from_device(d_b, N, group)
        if precompute:
            B.precompute(window_bits)
        got = {}
        for r in [1] + ROUNDS:
            c.set_option("msm_scatter_rounds", r)
            c.stats_reset()
            got[r] = B.msm_batch(d_s, K)[0] if K > 1 else B.msm(d_s)[0].reshape(1, -1)
            ran = int(c.stat("msm_scatter_rounds"))
            assert ran == r if r else ran in (1, 2, 4, 8, 16, 32), (r, ran)      # k_scatter_lds was launched, with this many rounds
            assert int(c.stat("msm_window_bits")) == window_bits
            if windows is not None:
                assert int(c.stat("msm_windows")) == windows, c.stat("msm_windows")
        assert np.array_equal(got[1], want)
        for r in ROUNDS:
            assert np.array_equal(got[r], got[1]), r
            assert np.array_equal(got[r], want), r
    finally:
        if B is not None:
            B.free()
        c.dfree(d_s)
        for k, val in DEFAULTS.items():
            c.set_option(k, val)


def test_split_g1_uniform(box, cref, points):
    _check(box, cref, points, rand_fr_array(N, seed=7302), windows=8)


def test_boolean_heavy_scalars(box, cref, points):
    """half the scalars 1 (one bucket of window 0 takes half of its entries), a quarter 0 (no digit at all), the rest uniform"""
    ss = rand_fr_array(N, seed=7303)
    kind = np.random.default_rng(7304).integers(0, 4, size=N)
    ss[kind < 2] = 0
    ss[kind < 2, 0] = 1
    ss[kind == 2] = 0
    _check(box, cref, points, ss, windows=8)


# ---- digits on the range boundaries ------------------------------------------------------------
C16, B16 = 16, 1 << 15
# bucket index |d| - 1 in four ranges of B / 4: 1 and B/4 are the first and last bucket of range 0, B/4 + 1 and B/2 of range 1,
# B/2 + 1 and 3B/4 of range 2, 3B/4 + 1 and B of range 3
MAGS = [1, B16 // 4, B16 // 4 + 1, B16 // 2, B16 // 2 + 1, 3 * B16 // 4, 3 * B16 // 4 + 1, B16]
DIGITS = MAGS + [-m for m in MAGS if m != B16]              # (a negative digit has magnitude below B: 2^c - B recodes as +B)


def _half(j, top):
    """a half scalar whose signed 16-bit digits are DIGITS[(j + w) % len] in windows 0 .. 6 and `top` > 0 in window 7"""
    return sum(DIGITS[(j + w) % len(DIGITS)] << (C16 * w) for w in range(7)) + (top << (C16 * 7))


def _split(k):
    """glv_split_scalar: k = k1 + k2 lambda with k2 = round(k / lambda), moved back by lambda^2 + lambda + 1 = 0 where k2 reaches 2^127"""
    k2 = (2 * k + LAMBDA) // (2 * LAMBDA)
    k1 = k - k2 * LAMBDA
    if k2 >= 1 << 127:
        k1, k2 = k1 - 1, k2 - LAMBDA - 1
    return k1, k2


def _signed_digits(m):
    """the recoding of k_glv_digits: digit w of the magnitude m, in (-B, B]"""
    out, carry = [], 0
    for w in range(8):
        raw = ((m >> (C16 * w)) & 0xFFFF) + carry
        carry = 1 if raw > B16 else 0
        out.append(raw - (1 << C16) if carry else raw)
    assert carry == 0
    return out


def _boundary_scalars():
    """k = k1 + k2 lambda over halves built digit by digit.  k2 in [2^112, 2^127) and |k1| < lambda / 2, so the library's split returns
    exactly these halves: k1 of both signs (the sign byte), k2 positive.  The top window of a half has no negative digit and no carry
    out; a top digit of B needs a negative window 6 (the half stays below 2^127), and a k1 keeps its top digit at B/2 + 1 at most."""
    n_d = len(DIGITS)
    k2s = []
    for j in range(n_d):
        top = MAGS[j % len(MAGS)]
        if top == B16 and DIGITS[(j + 6) % n_d] > 0:
            top = 3 * B16 // 4 + 1
        k2s.append(_half(j, top))
    k1s = [s * _half(j, MAGS[j % 5]) for j in range(n_d) for s in (1, -1)]
    assert all(0 < k2 < 1 << 127 for k2 in k2s) and all(2 * abs(k1) < LAMBDA for k1 in k1s)
    return [k1s[i % len(k1s)] + k2s[(i // len(k1s)) % len(k2s)] * LAMBDA for i in range(N)]


def test_digits_on_the_range_boundaries(box, cref, points):
    ks = _boundary_scalars()
    # the construction holds what it says: per window, which (magnitude, digit sign bit, half's sign byte) occur
    seen = [set() for _ in range(8)]
    for k in set(ks):
        assert 0 < k < o.R
        for half in _split(k):
            for w, d in enumerate(_signed_digits(abs(half))):
                seen[w].add((abs(d), d < 0, half < 0))
    for w in range(7):
        for m in MAGS:
            signs = {(neg, flip) for mag, neg, flip in seen[w] if mag == m}
            assert {n ^ f for n, f in signs} == {False, True}, (w, m)          # both signs of the sorted entry
            assert m == B16 or {n for n, _ in signs} == {False, True}, (w, m)  # and the digit's own sign bit beside the bucket index
    top = {(mag, neg ^ flip) for mag, neg, flip in seen[7]}
    assert {m for m, _ in top} >= set(MAGS)
    assert all((m, True) in top and (m, False) in top for m in MAGS[:5])        # (no negative half reaches a top digit above lambda / 2^113)
    _check(box, cref, points, fr_array(ks), windows=8)


def test_unsplit_scalars(box, cref, points):
    _check(box, cref, points, rand_fr_array(N, seed=7305), glv=0, windows=16)


def test_a_batch_of_two_vectors(box, cref, points):
    _check(box, cref, points, np.stack([rand_fr_array(N, seed=7306), rand_fr_array(N, seed=7307)]), windows=16)


def test_ten_windows_leave_blocks_idle(box, cref, points):
    """13-bit windows of split scalars: W = 10 is no multiple of 8, the grid is rounded up and some blocks own nothing"""
    _check(box, cref, points, rand_fr_array(N, seed=7308), window_bits=13, windows=10)


def test_shared_bucket_set(box, cref, points):
    """precomputed window multiples: the 16 windows write ONE set of buckets"""
    _check(box, cref, points, rand_fr_array(N, seed=7309), glv=0, precompute=True, windows=16)


def test_wide_windows_carry_their_low_bits(box, cref, points):
    _check(box, cref, points, rand_fr_array(N, seed=7310), window_bits=17, sort=1)


def test_g2(box, cref, points):
    _check(box, cref, points, rand_fr_array(N, seed=7311), group=2)
