"""GPU parity of the packed bucket-digit sums (k_dimsum_dense, option "msm_dimsum_dense", msm_impl.inc): the sums of the bucket reduction
folded in 256-thread blocks whose tree levels are renumbered onto the waves that have live additions.  Only WHICH thread performs WHICH
addition differs from k_dimsum_mixed, so every result must be the oracle's point and, bit for bit, the point of the same call with the
option off -- on forced window widths 8, 11, 12, 15, 16 (digit splits 4/3, 5/5, 6/5, 7/7, 8/7: 8 .. 256 buckets per sum, 8 .. 32 lanes per sum, 3 .. 5
tree levels; the endomorphism split forced so that 16-bit windows still fit the per-digit plan), n = 2^12 and 2^13, on inputs that put
doublings, cancellations and runs of infinity into the tree and leave ragged last blocks.  The stat "msm_dimsum_dense_launches" proves
which kernel ran."""
import numpy as np
import pytest

import bls12_381 as o
from conftest import g1_limbs, rand_fr_array

import vote_saver_protocol_amd as v

pytestmark = pytest.mark.gpu

N_MAX = 1 << 13
_CACHE = {}


@pytest.fixture(scope="module")
def contexts():
    on, off = v.Context(0), v.Context(0)
    for c, dense in ((on, 1), (off, 0)):                 # before the first upload: the context's self-check of the 28-bit path runs under the option too
        c.set_option("msm_dimsum_dense", dense); c.set_option("msm_glv", 2)
    yield on, off
    on.close(); off.close()


def _inputs(cref, kind, n):
    """(bases, scalars, the oracle's point), computed once per (kind, n)"""
    if (kind, n) in _CACHE:
        return _CACHE[(kind, n)]
    if "distinct" not in _CACHE:
        _CACHE["distinct"] = cref.g1_batch_mul_gen(rand_fr_array(N_MAX, seed=4101))
    distinct = _CACHE["distinct"]
    bases, ss = distinct[:n].copy(), rand_fr_array(n, seed=4200 + n)
    if kind == "all_equal":                              # every bucket sum a multiple of one point: doublings inside the tree
        bases = np.repeat(distinct[:1], n, axis=0)
    elif kind == "pairs":                                # P, -P with equal scalars in the first half: partial sums cancel to infinity
        for i in range(0, n // 2, 2):
            bases[i + 1] = g1_limbs(o.G1.neg(o.g1_from_limbs(bases[i])))
            ss[i + 1] = ss[i]
    elif kind == "one_bucket":                           # every scalar the same: one bucket per window, the other partial sums at infinity
        ss[:] = ss[0]
    elif kind == "bounded":                              # 64-bit scalars: the top windows are empty
        ss[:, 1:] = 0
    else:
        assert kind == "distinct"
    _CACHE[(kind, n)] = (bases, ss, cref.msm_g1(bases, ss, mixed=True))
    return _CACHE[(kind, n)]


def _msm(c, bases, ss):
    B = c.upload_bases(bases, 1); d_s = c.to_device(ss)
    try:
        before = c.stat("msm_dimsum_dense_launches")     # after the upload: the self-check of a context's first 28-bit table launches too
        got, _ = B.msm(d_s)
        return got, c.stat("msm_dimsum_dense_launches") - before, c.stat("msm_window_bits")
    finally:
        B.free(); c.dfree(d_s)


@pytest.mark.parametrize("kind", ["distinct", "all_equal", "pairs", "one_bucket", "bounded"])
@pytest.mark.parametrize("window_bits", [8, 11, 12, 15, 16])
def test_dense_bucket_digit_sums(contexts, cref, window_bits, kind):
    on, off = contexts
    try:
        for n in (1 << 12, 1 << 13):
            bases, ss, want = _inputs(cref, kind, n)
            on.set_option("msm_window_bits", window_bits); off.set_option("msm_window_bits", window_bits)
            got, launches, wb = _msm(on, bases, ss)
            assert wb == window_bits and launches > 0, (n, wb, launches)          # the packed kernel ran
            ref, launches_off, wb_off = _msm(off, bases, ss)
            assert wb_off == window_bits and launches_off == 0, (n, wb_off, launches_off)
            assert np.array_equal(got, want), (kind, n, window_bits)
            assert np.array_equal(got, ref), (kind, n, window_bits)
    finally:
        on.set_option("msm_window_bits", 0); off.set_option("msm_window_bits", 0)
