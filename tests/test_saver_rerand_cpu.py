"""CPU build of the batch rerandomization's shared rules: vote_saver_protocol_amd/csrc/saver_rerand.h compiled by g++ with the 32-bit-limb
types the kernels use and with the host's 64-bit-limb types (tests/cpu_build/saver_rerand_check.cpp).  One ballot goes through
saver_rerand_plan's columns -- every lane's share, the fold, the given point added by lane 0, one host lane per lane of a group -- and
must be the C oracle's saver_rerandomize ciphertext and the fixed part of its C', limb for limb: at msg_size 1, 3 and 25, with the edge
scalars for r', and where the given point equals the table's sum, is its opposite, or is infinity.  The G2 column gives z2 delta_g2, and
the scalar records with their one shared inversion are checked against big integers.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import ROOT, I, L, fr_array, g1_limbs, g2_limbs
from test_saver_ct_cpu import election_key

SRC = os.path.join(ROOT, "tests", "cpu_build", "saver_rerand_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs
EDGES = [0, 1, 15, 16, 1 << 252, o.R - 1]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libsaverrerandchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    l = C.CDLL(so)
    l.chk_key.restype = l.chk_hkey.restype = C.c_void_p
    return l


def bases_of(pk):
    """X_0 .. X_{n+1} | P2 in the order of the columns"""
    return [pk["delta_g1"]] + pk["delta_s_g1"] + [pk["delta_sum_s_g1"], pk["gamma_inverse_sum_s_g1"]]


class Emulated:
    def __init__(self, lib, pre, pk):
        self.lib, self.pre, self.pk, self.n = lib, pre, pk, len(pk["delta_s_g1"])
        self.X = bases_of(pk)
        self.bases = np.concatenate([g1_limbs(p) for p in self.X])
        self.pk_w = np.array(sv.pk_to_words(pk), np.uint64)
        self.h = C.c_void_p(getattr(lib, pre + "key")(C.c_size_t(self.n), _p(self.bases)))

    def free(self):
        getattr(self.lib, self.pre + "key_free")(self.h)

    def columns(self, rnd3, ct, Cc):
        """ct [n + 2, 12], Cc [12] -> the n + 3 columns"""
        rnd = fr_array(rnd3).reshape(12)
        given = np.ascontiguousarray(np.concatenate([ct.reshape(-1), Cc]))
        out = np.zeros((self.n + 3, 12), np.uint64)
        getattr(self.lib, self.pre + "ballot")(self.h, _p(rnd), _p(given), _p(out))
        return out

    def check(self, cref, delta_g2, rnd3, ct, A, B, Cc):
        """the columns against cref.saver_rerandomize: the ciphertext, and C' once (z1 z2) A is added to the last column"""
        got = self.columns(rnd3, ct, Cc)
        ct2, _, _, C2 = cref.saver_rerandomize(self.n, self.pk_w, delta_g2, fr_array(rnd3).reshape(12), ct, A, B, Cc)
        assert np.array_equal(got[:self.n + 2], ct2), (self.pre, rnd3)
        assert np.array_equal(got[self.n + 2], cref.g1_add(Cc, cref.g1_mul(g1_limbs(self.X[self.n + 2]), L(rnd3[0], 4)))), (self.pre, rnd3)
        assert np.array_equal(cref.g1_add(got[self.n + 2], cref.g1_mul(A, L(rnd3[1] * rnd3[2] % o.R, 4))), C2), (self.pre, rnd3)
        return got


def test_the_plan_of_the_columns(lib):
    longest, span = C.c_uint(0), C.c_uint(0)
    for n in (1, 3, 25, 64):
        # n + 3 columns of one pair under r', column c over base c from given point c, 8 lanes each; with spans end to end no group
        # straddles a wave; the longest chain is 8 terms + 3 levels + the given point
        assert lib.chk_plan_shape(C.c_size_t(n), C.byref(longest), C.byref(span)) == 0, n
        assert (longest.value, span.value) == (12, 8 * (n + 3)), n


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("n", [1, 3, 25])
def test_emulated_columns_give_the_oracles_rerandomized_ciphertext(lib, cref, pre, n):
    pk, _ = election_key(n, 170 + n)
    gen = o.splitmix64(11 * n)
    key = Emulated(lib, pre, pk)
    delta_g2 = cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0]
    scalars = EDGES + [o.rand_fr(gen) for _ in range(2)]
    try:
        for j, rp in enumerate(scalars if n < 25 else scalars[-3:]):
            pts = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(n + 4)]))
            B = cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0]
            z1 = (1, o.R - 1, o.rand_fr(gen))[j % 3]
            key.check(cref, delta_g2, (rp, z1, scalars[(j + 3) % len(scalars)]), np.ascontiguousarray(pts[:n + 2]), pts[n + 2], B, pts[n + 3])
    finally:
        key.free()


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("n", [1, 3, 25])
def test_given_point_equal_opposite_and_infinite(lib, cref, pre, n):
    """ct_0 = r' X_0: lane 0's addition doubles.  ct_1 = -r' X_1: it gives infinity, all-zero limbs.  ct_{n+1} at infinity: the table's
    sum alone.  C = -r' P2: the fixed part of C' is infinity.  r' = 0 leaves every given point as it is.  A key with X_1 at infinity
    leaves ct_1 alone"""
    pk, _ = election_key(n, 190 + n)
    gen = o.splitmix64(13 * n)
    key = Emulated(lib, pre, pk)
    delta_g2 = cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0]
    A, B = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0], cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0]
    try:
        for rp in (1, 15, 1 << 252, o.rand_fr(gen)):
            ct = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(n + 2)]))
            ct[0] = g1_limbs(o.G1.mul(key.X[0], rp))
            ct[1] = g1_limbs(o.G1.neg(o.G1.mul(key.X[1], rp)))
            ct[n + 1] = 0
            Cc = g1_limbs(o.G1.neg(o.G1.mul(key.X[n + 2], rp)))
            got = key.check(cref, delta_g2, (rp, o.rand_fr(gen), o.rand_fr(gen)), ct, A, B, Cc)
            assert np.array_equal(got[0], g1_limbs(o.G1.mul(key.X[0], 2 * rp % o.R)))
            assert not got[1].any() and not got[n + 2].any()
            assert np.array_equal(got[n + 1], g1_limbs(o.G1.mul(key.X[n + 1], rp)))
        ct = cref.g1_batch_mul_gen(fr_array([o.rand_fr(gen) for _ in range(n + 2)]))
        got = key.check(cref, delta_g2, (0, 1, 0), ct, A, B, A)
        assert np.array_equal(got[:n + 2], ct) and np.array_equal(got[n + 2], A)
    finally:
        key.free()
    pk["delta_s_g1"][0] = None
    flagged = Emulated(lib, pre, pk)
    try:
        got = flagged.check(cref, delta_g2, (o.rand_fr(gen), 1, 1), ct, A, B, A)
        assert np.array_equal(got[1], ct[1]) and not np.array_equal(got[0], ct[0])
    finally:
        flagged.free()


@pytest.mark.parametrize("pre", TYPES)
def test_the_g2_column_is_z2_delta(lib, cref, pre):
    gen = o.splitmix64(77)
    delta_g2 = cref.g2_batch_mul_gen(fr_array([o.rand_fr(gen)]))[0]
    out = np.zeros(24, np.uint64)
    for z2 in EDGES + [o.rand_fr(gen)]:
        getattr(lib, pre + "delta")(_p(delta_g2), _p(fr_array([5, 1, z2]).reshape(12)), _p(out))
        assert np.array_equal(out, cref.g2_mul(delta_g2, L(z2, 4))), (pre, z2)
    assert np.array_equal(out, g2_limbs(o.G2.mul(o.g2_from_limbs(delta_g2), z2)))
    getattr(lib, pre + "delta")(_p(np.zeros(24, np.uint64)), _p(fr_array([5, 1, 9]).reshape(12)), _p(out))      # delta_g2 at infinity: flagged
    assert not out.any()


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("count", [1, 2, 9])
def test_scalar_records_share_one_inversion(lib, pre, count):
    """r' | z1 | z1 z2 | 1 / z1 | z2 against big integers; z1 = 1 and R - 1 among the members, z2 = 0 too"""
    gen = o.splitmix64(300 + count)
    z1s = ([1, o.R - 1, 2] + [o.rand_fr(gen) for _ in range(count)])[:count]
    z2s = ([0, o.R - 1, 1] + [o.rand_fr(gen) for _ in range(count)])[:count]
    rps = [o.rand_fr(gen) for _ in range(count)]
    rnd = fr_array([x for t in zip(rps, z1s, z2s) for x in t]).reshape(-1)
    rec = np.zeros((count, 5, 4), np.uint64)
    getattr(lib, pre + "scalars")(_p(rnd), C.c_size_t(count), _p(rec))
    for k in range(count):
        assert [I(x) for x in rec[k]] == [rps[k], z1s[k], z1s[k] * z2s[k] % o.R, pow(z1s[k], -1, o.R), z2s[k]], (pre, k)


def test_both_limb_types_agree(lib, cref):
    pk, _ = election_key(3, 173)
    a, b = Emulated(lib, "chk_", pk), Emulated(lib, "chk_h", pk)
    pts = cref.g1_batch_mul_gen(fr_array([3, 5, 7, 11, 13, 17]))
    try:
        rnd3 = (o.R - 2, 12345, 1 << 200)
        assert np.array_equal(a.columns(rnd3, np.ascontiguousarray(pts[:5]), pts[5]), b.columns(rnd3, np.ascontiguousarray(pts[:5]), pts[5]))
    finally:
        a.free(); b.free()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """saver_rerand_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, a base at infinity, no code loaded into python"""
    exe = str(tmp_path / "saver_rerand_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSAVER_RERAND_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "saver_rerand_check: ok" in p.stdout, p.stdout + p.stderr
