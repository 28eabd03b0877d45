"""CPU build of the batch ciphertext's arithmetic: vote_saver_protocol_amd/csrc/saver_ct.h compiled by g++ with the 32-bit-limb type the
kernel uses and with the host's 64-bit-limb type.  One ballot goes through the kernel's own column descriptions, lane shares and fold order
(a host emulation of every lane group, tests/cpu_build/saver_ct_check.cpp) and must be oracle/saver.py encrypt_ct and r_enc P2, limb for
limb: at msg_size 1 and 3, with the edge scalars for r_enc and for the messages, and over the crafted key in which a lane's mixed
addition meets equal operands, a fold's addition opposite ones, and every sum is infinity.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
import saver as sv
from conftest import ROOT, L, g1_limbs

SRC = os.path.join(ROOT, "tests", "cpu_build", "saver_ct_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs
EDGES = [0, 1, 15, 16, 1 << 252, o.R - 1]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libsaverctchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    l = C.CDLL(so)
    l.chk_key.restype = l.chk_hkey.restype = C.c_void_p
    return l


def election_key(n, seed, crafted=False):
    """oracle/saver.py key over random points; crafted: delta_s_g1[0] = G_1 and delta_sum_s_g1 = t_g1[0] (curve points, so a key loads)"""
    gen = o.splitmix64(seed)
    pt = lambda: o.G1.mul(o.G1.gen, o.rand_fr(gen))
    gabc = [pt() for _ in range(n + 1)]
    pk, _, _ = sv.keygen(n, pt(), pt(), gabc, [o.rand_fr(gen) for _ in range(3 * n + 2)])
    if crafted:
        pk["delta_s_g1"][0] = gabc[1]
        pk["delta_sum_s_g1"] = pk["t_g1"][0]
    return pk, gabc


def bases_of(pk, gabc):
    """the 3 n + 3 fixed points in the order of saver_ct.h"""
    pts = [pk["delta_g1"]] + pk["delta_s_g1"] + [pk["delta_sum_s_g1"], pk["gamma_inverse_sum_s_g1"]] + gabc[1:] + pk["t_g1"]
    return np.concatenate([g1_limbs(p) for p in pts])


class Emulated:
    def __init__(self, lib, pre, pk, gabc):
        self.lib, self.pre, self.pk, self.gabc, self.n = lib, pre, pk, gabc, len(gabc) - 1
        self.bases = bases_of(pk, gabc)
        self.h = C.c_void_p(getattr(lib, pre + "key")(C.c_size_t(self.n), self.bases.ctypes.data_as(C.c_void_p)))

    def free(self):
        getattr(self.lib, self.pre + "key_free")(self.h)

    def columns(self, msg, r_enc):
        scal = np.concatenate([L(r_enc, 4)] + [L(m, 4) for m in msg])
        out = np.zeros((self.n + 3, 12), np.uint64)
        getattr(self.lib, self.pre + "ballot")(self.h, scal.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    def check(self, msg, r_enc):
        want = sv.encrypt_ct(self.pk, self.gabc, msg, r_enc) + [o.G1.mul(self.pk["gamma_inverse_sum_s_g1"], r_enc)]
        got = self.columns(msg, r_enc)
        assert np.array_equal(got, np.stack([g1_limbs(p) for p in want])), (self.pre, msg, r_enc)
        return want


def test_digits_and_the_plan_of_the_real_ballot(lib):
    k = L(0xfedcba9876543210 | (0xa << 252), 4)
    assert [lib.chk_digit(k.ctypes.data_as(C.c_void_p), w) for w in range(16)] == list(range(16))
    assert lib.chk_digit(k.ctypes.data_as(C.c_void_p), 63) == 0xa and lib.chk_digit(k.ctypes.data_as(C.c_void_p), 16) == 0
    longest, span = C.c_uint(0), C.c_uint(0)
    for n, chain, lanes in ((1, 12, 64), (3, 13, 128), (25, 32, 512), (64, 71, 1152)):
        # groups inside one wave, no overlap, whole waves; the longest chain: c_i's 8 + 4, psi's 8 + 5 with 32 lanes, then psi's (n + 1) + 6 with 64
        assert lib.chk_plan_shape(C.c_size_t(n), C.byref(longest), C.byref(span)) == 0, n
        assert (longest.value, span.value) == (chain, lanes), n


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("n", [1, 3])
def test_emulated_lane_groups_give_the_oracles_ciphertext(lib, pre, n):
    pk, gabc = election_key(n, 70 + n)
    gen = o.splitmix64(7 * n)
    scalars = EDGES + [o.rand_fr(gen) for _ in range(2)]
    key = Emulated(lib, pre, pk, gabc)
    try:
        for j, r_enc in enumerate(scalars):                           # every scalar as r_enc, and as a message block in every position
            key.check([scalars[(j + 1 + i) % len(scalars)] for i in range(n)], r_enc)
        key.check([1] + [0] * (n - 1), o.rand_fr(gen))                # a one-hot ballot
    finally:
        key.free()


@pytest.mark.parametrize("pre", TYPES)
def test_crafted_key_doubles_cancels_and_gives_infinity(lib, pre):
    """X_1 = G_1 and X_4 = Y_1: with m_1 = r_enc of one digit a lane adds a table entry to itself (c_1 = 2 r G_1); with m_1 = R - r_enc the
    last addition of c_1's fold has opposite operands (c_1 = infinity: all-zero limbs); r_enc = 0 with m = 0 sums nothing at all"""
    pk, gabc = election_key(3, 91, crafted=True)
    key = Emulated(lib, pre, pk, gabc)
    gen = o.splitmix64(92)
    try:
        for r_enc in (1, 15, 16, 1 << 252, o.rand_fr(gen)):
            ct = key.check([r_enc, 5, 0], r_enc)
            assert ct[1] == o.G1.mul(gabc[1], 2 * r_enc % o.R)
            ct = key.check([o.R - r_enc, 5, 0], r_enc)
            assert ct[1] is None and not key.columns([o.R - r_enc, 5, 0], r_enc)[1].any()
        assert not key.columns([0, 0, 0], 0).any()
        key.check([0, 0, 0], 0)
    finally:
        key.free()


def test_both_limb_types_agree(lib):
    pk, gabc = election_key(3, 73)
    a, b = Emulated(lib, "chk_", pk, gabc), Emulated(lib, "chk_h", pk, gabc)
    try:
        assert np.array_equal(a.columns([3, o.R - 1, 1 << 200], 12345), b.columns([3, o.R - 1, 1 << 200], 12345))
    finally:
        a.free(); b.free()


def test_stand_alone_program_under_sanitizers(tmp_path):
    """saver_ct_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, a base at infinity, no code loaded into python"""
    exe = str(tmp_path / "saver_ct_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSAVER_CT_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "saver_ct_check: ok" in p.stdout, p.stdout + p.stderr
