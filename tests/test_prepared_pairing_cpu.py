"""CPU build of the prepared G2 arguments and the shared-squaring Miller loop: vote_saver_protocol_amd/csrc/pairing.h prepare_g2 and
miller_multi compiled by g++ with the 32-bit-limb type the pairing kernels use (and the host's 64-bit-limb type).  The judge is the
existing miller_loop of the same header (tests/test_pairing_cpu.py checks that one against the oracle): miller_multi must give the
Fp12 product of the loops' values exactly, before any final exponentiation.  No GPU, no HIP, no oracle pairing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
from conftest import ROOT, g1_limbs, g2_limbs

SRC = os.path.join(ROOT, "tests", "cpu_build", "prepared_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libpreparedchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def pairs():
    """three random (P, Q)"""
    gen = o.splitmix64(68)
    return [(o.G1.mul(o.G1.gen, o.rand_fr(gen)), o.G2.mul(o.G2.gen, o.rand_fr(gen))) for _ in range(3)]


def multi_and_product(lib, pre, pairs, var=-1):
    g1 = np.concatenate([g1_limbs(p) if p is not None else np.zeros(12, np.uint64) for p, _ in pairs])
    g2 = np.concatenate([g2_limbs(q) if q is not None else np.zeros(24, np.uint64) for _, q in pairs])
    multi, prod = np.zeros(72, np.uint64), np.zeros(72, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    getattr(lib, pre + "multi_and_product")(p(g1), p(g2), C.c_size_t(len(pairs)), C.c_int(var), p(multi), p(prod))
    return multi, prod


@pytest.mark.parametrize("pre", TYPES)
def test_miller_multi_is_the_product_of_the_loops(pc, pre, pairs):
    multi, prod = multi_and_product(pc, pre, pairs)
    assert np.array_equal(multi, prod) and prod.any()
    single = [multi_and_product(pc, pre, [pr])[1] for pr in pairs]
    assert not any(np.array_equal(prod, s) for s in single)           # the product is of all three
    for var in range(3):                                              # one of the three left variable
        m, p = multi_and_product(pc, pre, pairs, var)
        assert np.array_equal(m, prod) and np.array_equal(p, prod), var


@pytest.mark.parametrize("pre", TYPES)
def test_one_prepared_pair_is_the_miller_loop_itself(pc, pre, pairs):
    for pr in pairs:
        multi, loop = multi_and_product(pc, pre, [pr])
        assert np.array_equal(multi, loop)
        multi, loop = multi_and_product(pc, pre, [pr], 0)
        assert np.array_equal(multi, loop)


@pytest.mark.parametrize("pre", TYPES)
def test_infinity_members_leave_the_product_of_the_others(pc, pre, pairs):
    (P0, Q0), (P1, Q1), (P2, Q2) = pairs
    others, _ = multi_and_product(pc, pre, [pairs[0], pairs[2]])
    one = np.zeros(72, np.uint64); one[0] = 1
    for middle in ((None, Q1), (P1, None), (None, None)):             # P = infinity; a prepared Q = infinity
        multi, prod = multi_and_product(pc, pre, [pairs[0], middle, pairs[2]])
        assert np.array_equal(multi, others) and np.array_equal(prod, others), middle
        multi, _ = multi_and_product(pc, pre, [pairs[0], middle, pairs[2]], 1)      # the same member as the variable pair
        assert np.array_equal(multi, others), middle
        multi, _ = multi_and_product(pc, pre, [middle])
        assert np.array_equal(multi, one)


@pytest.mark.parametrize("pre", TYPES)
def test_first_and_last_prepared_triples_are_the_unprepared_steps(pc, pre, pairs):
    """prepared[0] and prepared[67] against the doubling formulas written out in the test build on the T that the existing loop holds
    at its first and before its last step: an off-by-one in the line order moves either"""
    for _, Q in pairs:
        out = np.zeros(144, np.uint64)
        getattr(pc, pre + "line_ends")(g2_limbs(Q).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        first, last, want_first, want_last = out.reshape(4, 36)
        assert np.array_equal(first, want_first) and np.array_equal(last, want_last)
        assert not np.array_equal(first, last)
        # the first triple in big integers: T = (x, y, 1) gives E - B = 3 b' - y^2, 3 J = 3 x^2, H = 2 y, b' = 4 (1 + u)
        (x0, x1), (y0, y1) = Q
        p = o.P
        want = [(12 - (y0 * y0 - y1 * y1)) % p, (12 - 2 * y0 * y1) % p, 3 * (x0 * x0 - x1 * x1) % p, 6 * x0 * x1 % p, 2 * y0 % p, 2 * y1 % p]
        got = [sum(int(w) << (64 * i) for i, w in enumerate(first[6 * k:6 * k + 6])) for k in range(6)]
        assert got == want


def test_both_limb_types_agree(pc, pairs):
    a, _ = multi_and_product(pc, "chk_", pairs, 1)
    b, _ = multi_and_product(pc, "chk_h", pairs, 1)
    assert np.array_equal(a, b)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """prepared_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, no code loaded into python"""
    exe = str(tmp_path / "prepared_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPREPARED_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "prepared_check: ok" in p.stdout, p.stdout + p.stderr
