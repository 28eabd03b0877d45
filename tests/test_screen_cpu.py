"""CPU build of the screened ballot check's arithmetic: vote_saver_protocol_amd/csrc/screen.h compiled by g++ with the 32-bit-limb type
the kernels use and with the host's 64-bit-limb type.  screen_mul128 against the oracle's scalar multiplication at the edge
coefficients; the product tree, level by level as the host queues it, against one chain of products over the same values -- at the
sizes around one and two levels and with several ranges of which the last is shorter.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
from conftest import ROOT, I, L, g1_limbs

SRC = os.path.join(ROOT, "tests", "cpu_build", "screen_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs
SCALARS = [1, 2, 1 << 64, 1 << 127, (1 << 128) - 1, 0x0123456789abcdef_fedcba9876543210]


@pytest.fixture(scope="module")
def sc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libscreenchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    return C.CDLL(so)


def mul128(lib, pre, point, z):
    g1 = g1_limbs(point) if point is not None else np.zeros(12, np.uint64)
    out = np.zeros(12, np.uint64)
    getattr(lib, pre + "mul128")(g1.ctypes.data_as(C.c_void_p), C.c_uint64(z & (2**64 - 1)), C.c_uint64(z >> 64), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("pre", TYPES)
def test_mul128_is_the_oracles_multiple(sc, pre):
    P = o.G1.mul(o.G1.gen, o.rand_fr(o.splitmix64(128)))
    for z in SCALARS:
        assert np.array_equal(mul128(sc, pre, P, z), g1_limbs(o.G1.mul(P, z))), hex(z)


@pytest.mark.parametrize("pre", TYPES)
def test_mul128_of_infinity_and_by_the_group_order_edge(sc, pre):
    for z in SCALARS:
        assert not mul128(sc, pre, None, z).any()
    # z = 2^128 - 1 on P, plus P, is 2^64 (2^64 P): the top and the bottom bit of both words are read
    P = o.G1.mul(o.G1.gen, 7)
    twice = mul128(sc, pre, o.g1_from_limbs(mul128(sc, pre, P, 1 << 64)), 1 << 64)
    assert np.array_equal(twice, g1_limbs(o.G1.add(o.g1_from_limbs(mul128(sc, pre, P, (1 << 128) - 1)), P)))


def fp12_values(n, seed):
    gen = o.splitmix64(seed)
    vals = np.zeros((n, 72), np.uint64)
    for i in range(n):
        for k in range(12):
            vals[i, 6 * k:6 * k + 6] = L((o.rand_fr(gen) * o.rand_fr(gen)) % o.P, 6)
    return vals


def tree_and_serial(lib, pre, vals, length):
    n = vals.shape[0]
    ranges = (n + length - 1) // length
    t, s = np.zeros((ranges, 72), np.uint64), np.zeros((ranges, 72), np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    getattr(lib, pre + "tree_and_serial")(p(vals), C.c_size_t(n), C.c_size_t(length), p(t), p(s))
    return t, s


@pytest.fixture(scope="module")
def values():
    return fp12_values(300, 12)


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300])
def test_tree_product_is_the_serial_product(sc, pre, values, n):
    """one range: 16 and 256 are the sizes at which a level is added"""
    t, s = tree_and_serial(sc, pre, values[:n], n)
    assert np.array_equal(t, s) and s.any()
    if n == 1:
        assert np.array_equal(t[0], values[0])


@pytest.mark.parametrize("pre", TYPES)
@pytest.mark.parametrize("n,length", [(65, 17), (65, 16), (64, 16), (300, 75), (300, 19), (5, 1), (257, 256)])
def test_tree_product_of_several_ranges(sc, pre, values, n, length):
    """ranges back to back, the last one shorter (65 = 3 x 17 + 14; 257 = 256 + 1: a last range of one value beside one of two levels)"""
    t, s = tree_and_serial(sc, pre, values[:n], length)
    assert np.array_equal(t, s)
    whole, _ = tree_and_serial(sc, pre, values[:length], length)
    assert np.array_equal(t[0], whole[0])                            # range 0 does not depend on its neighbours


def test_both_limb_types_agree(sc, values):
    a, _ = tree_and_serial(sc, "chk_", values[:65], 65)
    b, _ = tree_and_serial(sc, "chk_h", values[:65], 65)
    assert np.array_equal(a, b)
    P = o.G1.mul(o.G1.gen, 11)
    assert np.array_equal(mul128(sc, "chk_", P, SCALARS[-1]), mul128(sc, "chk_h", P, SCALARS[-1]))


def test_stand_alone_program_under_sanitizers(tmp_path):
    """screen_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, no code loaded into python"""
    exe = str(tmp_path / "screen_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DSCREEN_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "screen_check: ok" in p.stdout, p.stdout + p.stderr
