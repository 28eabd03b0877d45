"""CPU build of the GT discrete-logarithm search: vote_saver_protocol_amd/csrc/gt_dlog.h compiled by g++ with the 32-bit-limb type the
decryption kernels use (and the host's 64-bit-limb type).  The base is one GT element of the oracle, the judge for powers is the
oracle's f12_pow.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
import pairing as pg
import wire
from conftest import L, ROOT

SRC = os.path.join(ROOT, "tests", "cpu_build", "dlog_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs
NONE = (1 << 64) - 1


@pytest.fixture(scope="module")
def dc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libdlogchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    lib = C.CDLL(so)
    for pre in TYPES:
        getattr(lib, pre + "find").restype = C.c_uint64
        getattr(lib, pre + "fingerprint").restype = C.c_uint64
    lib.chk_giant_steps.restype = C.c_uint64
    lib.chk_launch_lanes.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def base():
    """the oracle's e(G1, G2): the one slow oracle pairing of this file"""
    return pg.final_exp(pg.miller_loop(o.G2.gen, o.G1.gen))


@pytest.fixture(scope="module")
def powers(base):
    """base^m for m = 0 .. 203 by the oracle's f12_pow"""
    return [pg.f12_pow(base, m) for m in range(204)]


def words(poly):
    return np.frombuffer(wire.gt_to_tower_le(poly), dtype=np.uint64).copy()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


class Table:
    def __init__(self, lib, pre, base, b, fp_bits):
        self.lib, self.pre, self.b, self.fp_bits = lib, pre, b, fp_bits
        self.base = words(base)
        self.keys, self.js = np.zeros(1 << b, np.uint64), np.zeros(1 << b, np.uint32)
        getattr(lib, pre + "table")(p(self.base), C.c_uint(b), C.c_uint(fp_bits), p(self.keys), p(self.js))

    def find(self, value, max_value):
        v = words(value)
        return getattr(self.lib, self.pre + "find")(p(v), p(self.base), C.c_uint(self.b), C.c_uint(self.fp_bits), C.c_uint64(max_value), p(self.keys), p(self.js))


@pytest.mark.parametrize("pre", TYPES)
def test_every_m_up_to_the_bound_is_found_and_the_overshoot_is_cut(dc, pre, base, powers):
    """B = 8, max_value = 100: 13 giant steps reach 0 .. 103; 101, 102 and 103 are not results"""
    t = Table(dc, pre, base, 3, 64)
    assert sorted(t.js.tolist()) == list(range(8)) and (np.diff(t.keys.astype(object)) >= 0).all()
    assert dc.chk_giant_steps(C.c_uint64(100), C.c_uint(3)) == 13
    assert [t.find(powers[m], 100) for m in range(101)] == list(range(101))
    assert [t.find(powers[m], 100) for m in (101, 102, 103)] == [NONE] * 3
    assert [t.find(powers[m], 103) for m in (101, 102, 103)] == [101, 102, 103]     # the same table reaches them under a wider bound


@pytest.mark.parametrize("pre", TYPES)
def test_a_four_bit_fingerprint_still_finds_every_m_exactly(dc, pre, base, powers):
    """16 fingerprints for 8 entries and 26 giant steps: equal keys abound, in the table and between the walk and the table"""
    t = Table(dc, pre, base, 3, 4)
    assert int(t.keys.max()) < 16
    assert [t.find(powers[m], 200) for m in range(201)] == list(range(201))
    assert [t.find(powers[m], 200) for m in (201, 202, 203)] == [NONE] * 3
    t1 = Table(dc, pre, base, 3, 1)                                  # two fingerprints: at least four entries share one
    assert [t1.find(powers[m], 50) for m in range(0, 51, 7)] == list(range(0, 51, 7))


@pytest.mark.parametrize("pre", TYPES)
def test_the_giant_stride_inverts_the_power(dc, pre, base):
    for b in (1, 3, 8):
        out = np.zeros(72, np.uint64)
        getattr(dc, pre + "stride_times_power")(p(words(base)), C.c_uint(b), p(out))
        assert np.array_equal(out, words(pg.ONE)), b


@pytest.mark.parametrize("pre", TYPES)
def test_powers_by_full_width_exponents_are_the_oracles(dc, pre, base):
    gen = o.splitmix64(77)
    for e in (0, 1, 2, 101, (1 << 64) - 1, 1 << 64, o.R - 1, o.R, o.rand_fr(gen)):
        out = np.zeros(72, np.uint64)
        getattr(dc, pre + "power")(p(words(base)), p(L(e, 4)), p(out))
        assert np.array_equal(out, words(pg.f12_pow(base, e))), e
    assert np.array_equal(words(pg.f12_pow(base, o.R)), words(pg.ONE))


@pytest.mark.parametrize("pre", TYPES)
def test_a_value_that_is_no_small_power_is_not_found(dc, pre, base):
    """GT has prime order, so every value is some power of base: what must not be found is a value whose logarithm is outside the
    range.  A power of another pairing value, e(3 G1, 5 G2)^7 = base^105, is found under a bound of 105 and not under 100; e(G1, k G2)
    for a random k is not found at all"""
    other = pg.final_exp(pg.miller_loop(o.G2.mul(o.G2.gen, 5), o.G1.mul(o.G1.gen, 3)))
    t = Table(dc, pre, base, 3, 64)
    v = pg.f12_pow(other, 7)
    assert t.find(v, 100) == NONE and t.find(v, 105) == 105
    k = o.rand_fr(o.splitmix64(5))
    far = pg.f12_pow(base, k)                                        # = e(G1, k G2): a GT element whose logarithm is far outside the range
    assert t.find(far, 100) == NONE and t.find(far, 4000) == NONE
    t4 = Table(dc, pre, base, 3, 4)
    assert t4.find(far, 200) == NONE and t4.find(pg.f12_mul(far, far), 200) == NONE
    assert t4.find(pg.ZERO, 200) == NONE                             # not a group element at all


def test_both_limb_types_build_the_same_table(dc, base):
    a, b = Table(dc, "chk_", base, 4, 64), Table(dc, "chk_h", base, 4, 64)
    assert np.array_equal(a.keys, b.keys) and np.array_equal(a.js, b.js)
    x = words(base)
    assert dc.chk_fingerprint(p(x), C.c_uint(64)) == dc.chk_hfingerprint(p(x), C.c_uint(64))
    assert dc.chk_fingerprint(p(x), C.c_uint(4)) == dc.chk_fingerprint(p(x), C.c_uint(64)) & 15


def test_automatic_baby_bits_and_giant_steps(dc):
    want = {0: 1, 1: 1, 3: 1, 4: 2, 100: 4, (1 << 14) + 5: 8, (1 << 20): 11, (1 << 32) - 1: 16, (1 << 32): 17, (1 << 40) - 1: 20, (1 << 64) - 1: 20}
    assert {m: dc.chk_auto_baby_bits(C.c_uint64(m)) for m in want} == want
    assert dc.chk_giant_steps(C.c_uint64((1 << 64) - 1), C.c_uint(20)) == 1 << 44
    assert dc.chk_giant_steps(C.c_uint64((1 << 32) - 1), C.c_uint(16)) == 1 << 16
    assert dc.chk_giant_steps(C.c_uint64((1 << 14) + 5), C.c_uint(1)) == 8195


def test_lanes_of_one_launch_of_the_giant_search(dc):
    """whole 64-lane blocks per item out of about 2^16 lanes, at least one block, at most what the item's range takes"""
    lanes = lambda items, runs: dc.chk_launch_lanes(C.c_uint64(items), C.c_uint64(runs))
    assert lanes(520, 129) == 64 and lanes(512, 129) == 128 and lanes(260, 129) == 129
    assert lanes(25, 1024) == 1024 and lanes(25, 16384) == 2560 and lanes(1600, 1024) == 64 and lanes(65535, 3) == 3 and lanes(1, 1 << 18) == 1 << 16


def test_stand_alone_program_under_sanitizers(tmp_path):
    """dlog_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, no code loaded into python"""
    exe = str(tmp_path / "dlog_check_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DDLOG_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "dlog_check: ok" in r.stdout, r.stdout + r.stderr
