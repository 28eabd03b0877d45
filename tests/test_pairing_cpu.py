"""CPU build of the tower arithmetic and the pairing: vote_saver_protocol_amd/csrc/fp12.h and pairing.h compiled by g++ with the
32-bit-limb type the pairing kernels use (and the host's 64-bit-limb type), checked against oracle/pairing.py through the tower
conversion of oracle/wire.py.  No GPU, no HIP."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bls12_381 as o
import pairing as pg
import tower_cases as tc
import wire
from conftest import L, ROOT, g1_limbs, g2_limbs
from tower_cases import rand_fp, samples

P, R = o.P, o.R
SRC = os.path.join(ROOT, "tests", "cpu_build", "pairing_check.cpp")
TYPES = ["chk_", "chk_h"]                                           # 32-bit limbs, 64-bit limbs


@pytest.fixture(scope="module")
def pc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cpu_build") / "libpairingchk.so")
    flags = os.environ.get("VSP_MATHCHK_FLAGS", "-O2").split()
    subprocess.check_call(["g++"] + flags + ["-std=c++17", "-shared", "-fPIC", "-o", so, SRC])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def e_gen():
    """the oracle's e(G1, G2), polynomial form: the one slow oracle pairing most tests share"""
    return pg.final_exp(pg.miller_loop(o.G2.gen, o.G1.gen))


@pytest.fixture(scope="module")
def oracle_pairs():
    """(a G1, b G2, the oracle's own pairing of the two as 576 bytes) for four random (a, b)"""
    gen = o.splitmix64(2)
    out = []
    for _ in range(4):
        Pt, Q = o.G1.mul(o.G1.gen, o.rand_fr(gen)), o.G2.mul(o.G2.gen, o.rand_fr(gen))
        out.append((Pt, Q, wire.gt_to_tower_le(pg.final_exp(pg.miller_loop(Q, Pt)))))
    return out


def words(poly):
    return np.frombuffer(wire.gt_to_tower_le(poly), dtype=np.uint64).copy()


def op(lib, pre, code, a, b=None):
    out = np.zeros(72, np.uint64)
    wa, wb = words(a), words(b if b is not None else a)
    getattr(lib, pre + "f12_op")(code, wa.ctypes.data_as(C.c_void_p), wb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return wire.gt_from_tower_le(out.tobytes())


def product(lib, pre, pairs):
    g1 = np.concatenate([g1_limbs(p) if p is not None else np.zeros(12, np.uint64) for p, _ in pairs])
    g2 = np.concatenate([g2_limbs(q) if q is not None else np.zeros(24, np.uint64) for _, q in pairs])
    out = np.zeros(72, np.uint64)
    one = getattr(lib, pre + "pairing_product")(g1.ctypes.data_as(C.c_void_p), g2.ctypes.data_as(C.c_void_p), C.c_size_t(len(pairs)), out.ctypes.data_as(C.c_void_p))
    return out.tobytes(), bool(one)


_FROBENIUS = {}


def frobenius(a, k):
    """the oracle's a^(p^k), computed once per value (both limb types compare with it)"""
    key = (tuple(a), k)
    if key not in _FROBENIUS:
        _FROBENIUS[key] = pg.f12_pow(a, P ** k)
    return _FROBENIUS[key]


@pytest.mark.parametrize("pre", TYPES)
def test_fp12_operations_match_the_oracle(pc, pre):
    vals = samples()
    for i, a in enumerate(vals):
        b = vals[(i + 5) % len(vals)]
        assert op(pc, pre, 0, a, b) == pg.f12_mul(a, b), i
        assert op(pc, pre, 1, a) == pg.f12_mul(a, a), i
        assert op(pc, pre, 7, a, b) == pg.f12_add(a, b) and op(pc, pre, 8, a, b) == pg.f12_sub(a, b), i
        if any(a):
            inv = op(pc, pre, 2, a)
            assert inv == pg.f12_inv(a) and pg.f12_mul(inv, a) == pg.ONE, i
        else:
            assert op(pc, pre, 2, a) == pg.ZERO
    # every value: the conjugation is the Frobenius map p^6, w -> -w in the oracle's polynomial form (one value also through the
    # oracle's 2 286-bit power); p and p^2 against the oracle's power; and the maps compose
    assert frobenius(vals[0], 6) == [(-x) % P if k & 1 else x for k, x in enumerate(vals[0])]
    for a in vals:
        assert op(pc, pre, 3, a) == [(-x) % P if k & 1 else x for k, x in enumerate(a)]
        assert op(pc, pre, 4, a) == frobenius(a, 1)
        assert op(pc, pre, 5, a) == frobenius(a, 2)
        f1 = op(pc, pre, 4, a)
        assert op(pc, pre, 4, f1) == op(pc, pre, 5, a)
        assert op(pc, pre, 5, op(pc, pre, 5, op(pc, pre, 5, a))) == op(pc, pre, 3, a)


@pytest.mark.parametrize("pre", TYPES)
def test_the_shared_case_list_level_by_level(pc, pre):
    """every (level, op) of tower_cases.py -- the list the GPU selftests run -- through the g++ build of the same headers"""
    fn = getattr(pc, pre + "tower_op")
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for (level, op), (a, b, want) in sorted(tc.tower_cases().items()):
        out = np.zeros_like(a)
        assert fn(level, op, p(a), p(b), p(out), C.c_size_t(a.shape[0])) == 0
        bad = np.flatnonzero((out != want).any(axis=1))
        assert bad.size == 0, (level, op, bad[:8].tolist())
    out = np.zeros(72, np.uint64)
    for level, op in ((3, 0), (2, 14), (6, 5), (6, 9), (12, 13), (12, -1)):
        assert fn(level, op, p(out), p(out), p(out), C.c_size_t(1)) == 1


@pytest.mark.parametrize("pre", TYPES)
def test_sparse_line_product_equals_the_full_product(pc, pre):
    gen = o.splitmix64(14)
    for a in samples():
        l = [rand_fp(gen) for _ in range(6)]                        # l0 | l1 | l4 as Fp2 values
        line = np.zeros(72, np.uint64)
        for t, idx in enumerate((0, 1, 2, 3, 8, 9)):                # tower indices of v^0, v^1 (w^0) and v^1 w
            line[6 * idx:6 * idx + 6] = L(l[t], 6)
        lw = np.concatenate([L(x, 6) for x in l])
        out = np.zeros(72, np.uint64)
        getattr(pc, pre + "f12_sparse")(words(a).ctypes.data_as(C.c_void_p), lw.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        assert wire.gt_from_tower_le(out.tobytes()) == pg.f12_mul(a, wire.gt_from_tower_le(line.tobytes()))


@pytest.mark.parametrize("pre", TYPES)
def test_pairing_equals_the_oracle(pc, pre, e_gen, oracle_pairs):
    got, one = product(pc, pre, [(o.G1.gen, o.G2.gen)])
    assert got == wire.gt_to_tower_le(e_gen) and not one
    for Pt, Q, want in oracle_pairs:
        assert product(pc, pre, [(Pt, Q)])[0] == want
    inv = wire.gt_to_tower_le(pg.f12_inv(e_gen))
    assert product(pc, pre, [(o.G1.neg(o.G1.gen), o.G2.gen)])[0] == inv
    assert product(pc, pre, [(o.G1.gen, o.G2.neg(o.G2.gen))])[0] == inv
    assert inv == wire.gt_to_tower_le(pg.final_exp(pg.miller_loop(o.G2.gen, o.G1.neg(o.G1.gen))))


@pytest.mark.parametrize("pre", TYPES)
def test_infinity_and_products(pc, pre, e_gen):
    one = wire.gt_to_tower_le(pg.ONE)
    assert product(pc, pre, [(None, o.G2.gen)]) == (one, True)
    assert product(pc, pre, [(o.G1.gen, None)]) == (one, True)
    assert product(pc, pre, [(o.G1.gen, o.G2.gen), (o.G1.neg(o.G1.gen), o.G2.gen)]) == (one, True)
    P2, Q3 = o.G1.mul(o.G1.gen, 2), o.G2.mul(o.G2.gen, 3)
    got = product(pc, pre, [(o.G1.gen, o.G2.gen), (None, Q3), (P2, Q3)])
    assert got == (wire.gt_to_tower_le(pg.f12_pow(e_gen, 7)), False)


@pytest.mark.parametrize("pre", TYPES)
def test_bilinearity_with_255_bit_scalars(pc, pre, e_gen):
    gen = o.splitmix64(255)
    a, b = o.rand_fr(gen) | (1 << 254), o.rand_fr(gen) | (1 << 254)
    a, b = a % R, b % R
    assert a.bit_length() >= 253 and b.bit_length() >= 253
    got, _ = product(pc, pre, [(o.G1.mul(o.G1.gen, a), o.G2.mul(o.G2.gen, b))])
    assert got == wire.gt_to_tower_le(pg.f12_pow(e_gen, a * b % R))


@pytest.mark.parametrize("pre", TYPES)
def test_final_exponentiation_and_cyclotomic_square(pc, pre):
    """the final exponentiation of an arbitrary value against the oracle's plain power, and the Granger-Scott square against the
    general one on its result (the only values it is for)"""
    gen = o.splitmix64(12)
    f = [rand_fp(gen) for _ in range(12)]
    e = op(pc, pre, 9, f)
    assert e == pg.final_exp(f)
    assert op(pc, pre, 6, e) == pg.f12_mul(e, e)


def test_stand_alone_program_under_sanitizers(tmp_path):
    """pairing_check.cpp with its own main under AddressSanitizer and UBSan: both limb types, no code loaded into python"""
    exe = str(tmp_path / "pairing_check_san")
    # the sanitizer runtimes are linked statically: the program does not depend on the order of the libraries its environment loads
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPAIRING_CHECK_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "pairing_check: ok" in p.stdout, p.stdout + p.stderr
